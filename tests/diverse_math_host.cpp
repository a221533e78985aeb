// Test harness (CPU): the arithmetic of diverse-of-K IK - ikflow_amd/csrc/diverse_math.h, the very source the GPU runs - compiled with g++ and
// driven round by round the way k_diverse_select drives it, so that tests/test_diverse_math_host.py can hold it against numpy and brute force
// without a GPU.  Not part of the product.
#include <vector>

#include "../ikflow_amd/csrc/diverse_math.h"

using ikf::DiverseBest;
using ikf::DiverseFirst;

extern "C" void diverse_host_constants(int* out) {
  out[0] = IKF_DIVERSE_MAX_K;
  out[1] = IKF_DIVERSE_MAX_KEEP;
  out[2] = ikf::IKF_DIVERSE_MIN_BLOCK;
  out[3] = ikf::IKF_DIVERSE_MAX_BLOCK;
  out[4] = ikf::IKF_DIVERSE_PER_THREAD;
  out[5] = (int)sizeof(ikf_diverse_options);
}
extern "C" int diverse_host_block(int k) { return ikf::diverse_block(k); }
extern "C" int diverse_host_row_stride(int ndof) { return ikf::diverse_row_stride(ndof); }
extern "C" long long diverse_host_lds_bytes(int ndof, int k) { return (long long)ikf::diverse_lds_bytes(ndof, k); }

// One pose: q [k x N], score [k].  The candidates are split over n_slices slices (slice s owns r = s, s + n_slices, ...), each slice takes its
// local best, and the slices are merged in the order `order` gives - the kernel's threads and waves.
template <int N>
static void select(const float* q, const float* score, int k, int n_keep, float min_separation, const float* w, int n_slices, const int* order,
                   float* q_out, float* score_out, int* index_out, float* sep_out, int* kept_out, int* count_out) {
  std::vector<float> near2((size_t)k, ikf::rank_inf());
  std::vector<char> alive((size_t)k);
  const float sep2 = ikf::diverse_sep2(min_separation);
  int count = 0, kept = 0;
  std::vector<DiverseFirst> firsts((size_t)n_slices, ikf::diverse_first_none());
  for (int r = 0; r < k; ++r) {
    alive[r] = score[r] < ikf::rank_inf();
    if (alive[r]) {
      ikf::diverse_first_offer(firsts[r % n_slices], score[r], r);
      ++count;
    }
  }
  DiverseFirst first = firsts[order[0]];
  for (int s = 1; s < n_slices; ++s) ikf::diverse_first_merge(first, firsts[order[s]]);
  int p = first.r;
  if (count > 0) {
    for (int d = 0; d < N; ++d) q_out[d] = q[(size_t)p * N + d];
    score_out[0] = score[p];
    index_out[0] = p;
    sep_out[0] = ikf::rank_inf();
    kept = 1;
    for (int i = 1; i < n_keep; ++i) {
      std::vector<DiverseBest> part((size_t)n_slices, ikf::diverse_none());
      for (int r = 0; r < k; ++r) {
        if (alive[r] && r == p) alive[r] = 0;
        if (alive[r]) {
          near2[r] = ikf::diverse_near2(near2[r], ikf::diverse_dist2<N>(q + (size_t)r * N, q + (size_t)p * N, w));
          ikf::diverse_offer(part[r % n_slices], near2[r], r);
        }
      }
      DiverseBest best = part[order[0]];
      for (int s = 1; s < n_slices; ++s) ikf::diverse_merge(best, part[order[s]]);
      if (ikf::diverse_stop(best, sep2)) break;
      p = best.r;
      for (int d = 0; d < N; ++d) q_out[(size_t)i * N + d] = q[(size_t)p * N + d];
      score_out[i] = score[p];
      index_out[i] = p;
      sep_out[i] = sqrtf(best.n);
      kept = i + 1;
    }
  }
  for (int i = kept; i < n_keep; ++i) {
    for (int d = 0; d < N; ++d) q_out[(size_t)i * N + d] = 0.f;
    score_out[i] = ikf::rank_inf();
    index_out[i] = -1;
    sep_out[i] = ikf::rank_inf();
  }
  *kept_out = kept;
  *count_out = count;
}

extern "C" int diverse_host_select(int ndof, const float* q, const float* score, int k, int n_keep, float min_separation, const float* w, int n_slices,
                                   const int* order, float* q_out, float* score_out, int* index_out, float* sep_out, int* kept_out, int* count_out) {
  if (k < 1 || k > IKF_DIVERSE_MAX_K || n_keep < 1 || n_keep > IKF_DIVERSE_MAX_KEEP || n_keep > k || n_slices < 1) return 1;
#define SELECT(N) \
  case N: select<N>(q, score, k, n_keep, min_separation, w, n_slices, order, q_out, score_out, index_out, sep_out, kept_out, count_out); return 0;
  switch (ndof) {
    SELECT(4) SELECT(5) SELECT(6) SELECT(7) SELECT(8)
    default: return 1;
  }
#undef SELECT
}

extern "C" float diverse_host_dist2(int ndof, const float* a, const float* b, const float* w) {
  switch (ndof) {
    case 4: return ikf::diverse_dist2<4>(a, b, w);
    case 5: return ikf::diverse_dist2<5>(a, b, w);
    case 6: return ikf::diverse_dist2<6>(a, b, w);
    case 7: return ikf::diverse_dist2<7>(a, b, w);
    case 8: return ikf::diverse_dist2<8>(a, b, w);
    default: return -1.f;
  }
}
