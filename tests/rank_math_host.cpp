// Test harness (CPU): the arithmetic of best-of-K ranking - ikflow_amd/csrc/rank_math.h, the very source the GPU runs - compiled with g++ and
// driven row by row / list by list, so that tests/test_rank_math_host.py can hold it against the oracle and numpy without a GPU.  Not part of the product.
#include <vector>

#include "../ikflow_amd/csrc/rank_math.h"

using ikf::Chain;
using ikf::CollisionModel;

static CollisionModel g_cm;

extern "C" int rank_host_chain_bytes() { return (int)sizeof(Chain); }
extern "C" int rank_host_chunks(long long n_poses, int k, int n_cu) { return ikf::rank_chunks(n_poses, k, n_cu); }
extern "C" int rank_host_tile_poses(long long n_poses) { return ikf::rank_tile_poses(n_poses); }

// capsules in engine frames (ikf_capsule) and index pairs, as ikf_set_collision_model takes them
extern "C" void rank_host_set_collision(const ikf_capsule* caps, int n_caps, const int32_t* pairs, int n_pairs) {
  g_cm = CollisionModel{};
  g_cm.n_caps = n_caps;
  g_cm.n_pairs = n_pairs;
  for (int c = 0; c < n_caps; ++c) {
    g_cm.frame[c] = caps[c].frame;
    g_cm.radius[c] = caps[c].radius;
    for (int i = 0; i < 3; ++i) { g_cm.p0[c][i] = caps[c].p0[i]; g_cm.p1[c][i] = caps[c].p1[i]; }
  }
  for (int p = 0; p < n_pairs; ++p) { g_cm.pair_a[p] = (uint8_t)pairs[2 * p]; g_cm.pair_b[p] = (uint8_t)pairs[2 * p + 1]; }
}

template <int N>
static void scores(const Chain* ch, const ikf_rank_options* o, const float* poses, const float* q, const float* q_ref, long long m, int k, float* out,
                   float* clearance) {
  float w[IKF_MAX_CAPSULES * 6];
  for (int r = 0; r < k; ++r)
    for (long long j = 0; j < m; ++j) {
      const long long row = r * m + j;
      float qv[N], qr[N];
      for (int d = 0; d < N; ++d) { qv[d] = q[row * N + d]; qr[d] = q_ref ? q_ref[j * N + d] : 0.f; }
      out[row] = ikf::rank_row_score<N>(ch, &g_cm, qv, poses + j * 7, qr, q_ref != nullptr, *o, w);
      if (clearance) clearance[row] = ikf::capsule_clearance<N>(ch, &g_cm, qv, w);
    }
}

// row scores of k candidates of each of m poses, tile-major (row r * m + j); clearance: nullable, the rows' clearances under the model set above
extern "C" int rank_host_scores(const void* chain, const ikf_rank_options* o, const float* poses, const float* q, const float* q_ref, long long m, int k,
                                float* out, float* clearance) {
  const Chain* ch = static_cast<const Chain*>(chain);
  switch (ch->ndof) {
    case 4: scores<4>(ch, o, poses, q, q_ref, m, k, out, clearance); return 0;
    case 5: scores<5>(ch, o, poses, q, q_ref, m, k, out, clearance); return 0;
    case 6: scores<6>(ch, o, poses, q, q_ref, m, k, out, clearance); return 0;
    case 7: scores<7>(ch, o, poses, q, q_ref, m, k, out, clearance); return 0;
    case 8: scores<8>(ch, o, poses, q, q_ref, m, k, out, clearance); return 0;
    default: return 1;
  }
}

// The k scores of one pose split over n_slices lists as the kernel's threads split them (slice s takes repeats s, s + n_slices, ...; `reverse`:
// inserted in descending order), then merged into one list in the order `order` gives (a permutation of the slices).
template <int NK>
static void toplist(const float* s, int k, int n_slices, const int* order, int reverse, float* out_s, int* out_i) {
  std::vector<ikf::TopList<NK>> lists(n_slices);
  for (int sl = 0; sl < n_slices; ++sl) {
    lists[sl].clear();
    std::vector<int> mine;
    for (int r = sl; r < k; r += n_slices) mine.push_back(r);
    for (size_t a = 0; a < mine.size(); ++a) {
      const int r = reverse ? mine[mine.size() - 1 - a] : mine[a];
      lists[sl].insert(s[r], r);
    }
  }
  ikf::TopList<NK> acc = lists[order[0]];
  for (int a = 1; a < n_slices; ++a) acc.merge(lists[order[a]]);
  for (int t = 0; t < NK; ++t) { out_s[t] = acc.s[t]; out_i[t] = acc.i[t]; }
}
extern "C" int rank_host_toplist(int capacity, const float* s, int k, int n_slices, const int* order, int reverse, float* out_s, int* out_i) {
  switch (capacity) {
    case 1: toplist<1>(s, k, n_slices, order, reverse, out_s, out_i); return 0;
    case 4: toplist<4>(s, k, n_slices, order, reverse, out_s, out_i); return 0;
    case 16: toplist<16>(s, k, n_slices, order, reverse, out_s, out_i); return 0;
    default: return 1;
  }
}
