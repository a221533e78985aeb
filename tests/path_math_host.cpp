// Test harness (CPU): the arithmetic of path IK - ikflow_amd/csrc/path_math.h, the very source the GPU runs - compiled with g++ and driven
// node by node the way k_path_lattice drives it, so that tests/test_path_math_host.py can hold it against brute force and numpy without a GPU.
// Not part of the product.
#include <vector>

#include "../ikflow_amd/csrc/path_math.h"

using ikf::PathBest;

extern "C" void path_host_constants(int* out) {
  out[0] = ikf::IKF_PATH_BLOCK;
  out[1] = ikf::IKF_PATH_ROW;
  out[2] = ikf::IKF_PATH_STAGE;
  out[3] = ikf::IKF_PATH_BT_CHUNK;
  out[4] = IKF_PATH_MAX_K;
  out[5] = (int)sizeof(ikf_path_options);
}
extern "C" int path_host_span(int k) { return ikf::path_span(k); }
extern "C" int path_host_slices(int k) { return ikf::path_slices(k); }
extern "C" long long path_host_stages(long long T) { return ikf::path_stages(T); }
extern "C" long long path_host_bt_chunks(long long T) { return ikf::path_bt_chunks(T); }
extern "C" long long path_host_bp_bytes(long long T, int k) { return ikf::path_bp_bytes(T, k); }

// The lattice of T x k nodes (q [k*T x N] tile-major, node [k*T]) relaxed as the kernel does it: every node's predecessors split over n_slices
// slices (slice s takes j = s, s + n_slices, ...), the slices merged in the order `order` gives; back-pointers a byte per node; the walk back in
// chunks of `chunk` waypoints.
template <int N>
static void lattice(const float* q, const float* node, long long T, int k, const float* q_start, float node_weight, float max_step, int n_slices,
                    const int* order, int chunk, float* path_out, int* index_out, float* cost_out, int* reachable_out) {
  std::vector<float> cost(2 * (size_t)k);
  std::vector<uint8_t> bp((size_t)ikf::path_bp_bytes(T, k));
  for (long long t = 0; t < T; ++t) {
    float* cur = cost.data() + (t & 1) * k;
    const float* prev = cost.data() + ((t & 1) ^ 1) * k;
    int reach = 0;
    for (int r = 0; r < k; ++r) {
      const float* row = q + ((long long)r * T + t) * N;
      std::vector<PathBest> part(n_slices, ikf::path_none());
      if (t == 0) {
        part[0] = ikf::path_start<N>(q_start, q_start != nullptr, row, max_step);
      } else {
        for (int s = 0; s < n_slices; ++s)
          for (int j = s; j < k; j += n_slices) ikf::path_relax<N>(part[s], prev[j], q + ((long long)j * T + t - 1) * N, j, row, max_step);
      }
      PathBest best = part[order[0]];
      for (int s = 1; s < n_slices; ++s) ikf::path_merge(best, part[order[s]]);
      const float c = ikf::path_finish(best, node[(long long)r * T + t], node_weight);
      cur[r] = c;
      const bool ok = c < ikf::rank_inf();
      reach += ok ? 1 : 0;
      bp[t * k + r] = (uint8_t)(ok ? best.j : 0);
    }
    if (reachable_out) reachable_out[t] = reach;
  }
  const float* fc = cost.data() + ((T - 1) & 1) * k;
  int cur = ikf::path_argmin(fc, k);
  cost_out[0] = cur >= 0 ? fc[cur] : ikf::rank_inf();
  if (cur < 0) {
    for (long long i = 0; i < T * N; ++i) path_out[i] = 0.f;
    for (long long t = 0; t < T; ++t) index_out[t] = -1;
    return;
  }
  std::vector<int> idx(chunk);
  for (long long c = (T + chunk - 1) / chunk - 1; c >= 0; --c) {
    const long long t0 = c * chunk;
    const int n = T - t0 < chunk ? (int)(T - t0) : chunk;
    cur = ikf::path_backtrack_chunk(bp.data() + t0 * k, k, n, cur, idx.data());
    for (int i = 0; i < n; ++i) {
      index_out[t0 + i] = idx[i];
      for (int d = 0; d < N; ++d) path_out[(t0 + i) * N + d] = q[((long long)idx[i] * T + t0 + i) * N + d];
    }
  }
}

extern "C" int path_host_lattice(int ndof, const float* q, const float* node, long long T, int k, const float* q_start, float node_weight, float max_step,
                                 int n_slices, const int* order, int chunk, float* path_out, int* index_out, float* cost_out, int* reachable_out) {
  if (T < 1 || k < 1 || k > IKF_PATH_MAX_K || n_slices < 1) return 1;
  if (chunk < 1) chunk = ikf::IKF_PATH_BT_CHUNK;
#define LATTICE(N) \
  case N: lattice<N>(q, node, T, k, q_start, node_weight, max_step, n_slices, order, chunk, path_out, index_out, cost_out, reachable_out); return 0;
  switch (ndof) {
    LATTICE(4) LATTICE(5) LATTICE(6) LATTICE(7) LATTICE(8)
    default: return 1;
  }
#undef LATTICE
}

// edge(a, b) of two rows of 7 joints and whether the gate allows it
extern "C" float path_host_edge7(const float* a, const float* b, float max_step, int* allowed) {
  bool ok;
  const float e = ikf::path_edge<7>(a, b, max_step, &ok);
  *allowed = ok ? 1 : 0;
  return e;
}
