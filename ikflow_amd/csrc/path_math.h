// path_math.h - the arithmetic of path IK (path_kernels.hip; the definition: include/ikflow_amd_path.h): the edge between two candidate rows,
// the relaxation of one lattice node over a slice of its predecessors, the merge of slices, the end of the path, the walk back along the
// back-pointers, and the launch geometry.  Like kin_math.h and rank_math.h it holds nothing of the HIP runtime, so the same source compiles
// with g++: tests/test_path_math_host.py runs it on the CPU against brute force and against sequential numpy float32 arithmetic.
//
// Rounding: every function that adds or multiplies is compiled without contraction (#pragma clang fp contract(off), as solve_lu_pivot), so
// a sum of squares is separate multiplies and adds in source order and cost + edge + node_weight * node is two adds and one multiply.  The
// square root is correctly rounded.  Given the node costs, the lattice is therefore a function of its inputs alone, not of the compiler.
#pragma once
#include "rank_math.h"
#include "../../include/ikflow_amd_path.h"

#if defined(__HIPCC__)
#define IKF_PATH_HOST_DEVICE __host__ __device__ inline
#else
#define IKF_PATH_HOST_DEVICE inline
#endif

namespace ikf {

constexpr int IKF_PATH_BLOCK = 256;      // threads of the lattice workgroup (four waves)
constexpr int IKF_PATH_ROW = 8;          // floats of a candidate row in LDS (IKF_MAX_DOF: two 128-bit reads)
constexpr int IKF_PATH_STAGE = 2;        // waypoints whose rows are loaded together (k segments of STAGE * ndof contiguous floats)
constexpr int IKF_PATH_BT_CHUNK = 64;    // waypoints of back-pointers staged in LDS at a time by the walk back (<= 16 KiB at k = 256)
static_assert(IKF_PATH_ROW >= IKF_MAX_DOF, "a candidate row must fit its LDS slot");
static_assert(IKF_PATH_MAX_K <= IKF_PATH_BLOCK && IKF_PATH_MAX_K <= 256, "a thread per destination, a byte per back-pointer");

// The best predecessor found so far: (accumulated cost + edge, predecessor index).  Empty: (+inf, INT32_MAX).
struct PathBest {
  float c;
  int j;
};
IKF_HD PathBest path_none() { return PathBest{rank_inf(), 0x7fffffff}; }
// the strict total order (lower sum, then lower j)
IKF_HD bool path_before(float c, int j, const PathBest& b) { return c < b.c || (c == b.c && j < b.j); }

// edge(a, b); *allowed = false when the step gate forbids it (the value is then not to be used)
template <int NDOF>
IKF_HD float path_edge(const float* a, const float* b, float max_step, bool* allowed) {
#pragma clang fp contract(off)
  float s = 0.f;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < NDOF; ++j) {
    const float d = b[j] - a[j];
    if (max_step >= 0.f && fabsf(d) > max_step) ok = false;
    s = s + d * d;
  }
  *allowed = ok;
  return sqrtf(s);
}

// One predecessor j (accumulated cost prev_cost, row prev_row) offered to the node whose row is `row`.  Skipped before its edge is looked
// at when its cost is not below +inf; not taken when the edge is forbidden or the sum is not below +inf.
template <int NDOF>
IKF_HD void path_relax(PathBest& best, float prev_cost, const float* prev_row, int j, const float* row, float max_step) {
#pragma clang fp contract(off)
  if (!(prev_cost < rank_inf())) return;
  bool allowed;
  const float e = path_edge<NDOF>(prev_row, row, max_step, &allowed);
  if (!allowed) return;
  const float s = prev_cost + e;
  if (!(s < rank_inf())) return;
  if (path_before(s, j, best)) { best.c = s; best.j = j; }
}
// the best of two slices of the predecessors: total order, so any split and any merge order give the same result
IKF_HD void path_merge(PathBest& a, const PathBest& o) {
  if (o.c < rank_inf() && path_before(o.c, o.j, a)) a = o;
}
// cost of the node given its best predecessor (for waypoint 0: the start, (0, 0) or (edge(q_start, row), 0)) and its node cost
IKF_HD float path_finish(const PathBest& best, float node, float node_weight) {
#pragma clang fp contract(off)
  if (!(node < rank_inf()) || !(best.c < rank_inf())) return rank_inf();
  const float c = best.c + node_weight * node;
  return c < rank_inf() ? c : rank_inf();
}
// what waypoint 0 is relaxed against
template <int NDOF>
IKF_HD PathBest path_start(const float* q_start, bool has_start, const float* row, float max_step) {
  PathBest b = path_none();
  if (!has_start) { b.c = 0.f; b.j = 0; }
  else path_relax<NDOF>(b, 0.f, q_start, 0, row, max_step);
  return b;
}

// end of the path: argmin_r cost[r], the lower r on ties; -1 when no cost is below +inf
IKF_HD int path_argmin(const float* cost, int k) {
  PathBest b = path_none();
  for (int r = 0; r < k; ++r)
    if (cost[r] < rank_inf() && path_before(cost[r], r, b)) { b.c = cost[r]; b.j = r; }
  return b.c < rank_inf() ? b.j : -1;
}

// The walk back over n consecutive waypoints whose back-pointer rows are bp[0 .. n) x [k] (bp[i][r]: the predecessor of candidate r of the
// chunk's waypoint i): `cur` is the path's candidate at the chunk's last waypoint; writes the path's candidates idx[0 .. n) and returns the
// candidate at the waypoint in front of the chunk (meaningless in front of waypoint 0).
IKF_HD int path_backtrack_chunk(const uint8_t* bp, int k, int n, int cur, int* idx) {
  for (int i = n - 1; i >= 0; --i) {
    idx[i] = cur;
    cur = bp[(long long)i * k + cur];
  }
  return cur;
}

// ---- the launch geometry, pure integer arithmetic; the lattice kernel derives its roles from the same functions -----
// destinations a slice of the workgroup spans: the next power of two >= k; the block's IKF_PATH_BLOCK / path_span(k) slices split the predecessors
IKF_PATH_HOST_DEVICE int path_span(int k) {
  int kp = 1;
  while (kp < k && kp < IKF_PATH_BLOCK) kp <<= 1;
  return kp;
}
inline int path_slices(int k) { return IKF_PATH_BLOCK / path_span(k); }
IKF_PATH_HOST_DEVICE long long path_stages(long long T) { return (T + IKF_PATH_STAGE - 1) / IKF_PATH_STAGE; }
IKF_PATH_HOST_DEVICE long long path_bt_chunks(long long T) { return (T + IKF_PATH_BT_CHUNK - 1) / IKF_PATH_BT_CHUNK; }
// bytes of the back-pointer scratch of a T x k lattice: a byte per node, rounded up so that the walk back may read whole words
IKF_PATH_HOST_DEVICE long long path_bp_bytes(long long T, int k) { return ((T * k + 3) / 4 + 1) * 4; }

}  // namespace ikf
