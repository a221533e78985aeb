// exact_world_math.h - the arithmetic of exact IK under the exact collision rule (exact_world_kernels.hip; the definitions:
// include/ikflow_amd_exact_world.h): the verdict of one candidate row from capsule_endpoints / capsule_clearance (rank_math.h) and
// world_clearance (world_math.h) unchanged, the cloud rule's comparison, the selection over a pose's repeats, and the launch geometry.  Like
// sweep_math.h it holds nothing of the HIP runtime, so the same source compiles with g++: tests/test_exact_world_math_host.py runs it on the CPU
// against a numpy statement of the definition.
#pragma once
#include <stddef.h>

#include "world_math.h"
#include "../../include/ikflow_amd_exact_world.h"

namespace ikf {

// World and self rule on one candidate configuration: true when a rule rejects it.  Self rule (reject_self): capsule_clearance < self_min;
// world rule (n_obs > 0): world_clearance < world_min - on the end points the self rule's chain walk has left in w when it ran, as
// sweep_edge and rank_row_score_world do.  Strict `<`: a clearance equal to its threshold passes.  w: 6 floats per capsule, the caller's.
template <int NDOF>
IKF_HD bool exact_row_rejected(const Chain* __restrict__ ch, const CollisionModel* __restrict__ cm, const WorldObstacle* obs, int n_obs,
                               float world_min, bool reject_self, float self_min, const float qv[NDOF], float* w) {
  bool rejected = false;
  if (reject_self) rejected = capsule_clearance<NDOF>(ch, cm, qv, w) < self_min;
  if (!rejected && n_obs > 0) {
    if (!reject_self) capsule_endpoints<NDOF>(ch, cm, qv, w);
    rejected = world_clearance(obs, n_obs, cm, w).clearance < world_min;
  }
  return rejected;
}

// The same verdict from clearances that exist already (the host test's tables): each rule only when it applies.
IKF_HD bool exact_clearances_rejected(bool has_world, float world_clearance_v, float world_min, bool has_cloud, float cloud_clearance_v,
                                      float cloud_min, bool reject_self, float self_clearance_v, float self_min) {
  return (has_world && world_clearance_v < world_min) || (has_cloud && cloud_clearance_v < cloud_min) ||
         (reject_self && self_clearance_v < self_min);
}

// Cloud rule on a row of the round: a row with a candidate (first valid iteration != 0) whose cloud clearance is below the threshold loses it.
IKF_HD bool exact_cloud_rejected(int row_valid_iter, float cloud_clearance_v, float cloud_min) {
  return row_valid_iter != 0 && cloud_clearance_v < cloud_min;
}

// The selection of k_exact_select_first as a function (the kernel itself stays as it is): over the repeats of active pose j in the tile-major
// table row_valid_iter[r * n_active + j] - 0: no admissible candidate - the earliest iteration, and the highest repeat within it; -1: none.
IKF_HD int exact_select_repeat(const uint8_t* row_valid_iter, long long n_active, int repeat, long long j) {
  int best_it = 256, best_r = -1;
  for (int r = repeat - 1; r >= 0; --r) {
    const int it = row_valid_iter[(long long)r * n_active + j];
    if (it != 0 && it < best_it) {
      best_it = it;
      best_r = r;
    }
  }
  return best_r;
}

// launch geometry: one thread per row; one wave per workgroup, because every lane owns an LDS slice of (6 n_caps) | 1 floats (24 capsules:
// 37,120 B at 64 lanes) behind the staged obstacle table (at most 4 KB)
constexpr int IKF_EXACT_WORLD_THREADS = 64;
inline long long exact_world_blocks(long long rows) { return (rows + IKF_EXACT_WORLD_THREADS - 1) / IKF_EXACT_WORLD_THREADS; }
inline int exact_world_cap_stride(int n_caps) { return (n_caps * 6) | 1; }
inline size_t exact_world_lds_bytes(int n_obs, int n_caps) {
  return sizeof(float) * ((size_t)n_obs * IKF_WORLD_OBSTACLE_WORDS + (size_t)IKF_EXACT_WORLD_THREADS * (size_t)exact_world_cap_stride(n_caps));
}

}  // namespace ikf
