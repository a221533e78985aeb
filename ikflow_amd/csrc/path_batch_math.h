// path_batch_math.h - the integer geometry of batched path IK (include/ikflow_amd_path_batch.h; path_kernels.hip, sweep_kernels.hip): P paths of T
// waypoints each in ONE candidate layout of P * T waypoints.  Global waypoint g = p * T + t; row r * (P * T) + g is candidate r of waypoint t of
// path p.  Where a path's waypoints, node costs, back-pointers and mask words begin, and which path a wave of the sweep kernel works for.  Like
// path_math.h and sweep_math.h it holds nothing of the HIP runtime, so the same source compiles with g++ (tests/test_path_batch_math_host.py).
// There is no floating-point arithmetic here: the arithmetic of a batched path is path_math.h's and sweep_math.h's, unchanged.
#pragma once
#include "path_math.h"
#include "sweep_math.h"
#include "../../include/ikflow_amd_path_batch.h"

namespace ikf {

// waypoints of the whole batch: the row stride of the candidate layout
IKF_PATH_HOST_DEVICE long long path_batch_waypoints(long long P, long long T) { return P * T; }
// the first global waypoint of path p
IKF_PATH_HOST_DEVICE long long path_batch_offset(long long p, long long T) { return p * T; }
// row of candidate r of waypoint t of path p
IKF_PATH_HOST_DEVICE long long path_batch_row(long long P, long long T, long long p, long long t, int r) { return (long long)r * (P * T) + p * T + t; }

// Back-pointers: a block of path_bp_bytes(T, k) bytes per path - NOT T * k, which need not be a multiple of four: the walk back reads whole
// words from the start of its block, and the padding word of a block keeps a path's last read inside it.
IKF_PATH_HOST_DEVICE long long path_batch_bp_stride(long long T, int k) { return path_bp_bytes(T, k); }
IKF_PATH_HOST_DEVICE long long path_batch_bp_offset(long long p, long long T, int k) { return p * path_batch_bp_stride(T, k); }
IKF_PATH_HOST_DEVICE long long path_batch_bp_bytes(long long P, long long T, int k) { return P * path_batch_bp_stride(T, k); }

// the first word of path p in the sweep's mask over P * T waypoints (sweep_word_index(p * T + t, r, word, k) = this + sweep_word_index(t, r, word, k))
IKF_PATH_HOST_DEVICE long long path_batch_mask_offset(long long p, long long T, int k) { return sweep_word_index(p * T, 0, 0, k); }

// A wave of the sweep kernel's lattice source over a batch: sweep_wave_role gives its global waypoint g; this gives the path and the waypoint
// inside it.  t == 0: the wave stands for the path's start edge - there is no edge from waypoint T - 1 of path p - 1.
struct PathBatchRole {
  long long p, t;
};
IKF_PATH_HOST_DEVICE PathBatchRole path_batch_role(long long g, long long T) {
  PathBatchRole role;
  role.p = g / T;
  role.t = g - role.p * T;
  return role;
}
// the predecessor row of candidate j for a wave at global waypoint g (t > 0 only)
IKF_PATH_HOST_DEVICE long long path_batch_pred_row(long long P, long long T, long long g, int j) { return (long long)j * (P * T) + g - 1; }

}  // namespace ikf
