// A world track's nodes for gfx950 (include/ikflow_amd_track.h): the world clearance of row r * T + t of a tile-major lattice against key frame t
// of the handle's track.  The geometry of k_world_clearance: 64-thread workgroups, the lane's capsule end points in LDS (one slice per lane,
// stride (6 n_caps) | 1: odd, so the lanes' slices start in different banks), the frame's table staged in LDS and read as a broadcast.  One
// wave handles one (waypoint t, block of 64 candidates), so the frame is wave-uniform; a workgroup walks waves blockIdx.x, blockIdx.x +
// gridDim.x, ... in t-major order and restages the table only when its t changes.  Two sinks behind ONE call site of world_clearance: the
// caller's outputs (ikf_world_track_clearance), or - in a path call - node[row] = +inf in place where the clearance is below the threshold;
// there a row that is already +inf is skipped, so the ranking's verdict is never read back as anything else.  No atomics, no scratch.
#include "ikf_internal.h"

namespace ikf {

constexpr long long kTrackMaxGrid = 1LL << 20;

IKF_SWEEP_HOST_DEVICE int track_blocks(int k) { return (k + 63) / 64; }

template <int NDOF>
__global__ __launch_bounds__(64) void k_track_clearance(const TrackArgs a) {
  extern __shared__ float track_lds[];   // [n_obs x 16] the key frame's table, then [64][cap_stride] capsule end points
  const int lane = threadIdx.x;
  const int n_obs = a.n_obs;
  float* const FRAME = track_lds;
  float* const w = track_lds + n_obs * IKF_WORLD_OBSTACLE_WORDS + lane * ((a.n_caps * 6) | 1);
  const long long T = a.T;
  const int k = a.k;
  const int blocks = track_blocks(k);
  const long long n_waves = T * blocks;
  long long staged = -1;
  for (long long wave = blockIdx.x; wave < n_waves; wave += gridDim.x) {
    const long long t = wave / blocks;
    const int r = (int)(wave % blocks) * 64 + lane;
    if (t != staged) {   // (workgroup-uniform)
      const float* const src = reinterpret_cast<const float*>(a.frames + t * a.frame_stride * n_obs);
      __syncthreads();
      for (int i = lane; i < n_obs * IKF_WORLD_OBSTACLE_WORDS; i += 64) FRAME[i] = src[i];
      __syncthreads();
      staged = t;
    }
    if (r >= k) continue;
    const long long row = (long long)r * T + t;
    if (a.node && !(a.node[row] < rank_inf())) continue;
    float qv[NDOF];
    load_q<NDOF>(a.q, row, qv);
    capsule_endpoints<NDOF>(a.ch, a.cm, qv, w);
    const WorldHit hit = world_clearance(reinterpret_cast<const WorldObstacle*>(FRAME), n_obs, a.cm, w);
    if (a.node) {
      if (hit.clearance < a.min_clearance) a.node[row] = rank_inf();
    } else {
      if (a.clearance) a.clearance[row] = hit.clearance;
      if (a.obstacle) a.obstacle[row] = hit.obstacle;
      if (a.capsule) a.capsule[row] = hit.capsule;
      if (a.colliding) a.colliding[row] = hit.clearance < a.min_clearance ? 1 : 0;
    }
  }
}

hipError_t launch_track_clearance(int ndof, const TrackArgs& a, hipStream_t s) {
  if (a.T <= 0) return hipSuccess;
  if (!a.ch || !a.cm || !a.frames || !a.q || a.n_caps < 0 || a.n_caps > IKF_MAX_CAPSULES || a.n_obs < 1 || a.n_obs > IKF_WORLD_MAX_OBSTACLES ||
      a.frame_stride < 1 || a.k < 1 || (long long)a.k * a.T > 0x7fffffffLL)
    return hipErrorInvalidValue;
  const long long waves = (long long)a.T * track_blocks(a.k);
  const size_t lds = sizeof(float) * ((size_t)a.n_obs * IKF_WORLD_OBSTACLE_WORDS + 64 * (size_t)((a.n_caps * 6) | 1));   // <= 4096 + 37120 B
  const unsigned grid = (unsigned)(waves < kTrackMaxGrid ? waves : kTrackMaxGrid);
  IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_track_clearance<ND>), dim3(grid), dim3(64), lds, s, a));
  return hipGetLastError();
}

}  // namespace ikf
