// World collision for gfx950 (include/ikflow_amd_world.h): the clearance of every row's configuration from the handle's obstacles, with the
// closest (obstacle, capsule) pair.  The geometry of k_self_collision: one thread per row, 64-thread workgroups, the row's capsule end points in
// LDS (dynamic; one slice per thread, stride (6 n_caps) | 1: odd, so the lanes' slices start in different banks).  The obstacle table is staged once per
// workgroup into LDS (at most 64 x 16 words = 4 KB); in the loop of world_clearance (world_math.h: obstacle outside, capsule inside) every lane
// reads the same obstacle word, an LDS broadcast - no lane issues a global load for obstacle data.  No atomics, no waiting, no scratch.
#include "ikf_internal.h"

namespace ikf {

template <int NDOF>
__global__ __launch_bounds__(64) void k_world_clearance(const Chain* __restrict__ ch, const CollisionModel* __restrict__ cm, int cap_stride,
                                                        const WorldModel* __restrict__ world, int n_obs, float min_clearance,
                                                        const float* __restrict__ q, long long n, float* __restrict__ clearance,
                                                        int* __restrict__ obstacle, int* __restrict__ capsule, uint8_t* __restrict__ colliding) {
  extern __shared__ float world_lds[];   // [n_obs x 16] obstacle table, then [64][cap_stride] capsule end points
  float* const OBS = world_lds;
  float* const W = world_lds + n_obs * IKF_WORLD_OBSTACLE_WORDS;
  const float* const src = n_obs > 0 ? reinterpret_cast<const float*>(world->obs) : nullptr;   // (world may be null in an empty world)
  for (int i = threadIdx.x; i < n_obs * IKF_WORLD_OBSTACLE_WORDS; i += 64) OBS[i] = src[i];
  __syncthreads();
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  WorldHit hit = {3.0e38f, -1, -1};
  if (n_obs > 0) {
    float* const w = W + threadIdx.x * cap_stride;
    float qv[NDOF];
    load_q<NDOF>(q, row, qv);
    capsule_endpoints<NDOF>(ch, cm, qv, w);
    hit = world_clearance(reinterpret_cast<const WorldObstacle*>(OBS), n_obs, cm, w);
  }
  if (clearance) clearance[row] = hit.clearance;
  if (obstacle) obstacle[row] = hit.obstacle;
  if (capsule) capsule[row] = hit.capsule;
  if (colliding) colliding[row] = hit.clearance < min_clearance ? 1 : 0;
}

hipError_t launch_world_clearance(const Chain* ch, const CollisionModel* cm, int n_caps, const WorldModel* world, int n_obs, float min_clearance,
                                  int ndof, const float* q, long long n, float* clearance, int* obstacle, int* capsule, uint8_t* colliding,
                                  hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (!ch || !cm || !q || n_caps < 0 || n_caps > IKF_MAX_CAPSULES || n_obs < 0 || n_obs > IKF_WORLD_MAX_OBSTACLES || (n_obs > 0 && !world))
    return hipErrorInvalidValue;
  const int cap_stride = (n_caps * 6) | 1;
  const size_t lds = sizeof(float) * ((size_t)n_obs * IKF_WORLD_OBSTACLE_WORDS + 64 * (size_t)cap_stride);   // <= 4096 + 37120 B
  IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_world_clearance<ND>), dim3((unsigned)((n + 63) / 64)), dim3(64), lds, s, ch, cm, cap_stride, world,
                                             n_obs, min_clearance, q, n, clearance, obstacle, capsule, colliding));
  return hipGetLastError();
}

}  // namespace ikf
