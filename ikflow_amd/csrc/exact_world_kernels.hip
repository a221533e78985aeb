// Exact IK under the exact collision rule for gfx950 (include/ikflow_amd_exact_world.h; the arithmetic: exact_world_math.h).
//
// k_exact_lm_iters_clear is the round's LM loop (k_exact_lm_iters, kin_kernels.hip: lm_step_row / pose_error_f32, one thread per row) with the
// world and self rule on the row's candidate in the same launch.  The loop runs first, for every lane; the test follows it, once, for the lanes
// that left the loop with a candidate - so the lanes of a wave meet again before the clearance work instead of doing it at the iteration each of
// them happened to stop at.  Geometry of k_world_clearance: 64-thread workgroups, the obstacle table staged once per workgroup into LDS (every lane
// reads the same obstacle word: a broadcast), the row's capsule end points in a per-lane LDS slice of stride (6 n_caps) | 1.  No pose_first: under
// the rule no row is stopped by a sibling, so rows, flags and the rejected count do not depend on how the rows interleave.  A rejected row
// stores row_valid_iter = 0 - k_exact_select_first then sees admissible rows only - and is counted: one atomic add per wave, from a ballot.
//
// k_exact_mask_rows is the cloud rule: the rows' cloud clearances come from k_cloud_clearance (cloud_kernels.hip) on the round's rows, this
// kernel takes the candidate from the rows below the threshold and counts them the same way.
#include "ikf_internal.h"
#include "exact_world_math.h"

namespace ikf {

__device__ __forceinline__ void count_rejected(bool rejected, unsigned long long* counter) {
  const unsigned long long votes = __ballot(rejected);
  if (votes != 0ULL && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)votes) - 1)) atomicAdd(counter, (unsigned long long)__popcll(votes));
}

template <int NDOF, typename T>
__global__ __launch_bounds__(IKF_EXACT_WORLD_THREADS) void k_exact_lm_iters_clear(
    const Chain* __restrict__ ch, const CollisionModel* __restrict__ cm, int cap_stride, const WorldModel* __restrict__ world, int n_obs,
    float world_min, int reject_self, float self_min, const float* __restrict__ poses, const int* __restrict__ pose_idx, int n_active, int repeat,
    int n_steps, const float* q_in, float* q, uint8_t* __restrict__ row_valid_iter, float pos_thr, float rot_thr,
    unsigned long long* __restrict__ rejected_rows) {  // q_in: the seeds (may be q itself)
  extern __shared__ float exact_world_lds[];   // [n_obs x 16] obstacle table, then [64][cap_stride] capsule end points
  float* const OBS = exact_world_lds;
  float* const W = exact_world_lds + n_obs * IKF_WORLD_OBSTACLE_WORDS;
  const float* const src = n_obs > 0 ? reinterpret_cast<const float*>(world->obs) : nullptr;   // (world may be null in an empty world)
  for (int i = threadIdx.x; i < n_obs * IKF_WORLD_OBSTACLE_WORDS; i += IKF_EXACT_WORLD_THREADS) OBS[i] = src[i];
  __syncthreads();
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = row < (long long)n_active * repeat;
  float qv[NDOF];
  int first = 0;
  if (live) {
    const float* tgt = poses + (size_t)pose_idx[(int)(row % n_active)] * 7;
    load_q<NDOF>(q_in, row, qv);
    for (int it = 0; it < n_steps; ++it) {
      lm_step_row<NDOF, T>(ch, tgt, qv);
      float pe, re;
      pose_error_f32<NDOF>(ch, qv, tgt, &pe, &re);
      if (pe < pos_thr && re < rot_thr) {  // the candidate: the iteration and the q that k_exact_lm_iters records
        first = it + 1;
        break;
      }
    }
  }
  bool rejected = false;
  if (first != 0)
    rejected = exact_row_rejected<NDOF>(ch, cm, reinterpret_cast<const WorldObstacle*>(OBS), n_obs, world_min, reject_self != 0, self_min, qv,
                                        W + threadIdx.x * cap_stride);
  if (live) {
#pragma unroll
    for (int k = 0; k < NDOF; ++k) q[(size_t)row * NDOF + k] = qv[k];
    row_valid_iter[row] = rejected ? (uint8_t)0 : (uint8_t)first;
  }
  count_rejected(rejected, rejected_rows);
}

__global__ __launch_bounds__(256) void k_exact_mask_rows(uint8_t* __restrict__ row_valid_iter, const float* __restrict__ cloud_clearance,
                                                         float cloud_min, long long rows, unsigned long long* __restrict__ rejected_rows) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool rejected = false;
  if (row < rows) {
    rejected = exact_cloud_rejected(row_valid_iter[row], cloud_clearance[row], cloud_min);
    if (rejected) row_valid_iter[row] = 0;
  }
  count_rejected(rejected, rejected_rows);
}

hipError_t launch_exact_lm_iters_clear(const ExactClearArgs& a, int ndof, hipStream_t s) {
  const long long rows = (long long)a.n_active * a.repeat;
  if (rows <= 0) return hipSuccess;
  if (a.n_steps > 255) return hipErrorInvalidValue;  // (the first-valid iteration is recorded in a byte)
  if (!a.ch || !a.cm || !a.rejected_rows || a.n_caps < 0 || a.n_caps > IKF_MAX_CAPSULES || a.n_obs < 0 || a.n_obs > IKF_WORLD_MAX_OBSTACLES ||
      (a.n_obs > 0 && !a.world))
    return hipErrorInvalidValue;
  const int cap_stride = exact_world_cap_stride(a.n_caps);
  const size_t lds = exact_world_lds_bytes(a.n_obs, a.n_caps);   // <= 4096 + 37120 B
  const dim3 grid((unsigned)exact_world_blocks(rows)), block(IKF_EXACT_WORLD_THREADS);
  if (a.lm_precision == 0) {
    IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_exact_lm_iters_clear<ND, float>), grid, block, lds, s, a.ch, a.cm, cap_stride, a.world, a.n_obs,
                                               a.world_min, a.reject_self, a.self_min, a.poses, a.pose_idx, a.n_active, a.repeat, a.n_steps, a.q_in,
                                               a.q, a.row_valid_iter, a.pos_thr, a.rot_thr, a.rejected_rows));
  } else {
    IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_exact_lm_iters_clear<ND, double>), grid, block, lds, s, a.ch, a.cm, cap_stride, a.world, a.n_obs,
                                               a.world_min, a.reject_self, a.self_min, a.poses, a.pose_idx, a.n_active, a.repeat, a.n_steps, a.q_in,
                                               a.q, a.row_valid_iter, a.pos_thr, a.rot_thr, a.rejected_rows));
  }
  return hipGetLastError();
}

hipError_t launch_exact_mask_rows(uint8_t* row_valid_iter, const float* cloud_clearance, float cloud_min, long long rows,
                                  unsigned long long* rejected_rows, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!row_valid_iter || !cloud_clearance || !rejected_rows) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_exact_mask_rows, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, row_valid_iter, cloud_clearance, cloud_min, rows,
                     rejected_rows);
  return hipGetLastError();
}

}  // namespace ikf
