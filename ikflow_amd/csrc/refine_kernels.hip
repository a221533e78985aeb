// Refined candidates for gfx950 (include/ikflow_amd_refine.h): up to n_steps LM steps on every candidate row, each row against the pose of its
// tile position, stopping a row when it is inside the tolerances.  The arithmetic is refine_math.h over kin_math.h; this kernel only places it.
//
// The geometry of k_lm_step / k_exact_lm_iters: one thread per row, 256 per workgroup, the chain walk, the 6 x ndof Jacobian and the normal
// equations of a step in registers (every loop unrolled on the compile-time NDOF); the step loop itself is NOT unrolled, so the kernel holds one
// copy of the step and one of the pose error, like k_exact_lm_iters.  What that kernel has and this one lacks is the hand-over between the
// repeats of a pose (pose_first, the atomics): no row here waits on or is stopped by another.  Rows are independent, so q_out may be q_in.
#include "ikf_internal.h"

namespace ikf {

template <int NDOF, typename T>
__global__ __launch_bounds__(IKF_REFINE_THREADS) void k_refine_candidates(const Chain* __restrict__ ch, const float* __restrict__ poses, int n_poses,
                                                                        long long rows, const float* q_in, float* q_out,   // q_out may be q_in: no __restrict__ on the two
                                                                        int n_steps, float pos_tol, float rot_tol, uint8_t* __restrict__ steps_out,
                                                                        uint8_t* __restrict__ converged_out) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const float* tgt = poses + (size_t)(row % n_poses) * 7;
  float qv[NDOF];
  load_q<NDOF>(q_in, row, qv);
  int steps, converged;
  refine_row<NDOF, T>(ch, tgt, qv, n_steps, pos_tol, rot_tol, &steps, &converged);
#pragma unroll
  for (int j = 0; j < NDOF; ++j) q_out[(size_t)row * NDOF + j] = qv[j];
  if (steps_out) steps_out[row] = (uint8_t)steps;
  if (converged_out) converged_out[row] = (uint8_t)converged;
}

hipError_t launch_refine(const Chain* ch, int ndof, const float* poses, long long n_poses, int k, const float* q_in, float* q_out, int n_steps,
                         float pos_tol, float rot_tol, uint8_t* steps_out, uint8_t* converged_out, int lm_precision, hipStream_t s) {
  if (n_poses <= 0) return hipSuccess;
  const long long rows = n_poses * (long long)k;
  if (!ch || !poses || !q_in || !q_out || k < 1 || n_poses > 0x7fffffffLL || rows > 0x7fffffffLL || n_steps < 1 || n_steps > IKF_REFINE_MAX_STEPS)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)refine_blocks(rows)), block(IKF_REFINE_THREADS);
  if (lm_precision == 0) {
    IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_refine_candidates<ND, float>), grid, block, 0, s, ch, poses, (int)n_poses, rows, q_in, q_out,
                                               n_steps, pos_tol, rot_tol, steps_out, converged_out));
  } else {
    IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_refine_candidates<ND, double>), grid, block, 0, s, ch, poses, (int)n_poses, rows, q_in, q_out,
                                               n_steps, pos_tol, rot_tol, steps_out, converged_out));
  }
  return hipGetLastError();
}

}  // namespace ikf
