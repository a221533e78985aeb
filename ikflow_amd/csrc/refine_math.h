// refine_math.h - the arithmetic of refined candidates (refine_kernels.hip; the definitions: include/ikflow_amd_refine.h): the loop of one row over
// lm_step_row / pose_error_f32 (kin_math.h) unchanged, and the launch geometry.  Like kin_math.h it holds nothing of the HIP runtime, so the
// same source compiles with g++: tests/test_refine_math_host.py runs it on the CPU against a loop of the oracle.
#pragma once
#include "kin_math.h"
#include "../../include/ikflow_amd_refine.h"

namespace ikf {

// Up to n_steps LM steps on qv towards tgt (T: the step's arithmetic, as lm_step_row), the f32 pose error after every step, stopping at the
// first step after which both errors are below their tolerances.  *steps: steps applied (1 .. n_steps; 0 only for n_steps < 1);
// *converged: the loop stopped on its test.  A tolerance of 0, or a NaN error, never stops the row (the comparisons are false).
template <int NDOF, typename T>
IKF_HD void refine_row(const Chain* __restrict__ ch, const float* __restrict__ tgt, float qv[NDOF], int n_steps, float pos_tol, float rot_tol,
                       int* steps, int* converged) {
  int done = 0, conv = 0;
  for (int it = 0; it < n_steps; ++it) {
    lm_step_row<NDOF, T>(ch, tgt, qv);
    done = it + 1;
    float pe, re;
    pose_error_f32<NDOF>(ch, qv, tgt, &pe, &re);
    if (pe < pos_tol && re < rot_tol) { conv = 1; break; }
  }
  *steps = done;
  *converged = conv;
}

// launch geometry: one thread per row, 256 per workgroup
constexpr int IKF_REFINE_THREADS = 256;
inline long long refine_blocks(long long rows) { return (rows + IKF_REFINE_THREADS - 1) / IKF_REFINE_THREADS; }

}  // namespace ikf
