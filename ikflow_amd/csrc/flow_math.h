// flow_math.h - the per-element arithmetic of the conditional flow (affine coupling in both directions with its log-det share, the sigmoid
// layer and its inverse, one step of the two FixedLinearTransform directions, the limit clamp, the pose row of a flow row): what every flow
// form - per-layer, fused, chain, row-owner, cluster, forward and inverse - evaluates per element, defined ONCE and WITHOUT anything of the
// HIP runtime in it, so that the same source also compiles with g++ - tests/test_flow_math_host.py runs it on the CPU against fp64 and against
// oracle/flow_oracle.py.  The forms keep their own loops, shuffles and LDS traffic; they share the steps below.
// Statement shape matters to the compiler here: the forms the planner picks are instruction-identical to their hand-written predecessors only
// with the scale and the coupling step as two statements and the loops at the call site - keep it so.
// Test infrastructure compiles this header; the product only ever runs it on the GPU (the library has no CPU path).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define IKF_HD __device__ __forceinline__
#else
#define IKF_HD inline
#endif

namespace ikf {

// ---- where the conditional (target pose) of a flow row comes from ------------------------------------------
// pose of global row r = poses + stride * (idx ? idx[r % n_mod] : r % n_mod)
//   batch form      : idx = null, n_mod = n,  stride = 7      (ikflow_solver.py:338)
//   single-pose form: idx = null, n_mod = 1,  stride = 0..7   (ikflow_solver.py:333-336, y.expand)
//   exact-IK tiling : idx = active-pose list, n_mod = n_active (ikflow_solver.py:182-186, cond.repeat((R,1)))
struct PoseSource {
  const float* poses;
  const int* idx;
  long long n_mod;
  int stride;
  float softflow;
};

// pose row of global flow row `grow` (>= 0; n_mod >= 1).  One pose per row (grow < n_mod) and the single-pose broadcast (n_mod == 1) skip
// the 64-bit modulo.
IKF_HD long long pose_row(const PoseSource& ps, long long grow) {
  const long long pm = grow < ps.n_mod ? grow : (ps.n_mod == 1 ? 0 : grow % ps.n_mod);
  return ps.idx ? (long long)ps.idx[pm] : pm;
}

// ---- GLOWCouplingBlock (FrEIA): s_cl = clamp * 0.636 * atan(s);  forward y = exp(s_cl) x + t;  rev y = (x - t) exp(-s_cl) -------------------
IKF_HD float coupling_scale(float clamp, float s) { return clamp * (0.636f * atanf(s)); }
// the exponential factor and its use are separate steps: the wave-per-row kernels evaluate the factor in the lane that owns s and shuffle it
IKF_HD float coupling_fwd_factor(float s_cl) { return expf(s_cl); }
IKF_HD float coupling_inv_factor(float s_cl) { return expf(-s_cl); }
IKF_HD float coupling_fwd_apply(float x, float t, float e) { return e * x + t; }
IKF_HD float coupling_inv_apply(float x, float t, float e) { return (x - t) * e; }
// (written out, not composed: the factor evaluated after x - t keeps the planner's kernels instruction-identical)
IKF_HD float coupling_fwd(float x, float t, float s_cl) { return expf(s_cl) * x + t; }
IKF_HD float coupling_inv(float x, float t, float s_cl) { return (x - t) * expf(-s_cl); }
// an element's share of the log-determinant of the map that rewrote it
IKF_HD float coupling_fwd_ld(float s_cl) { return s_cl; }
IKF_HD float coupling_inv_ld(float s_cl) { return -s_cl; }

// ---- InvertibleSigmoidFlipped (ikflow/model.py:124-146) -------------------------------------------------------------------------------------
// rev: v = sigmoid(x); its log-det term log(v (1 - v)) = -|x| - 2 log1p(exp(-|x|)): no cancellation for large |x|
IKF_HD float sigmoid_rev(float x) { return 1.0f / (1.0f + expf(-x)); }
IKF_HD float sigmoid_rev_ld(float x) {
  const float ax = fabsf(x);
  return -ax - 2.0f * log1pf(expf(-ax));
}
// forward: the logit; its log-det term -log(v (1 - v))
IKF_HD float logit_fwd(float v) { return logf(v / (1.0f - v)); }
IKF_HD float logit_fwd_ld(float v) { return -(logf(v) + log1pf(-v)); }

// ---- FixedLinearTransform: forward v_j = sum_k x_k M[k][j] + b_j;  rev q_j = sum_k (x_k - b_k) M_inv[k][j] ----------------------------------
// one k step of a column of either direction (the loop over k stays with the caller: registers, LDS or wave shuffles feed it)
IKF_HD float linear_step(float x, float m, float acc) { return fmaf(x, m, acc); }
IKF_HD float linear_rev_in(float x, float b) { return x - b; }   // what the rev direction contracts
IKF_HD float linear_rev_step(float x, float b, float m, float acc) { return fmaf(x - b, m, acc); }

// clamp_to_joint_limits, joint j (hi[j] is read after the lower clamp, as the hand-written sites did)
IKF_HD float clamp_limit(float q, const float* lo, const float* hi, int j) { return fminf(fmaxf(q, lo[j]), hi[j]); }

}  // namespace ikf
