// The inverse pass WITH its log-determinant (ikf_flow_inverse) on the per-layer kernels: every shape the row-owner launch is not built for
// (TINY, widths other than 1024, other depths).  Per subnet: the first Linear (k_first_layer) and the hidden contractions (k_gemm_lrelu) of
// the plain inverse pass, then k_last_layer_coupling_inv below - the last Linear, the inverse affine coupling, the subnet's log-det share
// and, after subnet 2, the block's PermuteRandom reversed.  Blocks run N-1 .. 0, subnet 1 before subnet 2 (GLOWCouplingBlock rev).  The tail
// (k_inv_exit) applies the sigmoid of sigmoid_on_output graphs and FixedLinearTransform rev on all D columns.  Correct, not tuned.
//   log|det dx/dz| = - sum of every coupling's clamped s  (+ sum log(v (1 - v)), v = sigmoid(state), on sigmoid graphs)  + log|det M_inv|
// Per-element arithmetic: flow_math.h; the last-Linear prologue and the launcher's switch: last_linear_st / IKF_NOUT_DISPATCH (ikf_internal.h).
#include "ikf_internal.h"

namespace ikf {

// last Linear + inverse affine coupling: one wave per row, lane l owns k = 4 (64 g + l) .. +3 of the hidden row
//   which == 1 (runs first in a block): y2 = (x2 - t1) exp(-s1) on elements [L1, D), read from x_in;
//   which == 2: y1 = (x1 - t2) exp(-s2) on [0, L1), then out[d] = cat[perm_inv[d]];   ld[row] -= the subnet's sum of clamped s.
template <int OUT>
__global__ __launch_bounds__(256) void k_last_layer_coupling_inv(const float* __restrict__ w_last, const float* __restrict__ b_last,
                                                                 const float* __restrict__ h, FlowDims d, InvCouplingArgs ca, long long rows) {
  const int lane = threadIdx.x & 63;
  const long long wave0 = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
  const int width = d.width;
  const int D = d.D, L1 = d.L1;
  const int nl = ca.which == 1 ? d.L2 : L1;

  for (long long row = wave0; row < rows; row += nwaves) {
    float sv, tv;
    last_linear_st<OUT>(w_last, b_last, h, row, width, lane, nl, sv, tv);
    const float s_cl = lane < nl ? coupling_scale(d.clamp, sv) : 0.f;
    const float e = coupling_inv_factor(s_cl);
    const bool on = lane < D;
    const float* src_row = (ca.which == 1 ? ca.x_in : ca.state) + (size_t)row * D;
    const float xv = on ? src_row[lane] : 0.f;
    const int off = ca.which == 1 ? L1 : 0;   // first element this subnet rewrites
    const bool mine = lane >= off && lane < off + nl;
    const int src = mine ? lane - off : 0;
    const float t_j = __shfl(tv, src, 64), e_j = __shfl(e, src, 64);
    float out = mine ? coupling_inv_apply(xv, t_j, e_j) : xv;
    if (ca.which == 2) out = __shfl(out, on ? ca.perm_inv[lane] : 0, 64);   // PermuteRandom rev: out[d] = cat[perm_inv[d]]
    float ls = coupling_inv_ld(s_cl);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ls += __shfl_xor(ls, o, 64);
    if (on) ca.state[(size_t)row * D + lane] = out;
    if (lane == 0) ca.ld[row] = ca.first ? ls : ca.ld[row] + ls;
  }
}

hipError_t launch_last_layer_coupling_inv(const SubnetWeights& w, const FlowDims& d, const float* h_in, const InvCouplingArgs& ca,
                                          long long rows, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (d.width % 256 != 0) return hipErrorInvalidValue;
  IKF_NOUT_DISPATCH(w.n_out, hipLaunchKernelGGL((k_last_layer_coupling_inv<OUT>), dim3(last_layer_grid(rows)), dim3(256), 0, s, w.w_last,
                                               w.b_last, h_in, d, ca, rows))
  return hipGetLastError();
}

// one wave per row, lane j = output column j (D <= 16)
__global__ __launch_bounds__(256) void k_inv_exit(InvExitArgs a, long long rows) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;   // (uniform per wave)
  const int D = a.D;
  const bool on = lane < D;
  const int jc = on ? lane : 0;
  float v = on ? a.state[(size_t)row * D + lane] : 0.f;
  float ldt = 0.f;
  if (a.sigmoid) {   // InvertibleSigmoidFlipped rev: v = sigmoid(x); log-det term log(v (1 - v)) = -|x| - 2 log1p(exp(-|x|)) (no cancellation)
    ldt = on ? sigmoid_rev_ld(v) : 0.f;
    v = sigmoid_rev(v);
  }
  // FixedLinearTransform rev: (x - b).mm(M_inv), column jc
  const float xm = on ? linear_rev_in(v, a.b_lin[jc]) : 0.f;
  float q = 0.f;
  for (int k = 0; k < D; ++k) q = linear_step(__shfl(xm, k, 64), a.M_inv[k * D + jc], q);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) ldt += __shfl_xor(ldt, off, 64);
  if (on && a.x_out != nullptr) a.x_out[(size_t)row * D + lane] = q;
  if (lane < a.ndof && a.q_out != nullptr) {
    if (a.clamp_limits) q = clamp_limit(q, a.lo, a.hi, lane);
    a.q_out[(size_t)row * a.ndof + lane] = q;
  }
  if (lane == 0 && a.ld_out != nullptr) a.ld_out[row] = a.log_det0 + (a.ld[row] + ldt);
}

hipError_t launch_inv_exit(const InvExitArgs& a, long long rows, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  const unsigned grid = (unsigned)((rows + 3) / 4);
  hipLaunchKernelGGL(k_inv_exit, dim3(grid), dim3(256), 0, s, a, rows);
  return hipGetLastError();
}

}  // namespace ikf
