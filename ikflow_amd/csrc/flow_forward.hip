// The forward (training-direction) pass on the per-layer kernels: every shape the row-owner launch is not built for (TINY, widths other
// than 1024, other depths).  Per subnet: the first Linear (k_first_layer) and the hidden contractions (k_gemm_lrelu) of the inverse pass,
// then k_last_layer_coupling_fwd below - the last Linear, the forward affine coupling and the subnet's log-det share.  The head
// (k_fwd_entry) applies FixedLinearTransform forward (+ logit on sigmoid graphs) and PermuteRandom(0).  Correct, not tuned.
// Per-element arithmetic: flow_math.h; the last-Linear prologue and the launcher's switch: last_linear_st / IKF_NOUT_DISPATCH (ikf_internal.h).
#include "ikf_internal.h"

namespace ikf {

// one wave per row, lane d = state element d (D <= 16)
__global__ __launch_bounds__(256) void k_fwd_entry(FwdEntryArgs a, long long rows) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;   // (uniform per wave)
  const int D = a.D;
  const bool on = lane < D;
  const int jc = on ? lane : 0;
  const float xv = on ? a.x[(size_t)row * D + lane] : 0.f;
  // v = x.mm(M) + b, element jc
  float v = 0.f;
  for (int k = 0; k < D; ++k) v = linear_step(__shfl(xv, k, 64), a.M[k * D + jc], v);
  v += a.b_lin[jc];
  float ldt = 0.f;
  if (a.sigmoid) {   // InvertibleSigmoidFlipped forward: logit; log-det term -log(v (1 - v)) (ikflow/model.py:136-146)
    ldt = on ? logit_fwd_ld(v) : 0.f;
    v = logit_fwd(v);
  }
  // PermuteRandom(0) forward: out[d] = v[perm0[d]]
  const float out = __shfl(v, on ? a.perm0[lane] : 0, 64);
  if (on) a.state[(size_t)row * D + lane] = out;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) ldt += __shfl_xor(ldt, off, 64);
  if (lane == 0) a.ld[row] = a.log_det0 + ldt;
}

hipError_t launch_fwd_entry(const FwdEntryArgs& a, long long rows, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  const unsigned grid = (unsigned)((rows + 3) / 4);
  hipLaunchKernelGGL(k_fwd_entry, dim3(grid), dim3(256), 0, s, a, rows);
  return hipGetLastError();
}

// last Linear + forward affine coupling (GLOWCouplingBlock forward): one wave per row, lane l owns k = 4 (64 g + l) .. +3 of the hidden row
//   which == 2 (runs first in a block): y1 = exp(s2) x1 + t2 on elements [0, L1);   which == 1: y2 = exp(s1) x2 + t1 on [L1, D)
// then (which == 1, perm_next != null) PermuteRandom forward of the next block; the subnet's sum of clamped s goes to ld[row].
template <int OUT>
__global__ __launch_bounds__(256) void k_last_layer_coupling_fwd(const float* __restrict__ w_last, const float* __restrict__ b_last,
                                                                 const float* __restrict__ h, FlowDims d, FwdCouplingArgs ca, long long rows) {
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
    const float e = coupling_fwd_factor(s_cl);
    const bool on = lane < D;
    const float xv = on ? ca.state[(size_t)row * D + lane] : 0.f;
    const int off = ca.which == 1 ? L1 : 0;   // first element this subnet rewrites
    const int src = (lane >= off && lane < off + nl) ? lane - off : 0;
    const float t_j = __shfl(tv, src, 64), e_j = __shfl(e, src, 64);
    float out = (lane >= off && lane < off + nl) ? coupling_fwd_apply(xv, t_j, e_j) : xv;
    if (ca.perm_next != nullptr) out = __shfl(out, on ? ca.perm_next[lane] : 0, 64);
    float ls = coupling_fwd_ld(s_cl);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ls += __shfl_xor(ls, o, 64);
    const float ld = ca.ld[row] + ls;
    if (on) ca.state[(size_t)row * D + lane] = out;
    if (lane == 0) ca.ld[row] = ld;
    if (ca.is_final) {
      if (ca.z_out != nullptr && on) ca.z_out[(size_t)row * D + lane] = out;
      if (ca.ld_out != nullptr && lane == 0) ca.ld_out[row] = ld;
    }
  }
}

hipError_t launch_last_layer_coupling_fwd(const SubnetWeights& w, const FlowDims& d, const float* h_in, const FwdCouplingArgs& ca,
                                          long long rows, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (d.width % 256 != 0) return hipErrorInvalidValue;
  IKF_NOUT_DISPATCH(w.n_out, hipLaunchKernelGGL((k_last_layer_coupling_fwd<OUT>), dim3(last_layer_grid(rows)), dim3(256), 0, s, w.w_last,
                                               w.b_last, h_in, d, ca, rows))
  return hipGetLastError();
}

}  // namespace ikf
