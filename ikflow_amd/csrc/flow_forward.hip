// The forward (training-direction) pass on the per-layer kernels: every shape the row-owner launch is not built for (TINY, widths other
// than 1024, other depths).  Per subnet: the first Linear (k_first_layer) and the hidden contractions (k_gemm_lrelu) of the inverse pass,
// then k_last_layer_coupling_fwd below - the last Linear, the forward affine coupling and the subnet's log-det share.  The head
// (k_fwd_entry) applies FixedLinearTransform forward (+ logit on sigmoid graphs) and PermuteRandom(0).  Correct, not tuned.
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
  for (int k = 0; k < D; ++k) v = fmaf(__shfl(xv, k, 64), a.M[k * D + jc], v);
  v += a.b_lin[jc];
  float ldt = 0.f;
  if (a.sigmoid) {   // InvertibleSigmoidFlipped forward: logit; log-det term -log(v (1 - v)) (ikflow/model.py:136-146)
    ldt = on ? -(logf(v) + log1pf(-v)) : 0.f;
    v = logf(v / (1.0f - v));
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
  const int width = d.width, G = width >> 8;
  const int D = d.D, L1 = d.L1;
  const int nl = ca.which == 1 ? d.L2 : L1;

  for (long long row = wave0; row < rows; row += nwaves) {
    float a[OUT];
#pragma unroll
    for (int j = 0; j < OUT; ++j) a[j] = 0.f;
    for (int g = 0; g < G; ++g) {
      const float4 hv = reinterpret_cast<const float4*>(h + (size_t)row * width)[g * 64 + lane];
#pragma unroll
      for (int j = 0; j < OUT; ++j) {
        const float4 w = reinterpret_cast<const float4*>(w_last + (size_t)j * width)[g * 64 + lane];
        float sacc = a[j];
        sacc = fmaf(hv.x, w.x, sacc);
        sacc = fmaf(hv.y, w.y, sacc);
        sacc = fmaf(hv.z, w.z, sacc);
        sacc = fmaf(hv.w, w.w, sacc);
        a[j] = sacc;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
      for (int j = 0; j < OUT; ++j) a[j] += __shfl_xor(a[j], off, 64);
    // lane j < nl takes (s_j, t_j) = (a[j], a[nl + j]) + bias
    float sv = 0.f, tv = 0.f;
#pragma unroll
    for (int j = 0; j < OUT; ++j) {
      const float aj = a[j] + b_last[j];
      if (j == lane) sv = aj;
      if (j == lane + nl) tv = aj;
    }
    const float s_cl = lane < nl ? d.clamp * (0.636f * atanf(sv)) : 0.f;
    const float e = expf(s_cl);
    const bool on = lane < D;
    const float xv = on ? ca.state[(size_t)row * D + lane] : 0.f;
    const int off = ca.which == 1 ? L1 : 0;   // first element this subnet rewrites
    const int src = (lane >= off && lane < off + nl) ? lane - off : 0;
    const float t_j = __shfl(tv, src, 64), e_j = __shfl(e, src, 64);
    float out = (lane >= off && lane < off + nl) ? e_j * xv + t_j : xv;
    if (ca.perm_next != nullptr) out = __shfl(out, on ? ca.perm_next[lane] : 0, 64);
    float ls = s_cl;
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

template <int OUT>
static hipError_t launch_last_fwd_g(const SubnetWeights& w, const FlowDims& d, const float* h_in, const FwdCouplingArgs& ca, long long rows,
                                    hipStream_t s) {
  long long waves = (rows + 3) / 4;
  if (waves < 1) waves = 1;
  const unsigned grid = (unsigned)((waves + 3) / 4);
  hipLaunchKernelGGL((k_last_layer_coupling_fwd<OUT>), dim3(grid), dim3(256), 0, s, w.w_last, w.b_last, h_in, d, ca, rows);
  return hipGetLastError();
}

hipError_t launch_last_layer_coupling_fwd(const SubnetWeights& w, const FlowDims& d, const float* h_in, const FwdCouplingArgs& ca,
                                          long long rows, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (d.width % 256 != 0) return hipErrorInvalidValue;
  switch (w.n_out) {
    case 2: return launch_last_fwd_g<2>(w, d, h_in, ca, rows, s);
    case 4: return launch_last_fwd_g<4>(w, d, h_in, ca, rows, s);
    case 6: return launch_last_fwd_g<6>(w, d, h_in, ca, rows, s);
    case 8: return launch_last_fwd_g<8>(w, d, h_in, ca, rows, s);
    case 10: return launch_last_fwd_g<10>(w, d, h_in, ca, rows, s);
    case 12: return launch_last_fwd_g<12>(w, d, h_in, ca, rows, s);
    case 14: return launch_last_fwd_g<14>(w, d, h_in, ca, rows, s);
    case 16: return launch_last_fwd_g<16>(w, d, h_in, ca, rows, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace ikf
