// Test harness (CPU): the per-element arithmetic of the flow kernels - ikflow_amd/csrc/flow_math.h, the very source the GPU runs - compiled with
// g++ and driven element by element, so that tests/test_flow_math_host.py can hold it against fp64 and the oracle without a GPU.  Not part of
// the product.
#include "../ikflow_amd/csrc/flow_math.h"

// pose row of every flow row in rows[0 .. n)
extern "C" void flow_math_pose_rows(const int* idx, long long n_mod, const long long* rows, long long n, long long* out) {
  const ikf::PoseSource ps{nullptr, idx, n_mod, 7, 0.f};
  for (long long i = 0; i < n; ++i) out[i] = ikf::pose_row(ps, rows[i]);
}

// one scalar step on every element.  a, b, c: the step's operands (those it does not take are ignored)
extern "C" int flow_math_step(int what, const float* a, const float* b, const float* c, long long n, float* out) {
  for (long long i = 0; i < n; ++i) {
    switch (what) {
      case 0: out[i] = ikf::coupling_scale(a[i], b[i]); break;                 // (clamp, s)
      case 1: out[i] = ikf::coupling_inv(a[i], b[i], c[i]); break;             // (x, t, s_cl)
      case 2: out[i] = ikf::coupling_fwd(a[i], b[i], c[i]); break;
      case 3: out[i] = ikf::coupling_inv_apply(a[i], b[i], ikf::coupling_inv_factor(c[i])); break;   // the wave kernels' two-step spelling
      case 4: out[i] = ikf::coupling_fwd_apply(a[i], b[i], ikf::coupling_fwd_factor(c[i])); break;
      case 5: out[i] = ikf::coupling_fwd(ikf::coupling_inv(a[i], b[i], c[i]), b[i], c[i]); break;    // round trip
      case 6: out[i] = ikf::coupling_fwd_ld(c[i]) + ikf::coupling_inv_ld(c[i]); break;
      case 7: out[i] = ikf::sigmoid_rev(a[i]); break;
      case 8: out[i] = ikf::sigmoid_rev_ld(a[i]); break;
      case 9: out[i] = ikf::logit_fwd(a[i]); break;
      case 10: out[i] = ikf::logit_fwd_ld(a[i]); break;
      default: return 1;
    }
  }
  return 0;
}

// the exit transform of the inverse pass, composed from the header as k_inv_exit composes it: sigmoid (+ its log-det term), (x - b).mm(M_inv) on
// all D columns -> x_out, [:, :ndof] (+ limit clamp) -> q_out, log_det0 + (ld_in + the row's sigmoid terms) -> ld_out
extern "C" void flow_math_exit(const float* state, const float* ld_in, long long n, int D, int ndof, int sigmoid, int clamp_limits, const float* M_inv,
                               const float* b_lin, const float* lo, const float* hi, float log_det0, float* x_out, float* q_out, float* ld_out) {
  for (long long r = 0; r < n; ++r) {
    float xm[16], ldt = 0.f;
    for (int k = 0; k < D; ++k) {
      float v = state[r * D + k];
      if (sigmoid) {
        ldt += ikf::sigmoid_rev_ld(v);
        v = ikf::sigmoid_rev(v);
      }
      xm[k] = ikf::linear_rev_in(v, b_lin[k]);
    }
    for (int j = 0; j < D; ++j) {
      float q = 0.f;
      for (int k = 0; k < D; ++k) q = ikf::linear_step(xm[k], M_inv[k * D + j], q);
      x_out[r * D + j] = q;
      if (j < ndof) q_out[r * ndof + j] = clamp_limits ? ikf::clamp_limit(q, lo, hi, j) : q;
    }
    ld_out[r] = log_det0 + (ld_in[r] + ldt);
  }
}
