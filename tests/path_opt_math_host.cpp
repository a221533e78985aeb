// Test harness (CPU): the arithmetic of the path optimiser - ikflow_amd/csrc/path_opt_math.h, the very source the GPU runs - compiled with g++ and
// driven path by path, so that tests/test_path_opt_math_host.py can hold it against a dense fp64 solve without a GPU.  The loop below is
// k_path_opt's (path_opt_kernels.hip) on one thread: residual pass, forward, backward, update, the step's test.  Not part of the product.
#include <vector>

#include "../ikflow_amd/csrc/path_opt_math.h"

using ikf::Chain;

template <int N>
static double residual_pass(const Chain* ch, const float* wp, const float* qs, const float* Q, long long T, double w, double* W) {
  const int WPD = (int)ikf::path_opt_wp_doubles(N);
  for (long long t = 0; t < T; ++t) {
    const float* qv = Q + t * N;
    const float* pred = t > 0 ? Q + (t - 1) * N : qs;
    const float* next = t + 1 < T ? Q + (t + 1) * N : nullptr;
    double e[6], J[6][N], A[N][N], g[N];
    ikf::path_opt_residual<N>(ch, wp + t * 7, qv, e, J);
    ikf::path_opt_block<N>(e, J, qv, pred, next, w, A, g);
    double* o = W + t * WPD;
    for (int r = 0; r < N; ++r)
      for (int c = 0; c < N; ++c) o[r * N + c] = A[r][c];
    for (int j = 0; j < N; ++j) o[ikf::path_opt_off_y(N) + j] = g[j];
    o[ikf::path_opt_off_f(N)] = ikf::path_opt_term<N>(e, qv, pred, w);
  }
  return ikf::path_opt_objective(W + ikf::path_opt_off_f(N), WPD, T);
}

template <int N>
static int optimise(const Chain* ch, const float* wp, long long T, const float* q_in, const float* qs, double w, int n_iters, float* Q, double* F_out) {
  const int WPD = (int)ikf::path_opt_wp_doubles(N);
  std::vector<double> Wv((size_t)T * WPD);
  std::vector<float> prev((size_t)T * N);
  double* W = Wv.data();
  for (long long i = 0; i < T * N; ++i) Q[i] = q_in[i];
  double F = residual_pass<N>(ch, wp, qs, Q, T, w, W);
  F_out[0] = F;
  int iters = 0;
  for (int it = 0; it < n_iters; ++it) {
    for (long long t = 0; t < T; ++t) {
      double(*A)[N] = reinterpret_cast<double(*)[N]>(W + t * WPD);
      double* y = W + t * WPD + ikf::path_opt_off_y(N);
      const double(*Lp)[N] = t > 0 ? reinterpret_cast<const double(*)[N]>(W + (t - 1) * WPD) : nullptr;
      ikf::path_opt_forward<N>(Lp, t > 0 ? W + (t - 1) * WPD + ikf::path_opt_off_y(N) : nullptr, w, A, y);
    }
    for (long long t = T - 1; t >= 0; --t) {
      const double(*L)[N] = reinterpret_cast<const double(*)[N]>(W + t * WPD);
      ikf::path_opt_backward<N>(L, W + t * WPD + ikf::path_opt_off_y(N), t + 1 < T ? W + (t + 1) * WPD + ikf::path_opt_off_d(N) : nullptr, w,
                                W + t * WPD + ikf::path_opt_off_d(N));
    }
    for (long long t = 0; t < T; ++t) {
      for (int j = 0; j < N; ++j) prev[t * N + j] = Q[t * N + j];
      ikf::path_opt_update<N>(ch, W + t * WPD + ikf::path_opt_off_d(N), Q + t * N);
    }
    const double Fn = residual_pass<N>(ch, wp, qs, Q, T, w, W);
    F_out[it + 1] = Fn;
    if (!(Fn < F)) {
      for (long long i = 0; i < T * N; ++i) Q[i] = prev[i];
      break;
    }
    F = Fn;
    ++iters;
  }
  return iters;
}

#define PO_DISPATCH(nd, ...)                 \
  switch (nd) {                              \
    case 4: { constexpr int N = 4; __VA_ARGS__; } \
    case 5: { constexpr int N = 5; __VA_ARGS__; } \
    case 6: { constexpr int N = 6; __VA_ARGS__; } \
    case 7: { constexpr int N = 7; __VA_ARGS__; } \
    case 8: { constexpr int N = 8; __VA_ARGS__; } \
    default: break;                          \
  }

// the monotone loop on one path: q_out [T x ndof], F_out [n_iters + 1] (F of the input, then of every step tried; untouched behind the stop);
// returns the steps kept, -1: bad ndof
extern "C" int po_host_optimise(const void* chain, const float* wp, long long T, const float* q_in, const float* q_start, double w, int n_iters,
                                float* q_out, double* F_out) {
  const Chain* ch = static_cast<const Chain*>(chain);
  PO_DISPATCH(ch->ndof, return optimise<N>(ch, wp, T, q_in, q_start, w, n_iters, q_out, F_out));
  return -1;
}
// lm_step_row<NDOF, double> (kin_math.h) on n rows, in place
extern "C" int po_host_lm(const void* chain, const float* tgt, float* q, long long n) {
  const Chain* ch = static_cast<const Chain*>(chain);
  PO_DISPATCH(ch->ndof, for (long long i = 0; i < n; ++i) ikf::lm_step_row<N, double>(ch, tgt + i * 7, q + i * N); return 0);
  return -1;
}
// the evaluator's fold
extern "C" float po_host_cost(int ndof, const float* path, const float* q_start, const float* node, const uint64_t* edge_free, long long T,
                              float node_weight, float max_step, int* reason, int* where) {
  PO_DISPATCH(ndof, return ikf::path_opt_cost<N>(path, q_start, node, edge_free, T, node_weight, max_step, reason, where));
  return -1.f;
}
extern "C" long long po_host_wp_doubles(int ndof) { return ikf::path_opt_wp_doubles(ndof); }
extern "C" long long po_host_scratch_doubles(long long P, long long T, int ndof) { return ikf::path_opt_scratch_doubles(P, T, ndof); }
extern "C" int po_host_chain_bytes() { return (int)sizeof(Chain); }
