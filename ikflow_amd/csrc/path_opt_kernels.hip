// Path optimiser for gfx950 (include/ikflow_amd_path_opt.h): a damped least-squares pass over whole joint-space paths, the waypoints coupled by
// the smoothness term.  The arithmetic is path_opt_math.h; these kernels only place it.
//
// k_path_opt<NDOF>: ONE workgroup of 256 threads per path, all n_iters steps inside ONE launch, no workgroup reads what another writes, no atomics.
//   residual pass  thread t, t + 256, ...: chain walk, e_t, J_t, the block H_tt, g_t and f_t of waypoint t in fp64 (path_opt_residual / _block /
//                  _term) into the path's scratch; thread 0 then sums F over t ascending.
//   recurrence     wave 0 alone, sequential in t.  Every lane holds the factor of S_{t-1} (wave-uniform registers); lane c < NDOF solves for column c
//                  of S_{t-1}^-1 (path_opt_inverse_column), the lower triangle of S_t = H_tt - w^2 S_{t-1}^-1 is gathered entry by entry with
//                  __shfl from the lane that owns the column, and every lane factors S_t.  Lane 0 stores the factor and y_t over H_tt and g_t.
//                  Backward: d_t = S_t^-1 (y_t + w d_{t+1}), wave-uniform, lane 0 stores d_t.  A barrier separates forward from backward and the
//                  recurrence from the phases around it: what wave 0 reads back was stored before a barrier.
//   update         thread t, t + 256, ...: the previous iterate is saved, q_t <- clamp(f32(q_t + d_t)).
//   The next residual pass is the step's test: F_new < F_old keeps it, anything else restores the previous iterate and ends the loop.
// Per-path scratch is global memory of the handle (path_opt_wp_doubles(ndof) doubles per waypoint, the iterate and the previous iterate): T is
// not bounded by LDS.  LDS: two words.
// k_path_opt_commit<NDOF>: a workgroup per path.  Thread 0 folds the k = 1 node scores, the step gate and the sweep's words into the evaluator's
// cost (path_opt_cost) for the optimised path and - validate - the input path and applies the commit rule; all threads then copy the chosen rows.
// Without an optimised path it is the evaluator as a query (ikf_path_cost).
#include "ikf_internal.h"
#include "path_opt_math.h"

namespace ikf {

template <int NDOF>
__device__ __forceinline__ void path_opt_residual_pass(const PathOptArgs& a, const float* __restrict__ wp, const float* qs, const float* Q, double* W,
                                                       long long T, double w) {
  const int WPD = (int)path_opt_wp_doubles(NDOF);
  for (long long t = threadIdx.x; t < T; t += IKF_PATH_OPT_BLOCK) {
    float qv[NDOF];
    load_q<NDOF>(Q, t, qv);
    const float* pred = t > 0 ? Q + (t - 1) * NDOF : qs;
    const float* next = t + 1 < T ? Q + (t + 1) * NDOF : nullptr;
    double e[6], J[6][NDOF], A[NDOF][NDOF], g[NDOF];
    path_opt_residual<NDOF>(a.ch, wp + t * 7, qv, e, J);
    path_opt_block<NDOF>(e, J, qv, pred, next, w, A, g);
    double* const o = W + t * WPD;
#pragma unroll
    for (int r = 0; r < NDOF; ++r)
#pragma unroll
      for (int c = 0; c < NDOF; ++c) o[r * NDOF + c] = A[r][c];
#pragma unroll
    for (int j = 0; j < NDOF; ++j) o[path_opt_off_y(NDOF) + j] = g[j];
    o[path_opt_off_f(NDOF)] = path_opt_term<NDOF>(e, qv, pred, w);
  }
}

template <int NDOF>
__device__ __forceinline__ void path_opt_load_block(const double* o, double A[NDOF][NDOF], double y[NDOF]) {
#pragma unroll
  for (int r = 0; r < NDOF; ++r)
#pragma unroll
    for (int c = 0; c < NDOF; ++c) A[r][c] = o[r * NDOF + c];
#pragma unroll
  for (int j = 0; j < NDOF; ++j) y[j] = o[path_opt_off_y(NDOF) + j];
}

template <int NDOF>
__global__ __launch_bounds__(IKF_PATH_OPT_BLOCK) void k_path_opt(const PathOptArgs a) {
  const int WPD = (int)path_opt_wp_doubles(NDOF);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long p = blockIdx.x, T = a.T, base = p * T;
  const float* const wp = a.waypoints + base * 7;
  const float* const in = a.path_in + base * NDOF;
  const float* const qs = a.q_start ? a.q_start + p * NDOF : nullptr;
  float* const Q = a.q + base * NDOF;
  float* const Qp = a.q_prev + base * NDOF;
  double* const W = a.work + base * WPD;
  const double w = a.w;
  __shared__ double s_F;
  __shared__ int s_keep;

  for (long long i = tid; i < T * NDOF; i += IKF_PATH_OPT_BLOCK) Q[i] = in[i];
  if (a.skip_cost && !(a.skip_cost[p] < rank_inf())) {   // a lattice's "no path": nothing to optimise (block-uniform)
    if (tid == 0) a.iters_out[p] = 0;
    return;
  }
  __syncthreads();
  path_opt_residual_pass<NDOF>(a, wp, qs, Q, W, T, w);
  __syncthreads();
  if (tid == 0) s_F = path_opt_objective(W + path_opt_off_f(NDOF), WPD, T);
  int iters = 0;
  for (int it = 0; it < a.n_iters; ++it) {
    // ---- forward: wave 0, lane c = column c of the inverse ----
    double L[NDOF][NDOF], y[NDOF];
    if (wave == 0) {
      const int c = lane < NDOF ? lane : NDOF - 1;
      for (long long t = 0; t < T; ++t) {
        double A[NDOF][NDOF], g[NDOF];
        path_opt_load_block<NDOF>(W + t * WPD, A, g);
        if (t > 0) {
          double x[NDOF];
          path_opt_inverse_column<NDOF>(L, c, x);
#pragma unroll
          for (int cc = 0; cc < NDOF; ++cc)
#pragma unroll
            for (int r = cc; r < NDOF; ++r) A[r][cc] = path_opt_schur(A[r][cc], w, __shfl(x[r], cc));
          double z[NDOF];
#pragma unroll
          for (int j = 0; j < NDOF; ++j) z[j] = y[j];
          path_opt_subst<NDOF>(L, z);
#pragma unroll
          for (int j = 0; j < NDOF; ++j) g[j] = path_opt_carry(g[j], w, z[j]);
        }
        path_opt_factor<NDOF>(A);
#pragma unroll
        for (int r = 0; r < NDOF; ++r)
#pragma unroll
          for (int cc = 0; cc < NDOF; ++cc) L[r][cc] = A[r][cc];
#pragma unroll
        for (int j = 0; j < NDOF; ++j) y[j] = g[j];
        if (lane == 0) {
          double* const o = W + t * WPD;
#pragma unroll
          for (int r = 0; r < NDOF; ++r)
#pragma unroll
            for (int cc = 0; cc <= r; ++cc) o[r * NDOF + cc] = L[r][cc];
#pragma unroll
          for (int j = 0; j < NDOF; ++j) o[path_opt_off_y(NDOF) + j] = y[j];
        }
      }
    }
    __syncthreads();
    // ---- backward: wave 0, wave-uniform ----
    if (wave == 0) {
      double dn[NDOF];
      for (long long t = T - 1; t >= 0; --t) {
        if (t < T - 1) path_opt_load_block<NDOF>(W + t * WPD, L, y);   // (t = T - 1: still in registers)
        double d[NDOF];
        path_opt_backward<NDOF>(L, y, t < T - 1 ? dn : nullptr, w, d);
#pragma unroll
        for (int j = 0; j < NDOF; ++j) dn[j] = d[j];
        if (lane == 0) {
#pragma unroll
          for (int j = 0; j < NDOF; ++j) W[t * WPD + path_opt_off_d(NDOF) + j] = d[j];
        }
      }
    }
    __syncthreads();
    // ---- update ----
    for (long long t = tid; t < T; t += IKF_PATH_OPT_BLOCK) {
      float qv[NDOF];
      load_q<NDOF>(Q, t, qv);
      double d[NDOF];
#pragma unroll
      for (int j = 0; j < NDOF; ++j) {
        d[j] = W[t * WPD + path_opt_off_d(NDOF) + j];
        Qp[t * NDOF + j] = qv[j];
      }
      path_opt_update<NDOF>(a.ch, d, qv);
#pragma unroll
      for (int j = 0; j < NDOF; ++j) Q[t * NDOF + j] = qv[j];
    }
    __syncthreads();
    // ---- the step's test: the next step's residual pass ----
    path_opt_residual_pass<NDOF>(a, wp, qs, Q, W, T, w);
    __syncthreads();
    if (tid == 0) {
      const double Fn = path_opt_objective(W + path_opt_off_f(NDOF), WPD, T);
      const bool keep = Fn < s_F;
      if (keep) s_F = Fn;
      s_keep = keep ? 1 : 0;
    }
    __syncthreads();
    if (!s_keep) {
      for (long long i = tid; i < T * NDOF; i += IKF_PATH_OPT_BLOCK) Q[i] = Qp[i];
      break;
    }
    ++iters;
  }
  if (tid == 0) a.iters_out[p] = iters;
}

template <int NDOF>
__global__ __launch_bounds__(IKF_PATH_OPT_BLOCK) void k_path_opt_commit(const PathOptCommitArgs a) {
  const int tid = threadIdx.x;
  const long long p = blockIdx.x, T = a.T, base = p * T;
  const float* const in = a.path_in + base * NDOF;
  const float* const optp = a.path_opt ? a.path_opt + base * NDOF : nullptr;
  __shared__ int s_take;
  if (tid == 0) {
    const float* const qs = a.q_start ? a.q_start + p * NDOF : nullptr;
    const float nw = a.node_weight, step = a.max_joint_step;
    int info[4] = {0, 0, IKF_PATH_OPT_NO_DESCENT, -1};
    float cost = rank_inf();
    int take = 0;
    if (!optp) {   // the evaluator as a query
      cost = path_opt_cost<NDOF>(in, qs, a.node_in + base, a.edge_in ? a.edge_in + base : nullptr, T, nw, step, &info[2], &info[3]);
      info[1] = info[2] == IKF_PATH_OPT_COMMITTED ? 1 : 0;
    } else if (!(a.skip_cost && !(a.skip_cost[p] < rank_inf()))) {
      int r_opt, w_opt;
      const float c_opt = path_opt_cost<NDOF>(optp, qs, a.node_opt + base, a.edge_opt ? a.edge_opt + base : nullptr, T, nw, step, &r_opt, &w_opt);
      info[0] = a.iters[p];
      if (!a.validate) {
        take = 1;
        cost = c_opt;
        info[2] = r_opt;
        info[3] = w_opt;
      } else {
        int r_in, w_in;
        const float c_in = path_opt_cost<NDOF>(in, qs, a.node_in + base, a.edge_in ? a.edge_in + base : nullptr, T, nw, step, &r_in, &w_in);
        if (info[0] == 0) { info[2] = IKF_PATH_OPT_NO_DESCENT; }
        else if (r_opt != IKF_PATH_OPT_COMMITTED) { info[2] = r_opt; info[3] = w_opt; }
        else if (!(c_opt < c_in)) { info[2] = IKF_PATH_OPT_COST; }
        else { info[2] = IKF_PATH_OPT_COMMITTED; }
        take = info[2] == IKF_PATH_OPT_COMMITTED ? 1 : 0;
        cost = take ? c_opt : c_in;
      }
      info[1] = take;
    }
    a.cost_out[p] = cost;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a.info_keep[p * 4 + i] = info[i];
      if (a.info_out) a.info_out[p * 4 + i] = info[i];
    }
    s_take = take;
  }
  __syncthreads();
  if (!a.path_out) return;
  const float* const src = s_take ? optp : in;
  float* const out = a.path_out + base * NDOF;
  for (long long i = tid; i < T * NDOF; i += IKF_PATH_OPT_BLOCK) out[i] = src[i];
}

static bool path_opt_shape_ok(int P, int T) { return P >= 1 && T >= 1 && (long long)P * T <= 0x7fffffffLL; }

hipError_t launch_path_opt(int ndof, const PathOptArgs& a, hipStream_t s) {
  if (!path_opt_shape_ok(a.P, a.T) || a.n_iters < 1 || a.n_iters > IKF_PATH_OPT_MAX_ITERS || !(a.w >= 0.0) || !a.ch || !a.waypoints || !a.path_in ||
      !a.q || !a.q_prev || !a.work || !a.iters_out)
    return hipErrorInvalidValue;
  IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_path_opt<ND>), dim3((unsigned)a.P), dim3(IKF_PATH_OPT_BLOCK), 0, s, a); return hipGetLastError());
  return hipErrorInvalidValue;
}

hipError_t launch_path_opt_commit(int ndof, const PathOptCommitArgs& a, hipStream_t s) {
  if (!path_opt_shape_ok(a.P, a.T) || !a.path_in || !a.cost_out || !a.info_keep) return hipErrorInvalidValue;
  if (a.path_opt ? (!a.node_opt || !a.iters || !a.path_out || (a.validate && !a.node_in)) : !a.node_in) return hipErrorInvalidValue;
  IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_path_opt_commit<ND>), dim3((unsigned)a.P), dim3(IKF_PATH_OPT_BLOCK), 0, s, a); return hipGetLastError());
  return hipErrorInvalidValue;
}

}  // namespace ikf
