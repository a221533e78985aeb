// path_opt_math.h - the arithmetic of the path optimiser (path_opt_kernels.hip; the definition: include/ikflow_amd_path_opt.h): residual, Jacobian
// and normal block of one waypoint, the block Cholesky (Thomas) recurrence that couples the waypoints, the objective, the update, the evaluator's
// cost fold and the scratch sizes.  Like path_math.h and refine_math.h it holds nothing of the HIP runtime, so the same source compiles with g++:
// tests/test_path_opt_math_host.py runs it on the CPU against a dense fp64 solve built from the oracle.
//
// Rounding: the recurrence, the objective's sums and the cost fold are compiled without contraction (#pragma clang fp contract(off), as
// solve_lu_pivot and path_math.h), and every matrix entry is ONE sequential expression of this header: entry (r, c) of S_t is
// path_opt_schur(H[r][c], w, x_c[r]) with x_c = path_opt_inverse_column(L, c), whoever computes it.  The kernel spreads the columns c over the
// lanes of a wave, the host build walks them in a loop: the same numbers.  The chain walk and the quaternion are kin_math.h's, unchanged.
#pragma once
#include "path_batch_math.h"
#include "../../include/ikflow_amd_path_opt.h"

namespace ikf {

constexpr int IKF_PATH_OPT_BLOCK = 256;   // threads of the optimiser's workgroup (four waves)

// ---- one waypoint ---------------------------------------------------------------------------------------------------------------------------
// e and J of lm_step_row<NDOF, double> (kin_math.h), the same expressions in the same order
template <int NDOF>
IKF_HD void path_opt_residual(const Chain* __restrict__ ch, const float* __restrict__ tgt, const float* qv, double e[6], double J[6][NDOF]) {
  double qd[NDOF];
#pragma unroll
  for (int j = 0; j < NDOF; ++j) qd[j] = (double)qv[j];
  double R[9], p[3], axw[NDOF][3], orw[NDOF][3];
  fk_walk<double, NDOF, true>(ch, qd, R, p, axw, orw);
  double qc[4];
  mat_to_quat<double>(R, qc);
  const double w1 = tgt[3], x1 = tgt[4], y1 = tgt[5], z1 = tgt[6];
  const double w2 = qc[0], x2 = -qc[1], y2 = -qc[2], z2 = -qc[3];
  const double ew = w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2;
  const double ex = w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2;
  const double ey = w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2;
  const double ez = w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2;
  e[0] = atan2_t(2.0 * (ew * ex + ey * ez), 1.0 - 2.0 * (ex * ex + ey * ey));
  e[1] = asin_t(fmin(fmax(2.0 * (ew * ey - ez * ex), -1.0), 1.0));
  e[2] = atan2_t(2.0 * (ew * ez + ex * ey), 1.0 - 2.0 * (ey * ey + ez * ez));
  e[3] = (double)tgt[0] - p[0];
  e[4] = (double)tgt[1] - p[1];
  e[5] = (double)tgt[2] - p[2];
#pragma unroll
  for (int j = 0; j < NDOF; ++j) {
    if (ch->joints[j].kind == 1) {
      const double rx = p[0] - orw[j][0], ry = p[1] - orw[j][1], rz = p[2] - orw[j][2];
      J[0][j] = axw[j][0]; J[1][j] = axw[j][1]; J[2][j] = axw[j][2];
      J[3][j] = axw[j][1] * rz - axw[j][2] * ry;
      J[4][j] = axw[j][2] * rx - axw[j][0] * rz;
      J[5][j] = axw[j][0] * ry - axw[j][1] * rx;
    } else {
      J[0][j] = J[1][j] = J[2][j] = 0.0;
      J[3][j] = axw[j][0]; J[4][j] = axw[j][1]; J[5][j] = axw[j][2];
    }
  }
}

// H_tt = J^T J + (lambda + w deg) I (both triangles) and g_t = J^T e + w ((pred - q) + (next - q)); pred / next null where the path has no such
// neighbour (pred of waypoint 0: q_start).  deg = neighbours.  With w = 0: A and g of lm_step_row<NDOF, double>.
template <int NDOF>
IKF_HD void path_opt_block(const double e[6], const double J[6][NDOF], const float* qv, const float* pred, const float* next, double w,
                           double A[NDOF][NDOF], double g[NDOF]) {
  const double deg = (pred ? 1.0 : 0.0) + (next ? 1.0 : 0.0);
#pragma unroll
  for (int a = 0; a < NDOF; ++a) {
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      double sacc = 0.0;
#pragma unroll
      for (int r = 0; r < 6; ++r) sacc += J[r][a] * J[r][b];
      A[a][b] = a == b ? (sacc + 1e-4) + w * deg : sacc;
      A[b][a] = A[a][b];
    }
    double gs = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) gs += J[r][a] * e[r];
    double sm = 0.0;
    if (pred) sm += (double)pred[a] - (double)qv[a];
    if (next) sm += (double)next[a] - (double)qv[a];
    g[a] = gs + w * sm;
  }
}

// f_t = |e_t|^2 + w |q_t - pred|^2: the pose term over its six entries in order, then the difference term over the joints in order
template <int NDOF>
IKF_HD double path_opt_term(const double e[6], const float* qv, const float* pred, double w) {
#pragma clang fp contract(off)
  double pose = 0.0;
#pragma unroll
  for (int r = 0; r < 6; ++r) pose = pose + e[r] * e[r];
  if (!pred) return pose;
  double ds = 0.0;
#pragma unroll
  for (int j = 0; j < NDOF; ++j) {
    const double d = (double)qv[j] - (double)pred[j];
    ds = ds + d * d;
  }
  return pose + w * ds;
}
// F = ((f_0 + f_1) + f_2) + ...
IKF_HD double path_opt_objective(const double* f, long long stride, long long T) {
#pragma clang fp contract(off)
  double F = 0.0;
  for (long long t = 0; t < T; ++t) F = F + f[t * stride];
  return F;
}

// ---- the recurrence --------------------------------------------------------------------------------------------------------------------------
// A = L L^T in place (lower triangle), the order of solve_cholesky's factorisation
template <int NDOF>
IKF_HD void path_opt_factor(double A[NDOF][NDOF]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int c = 0; c < NDOF; ++c) {
    double dsum = A[c][c];
#pragma unroll
    for (int k = 0; k < c; ++k) dsum -= A[c][k] * A[c][k];
    const double lcc = sqrt(dsum);
    A[c][c] = lcc;
    const double inv = 1.0 / lcc;
#pragma unroll
    for (int r = c + 1; r < NDOF; ++r) {
      double v = A[r][c];
#pragma unroll
      for (int k = 0; k < c; ++k) v -= A[r][k] * A[c][k];
      A[r][c] = v * inv;
    }
  }
}
// g <- (L L^T)^-1 g: solve_cholesky's two triangular solves
template <int NDOF>
IKF_HD void path_opt_subst(const double L[NDOF][NDOF], double g[NDOF]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int r = 0; r < NDOF; ++r) {
    double v = g[r];
#pragma unroll
    for (int k = 0; k < r; ++k) v -= L[r][k] * g[k];
    g[r] = v / L[r][r];
  }
#pragma unroll
  for (int r = NDOF - 1; r >= 0; --r) {
    double v = g[r];
#pragma unroll
    for (int k = r + 1; k < NDOF; ++k) v -= L[k][r] * g[k];
    g[r] = v / L[r][r];
  }
}
// column c of (L L^T)^-1 (c is a run-time value: a select, no indexed register)
template <int NDOF>
IKF_HD void path_opt_inverse_column(const double L[NDOF][NDOF], int c, double x[NDOF]) {
#pragma unroll
  for (int r = 0; r < NDOF; ++r) x[r] = r == c ? 1.0 : 0.0;
  path_opt_subst<NDOF>(L, x);
}
// entry (r, c) of S_t = H_tt - w^2 S_{t-1}^-1, from entry r of column c of the inverse
IKF_HD double path_opt_schur(double h, double w, double x) {
#pragma clang fp contract(off)
  return h - (w * w) * x;
}
// entry j of y_t = g_t + w z (z = S_{t-1}^-1 y_{t-1}), and of the backward right-hand side y_t + w d_{t+1}
IKF_HD double path_opt_carry(double g, double w, double z) {
#pragma clang fp contract(off)
  return g + w * z;
}

// One forward step on one thread: Lp the factor of S_{t-1} and yp = y_{t-1} (null for t = 0); A holds H_tt and leaves as the factor of S_t
// (lower triangle), y holds g_t and leaves as y_t.  The kernel computes the same entries with the columns c across a wave's lanes.
template <int NDOF>
IKF_HD void path_opt_forward(const double (*Lp)[NDOF], const double* yp, double w, double A[NDOF][NDOF], double y[NDOF]) {
  if (Lp) {
    for (int c = 0; c < NDOF; ++c) {
      double x[NDOF];
      path_opt_inverse_column<NDOF>(Lp, c, x);
      for (int r = c; r < NDOF; ++r) A[r][c] = path_opt_schur(A[r][c], w, x[r]);
    }
    double z[NDOF];
    for (int j = 0; j < NDOF; ++j) z[j] = yp[j];
    path_opt_subst<NDOF>(Lp, z);
    for (int j = 0; j < NDOF; ++j) y[j] = path_opt_carry(y[j], w, z[j]);
  }
  path_opt_factor<NDOF>(A);
}
// One backward step: d_t = S_t^-1 (y_t + w d_{t+1}) (dn null for t = T - 1); d leaves as d_t
template <int NDOF>
IKF_HD void path_opt_backward(const double L[NDOF][NDOF], const double y[NDOF], const double* dn, double w, double d[NDOF]) {
#pragma unroll
  for (int j = 0; j < NDOF; ++j) d[j] = dn ? path_opt_carry(y[j], w, dn[j]) : y[j];
  path_opt_subst<NDOF>(L, d);
}

// q_t <- clamp(f32(q_t + d_t), lo, hi); a NaN stays a NaN (it ends the loop: F of the new iterate is then not below the old one)
template <int NDOF>
IKF_HD void path_opt_update(const Chain* __restrict__ ch, const double d[NDOF], float qv[NDOF]) {
#pragma unroll
  for (int j = 0; j < NDOF; ++j) {
    const float qn = (float)((double)qv[j] + d[j]);
    qv[j] = qn < ch->lo[j] ? ch->lo[j] : (qn > ch->hi[j] ? ch->hi[j] : qn);
  }
}

// ---- the evaluator's cost fold: the lattice's recurrence (path_math.h) with one row and one predecessor per waypoint ----------------------------
// path [T][NDOF], node [T] (the k = 1 row scores), edge_free [T] words of the k = 1 lattice mask (bit 0 of word t: the edge that ends at waypoint
// t, for t = 0 the start edge) or null: no sweep.  Returns the cost; *reason 0 / IKF_PATH_OPT_NODE / IKF_PATH_OPT_EDGE and *where as the header says.
template <int NDOF>
IKF_HD float path_opt_cost(const float* path, const float* q_start, const float* node, const uint64_t* edge_free, long long T,
                           float node_weight, float max_step, int* reason, int* where) {
  float cost = 0.f;
  for (long long t = 0; t < T; ++t) {
    const float* row = path + t * NDOF;
    if (!(node[t] < rank_inf())) { *reason = IKF_PATH_OPT_NODE; *where = (int)t; return rank_inf(); }
    PathBest best = path_none();
    const bool swept_free = !edge_free || (edge_free[t] & 1ULL) != 0ULL;
    if (t == 0) {
      if (!q_start || swept_free) best = path_start<NDOF>(q_start, q_start != nullptr, row, max_step);
    } else if (swept_free) {
      path_relax<NDOF>(best, cost, row - NDOF, 0, row, max_step);
    }
    if (!(best.c < rank_inf())) { *reason = IKF_PATH_OPT_EDGE; *where = (int)t; return rank_inf(); }
    cost = path_finish(best, node[t], node_weight);
    if (!(cost < rank_inf())) { *reason = IKF_PATH_OPT_NODE; *where = (int)t; return rank_inf(); }
  }
  *reason = IKF_PATH_OPT_COMMITTED;
  *where = -1;
  return cost;
}

// ---- scratch, pure integer arithmetic ------------------------------------------------------------------------------------------------------------
// doubles per waypoint: the block H_tt / the factor of S_t [ndof][ndof], g_t / y_t [ndof], d_t [ndof], f_t
IKF_PATH_HOST_DEVICE long long path_opt_wp_doubles(int ndof) { return (long long)ndof * ndof + 2 * ndof + 1; }
IKF_PATH_HOST_DEVICE int path_opt_off_y(int ndof) { return ndof * ndof; }
IKF_PATH_HOST_DEVICE int path_opt_off_d(int ndof) { return ndof * ndof + ndof; }
IKF_PATH_HOST_DEVICE int path_opt_off_f(int ndof) { return ndof * ndof + 2 * ndof; }
IKF_PATH_HOST_DEVICE long long path_opt_scratch_doubles(long long P, long long T, int ndof) { return P * T * path_opt_wp_doubles(ndof); }
// floats: the iterate and the previous iterate, [P * T][ndof] each
IKF_PATH_HOST_DEVICE long long path_opt_iterate_floats(long long P, long long T, int ndof) { return P * T * ndof; }

}  // namespace ikf
