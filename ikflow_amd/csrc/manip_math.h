// manip_math.h - the arithmetic of the singularity rule (manip_kernels.hip): Yoshikawa's manipulability measure of one configuration, from the fp64
// geometric Jacobian of lm_step_row (kin_math.h).  Like cloud_math.h and path_math.h it holds nothing of the HIP runtime, so the same source
// compiles with g++: tests/test_manip_math_host.py runs it on the CPU against an fp64 singular-value reference.  Definitions:
// include/ikflow_amd_manip.h.
//
//   J        6 x NDOF, rows 0-2 angular, rows 3-5 linear; a revolute joint gives [axis; axis x (p_ee - origin)], a prismatic one [0; axis]
//   part     FULL: all 6 rows; LINEAR: rows 3-5; ANGULAR: rows 0-2 - r rows
//   G        the p x p Gram matrix, p = min(r, NDOF): J J^T when NDOF >= r, else J^T J
//   w        the product of the pivots of an undamped fp64 Cholesky factorisation of G = sqrt(det G) = the product of the p singular values
// A pivot <= 0 ends the factorisation with w = 0 (a rank-deficient Jacobian: exactly singular).  A NaN joint gives w = NaN whatever the part: the
// arithmetic alone would not carry it everywhere (the angular rows do not depend on a sliding joint, nor on the last joint), so it is tested.
// A row is BELOW a floor f exactly when !(w >= f): a NaN row is below every floor.
//
// Registers: with NDOF >= r the Gram matrix is accumulated column by column - J is never held, only one column of it beside the recorded axes and
// origins and the lower triangle of G (21 doubles); with NDOF < r (4 or 5 joints, FULL) J is 6 x 5 at the most.
#pragma once
#include "kin_math.h"
#include "../../include/ikflow_amd_manip.h"

namespace ikf {

// column j of the geometric Jacobian, from the walk's records and the tool point
template <typename T>
IKF_HD void jacobian_column(int kind, const T ax[3], const T org[3], const T p[3], T col[6]) {
  if (kind == 1) {
    const T rx = p[0] - org[0], ry = p[1] - org[1], rz = p[2] - org[2];
    col[0] = ax[0]; col[1] = ax[1]; col[2] = ax[2];
    col[3] = ax[1] * rz - ax[2] * ry;
    col[4] = ax[2] * rx - ax[0] * rz;
    col[5] = ax[0] * ry - ax[1] * rx;
  } else {
    col[0] = col[1] = col[2] = (T)0;
    col[3] = ax[0]; col[4] = ax[1]; col[5] = ax[2];
  }
}

// product of the pivots of G = L L^T (lower triangle filled, overwritten); 0 from the first pivot <= 0 on
template <int P>
IKF_HD double cholesky_pivot_product(double G[P][P]) {
  double w = 1.0;
#pragma unroll
  for (int c = 0; c < P; ++c) {
    double d = G[c][c];
#pragma unroll
    for (int k = 0; k < c; ++k) d -= G[c][k] * G[c][k];
    if (d <= 0.0) return 0.0;
    const double lcc = sqrt(d);
    w *= lcc;
    const double inv = 1.0 / lcc;
#pragma unroll
    for (int r = c + 1; r < P; ++r) {
      double v = G[r][c];
#pragma unroll
      for (int k = 0; k < c; ++k) v -= G[r][k] * G[c][k];
      G[r][c] = v * inv;
    }
  }
  return w;
}

// the measure over rows ROW0 .. ROW0 + R - 1 of J
template <int NDOF, int R, int ROW0>
IKF_HD double manip_measure(const Chain* __restrict__ ch, const double axw[NDOF][3], const double orw[NDOF][3], const double p[3]) {
  constexpr int P = R < NDOF ? R : NDOF;
  double G[P][P];
  if constexpr (NDOF >= R) {   // G = J J^T, a column of J at a time
#pragma unroll
    for (int a = 0; a < P; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) G[a][b] = 0.0;
#pragma unroll
    for (int j = 0; j < NDOF; ++j) {
      double col[6];
      jacobian_column<double>(ch->joints[j].kind, axw[j], orw[j], p, col);
#pragma unroll
      for (int a = 0; a < P; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) G[a][b] += col[ROW0 + a] * col[ROW0 + b];
    }
  } else {                     // G = J^T J
    double J[NDOF][6];
#pragma unroll
    for (int j = 0; j < NDOF; ++j) jacobian_column<double>(ch->joints[j].kind, axw[j], orw[j], p, J[j]);
#pragma unroll
    for (int a = 0; a < P; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) {
        double sacc = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) sacc += J[a][ROW0 + r] * J[b][ROW0 + r];
        G[a][b] = sacc;
      }
  }
  return cholesky_pivot_product<P>(G);
}

template <int NDOF>
IKF_HD float manip_row(const Chain* __restrict__ ch, const float q[NDOF], int part) {
  double qd[NDOF];
  bool nan = false;
#pragma unroll
  for (int j = 0; j < NDOF; ++j) {
    qd[j] = (double)q[j];
    nan = nan || q[j] != q[j];
  }
  double R[9], p[3], axw[NDOF][3], orw[NDOF][3];
  fk_walk<double, NDOF, true>(ch, qd, R, p, axw, orw);
  double w;
  if (part == IKF_MANIP_FULL) w = manip_measure<NDOF, 6, 0>(ch, axw, orw, p);
  else if (part == IKF_MANIP_LINEAR) w = manip_measure<NDOF, 3, 3>(ch, axw, orw, p);
  else w = manip_measure<NDOF, 3, 0>(ch, axw, orw, p);
  return nan ? (float)NAN : (float)w;
}

// the rule
IKF_HD bool manip_below(float w, float floor) { return !(w >= floor); }

}  // namespace ikf
