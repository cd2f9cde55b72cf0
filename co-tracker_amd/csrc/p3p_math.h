// The rules behind ctk_fit_p3p (include/ctk.h, "fit p3p"), restated ONCE for the device kernel (p3p.hip) and for a host build of the
// same text (tests/test_p3p_host.py compiles this header with g++ and compares it with the numpy restatement of
// tests/p3p_reference.py -- no GPU needed to pin it).  Decisions are INTEGER or single comparisons; everything in double is ONE IEEE
// operation per step in the order written here (compile with -ffp-contract=off); no library square root and no trigonometry is taken
// anywhere (ctk_pose_rsqrt and ctk_pose_polar are the only ones); no sum depends on the order of accumulation: the device, the host
// build and numpy agree on every bit.  What is not named here is ctk_fit_resection's (resection_math.h) and, through it,
// ctk_fit_pose's, ctk_fit_planes' and ctk_fit_motion's: the gather, the fit list (ctk_resection_point; ascending n; the first
// CTK_RESECTION_LIST_MAX entries, M of them; stats[3] bit 3), project and within (ctk_resection_apply, ctk_resection_error,
// ctk_resection_within), the `still` rule, the score with its tie rule (ctk_resection_better) and min_points, the three Gauss-Newton
// rounds (ctk_resection_entry / _terms / _update), the outputs, no fit and stats: all reused without change.
//
// What is new is the candidates: there is NO seed.  (X_i, Q_i), i = 0, 1, 2: three entries of the fit list; y_i = ctk_pose_ray(Q_i).
//   sample      candidate k < K (`hypotheses`, 1..1024) takes the FIRST THREE of the four distinct indices
//               ctk_plane_sample(seed, f, k, M, .) (M >= min_points >= 6 where candidates are made).
//   unknowns    the scales l_i of the camera points Y_i = l_i y_i, under the three equations
//               l_i^2 yy_i + l_j^2 yy_j - 2 l_i l_j c_ij = d_ij for (i, j) = (0, 1), (0, 2), (1, 2); yy_i = dot(y_i, y_i),
//               c_ij = dot(y_i, y_j), d_ij = dot(X_i - X_j, X_i - X_j) (a difference per component, then the dot).
//   start       the point's own distance from the structure's camera: XX_i = dot(X_i, X_i); l_i = XX_i * rsqrt(XX_i * yy_i).  A point
//               with XX_i not > 0, or not finite, skips the candidate.
//   newton      CTK_P3P_ROUNDS = 6 rounds on the 3 x 3 system.  Residual of row (i, j): p = (l_i l_i) yy_i, q = (l_j l_j) yy_j,
//               m = (l_i l_j) c_ij; r = ((p + q) - 2 m) - d_ij.  The row's two non-zeros: a = 2 (l_i yy_i - l_j c_ij) in column i,
//               b = 2 (l_j yy_j - l_i c_ij) in column j (products, a difference, an exact doubling).  The step solves J x = r by
//               cofactors (ctk_p3p_solve: C row r = cross(J row r + 1, J row r + 2), indices mod 3; det = dot(J row 0, C row 0);
//               id = 1 / det, the one division; x_i = dot(column i of C, r) id) and l_i = l_i - x_i.  [structure_math.h's cofactor
//               solve is for a SYMMETRIC matrix of determinant > 0; J is neither, so the same form is written once here.]
//               A determinant that is zero or not finite skips the candidate.  After the rounds every l_i must be finite and > 0,
//               else skip.
//   pose        A = [X_1 - X_0, X_2 - X_0, their cross product] as columns and B likewise from the Y_i (Y_i = l_i y_i, a product per
//               component).  C = the cofactors of A as above, det A = dot(A row 0, C row 0); det A not > 0 (a collinear or repeated
//               triple) skips the candidate.  id = 1 / det A; M_ij = dot(B row i, C row j) id (= B A^-1); R = the four polar steps of
//               M (ctk_pose_polar), t_i = Y_0i - dot(R row i, X_0); the candidate stands iff ctk_pose_valid(R, t, det R).
//   fixed       k = K is (I, 0): the only candidate on a `still` frame, as in resection.  stats[2] is in 0 .. K.
//   scoring     every candidate, the fixed one included, is scored as X' = R X + t through ctk_resection_apply.
//
// Known limit.  Newton finds the P3P root NEAREST the structure's own distances: one root per triple, not the up to four a closed-form
// solver returns.  Measured on the CPU (noise-free, 300 points 3..12 deep, 400 clean triples a row): the share of clean triples that
// return the planted pose is 0.99 / 0.98 / 0.97 / 0.95 for a camera displaced by 0.3 / 1 / 2 / 3 units, with 0.02 and 0.3 rad of turn
// alike; four rounds give 0.92 at the far end, twelve no more than eight.  A camera further from the structure's camera than the
// nearest point is deep was not tried.  The rest are resection's limits.
#pragma once
#include <math.h>
#include <stdint.h>

#include "resection_math.h"

#define CTK_P3P_ROUNDS 6

// the cofactors of a 3 x 3 matrix, row major: row r = cross(row r + 1, row r + 2) -> the determinant, dot(row 0 of A, row 0 of C)
CTK_MM_HD double ctk_p3p_cofactors(const double* A, double* C) {
  ctk_pose_cross(A + 3, A + 6, C);
  ctk_pose_cross(A + 6, A, C + 3);
  ctk_pose_cross(A, A + 3, C + 6);
  return ctk_pose_dot(A, C);
}

// J x = r -> the solve stands (the determinant is neither zero nor not finite)
CTK_MM_HD bool ctk_p3p_solve(const double* J, const double* r, double* x) {
  double C[9];
  const double det = ctk_p3p_cofactors(J, C);
  x[0] = 0.0, x[1] = 0.0, x[2] = 0.0;
  if (det == 0.0 || !ctk_plane_finite(det)) return false;
  const double id = 1.0 / det;
  for (int i = 0; i < 3; ++i) {
    const double col[3] = {C[i], C[3 + i], C[6 + i]};
    const double n = ctk_pose_dot(col, r);
    x[i] = n * id;
  }
  return true;
}

// the start of one scale: the point's own distance from the structure's camera over the length of its ray
CTK_MM_HD bool ctk_p3p_start(const double* X, double yy, double* l) {
  const double XX = ctk_pose_dot(X, X);
  *l = 0.0;
  if (!(XX > 0.0) || !ctk_plane_finite(XX)) return false;
  const double w = XX * yy;
  *l = XX * ctk_pose_rsqrt(w);
  return true;
}

// one row of the Newton system: the residual and the two non-zeros of the Jacobian
CTK_MM_HD void ctk_p3p_row(double li, double lj, double yyi, double yyj, double c, double d, double* r, double* a, double* b) {
  const double li2 = li * li, lj2 = lj * lj, lij = li * lj;
  const double p = li2 * yyi, q = lj2 * yyj, m = lij * c;
  const double s = p + q, m2 = 2.0 * m;
  const double e = s - m2;
  *r = e - d;
  const double ui = li * yyi, vj = lj * c, uj = lj * yyj, vi = li * c;
  const double wa = ui - vj, wb = uj - vi;
  *a = 2.0 * wa, *b = 2.0 * wb;
}

// three entries of the fit list (X: nine doubles, three a point; q: six integers, (Qx, Qy) a point) -> the candidate stands; *p
CTK_MM_HD bool ctk_p3p_candidate(const CtkPoseCam& k, const double* X, const int* q, CtkPose* p) {
  ctk_resection_eye(p);
  double y[9], yy[3], l[3];
  bool ok = true;
  for (int i = 0; i < 3; ++i) {
    ctk_pose_ray(k, q[i * 2], q[i * 2 + 1], y + i * 3);
    yy[i] = ctk_pose_dot(y + i * 3, y + i * 3);
    ok = ctk_p3p_start(X + i * 3, yy[i], &l[i]) && ok;
  }
  if (!ok) return false;
  const double c01 = ctk_pose_dot(y, y + 3), c02 = ctk_pose_dot(y, y + 6), c12 = ctk_pose_dot(y + 3, y + 6);
  const double e01[3] = {X[0] - X[3], X[1] - X[4], X[2] - X[5]}, e02[3] = {X[0] - X[6], X[1] - X[7], X[2] - X[8]};
  const double e12[3] = {X[3] - X[6], X[4] - X[7], X[5] - X[8]};
  const double d01 = ctk_pose_dot(e01, e01), d02 = ctk_pose_dot(e02, e02), d12 = ctk_pose_dot(e12, e12);
  for (int round = 0; round < CTK_P3P_ROUNDS; ++round) {
    double J[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r[3], x[3];
    ctk_p3p_row(l[0], l[1], yy[0], yy[1], c01, d01, &r[0], &J[0], &J[1]);
    ctk_p3p_row(l[0], l[2], yy[0], yy[2], c02, d02, &r[1], &J[3], &J[5]);
    ctk_p3p_row(l[1], l[2], yy[1], yy[2], c12, d12, &r[2], &J[7], &J[8]);
    ok = ctk_p3p_solve(J, r, x) && ok;
    l[0] = l[0] - x[0], l[1] = l[1] - x[1], l[2] = l[2] - x[2];
  }
  for (int i = 0; i < 3; ++i) ok = ok && l[i] > 0.0 && ctk_plane_finite(l[i]);
  if (!ok) return false;
  double Y[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Y[i * 3 + j] = l[i] * y[i * 3 + j];
  const double a1[3] = {X[3] - X[0], X[4] - X[1], X[5] - X[2]}, a2[3] = {X[6] - X[0], X[7] - X[1], X[8] - X[2]};
  const double b1[3] = {Y[3] - Y[0], Y[4] - Y[1], Y[5] - Y[2]}, b2[3] = {Y[6] - Y[0], Y[7] - Y[1], Y[8] - Y[2]};
  double a3[3], b3[3];
  ctk_pose_cross(a1, a2, a3);
  ctk_pose_cross(b1, b2, b3);
  const double A[9] = {a1[0], a2[0], a3[0], a1[1], a2[1], a3[1], a1[2], a2[2], a3[2]};
  const double B[9] = {b1[0], b2[0], b3[0], b1[1], b2[1], b3[1], b1[2], b2[2], b3[2]};
  double C[9];
  const double detA = ctk_p3p_cofactors(A, C);
  if (!(detA > 0.0)) return false;
  const double id = 1.0 / detA;
  CtkPose w;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double n = ctk_pose_dot(B + i * 3, C + j * 3);
      w.R[i * 3 + j] = n * id;
    }
  const double det = ctk_pose_polar(w.R);
  for (int i = 0; i < 3; ++i) {
    const double n = ctk_pose_dot(w.R + i * 3, X);
    w.t[i] = Y[i] - n;
  }
  if (!ctk_pose_valid(w, det)) return false;
  *p = w;
  return true;
}
