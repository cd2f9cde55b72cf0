// The rules behind ctk_fit_resection (include/ctk.h, "fit resection"), restated ONCE for the device kernel (resection.hip) and for a host
// build of the same text (tests/test_resection_host.py compiles this header with g++ and compares it with the numpy restatement of
// tests/resection_reference.py -- no GPU needed to pin it).  Decisions are INTEGER or single comparisons; everything in double is ONE
// IEEE operation per step in the order written here (compile with -ffp-contract=off); no library square root and no trigonometry is
// taken anywhere (ctk_pose_polar is the only orthogonalisation); no sum depends on the order of accumulation: the device, the host
// build and numpy agree on every bit.  What is not named here is ctk_fit_pose's (pose_math.h) and, through it, ctk_fit_epipolar's,
// ctk_fit_planes' and ctk_fit_motion's: positions in 1/16 pixel (ctk_motion_quant), the pair rule with its three source forms
// (ctk_objects_source), ctk_pose_dot, ctk_pose_polar, ctk_pose_valid, ctk_pose_sum_index, ctk_plane_fix, ctk_plane_solve, all reused without change.
//
// Q = the position on frame f, 1/16 pixel.  X = a point of `structure`, three floats widened to double, in the SOURCE camera's
// coordinates; the pose maps them to frame-f coordinates, X' = R X + t, in the structure's unit: X'_i = dot(row i of R, X) + t_i.
//   fit list    the correspondences (ctk_fit_pose's gather) whose `valid` byte is nonzero and whose three structure floats are finite,
//               in ascending n; the first CTK_RESECTION_LIST_MAX = 4096 of them take part (M of them), more set stats[3] bit 3.
//   project     of X': where !(Z' > 0) the error is +inf and the point is behind.  iz = 1 / Z' (the one division per projection);
//               u = X' iz, v = Y' iz; px = fx u + cx, py = fy v + cy; dx = px - Qx / 16, dy = py - Qy / 16; e = dx dx + dy dy; a NaN counts as +inf.  Within tol iff
//               e <= tol2 with tol2 = (double)tol * (double)tol: no root.
//   seed        twelve floats (R0 | t0).  One that is not finite: (I | 0).  R0 takes ctk_pose_polar; where ctk_pose_valid then fails (the
//               determinant is not > 0, as for an all-zero seed): (I | 0) as well.  a = R0 X: a_i = dot(row i of R0, X).
//   candidates  k < K (`hypotheses`): i = ctk_motion_sample(seed, f, k, M, translation) picks an entry; with its ray y (ctk_pose_ray of
//               Q): yy = dot(y, y), tt = dot(t0, t0), yt = dot(y, t0), ya = dot(y, a), ta = dot(t0, a); den = yy tt - yt yt;
//               s = (yt ya - yy ta) / den: the least-squares scale of lambda y = a + s t0; +inf where !(den > 0).  An s that is not
//               finite or not > 0 is skipped.  The candidate is X' = a + s t0 (a product, a sum per component).  Then k = K: (R0, t0)
//               as s = 1; k = K + 1: (R0, 0) as s = 0; k = K + 2: (I, 0), X' = X.
//   score       the number of fit-list entries within tol (an integer); the largest wins, the lowest k on ties; below min_points
//               (6..8192), or M < min_points: no fit.  The winner's pose: R0 or I, t = s t0 (t0, 0, 0 for the fixed ones).
//   still       every structure point with a correspondence (beyond the list cap too; there is at least one) sits where it sat on the
//               source frame, Q = P in 1/16 pixel (integers): as far as the tracks tell the frame IS the source frame, on which the
//               structure's own rounding is all a refit could follow.  Then only k = K + 2, (I, 0), is scored and no round is run:
//               the pose is exactly (I | 0); stats[3] bit 5 says so.
//   refit       three Gauss-Newton rounds on the reprojection error over the entries within tol under the round's pose.  Per entry
//               with the projection's iz: gx = (fx iz, 0, -(fx iz) u), gy = (0, fy iz, -(fy iz) v): the gradients of px and py by X';
//               per component v = (cross(X', g), g, r) with r = dx or dy: seven numbers.  c2 = 256 (fx fx + fy fy).  The entry takes
//               part iff all fourteen v_i v_i <= 16 c2 (|v_i| <= 64 |(fx, fy)|: a point nearer than 1/64 of the unit, a ray beyond
//               83 degrees off the axis or a residual of 64 focal lengths is left out; stats[3] bit 2).  With ic2 = 1 / c2 (one
//               division per launch) that cap bounds every |(v_i v_j) ic2| by 16 (1 + 2^-51), so the 28 sums of
//               ctk_plane_fix((v_i v_j) ic2) -- a product, a product, llrint(. 2^44); ctk_pose_terms' order, both components -- over
//               at most 4096 entries x 2 stay below 2^61 (1 + 2^-51) in int64.  n = the entries taking part; n < 6: the
//               round keeps its pose.  The 8 x 8 system: N[i][j] = S_ij 2^-44 for i, j < 6, N[6][6] = N[7][7] = 1, zero elsewhere;
//               b[i] = -(S_i6 2^-44); ctk_plane_solve gives (dw, dt).  R' = polar(R + [dw]x R), t' = t + dt (no gauge: the structure
//               fixes the scale).  The round fails -- its pose stays, stats[3] bit 0 / 1 / 4 for rounds 1 / 2 / 3 -- when n < 6, the
//               solve fails or ctk_pose_valid(R', t') fails.
//   outputs     pose float32 [3,4] = (R | t), the (float) of the doubles.  Per slot n < N_out: label -1 and error -1 without a
//               correspondence or with the point not in the structure; else under the final pose (the doubles) label 1 within tol,
//               0 otherwise, error = (float)e (+inf behind the camera); entries beyond the list cap are classified too.
//               stats = (M, slots labelled 1, the winning k or -1, bits).
//   no fit      pose (I | 0); label 0 and error -1 for every structure point with a correspondence; stats = (M, 0, -1, bits).
#pragma once
#include <math.h>
#include <stdint.h>

#include "epipolar_math.h"
#include "motion_math.h"
#include "plane_math.h"
#include "pose_math.h"

#define CTK_RESECTION_LIST_MAX 4096
#define CTK_RESECTION_MIN_POINTS 6
#define CTK_RESECTION_HYPOTHESES_MAX 1024
#define CTK_RESECTION_ROUNDS 3
#define CTK_RESECTION_SOLVE_MIN 6
#define CTK_RESECTION_FLT_MAX 3.402823466e+38f
#define CTK_RESECTION_BIT_CAP 8
#define CTK_RESECTION_BIT_STILL 32

CTK_MM_HD bool ctk_resection_finite32(float v) { return fabsf(v) <= CTK_RESECTION_FLT_MAX; }  // (a NaN fails the comparison)

// a structure point -> it may be on the fit list; X: its doubles
CTK_MM_HD bool ctk_resection_point(const float* s, int8_t valid, double* X) {
  X[0] = (double)s[0], X[1] = (double)s[1], X[2] = (double)s[2];
  return valid != 0 && ctk_resection_finite32(s[0]) && ctk_resection_finite32(s[1]) && ctk_resection_finite32(s[2]);
}

CTK_MM_HD void ctk_resection_eye(CtkPose* p) {
  for (int i = 0; i < 9; ++i) p->R[i] = i % 4 == 0 ? 1.0 : 0.0;
  for (int i = 0; i < 3; ++i) p->t[i] = 0.0;
}

// twelve floats (R | t) -> the seed
CTK_MM_HD void ctk_resection_seed(const float* m, CtkPose* p) {
  bool ok = true;
  for (int i = 0; i < 12; ++i) ok = ok && ctk_resection_finite32(m[i]);
  if (ok) {
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) p->R[r * 3 + c] = (double)m[r * 4 + c];
      p->t[r] = (double)m[r * 4 + 3];
    }
    const double det = ctk_pose_polar(p->R);
    ok = ctk_pose_valid(*p, det);
  }
  if (!ok) ctk_resection_eye(p);
}

CTK_MM_HD double ctk_resection_tol2(float tol) {
  const double t = (double)tol;
  return t * t;
}

CTK_MM_HD double ctk_resection_c2(const CtkPoseCam& k) {
  const double a = k.fx * k.fx, b = k.fy * k.fy;
  const double s = a + b;
  return 256.0 * s;
}

// X' = R X + t
CTK_MM_HD void ctk_resection_apply(const CtkPose& p, const double* X, double* Xc) {
  for (int i = 0; i < 3; ++i) {
    const double d = ctk_pose_dot(p.R + i * 3, X);
    Xc[i] = d + p.t[i];
  }
}

// X' = a + s t0
CTK_MM_HD void ctk_resection_shift(const double* a, double s, const double* t0, double* Xc) {
  for (int i = 0; i < 3; ++i) {
    const double p = s * t0[i];
    Xc[i] = a[i] + p;
  }
}

// the squared reprojection error of X' against Q in px^2, +inf behind the camera; uvd: u, v, dx, dy, iz where it is in front
CTK_MM_HD double ctk_resection_error(const CtkPoseCam& k, const double* Xc, int qx, int qy, double* uvd) {
  if (!(Xc[2] > 0.0)) return INFINITY;
  const double iz = 1.0 / Xc[2];
  const double u = Xc[0] * iz, v = Xc[1] * iz;
  const double pu = k.fx * u, pv = k.fy * v;
  const double px = pu + k.cx, py = pv + k.cy;
  const double qu = (double)qx / 16.0, qv = (double)qy / 16.0;
  const double dx = px - qu, dy = py - qv;
  const double e0 = dx * dx, e1 = dy * dy;
  const double e = e0 + e1;
  uvd[0] = u, uvd[1] = v, uvd[2] = dx, uvd[3] = dy, uvd[4] = iz;
  return e != e ? INFINITY : e;
}

CTK_MM_HD bool ctk_resection_within(double e, double tol2) { return e <= tol2; }

// the scale of the candidate that entry (a, Q) gives under the seed's translation t0; +inf where there is none
CTK_MM_HD double ctk_resection_scale(const CtkPoseCam& k, const double* a, int qx, int qy, const double* t0) {
  double y[3];
  ctk_pose_ray(k, qx, qy, y);
  const double yy = ctk_pose_dot(y, y), tt = ctk_pose_dot(t0, t0), yt = ctk_pose_dot(y, t0), ya = ctk_pose_dot(y, a), ta = ctk_pose_dot(t0, a);
  const double d0 = yy * tt, d1 = yt * yt;
  const double den = d0 - d1;
  if (!(den > 0.0)) return INFINITY;
  const double n0 = yt * ya, n1 = yy * ta;
  const double num = n0 - n1;
  return num / den;
}

CTK_MM_HD bool ctk_resection_scale_ok(double s) { return s > 0.0 && ctk_plane_finite(s); }

// an entry within tol (X', and uvd as ctk_resection_error left it) -> takes part; vx, vy: its two rows of seven numbers
CTK_MM_HD bool ctk_resection_entry(const CtkPoseCam& k, double c2, const double* Xc, const double* uvd, double* vx, double* vy) {
  const double iz = uvd[4];
  const double ax = k.fx * iz, ay = k.fy * iz;
  const double bx = ax * uvd[0], by = ay * uvd[1];
  const double gx[3] = {ax, 0.0, -bx}, gy[3] = {0.0, ay, -by};
  ctk_pose_cross(Xc, gx, vx);
  ctk_pose_cross(Xc, gy, vy);
  for (int i = 0; i < 3; ++i) vx[3 + i] = gx[i], vy[3 + i] = gy[i];
  vx[6] = uvd[2], vy[6] = uvd[3];
  const double cap = 16.0 * c2;
  bool in = true;
  for (int i = 0; i < 7; ++i) {
    const double qx = vx[i] * vx[i], qy = vy[i] * vy[i];
    in = in && qx <= cap && qy <= cap;
  }
  return in;
}

CTK_MM_HD double ctk_resection_ic2(double c2) { return 1.0 / c2; }

// the terms of an entry's component that takes part, added to s (28 sums in ctk_pose_terms' order)
CTK_MM_HD void ctk_resection_terms(const double* v, double ic2, int64_t* s) {
  int n = 0;
  CTK_EPI_UNROLL
  for (int i = 0; i < 6; ++i) {
    CTK_EPI_UNROLL
    for (int j = i; j < 6; ++j) {
      const double q = v[i] * v[j];
      s[n] += ctk_plane_fix(q * ic2);
      ++n;
    }
  }
  CTK_EPI_UNROLL
  for (int i = 0; i < 7; ++i) {
    const double q = v[i] * v[6];
    s[n] += ctk_plane_fix(q * ic2);
    ++n;
  }
}

// one round's update from its sums and the count n of the entries that took part; work: CTK_POSE_SOLVE_DOUBLES -> the round stands
CTK_MM_HD bool ctk_resection_update(const CtkPose& cur, const int64_t* s, int n, double* work, CtkPose* next) {
  if (n < CTK_RESECTION_SOLVE_MIN) return false;
  double* N = work;
  double* b = N + 64;
  double* L = b + 8;
  double* D = L + 64;
  double* v = D + 8;
  double* z = v + 8;
  double* h = z + 8;
  for (int i = 0; i < 64; ++i) N[i] = 0.0;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      const int lo = i < j ? i : j, hi = i < j ? j : i;
      N[i * 8 + j] = (double)s[ctk_pose_sum_index(lo, hi)] * CTK_PLANE_UNFIX;
    }
  N[6 * 8 + 6] = 1.0, N[7 * 8 + 7] = 1.0;
  for (int i = 0; i < 6; ++i) b[i] = -((double)s[21 + i] * CTK_PLANE_UNFIX);
  b[6] = 0.0, b[7] = 0.0;
  if (!ctk_plane_solve(N, b, L, D, v, z, h)) return false;
  double W[9];
  ctk_pose_skew_times(h, cur.R, W);
  for (int i = 0; i < 9; ++i) next->R[i] = cur.R[i] + W[i];
  const double det = ctk_pose_polar(next->R);
  for (int i = 0; i < 3; ++i) next->t[i] = cur.t[i] + h[3 + i];
  return ctk_pose_valid(*next, det);
}

// the candidates' counts are compared as (count, lowest k): -> a is better than b
CTK_MM_HD bool ctk_resection_better(int count_a, int k_a, int count_b, int k_b) { return count_a > count_b || (count_a == count_b && k_a < k_b); }
