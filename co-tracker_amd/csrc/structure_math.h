// The rules behind ctk_fit_structure (include/ctk.h, "fit structure"), restated ONCE for the device kernel (structure.hip) and for a host
// build of the same text (tests/test_structure_host.py compiles this header with g++ and compares it with the numpy restatement of
// tests/structure_reference.py -- no GPU needed to pin it).  Decisions are INTEGER or single comparisons; everything in double is ONE
// IEEE operation per step in the order written here (compile with -ffp-contract=off); no library square root and no trigonometry is
// taken anywhere.  Every point is summed by ONE thread over its views in ASCENDING view order, so the plain double sums below are
// deterministic as they stand: no fixed-point sums are needed here (resection_math.h needs them because a workgroup shares one sum).
// The device, the host build and numpy agree on every bit.  What is not named here is ctk_fit_resection's (resection_math.h) and,
// through it, ctk_fit_pose's (pose_math.h): positions in 1/16 pixel (ctk_motion_quant), ctk_pose_ray, ctk_pose_dot, ctk_pose_cross,
// ctk_pose_polar, ctk_pose_valid, ctk_resection_apply, ctk_resection_error, ctk_resection_within, ctk_resection_tol2,
// ctk_resection_finite32, all reused without change.
//
//   views       the frames f0 + j, 0 <= j < F <= CTK_STRUCTURE_VIEWS_MAX = 256, each with twelve floats (R | t) of `pose` (X_f = R X_source
//               + t, as ctk_fit_resection writes it) and optionally four int32 of `pose_stats`.  View j COUNTS iff its twelve floats are
//               finite, R passes the four polar steps and ctk_pose_valid (ctk_resection_seed's checks; a failure drops the view, it
//               does not become the identity), and pose_stats is NULL or pose_stats[j][2] >= 0.  Its centre: c_i = -dot(column i of R, t).
//   observation slot n on view j: the view counts, f0 + j >= first_row[n] (when given), both coordinates quantise, the slot is visible
//               there (the byte, or ctk_draw_visible of the logits).  One frame is gathered: no source frame, no pair rule.  m = their
//               number.  y = ctk_pose_ray(Q); d_i = dot(column i of R, y) (= R^T y).
//   start       the linear midpoint solution.  Per observation: w = 1 / dot(d, d); P_ij = -((d_i d_j) w) off the diagonal and
//               1 - (d_i d_i) w on it, six entries in the order 00 01 02 11 12 22; A_ij += P_ij; b_i += dot(row i of P, c).
//   solve       of a symmetric 3 x 3 system A x = b: the cofactors C00 = A11 A22 - A12 A12, C01 = A02 A12 - A01 A22, C02 = A01 A12 -
//               A02 A11, C11 = A00 A22 - A02 A02, C12 = A01 A02 - A00 A12, C22 = A00 A11 - A01 A01 (two products, one difference);
//               det = dot((A00, A01, A02), (C00, C01, C02)); it fails where det is not > 0 or not finite; id = 1 / det (the one
//               division); x_i = dot(row i of C, b) id; it fails where an x_i is not finite.
//               No start when m < 2 or the solve fails: the slot is rejected, bit 3.
//   rounds      three Gauss-Newton rounds on the reprojection error.  Round r = 0, 1, 2 uses the observations with
//               e <= (g_r t)(g_r t), t = (double)tol, g = 4, 2, 1 (a product, a product): the graduated gate lets one bad view of a
//               track drop out.  Per observation under X: X' = ctk_resection_apply, e = ctk_resection_error with its u, v, dx, dy, iz;
//               gx = (fx iz, 0, -((fx iz) u)), gy = (0, fy iz, -((fy iz) v)) (resection_math.h's); jx_i = dot(gx, column i of R), jy_i
//               likewise; H_ij += (jx_i jx_j) + (jy_i jy_j) in the six-entry order; g_i += (jx_i dx) + (jy_i dy).  delta = solve(H, -g),
//               X = X + delta.  The round keeps its X -- bits 0 / 1 / 2 for rounds 1 / 2 / 3 -- when fewer than min_views observations
//               take part, the solve fails, or an X_i stops being finite.
//   accept      under the final X the COUNTED views are the observations within tol (e <= t t; behind a camera e = +inf), in ascending
//               j; a = the first of them.  w_j = X - c_j; cr = cross(w_a, w_j); parallax holds iff for some counted j
//               dot(cr, cr) >= (dot(w_a, w_a) dot(w_j, w_j)) (double)min_sin2: one comparison, no root, no division (bit 4 where it
//               does not hold).  The error is (the sum of e over the counted views, ascending) / (double)counted, one division.
//               Accepted iff counted >= min_views (2..256), 2 counted >= m, parallax holds and the three output floats are finite.
//               [the majority rule, bit 6 where it fails, is a rule the work showed to be needed: with min_views = 3 of 12 views a
//               point that moves by itself finds three neighbouring views that agree, and the gates let the others drop; planted
//               movers came back 84 of 2000 against the 59 a float64 triangulation over all their views keeps, 37 with the rule]
//               The start is not robust: one wrong view of about 5 tol among 8 is dropped by the gates, one of 40 tol leaves no
//               view within the first gate and the slot is rejected (never accepted on the wrong views).
//   into        -1: every point is written as it is, (float)X_i.  k = into in [0, F): every written point is ctk_resection_apply of view k
//               (double, then float): the structure is stated in the camera of frame f0 + k.  Where view k does not count there is no
//               structure: every point is zero, the label is 0 for every slot with an observation (m >= 1) or in the old structure
//               and -1 for every other slot, error -1, stats = (m, 0, -1, bit 5); nothing is triangulated.
//   carry       with structure_in / valid_in: a slot is IN THE OLD STRUCTURE when its valid byte is nonzero, its three floats are
//               finite and first_row[n] <= source_frame (when first_row is given: a released and reassigned slot is not carried).  It is
//               CARRIED when, besides, the three floats of its old point through the into pose (or as they are, into = -1) are
//               finite.  [a rule the work showed to be needed: a carried point must be writable]
//               refine = 0: a carried slot is not gathered and not triangulated: label 2, error -1, stats = (0, 0, -1, 0).
//               refine = 1: it is triangulated like every other slot; accepted, the new point wins (label 1); rejected, the old one is
//               written (label 2, error -1, the stats of the attempt).
//   origin      origin_out = (R_k R_o | R_k t_o + t_k) in double, then float: entry (i, j) = dot(row i of R_k, column j of R_o), the
//               translation dot(row i of R_k, t_o) + t_k_i; R_o, t_o are the floats of origin_in widened (the identity for NULL).
//               A copy of origin_in's floats where into < 0 or view k does not count.
//   outputs     points float32 [N_out,3], zero where the label is < 1.  label int8: -1 fewer than 2 observations and not carried; 0
//               triangulated (m >= 2) and rejected; 1 triangulated and accepted; 2 carried.  error float32: the mean squared
//               reprojection error over the counted views in px^2, -1 where the label is not 1.  stats int32 [N_out,4] = (m, counted
//               views, the first counted view or -1, bits).  A slot with m < 2 has stats (m, 0, -1, bit 3).
#pragma once
#include <math.h>
#include <stdint.h>

#include "resection_math.h"

#define CTK_STRUCTURE_VIEWS_MAX 256
#define CTK_STRUCTURE_POINTS_MAX 8192
#define CTK_STRUCTURE_MIN_VIEWS 2
#define CTK_STRUCTURE_ROUNDS 3
#define CTK_STRUCTURE_BIT_ROUND1 1
#define CTK_STRUCTURE_BIT_ROUND2 2
#define CTK_STRUCTURE_BIT_ROUND3 4
#define CTK_STRUCTURE_BIT_NO_START 8
#define CTK_STRUCTURE_BIT_NO_PARALLAX 16
#define CTK_STRUCTURE_BIT_INTO 32
#define CTK_STRUCTURE_BIT_MINORITY 64

// a counting view: its pose with R orthogonalised, and its centre
struct CtkStructureView {
  CtkPose p;
  double c[3];
};

// the sums of one pass of one slot: the six of the matrix (00 01 02 11 12 22), the three of the right-hand side
struct CtkStructureSums {
  double A[6];
  double b[3];
};

CTK_MM_HD void ctk_structure_zero(CtkStructureSums* s) {
  for (int i = 0; i < 6; ++i) s->A[i] = 0.0;
  for (int i = 0; i < 3; ++i) s->b[i] = 0.0;
}

// twelve floats (R | t) and whether pose_stats lets the view count -> the view counts; then *v
CTK_MM_HD bool ctk_structure_view(const float* m, bool stats_ok, CtkStructureView* v) {
  bool ok = stats_ok;
  for (int i = 0; i < 12; ++i) ok = ok && ctk_resection_finite32(m[i]);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) v->p.R[r * 3 + c] = ok ? (double)m[r * 4 + c] : (r == c ? 1.0 : 0.0);
    v->p.t[r] = ok ? (double)m[r * 4 + 3] : 0.0;
  }
  if (ok) {
    const double det = ctk_pose_polar(v->p.R);
    ok = ctk_pose_valid(v->p, det);
  }
  for (int i = 0; i < 3; ++i) {
    const double col[3] = {v->p.R[i], v->p.R[3 + i], v->p.R[6 + i]};
    v->c[i] = -ctk_pose_dot(col, v->p.t);
  }
  return ok;
}

// o = R^T a
CTK_MM_HD void ctk_structure_rt(const double* R, const double* a, double* o) {
  for (int i = 0; i < 3; ++i) {
    const double col[3] = {R[i], R[3 + i], R[6 + i]};
    o[i] = ctk_pose_dot(a, col);
  }
}

// one observation's term of the start
CTK_MM_HD void ctk_structure_start_term(const CtkPoseCam& k, const CtkStructureView& v, int qx, int qy, CtkStructureSums* s) {
  double y[3], d[3];
  ctk_pose_ray(k, qx, qy, y);
  ctk_structure_rt(v.p.R, y, d);
  const double dd = ctk_pose_dot(d, d);
  const double w = 1.0 / dd;
  const double d00 = d[0] * d[0], d01 = d[0] * d[1], d02 = d[0] * d[2], d11 = d[1] * d[1], d12 = d[1] * d[2], d22 = d[2] * d[2];
  const double e00 = d00 * w, e01 = d01 * w, e02 = d02 * w, e11 = d11 * w, e12 = d12 * w, e22 = d22 * w;
  const double P[6] = {1.0 - e00, -e01, -e02, 1.0 - e11, -e12, 1.0 - e22};
  for (int i = 0; i < 6; ++i) s->A[i] = s->A[i] + P[i];
  const double r0[3] = {P[0], P[1], P[2]}, r1[3] = {P[1], P[3], P[4]}, r2[3] = {P[2], P[4], P[5]};
  const double b0 = ctk_pose_dot(r0, v.c), b1 = ctk_pose_dot(r1, v.c), b2 = ctk_pose_dot(r2, v.c);
  s->b[0] = s->b[0] + b0, s->b[1] = s->b[1] + b1, s->b[2] = s->b[2] + b2;
}

CTK_MM_HD bool ctk_structure_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // (a NaN fails the comparison)

// A x = b, A symmetric in the six-entry order -> the solve stands
CTK_MM_HD bool ctk_structure_solve(const double* A, const double* b, double* x) {
  const double a00 = A[0], a01 = A[1], a02 = A[2], a11 = A[3], a12 = A[4], a22 = A[5];
  const double p0 = a11 * a22, q0 = a12 * a12, p1 = a02 * a12, q1 = a01 * a22, p2 = a01 * a12, q2 = a02 * a11;
  const double p3 = a00 * a22, q3 = a02 * a02, p4 = a01 * a02, q4 = a00 * a12, p5 = a00 * a11, q5 = a01 * a01;
  const double c00 = p0 - q0, c01 = p1 - q1, c02 = p2 - q2, c11 = p3 - q3, c12 = p4 - q4, c22 = p5 - q5;
  const double r0[3] = {c00, c01, c02}, r1[3] = {c01, c11, c12}, r2[3] = {c02, c12, c22}, top[3] = {a00, a01, a02};
  const double det = ctk_pose_dot(top, r0);
  x[0] = 0.0, x[1] = 0.0, x[2] = 0.0;
  if (!(det > 0.0) || !ctk_structure_finite(det)) return false;
  const double id = 1.0 / det;
  const double n0 = ctk_pose_dot(r0, b), n1 = ctk_pose_dot(r1, b), n2 = ctk_pose_dot(r2, b);
  x[0] = n0 * id, x[1] = n1 * id, x[2] = n2 * id;
  return ctk_structure_finite(x[0]) && ctk_structure_finite(x[1]) && ctk_structure_finite(x[2]);
}

// the squared gate of round r
CTK_MM_HD double ctk_structure_gate2(float tol, int round) {
  const double t = (double)tol;
  const double g = round == 0 ? 4.0 : (round == 1 ? 2.0 : 1.0);
  const double gt = g * t;
  return gt * gt;
}

// the squared reprojection error of X on a view; uvd as ctk_resection_error leaves it
CTK_MM_HD double ctk_structure_error(const CtkPoseCam& k, const CtkStructureView& v, const double* X, int qx, int qy, double* uvd) {
  double Xc[3];
  ctk_resection_apply(v.p, X, Xc);
  return ctk_resection_error(k, Xc, qx, qy, uvd);
}

// one observation's term of a round (it lies within the round's gate; uvd: ctk_structure_error's)
CTK_MM_HD void ctk_structure_round_term(const CtkPoseCam& k, const CtkStructureView& v, const double* uvd, CtkStructureSums* s) {
  const double iz = uvd[4];
  const double ax = k.fx * iz, ay = k.fy * iz;
  const double bx = ax * uvd[0], by = ay * uvd[1];
  const double gx[3] = {ax, 0.0, -bx}, gy[3] = {0.0, ay, -by};
  double jx[3], jy[3];
  ctk_structure_rt(v.p.R, gx, jx);
  ctk_structure_rt(v.p.R, gy, jy);
  int n = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) {
      const double p = jx[i] * jx[j], q = jy[i] * jy[j];
      const double h = p + q;
      s->A[n] = s->A[n] + h;
      ++n;
    }
  for (int i = 0; i < 3; ++i) {
    const double p = jx[i] * uvd[2], q = jy[i] * uvd[3];
    const double h = p + q;
    s->b[i] = s->b[i] + h;
  }
}

// one round's update from its sums and the number n of observations that took part -> the round stands; then X is the new point
CTK_MM_HD bool ctk_structure_update(const CtkStructureSums& s, int n, int min_views, double* X) {
  if (n < min_views) return false;
  const double nb[3] = {-s.b[0], -s.b[1], -s.b[2]};
  double delta[3];
  if (!ctk_structure_solve(s.A, nb, delta)) return false;
  const double x0 = X[0] + delta[0], x1 = X[1] + delta[1], x2 = X[2] + delta[2];
  if (!(ctk_structure_finite(x0) && ctk_structure_finite(x1) && ctk_structure_finite(x2))) return false;
  X[0] = x0, X[1] = x1, X[2] = x2;
  return true;
}

CTK_MM_HD int ctk_structure_round_bit(int round) {
  return round == 0 ? CTK_STRUCTURE_BIT_ROUND1 : (round == 1 ? CTK_STRUCTURE_BIT_ROUND2 : CTK_STRUCTURE_BIT_ROUND3);
}

// w = X - c of a counted view
CTK_MM_HD void ctk_structure_arm(const double* X, const CtkStructureView& v, double* w) {
  w[0] = X[0] - v.c[0], w[1] = X[1] - v.c[1], w[2] = X[2] - v.c[2];
}

// the arms of the first counted view and of a counted view -> they show parallax
CTK_MM_HD bool ctk_structure_parallax(const double* wa, const double* wj, float min_sin2) {
  double cr[3];
  ctk_pose_cross(wa, wj, cr);
  const double l = ctk_pose_dot(cr, cr), na = ctk_pose_dot(wa, wa), nj = ctk_pose_dot(wj, wj);
  const double nn = na * nj;
  const double r = nn * (double)min_sin2;
  return l >= r;
}

CTK_MM_HD double ctk_structure_mean(double sum, int counted) { return sum / (double)counted; }

// a point as it is written: through the into view (or as it is) -> its three floats are finite
CTK_MM_HD bool ctk_structure_out(const CtkStructureView* into, const double* X, float* o) {
  double Xo[3] = {X[0], X[1], X[2]};
  if (into != nullptr) ctk_resection_apply(into->p, X, Xo);
  o[0] = (float)Xo[0], o[1] = (float)Xo[1], o[2] = (float)Xo[2];
  return ctk_resection_finite32(o[0]) && ctk_resection_finite32(o[1]) && ctk_resection_finite32(o[2]);
}

// a slot of the old structure -> it is in it; X: its doubles
CTK_MM_HD bool ctk_structure_old(const float* s, int8_t valid, bool has_first, int first, int source_frame, double* X) {
  X[0] = (double)s[0], X[1] = (double)s[1], X[2] = (double)s[2];
  return valid != 0 && ctk_resection_finite32(s[0]) && ctk_resection_finite32(s[1]) && ctk_resection_finite32(s[2]) &&
         (!has_first || first <= source_frame);
}

// origin_in (twelve floats, or NULL: the identity) through the into view (NULL: a copy) -> twelve floats
CTK_MM_HD void ctk_structure_origin(const float* in, const CtkStructureView* into, float* o) {
  float m[12];
  for (int i = 0; i < 12; ++i) m[i] = in != nullptr ? in[i] : (i % 5 == 0 ? 1.0f : 0.0f);
  if (into == nullptr) {
    for (int i = 0; i < 12; ++i) o[i] = m[i];
    return;
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 4; ++j) {
      const double col[3] = {(double)m[j], (double)m[4 + j], (double)m[8 + j]};
      const double d = ctk_pose_dot(into->p.R + i * 3, col);
      o[i * 4 + j] = j < 3 ? (float)d : (float)(d + into->p.t[i]);
    }
  }
}

// The whole of one slot once its observations can be fetched: obs(j, &qx, &qy) -> slot n is observed on view j (a counting one).  The
// device kernel and the host build walk the views through this one text.  old: the slot's old point where it is carried, else
// nullptr (refine = 0 never comes here with a carried slot).  -> the label; point, *error, stats: as they are written.
template <typename Obs>
CTK_MM_HD int ctk_structure_slot(const CtkPoseCam& cam, const CtkStructureView* views, const uint8_t* counts, int F, int into, float tol,
                                 float min_sin2, int min_views, const float* old, Obs obs, float* point, float* error, int32_t* stats) {
  const int fallback = old != nullptr ? 2 : 0;
  point[0] = old != nullptr ? old[0] : 0.0f, point[1] = old != nullptr ? old[1] : 0.0f, point[2] = old != nullptr ? old[2] : 0.0f;
  *error = -1.0f;
  stats[0] = 0, stats[1] = 0, stats[2] = -1, stats[3] = 0;
  // the start
  CtkStructureSums s;
  ctk_structure_zero(&s);
  int m = 0;
  for (int j = 0; j < F; ++j) {
    int qx, qy;
    if (counts[j] == 0 || !obs(j, &qx, &qy)) continue;
    ctk_structure_start_term(cam, views[j], qx, qy, &s);
    ++m;
  }
  stats[0] = m;
  double X[3];
  if (m < 2 || !ctk_structure_solve(s.A, s.b, X)) {
    stats[3] = CTK_STRUCTURE_BIT_NO_START;
    return m < 2 && old == nullptr ? -1 : fallback;
  }
  int bits = 0;
  for (int round = 0; round < CTK_STRUCTURE_ROUNDS; ++round) {
    const double gate2 = ctk_structure_gate2(tol, round);
    ctk_structure_zero(&s);
    int n = 0;
    for (int j = 0; j < F; ++j) {
      int qx, qy;
      if (counts[j] == 0 || !obs(j, &qx, &qy)) continue;
      double uvd[5];
      if (!ctk_resection_within(ctk_structure_error(cam, views[j], X, qx, qy, uvd), gate2)) continue;
      ctk_structure_round_term(cam, views[j], uvd, &s);
      ++n;
    }
    if (!ctk_structure_update(s, n, min_views, X)) bits |= ctk_structure_round_bit(round);
  }
  // the counted views and the parallax
  const double tol2 = ctk_resection_tol2(tol);
  int counted = 0, a = -1;
  bool parallax = false;
  double wa[3] = {0.0, 0.0, 0.0}, sum = 0.0;
  for (int j = 0; j < F; ++j) {
    int qx, qy;
    if (counts[j] == 0 || !obs(j, &qx, &qy)) continue;
    double uvd[5];
    const double e = ctk_structure_error(cam, views[j], X, qx, qy, uvd);
    if (!ctk_resection_within(e, tol2)) continue;
    double wj[3];
    ctk_structure_arm(X, views[j], wj);
    if (a < 0) a = j, wa[0] = wj[0], wa[1] = wj[1], wa[2] = wj[2];
    parallax = ctk_structure_parallax(wa, wj, min_sin2) || parallax;
    sum = sum + e;
    ++counted;
  }
  if (!parallax) bits |= CTK_STRUCTURE_BIT_NO_PARALLAX;
  const bool majority = 2 * counted >= m;
  if (!majority) bits |= CTK_STRUCTURE_BIT_MINORITY;
  stats[1] = counted, stats[2] = a, stats[3] = bits;
  float o[3];
  const bool writable = ctk_structure_out(into >= 0 ? &views[into] : nullptr, X, o);
  if (!(counted >= min_views && majority && parallax && writable)) return fallback;
  point[0] = o[0], point[1] = o[1], point[2] = o[2];
  *error = (float)ctk_structure_mean(sum, counted);
  return 1;
}
