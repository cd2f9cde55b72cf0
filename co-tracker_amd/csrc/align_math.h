// The rules behind ctk_fit_align (include/ctk.h, "fit align"), restated ONCE for the device kernel (align.hip) and for a host build of
// the same text (tests/test_align_host.py compiles this header with g++ and compares it with the numpy restatement of
// tests/align_reference.py -- no GPU needed to pin it).  Decisions are INTEGER or single comparisons; everything in double is ONE IEEE
// operation per step in the order written here (compile with -ffp-contract=off); no library square root and no trigonometry is taken
// anywhere (ctk_pose_rsqrt and ctk_pose_polar are the only ones); no sum depends on the order of accumulation: the device, the host
// build and numpy agree on every bit.  Reused without change: ctk_plane_sample, ctk_plane_fix, ctk_plane_solve (plane_math.h),
// ctk_pose_dot / _cross / _skew_times / _rsqrt / _polar / _valid (pose_math.h), ctk_resection_finite32 / _tol2 / _better
// (resection_math.h), ctk_p3p_cofactors (p3p_math.h), ctk_structure_gate2 (structure_math.h).
//
// Y ~ s R X + t with s > 0: X = a[n], Y = b[n], three floats each widened to double once.  (fx, fy, cx, cy): a pinhole camera of b's
// frame, in which the tolerance is stated.
//   correspondence  slot n is one iff valid_a[n] and valid_b[n] are nonzero, all six floats are finite with |v| <= 2^20
//               (CTK_PLANE_REACH; one comparison each, a NaN fails it) and Y_z > 0.
//   fit list    the correspondences whose mask byte is nonzero (no mask: all), in ascending n; the first CTK_RESECTION_LIST_MAX = 4096
//               of them take part (M of them), more set stats[3] bit 3.  Every correspondence is classified, listed or not.
//   sample      candidate k < K (`hypotheses`, 1..1024) takes the FIRST THREE of ctk_plane_sample(seed, 0, k, M, .); with M = 3, where
//               that sampler is not defined, every candidate is the entries (0, 1, 2).
//   candidate   (ctk_align_candidate) the sides e01 = P1 - P0, e02 = P2 - P0, e12 = P2 - P1 of both triangles;
//               da = (dot(e01, e01) + dot(e02, e02)) + dot(e12, e12) in a, db in b; either not > 0 or not finite skips the candidate;
//               s2 = db / da must be > 0 and finite; s = s2 * ctk_pose_rsqrt(s2).  The frames: A = [s e01, s e02, their cross product]
//               as columns from a (a product per component: with the sides scaled, B A^-1 is a rotation up to noise and the polar
//               steps converge for every s) and B = [e01, e02, their cross product] from b.  C = the cofactors of A,
//               det A = dot(A row 0, C row 0); det A not > 0, or det B not > 0 (a collinear or repeated triple in either set: p3p's
//               test), skips the candidate.  id = 1 / det A; M_ij = dot(B row i, C row j) id; R = ctk_pose_polar(M);
//               t_i = Y0_i - s dot(R row i, X0) (a dot, a product, a difference); the candidate stands iff ctk_pose_valid(R, t, det R)
//               and s <= the largest float32.
//   fixed       k = K is (1, I, 0).  stats[2] is in 0 .. K.
//   identical   every correspondence (beyond the mask and the cap too; there is at least one) has the same three floats in a and b
//               (==): only k = K is scored; stats[3] bit 5.  The rounds still run: under (1, I, 0) Z = X exactly (products by 1 and 0,
//               sums with 0), every residual is 0, the right-hand side is 0, ctk_plane_solve returns zero increments, and
//               s (1 + 0), polar(I + 0) = I and t + 0 leave the transform bit for bit.  Without this rule a sampled candidate that
//               also takes every entry would win the tie by its lower k with a rotation that is I only to the last bits.
//   apply       Z_i = s dot(R row i, X) + t_i (a dot, a product, a sum).
//   within      (ctk_align_within) Z_z > 0; nx = fx (Z_x Y_z - Y_x Z_z), ny = fy (Z_y Y_z - Y_y Z_z), w = Z_z Y_z:
//               nx nx + ny ny <= tol2 (w w) -- the squared pixel distance of the two projections against tol2 = (double)tol (double)tol
//               without a division or a root; and |Z_z - Y_z| <= dtol Y_z, one product and one comparison.  A NaN fails.
//   score       the number of fit-list entries within (tol, depth_tol): the largest wins, the lowest k on ties
//               (ctk_resection_better); no fit below min_points (3..8192), with M < 3, or with no candidate.
//   refit       CTK_ALIGN_ROUNDS = 3 Gauss-Newton rounds over the entries within (g tol, g depth_tol), g = 4, 2, 1
//               (ctk_structure_gate2; dtol = g (double)depth_tol), under the round's transform.  Seven parameters about b's camera
//               centre: Z' = (1 + d)(I + [w]x) Z + T, so s' = s (1 + d), R' = polar(R + [w]x R),
//               t' = ((t + cross(w, t)) + d t) + T.  The residual is what the score judges, each part in units of its tolerance up to
//               the common factor tol / fx: rx = u - ub and ry = (fy / fx)(v - vb), the two pixel differences, with (u, v) = (Z_x, Z_y)
//               / Z_z and (ub, vb) = (Y_x, Y_y) / Y_z; rz = (tol / (fx depth_tol)) (Z_z - Y_z) / Y_z, the relative depth difference
//               (ctk_align_weights: two divisions, once per call).  [Not (Z - Y) / Y_z taken as three numbers alike, the textbook
//               residual: noise along a point's ray has sideways components in 3-D, so with 0.5 % depth noise its converged float64
//               fit leaves points that agree to 0.3 px up to 8.5 px apart at 40 points and drops 84 of 560 unmoved ones at tol = 2
//               (tests/test_align_host.py::test_the_textbook_residual).]
//               e = the largest frexp exponent of Y_z over the round's entries (an integer maximum: the inliers' reach); T is solved
//               in units of 2^e.  Per entry: ia = 1 / Z_z, ib = 1 / Y_z, ha = ldexp(ia, e), hb = ldexp(ib, e) (exact); its three rows
//               of eight numbers, the gradient by (w, T 2^-e, d) and the residual:
//                 (-(u v), 1 + u u, -v, ha, 0, -(u ha), 0, rx)                  times q_x = 1/16
//                 (-(1 + v v), u v, u, 0, ha, -(v ha), 0, v - vb)               times q_y = (fy / fx) / 16
//                 (Z_y ib, -(Z_x ib), 0, 0, 0, hb, Z_z ib, (Z_z - Y_z) ib)      times q_z = (tol / (fx depth_tol)) / 16
//               (a scaling about the camera centre moves no projection: the scale's column is 0 in the pixel rows, and the depth
//               row fixes it).  The entry takes part iff every one of its 24 numbers x has x x <= 16 (a point nearer than 1/64 of
//               the reach, a ray beyond 82 degrees off the axis or a camera whose weights exceed these is left out; stats[3]
//               bit 2): every product is then at most 16, so the 36 sums of ctk_plane_fix(x_i x_j) -- the 28 of i <= j < 7 row by
//               row, the 7 of (i, 7), then (7, 7) -- over at most 4096 entries x 3 rows stay below 2^62 in int64.
//               The 8 x 8 system: N[i][j] = S_ij 2^-44 for i, j < 7, N[7][7] = 1 (the padded row), b[i] = -(S_i7 2^-44), b[7] = 0;
//               ctk_plane_solve gives (w, T 2^-e, d, 0); T = ldexp(., e).  The round fails -- its transform stays, stats[3] bit 1 --
//               with fewer than 3 entries taking part, when the solve fails, ctk_pose_valid(R', t') fails, or s' is not > 0 or
//               exceeds the largest float32.
//   outputs     sim float32 [3,4]: row r = ((float)(s R[r][c]), (float)t[r]); scale = (float)s.  Per slot: label -1 and error -1
//               without a correspondence; else under the final transform label 1 within (tol, depth_tol), 0 otherwise;
//               error = (float)((nx nx + ny ny) / (w w)), +inf where !(Z_z > 0) or the quotient is a NaN.
//               stats = (M, slots labelled 1, the winning k or -1, bits).
//   no fit      sim all zero, scale 0; label 0 and error -1 for every correspondence; stats = (M, 0, -1, bits).
#pragma once
#include <math.h>
#include <stdint.h>

#include "p3p_math.h"
#include "structure_math.h"

#define CTK_ALIGN_ROUNDS 3
#define CTK_ALIGN_MIN_POINTS 3
#define CTK_ALIGN_SUMS 36
#define CTK_ALIGN_SOLVE_MIN 3
#define CTK_ALIGN_BIT_ROUND 2
#define CTK_ALIGN_BIT_LEFT 4
#define CTK_ALIGN_NO_REACH (-100000)  // the reach of an empty set of entries

// Y ~ s R X + t
struct CtkAlign {
  double s;
  double R[9];
  double t[3];
};

CTK_MM_HD void ctk_align_eye(CtkAlign* c) {
  c->s = 1.0;
  for (int i = 0; i < 9; ++i) c->R[i] = i % 4 == 0 ? 1.0 : 0.0;
  for (int i = 0; i < 3; ++i) c->t[i] = 0.0;
}

CTK_MM_HD bool ctk_align_coord(float v) { return fabsf(v) <= (float)CTK_PLANE_REACH; }  // (a NaN fails the comparison)

// slot n of both sets -> a correspondence; X, Y: the doubles; *same: the six floats agree
CTK_MM_HD bool ctk_align_point(const float* a, int8_t valid_a, const float* b, int8_t valid_b, double* X, double* Y, bool* same) {
  bool ok = valid_a != 0 && valid_b != 0;
  for (int i = 0; i < 3; ++i) {
    X[i] = (double)a[i], Y[i] = (double)b[i];
    ok = ok && ctk_align_coord(a[i]) && ctk_align_coord(b[i]);
  }
  *same = a[0] == b[0] && a[1] == b[1] && a[2] == b[2];
  return ok && b[2] > 0.0f;
}

// the sample of candidate k among M >= 3 entries
CTK_MM_HD void ctk_align_sample(uint32_t seed, int k, int M, int* i) {
  if (M < 4) {
    i[0] = 0, i[1] = 1, i[2] = 2;
    return;
  }
  int idx[4];
  ctk_plane_sample(seed, 0, k, M, idx);
  i[0] = idx[0], i[1] = idx[1], i[2] = idx[2];
}

// the three sides of a triangle (P: nine doubles) -> the sum of their squared lengths
CTK_MM_HD double ctk_align_sides(const double* P, double* e01, double* e02) {
  double e12[3];
  for (int i = 0; i < 3; ++i) e01[i] = P[3 + i] - P[i], e02[i] = P[6 + i] - P[i], e12[i] = P[6 + i] - P[3 + i];
  const double d0 = ctk_pose_dot(e01, e01), d1 = ctk_pose_dot(e02, e02), d2 = ctk_pose_dot(e12, e12);
  const double d01 = d0 + d1;
  return d01 + d2;
}

// two sides -> the frame [e1, e2, cross(e1, e2)] as the columns of F, row major
CTK_MM_HD void ctk_align_frame(const double* e1, const double* e2, double* F) {
  double e3[3];
  ctk_pose_cross(e1, e2, e3);
  for (int i = 0; i < 3; ++i) F[i * 3] = e1[i], F[i * 3 + 1] = e2[i], F[i * 3 + 2] = e3[i];
}

// three entries of the fit list (X, Y: nine doubles each, three a point) -> the candidate stands; *c
CTK_MM_HD bool ctk_align_candidate(const double* X, const double* Y, CtkAlign* c) {
  ctk_align_eye(c);
  double a1[3], a2[3], b1[3], b2[3];
  const double da = ctk_align_sides(X, a1, a2), db = ctk_align_sides(Y, b1, b2);
  if (!(da > 0.0) || !ctk_plane_finite(da) || !(db > 0.0) || !ctk_plane_finite(db)) return false;
  const double s2 = db / da;
  if (!(s2 > 0.0) || !ctk_plane_finite(s2)) return false;
  CtkAlign w;
  w.s = s2 * ctk_pose_rsqrt(s2);
  for (int i = 0; i < 3; ++i) a1[i] = w.s * a1[i], a2[i] = w.s * a2[i];
  double A[9], B[9], C[9], CB[9];
  ctk_align_frame(a1, a2, A);
  ctk_align_frame(b1, b2, B);
  const double detA = ctk_p3p_cofactors(A, C), detB = ctk_p3p_cofactors(B, CB);
  if (!(detA > 0.0) || !(detB > 0.0)) return false;
  const double id = 1.0 / detA;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double n = ctk_pose_dot(B + i * 3, C + j * 3);
      w.R[i * 3 + j] = n * id;
    }
  const double det = ctk_pose_polar(w.R);
  for (int i = 0; i < 3; ++i) {
    const double n = ctk_pose_dot(w.R + i * 3, X);
    const double p = w.s * n;
    w.t[i] = Y[i] - p;
  }
  CtkPose q;
  for (int i = 0; i < 9; ++i) q.R[i] = w.R[i];
  for (int i = 0; i < 3; ++i) q.t[i] = w.t[i];
  if (!ctk_pose_valid(q, det) || !(w.s <= CTK_POSE_FLT_MAX)) return false;
  *c = w;
  return true;
}

// Z = s R X + t
CTK_MM_HD void ctk_align_apply(const CtkAlign& c, const double* X, double* Z) {
  for (int i = 0; i < 3; ++i) {
    const double d = ctk_pose_dot(c.R + i * 3, X);
    const double p = c.s * d;
    Z[i] = p + c.t[i];
  }
}

// the two sides of the pixel comparison: *num = nx nx + ny ny, *den = w w (the squared pixel distance is their quotient)
CTK_MM_HD void ctk_align_pixels(const CtkPoseCam& k, const double* Z, const double* Y, double* num, double* den) {
  const double ax = Z[0] * Y[2], bx = Y[0] * Z[2], ay = Z[1] * Y[2], by = Y[1] * Z[2];
  const double ex = ax - bx, ey = ay - by;
  const double nx = k.fx * ex, ny = k.fy * ey;
  const double qx = nx * nx, qy = ny * ny;
  *num = qx + qy;
  const double w = Z[2] * Y[2];
  *den = w * w;
}

CTK_MM_HD bool ctk_align_within(const CtkPoseCam& k, const double* Z, const double* Y, double tol2, double dtol) {
  if (!(Z[2] > 0.0)) return false;
  double num, den;
  ctk_align_pixels(k, Z, Y, &num, &den);
  const double lim = tol2 * den;
  const double d = Z[2] - Y[2];
  const double dl = dtol * Y[2];
  return num <= lim && fabs(d) <= dl;
}

// the error of a correspondence as it is written
CTK_MM_HD float ctk_align_error(const CtkPoseCam& k, const double* Z, const double* Y) {
  if (!(Z[2] > 0.0)) return INFINITY;
  double num, den;
  ctk_align_pixels(k, Z, Y, &num, &den);
  const double e = num / den;
  return e != e ? INFINITY : (float)e;
}

// the depth gate of round r
CTK_MM_HD double ctk_align_dgate(float depth_tol, int round) {
  const double g = round == 0 ? 4.0 : (round == 1 ? 2.0 : 1.0);
  return g * (double)depth_tol;
}

// the reach of one entry: the frexp exponent of Y_z > 0
CTK_MM_HD int ctk_align_reach(const double* Y) {
  int ex;
  (void)frexp(Y[2], &ex);
  return ex;
}

// the weights of the three rows of an entry: the residual's components in units of their tolerances, up to the common factor tol / fx
struct CtkAlignWeights {
  double y, z;  // (the x row has weight 1)
};

CTK_MM_HD CtkAlignWeights ctk_align_weights(const CtkPoseCam& k, float tol, float depth_tol) {
  CtkAlignWeights w;
  w.y = k.fy / k.fx;
  const double p = k.fx * (double)depth_tol;
  w.z = (double)tol / p;
  return w;
}

// an entry within the round's gates under reach e -> takes part; v: its three rows of eight numbers
CTK_MM_HD bool ctk_align_entry(const CtkAlignWeights& w, const double* Z, const double* Y, int e, double* v) {
  const double ia = 1.0 / Z[2], ib = 1.0 / Y[2];
  const double ha = ldexp(ia, e), hb = ldexp(ib, e);
  const double qx = 0.0625, qy = 0.0625 * w.y, qz = 0.0625 * w.z;
  const double u = Z[0] * ia, t = Z[1] * ia, ub = Y[0] * ib, tb = Y[1] * ib;
  const double uu = u * u, ut = u * t, tt = t * t;
  const double cu = 1.0 + uu, ct = 1.0 + tt, hu = u * ha, ht = t * ha;
  const double rx = u - ub, ry = t - tb, dz = Z[2] - Y[2];
  const double a0 = Z[0] * ib, a1 = Z[1] * ib, a2 = Z[2] * ib, rz = dz * ib;
  const double rows[24] = {-(ut * qx), cu * qx,    -(t * qx), ha * qx, 0.0,     -(hu * qx), 0.0,     rx * qx,  //
                           -(ct * qy), ut * qy,    u * qy,    0.0,     ha * qy, -(ht * qy), 0.0,     ry * qy,  //
                           a1 * qz,    -(a0 * qz), 0.0,       0.0,     0.0,     hb * qz,    a2 * qz, rz * qz};
  bool in = true;
  for (int i = 0; i < 24; ++i) {
    v[i] = rows[i];
    in = in && rows[i] * rows[i] <= 16.0;
  }
  return in;
}

// the terms of one row of an entry that takes part, added to s (36 sums)
CTK_MM_HD void ctk_align_terms(const double* v, int64_t* s) {
  int n = 0;
  CTK_EPI_UNROLL
  for (int i = 0; i < 7; ++i) {
    CTK_EPI_UNROLL
    for (int j = i; j < 7; ++j) {
      s[n] += ctk_plane_fix(v[i] * v[j]);
      ++n;
    }
  }
  CTK_EPI_UNROLL
  for (int i = 0; i < 8; ++i) {
    s[n] += ctk_plane_fix(v[i] * v[7]);
    ++n;
  }
}

// the place of S_ij, i <= j < 7, among the first 28 sums
CTK_MM_HD int ctk_align_sum_index(int i, int j) { return i * 7 - i * (i - 1) / 2 + (j - i); }

// one round's update from its sums, the count n of the entries that took part and their reach e; work: CTK_POSE_SOLVE_DOUBLES
// -> the round stands
CTK_MM_HD bool ctk_align_update(const CtkAlign& cur, const int64_t* s, int n, int e, double* work, CtkAlign* next) {
  if (n < CTK_ALIGN_SOLVE_MIN) return false;
  double* N = work;
  double* b = N + 64;
  double* L = b + 8;
  double* D = L + 64;
  double* v = D + 8;
  double* z = v + 8;
  double* h = z + 8;
  for (int i = 0; i < 64; ++i) N[i] = 0.0;
  for (int i = 0; i < 7; ++i)
    for (int j = 0; j < 7; ++j) {
      const int lo = i < j ? i : j, hi = i < j ? j : i;
      N[i * 8 + j] = (double)s[ctk_align_sum_index(lo, hi)] * CTK_PLANE_UNFIX;
    }
  N[7 * 8 + 7] = 1.0;
  for (int i = 0; i < 7; ++i) b[i] = -((double)s[28 + i] * CTK_PLANE_UNFIX);
  b[7] = 0.0;
  if (!ctk_plane_solve(N, b, L, D, v, z, h)) return false;
  double W[9], wt[3];
  ctk_pose_skew_times(h, cur.R, W);
  CtkPose q;
  for (int i = 0; i < 9; ++i) q.R[i] = cur.R[i] + W[i];
  const double det = ctk_pose_polar(q.R);
  ctk_pose_cross(h, cur.t, wt);
  for (int i = 0; i < 3; ++i) {
    const double t0 = cur.t[i] + wt[i];
    const double dt = h[6] * cur.t[i];
    const double t1 = t0 + dt;
    q.t[i] = t1 + ldexp(h[3 + i], e);
  }
  const double o = 1.0 + h[6];
  next->s = cur.s * o;
  for (int i = 0; i < 9; ++i) next->R[i] = q.R[i];
  for (int i = 0; i < 3; ++i) next->t[i] = q.t[i];
  return ctk_pose_valid(q, det) && next->s > 0.0 && next->s <= CTK_POSE_FLT_MAX;
}

// the transform as it is written: sim float32 [3,4] and scale
CTK_MM_HD void ctk_align_out(const CtkAlign& c, float* sim, float* scale) {
  for (int r = 0; r < 3; ++r) {
    for (int j = 0; j < 3; ++j) {
      const double p = c.s * c.R[r * 3 + j];
      sim[r * 4 + j] = (float)p;
    }
    sim[r * 4 + 3] = (float)c.t[r];
  }
  *scale = (float)c.s;
}
