// The rules behind ctk_fit_pose (include/ctk.h, "fit pose"), restated ONCE for the device kernel (pose.hip) and for a host build of the
// same text (tests/test_pose_host.py compiles this header with g++ and compares it with the numpy restatement of
// tests/pose_reference.py -- no GPU needed to pin it).  Decisions are INTEGER or single comparisons; everything in double is ONE IEEE
// operation per step in the order written here (compile with -ffp-contract=off); no library square root is taken anywhere
// (plane_math.h:28 has the reason: the reciprocal root below is products and differences only); no sum depends on the order of
// accumulation: the device, the host build and numpy agree on every bit.  What is not named here is ctk_fit_epipolar's
// (epipolar_math.h), ctk_fit_planes' (plane_math.h) and ctk_fit_motion's (motion_math.h): positions in 1/16 pixel (ctk_motion_quant),
// the pair rule with its three source forms (ctk_objects_source), ctk_plane_fix and ctk_plane_solve, all reused without change.
//
// P = source, Q = frame f, 1/16 pixel; (Q, 1)^T F (P, 1) = 0 as ctk_fit_epipolar writes F.  The pose maps source-camera coordinates to
// frame-f coordinates, X_f = R X_s + t with |t| = 1, so E = [t]x R.  fx, fy, cx, cy: a pinhole camera in raw-video pixels, the same on
// both frames; the floats are widened to double once.  dot(a, b) = (a0 b0 + a1 b1) + a2 b2; cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2,
// a0 b1 - a1 b0), two products and one difference per component; [a]x M = the matrix whose column c is cross(a, column c of M).
//   fit list    the M correspondences whose input label byte is 1 and whose mask byte is nonzero (or no mask), in ascending n.
//   rays        x = ((Px / 16 - cx) / fx, (Py / 16 - cy) / fy, 1), y likewise from Q: an exact scaling, a difference, a division.
//   E           from the float32 matrix F: no fit when all nine entries are zero (epipolar's no-fit row) or one is not finite.
//               G = F K: G[r][0] = F[r][0] fx, G[r][1] = F[r][1] fy, G[r][2] = (F[r][0] cx + F[r][1] cy) + F[r][2];
//               E = K^T G: E[0][c] = fx G[0][c], E[1][c] = fy G[1][c], E[2][c] = (cx G[0][c] + cy G[1][c]) + G[2][c]; every entry is
//               then divided by the entry of largest magnitude (the lowest index on ties); an entry that is then not finite: no fit.
//   rsqrt       of a > 0, finite: a = m 2^ex by frexp, m in [0.5, 1); ex odd: m = 2 m, ex = ex - 1, so that m lies in [0.5, 2) and ex
//               is even (all exact).  y = 1; eight steps of y = y * (1.5 - (0.5 m) * (y * y)); the result is ldexp(y, -ex / 2).  It
//               lies within 4e-16 relative of the true value.
//   decompose   closed form, no SVD (Horn 1990).  A = E E^T (A[i][j] = dot(E[i], E[j])); h = ((A00 + A11) + A22) * 0.5; TT = h I - A
//               (off the diagonal: -A[i][j]), which equals t t^T up to E's scale.  i = the largest diagonal entry of TT, the lowest
//               index on ties; it must be > 0 and finite.  t0 = TT[i] * rsqrt(TT[i][i]); n0 = dot(t0, t0), which must be > 0 and
//               finite.  C = the cofactor matrix of E: row r = cross(E[r+1], E[r+2]), indices mod 3.  W = [t0]x E.
//               Ra = (C - W) / n0, Rb = (C + W) / n0, entry by entry.  tn = t0 * rsqrt(n0): the unit translation.
//               The four candidates are k = 0..3: (Ra, tn), (Ra, -tn), (Rb, tn), (Rb, -tn).
//   polar       every R is orthogonalised by four steps of R = 0.5 * R (3 I - R^T R): A[i][j] = dot(column i, column j);
//               B = 3 I - A (off the diagonal: -A[i][j]); R'[i][j] = dot(row i of R, column j of B) * 0.5.  Then
//               det = (R00 (R11 R22 - R12 R21) - R01 (R10 R22 - R12 R20)) + R02 (R10 R21 - R11 R20).  A candidate whose determinant is
//               not > 0 or not finite, or with an entry of R or tn whose magnitude exceeds the largest float32 (the steps diverge on
//               a matrix that is far from a rotation; the pose is written as float32), is skipped.
//   triangulate a correspondence under (R, t): a = R x; aa = dot(a, a), yy = dot(y, y), ay = dot(a, y), at = dot(a, t),
//               yt = dot(y, t); den = aa yy - ay ay; z_s = (ay yt - at yy) / den, z_f = (aa yt - ay at) / den: the least-squares
//               solution of z_s a + t = z_f y.  Where !(den > 0) both depths are +inf.
//   cheirality  each candidate counts the fit-list entries with z_s > 0 and z_f > 0 (integers); the largest count wins, the lowest k on
//               ties.  No candidate left: no fit.
//   refine      two Gauss-Newton rounds on the Sampson error over the fit list.  Per entry under (R, t): p = R x; c = cross(y, t);
//               e = cross(t, p) (= E x); r = dot(y, e); b0 = dot(column 0 of R, c), b1 = dot(column 1 of R, c) (= E^T y);
//               g = ((e0 e0 + e1 e1) + b0 b0) + b1 b1, epipolar's four-term gradient sum; Jw = cross(p, c); Jt = cross(p, y);
//               v = (Jw, Jt, r), seven numbers.  The entry takes part iff g > 0 and every v_i v_i <= 16 g (one product each side).
//               That cap bounds every |(v_i v_j) / g| by 16, so the 28 sums S_ij, i <= j, of ctk_plane_fix((v_i v_j) / g) -- a product,
//               a division, llrint(. 2^44) -- over at most 8192 entries stay below 16 * 2^44 * 2^13 = 2^61 in int64.  Their order: the
//               21 of the 6 x 6 matrix row by row (i <= j < 6), then S_06 .. S_56, then S_66.  n = the number of entries taking part
//               (an integer); an entry of the fit list that does not take part sets stats[3] bit 2.
//               The 8 x 8 system: N[i][j] = S_ij 2^-44 for i, j < 6; the gauge: N[3+i][3+j] = N[3+i][3+j] + (t_i t_j) n; N[6][6] =
//               N[7][7] = 1 and zero elsewhere; b[i] = -(S_i6 2^-44), b[6] = b[7] = 0; ctk_plane_solve gives (dw, dt).
//               Update: R' = polar(R + [dw]x R) (one sum per entry), u = t + dt, n2 = dot(u, u), t' = u * rsqrt(n2).  The round
//               fails -- its pose stays, stats[3] bit 0 / 1 -- when the solve fails, n2 is not > 0 or not finite, the determinant of
//               R' is not > 0 or not finite, or an entry of R' or t' exceeds the largest float32.
//   outputs     pose float32 [3,4] = (R | t), the (float) of the doubles.  depth float32 [N_out,2] = ((float)z_s, (float)z_f) under the
//               final pose, in units of the baseline, for EVERY correspondence, off the fit list too, negative as they come; a NaN is
//               written as the quiet NaN 0x7FC00000.  stats = (M, fit-list entries with z_s > 0 and z_f > 0 under the final pose,
//               the chosen k, bits).
//   no fit      F is no fit, M < min_points (8..8192), the decomposition fails, or no candidate is left: pose (I | 0), every
//               correspondence's depth the quiet NaN 0x7FC00000, stats = (M, 0, -1, 0).  A slot without a correspondence: NaN depths
//               in either case.
#pragma once
#include <math.h>
#include <stdint.h>

#include "epipolar_math.h"
#include "motion_math.h"
#include "plane_math.h"

#define CTK_POSE_MIN_POINTS 8
#define CTK_POSE_SUMS 28
#define CTK_POSE_ROUNDS 2
#define CTK_POSE_NAN_BITS 0x7FC00000u
#define CTK_POSE_FLT_MAX 3.4028234663852886e38  // the largest float32, as a double
#define CTK_POSE_SOLVE_DOUBLES CTK_PLANE_SOLVE_DOUBLES  // the same ctk_plane_solve layout

struct CtkPoseCam {
  double fx, fy, cx, cy;
};

// R row major, t
struct CtkPose {
  double R[9];
  double t[3];
};

CTK_MM_HD double ctk_pose_dot(const double* a, const double* b) {
  const double p0 = a[0] * b[0], p1 = a[1] * b[1], p2 = a[2] * b[2];
  const double s = p0 + p1;
  return s + p2;
}

CTK_MM_HD void ctk_pose_cross(const double* a, const double* b, double* o) {
  const double p0 = a[1] * b[2], q0 = a[2] * b[1], p1 = a[2] * b[0], q1 = a[0] * b[2], p2 = a[0] * b[1], q2 = a[1] * b[0];
  o[0] = p0 - q0, o[1] = p1 - q1, o[2] = p2 - q2;
}

// W = [a]x M, both row major
CTK_MM_HD void ctk_pose_skew_times(const double* a, const double* M, double* W) {
  for (int c = 0; c < 3; ++c) {
    const double col[3] = {M[c], M[3 + c], M[6 + c]};
    double o[3];
    ctk_pose_cross(a, col, o);
    W[c] = o[0], W[3 + c] = o[1], W[6 + c] = o[2];
  }
}

// the reciprocal square root of a > 0, finite
CTK_MM_HD double ctk_pose_rsqrt(double a) {
  int ex;
  double m = frexp(a, &ex);
  if (ex & 1) m = m * 2.0, ex -= 1;
  const double hm = 0.5 * m;
  double y = 1.0;
  for (int i = 0; i < 8; ++i) {
    const double yy = y * y;
    const double p = hm * yy;
    const double d = 1.5 - p;
    y = y * d;
  }
  return ldexp(y, -(ex / 2));
}

// a position in 1/16 pixel -> its ray
CTK_MM_HD void ctk_pose_ray(const CtkPoseCam& k, int px, int py, double* x) {
  const double u = (double)px / 16.0, v = (double)py / 16.0;
  const double du = u - k.cx, dv = v - k.cy;
  x[0] = du / k.fx, x[1] = dv / k.fy, x[2] = 1.0;
}

// the float32 pixel matrix of ctk_fit_epipolar -> a fit; E: nine doubles, the largest of magnitude 1
CTK_MM_HD bool ctk_pose_essential(const float* F, const CtkPoseCam& k, double* E) {
  bool zero = true, finite = true;
  double Fd[9], G[9];
  for (int i = 0; i < 9; ++i) {
    zero = zero && F[i] == 0.0f;
    finite = finite && fabsf(F[i]) <= 3.402823466e+38f;
    Fd[i] = (double)F[i];
  }
  for (int i = 0; i < 9; ++i) E[i] = 0.0;
  if (zero || !finite) return false;
  for (int r = 0; r < 3; ++r) {
    G[r * 3] = Fd[r * 3] * k.fx, G[r * 3 + 1] = Fd[r * 3 + 1] * k.fy;
    const double a = Fd[r * 3] * k.cx, b = Fd[r * 3 + 1] * k.cy;
    const double s = a + b;
    G[r * 3 + 2] = s + Fd[r * 3 + 2];
  }
  double U[9];
  for (int c = 0; c < 3; ++c) {
    U[c] = k.fx * G[c], U[3 + c] = k.fy * G[3 + c];
    const double a = k.cx * G[c], b = k.cy * G[3 + c];
    const double s = a + b;
    U[6 + c] = s + G[6 + c];
  }
  const double den = U[ctk_epi_largest(U, 9)];
  bool ok = true;
  for (int i = 0; i < 9; ++i) {
    E[i] = U[i] / den;
    ok = ok && ctk_plane_finite(E[i]);
  }
  return ok;
}

// four steps towards the nearest orthogonal matrix, in place -> the determinant
CTK_MM_HD double ctk_pose_polar(double* R) {
  for (int step = 0; step < 4; ++step) {
    double B[9], O[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        const double ci[3] = {R[i], R[3 + i], R[6 + i]}, cj[3] = {R[j], R[3 + j], R[6 + j]};
        const double a = ctk_pose_dot(ci, cj);
        B[i * 3 + j] = i == j ? 3.0 - a : -a;
      }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        const double cj[3] = {B[j], B[3 + j], B[6 + j]};
        O[i * 3 + j] = ctk_pose_dot(R + i * 3, cj) * 0.5;
      }
    for (int i = 0; i < 9; ++i) R[i] = O[i];
  }
  const double m0a = R[4] * R[8], m0b = R[5] * R[7], m1a = R[3] * R[8], m1b = R[5] * R[6], m2a = R[3] * R[7], m2b = R[4] * R[6];
  const double m0 = m0a - m0b, m1 = m1a - m1b, m2 = m2a - m2b;
  const double d0 = R[0] * m0, d1 = R[1] * m1, d2 = R[2] * m2;
  const double d01 = d0 - d1;
  return d01 + d2;
}

// an orthogonalised R with its determinant, and t -> the candidate stands
CTK_MM_HD bool ctk_pose_valid(const CtkPose& p, double det) {
  bool ok = det > 0.0 && ctk_plane_finite(det);
  for (int i = 0; i < 9; ++i) ok = ok && fabs(p.R[i]) <= CTK_POSE_FLT_MAX;
  for (int i = 0; i < 3; ++i) ok = ok && fabs(p.t[i]) <= CTK_POSE_FLT_MAX;
  return ok;
}

// E -> the decomposition stands; cand[0..3], ok[0..3]
CTK_MM_HD bool ctk_pose_decompose(const double* E, CtkPose* cand, bool* ok) {
  for (int k = 0; k < 4; ++k) {
    ok[k] = false;
    for (int i = 0; i < 9; ++i) cand[k].R[i] = i % 4 == 0 ? 1.0 : 0.0;
    for (int i = 0; i < 3; ++i) cand[k].t[i] = 0.0;
  }
  double A[9], TT[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[i * 3 + j] = ctk_pose_dot(E + i * 3, E + j * 3);
  const double tr01 = A[0] + A[4];
  const double tr = tr01 + A[8];
  const double h = tr * 0.5;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) TT[i * 3 + j] = i == j ? h - A[i * 3 + j] : -A[i * 3 + j];
  int i = 0;
  if (TT[4] > TT[i * 4]) i = 1;
  if (TT[8] > TT[i * 4]) i = 2;
  const double d = TT[i * 4];
  if (!(d > 0.0) || !ctk_plane_finite(d)) return false;
  const double s = ctk_pose_rsqrt(d);
  const double t0[3] = {TT[i * 3] * s, TT[i * 3 + 1] * s, TT[i * 3 + 2] * s};
  const double n0 = ctk_pose_dot(t0, t0);
  if (!(n0 > 0.0) || !ctk_plane_finite(n0)) return false;
  double C[9], W[9];
  for (int r = 0; r < 3; ++r) ctk_pose_cross(E + ((r + 1) % 3) * 3, E + ((r + 2) % 3) * 3, C + r * 3);
  ctk_pose_skew_times(t0, E, W);
  const double sn = ctk_pose_rsqrt(n0);
  const double tn[3] = {t0[0] * sn, t0[1] * sn, t0[2] * sn};
  for (int ab = 0; ab < 2; ++ab) {
    CtkPose p;
    for (int j = 0; j < 9; ++j) {
      const double m = ab == 0 ? C[j] - W[j] : C[j] + W[j];
      p.R[j] = m / n0;
    }
    const double det = ctk_pose_polar(p.R);
    for (int sg = 0; sg < 2; ++sg) {
      for (int j = 0; j < 3; ++j) p.t[j] = sg == 0 ? tn[j] : -tn[j];
      cand[ab * 2 + sg] = p;
      ok[ab * 2 + sg] = ctk_pose_valid(p, det);
    }
  }
  return true;
}

// the depths of a correspondence with rays x, y under a pose
CTK_MM_HD void ctk_pose_depths(const CtkPose& p, const double* x, const double* y, double* zs, double* zf) {
  const double a[3] = {ctk_pose_dot(p.R, x), ctk_pose_dot(p.R + 3, x), ctk_pose_dot(p.R + 6, x)};
  const double aa = ctk_pose_dot(a, a), yy = ctk_pose_dot(y, y), ay = ctk_pose_dot(a, y), at = ctk_pose_dot(a, p.t), yt = ctk_pose_dot(y, p.t);
  const double d0 = aa * yy, d1 = ay * ay;
  const double den = d0 - d1;
  if (!(den > 0.0)) {
    *zs = INFINITY, *zf = INFINITY;
    return;
  }
  const double s0 = ay * yt, s1 = at * yy, f0 = aa * yt, f1 = ay * at;
  const double ns = s0 - s1, nf = f0 - f1;
  *zs = ns / den, *zf = nf / den;
}

CTK_MM_HD bool ctk_pose_front(double zs, double zf) { return zs > 0.0 && zf > 0.0; }

CTK_MM_HD float ctk_pose_nan() {
  const uint32_t b = CTK_POSE_NAN_BITS;
  float f;
  __builtin_memcpy(&f, &b, sizeof f);
  return f;
}

// a depth as it is written
CTK_MM_HD float ctk_pose_depth_out(double z) { return z != z ? ctk_pose_nan() : (float)z; }

// the counts of the four candidates -> the winner, or -1
CTK_MM_HD int ctk_pose_choose(const int* count, const bool* ok) {
  int k = -1, best = -1;
  for (int i = 0; i < 4; ++i)
    if (ok[i] && count[i] > best) best = count[i], k = i;
  return k;
}

// one entry of the fit list under a pose -> takes part; then v: its seven numbers, *g: its gradient sum
CTK_MM_HD bool ctk_pose_entry(const CtkPose& P, const double* x, const double* y, double* v, double* g) {
  const double p[3] = {ctk_pose_dot(P.R, x), ctk_pose_dot(P.R + 3, x), ctk_pose_dot(P.R + 6, x)};
  double c[3], e[3];
  ctk_pose_cross(y, P.t, c);
  ctk_pose_cross(P.t, p, e);
  const double c0[3] = {P.R[0], P.R[3], P.R[6]}, c1[3] = {P.R[1], P.R[4], P.R[7]};
  const double b0 = ctk_pose_dot(c0, c), b1 = ctk_pose_dot(c1, c);
  const double g0 = e[0] * e[0], g1 = e[1] * e[1], g2 = b0 * b0, g3 = b1 * b1;
  const double g01 = g0 + g1;
  const double g012 = g01 + g2;
  const double gg = g012 + g3;
  ctk_pose_cross(p, c, v);
  ctk_pose_cross(p, y, v + 3);
  v[6] = ctk_pose_dot(y, e);
  *g = gg;
  bool in = gg > 0.0;
  const double cap = 16.0 * gg;
  for (int i = 0; i < 7; ++i) {
    const double q = v[i] * v[i];
    in = in && q <= cap;
  }
  return in;
}

// the terms of an entry that takes part, added to s (28 sums; every index a compile-time constant once unrolled)
CTK_MM_HD void ctk_pose_terms(const double* v, double g, int64_t* s) {
  int n = 0;
  CTK_EPI_UNROLL
  for (int i = 0; i < 6; ++i) {
    CTK_EPI_UNROLL
    for (int j = i; j < 6; ++j) {
      const double q = v[i] * v[j];
      s[n] += ctk_plane_fix(q / g);
      ++n;
    }
  }
  CTK_EPI_UNROLL
  for (int i = 0; i < 7; ++i) {
    const double q = v[i] * v[6];
    s[n] += ctk_plane_fix(q / g);
    ++n;
  }
}

// the place of S_ij, i <= j < 6, among the first 21 sums
CTK_MM_HD int ctk_pose_sum_index(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

// one round's update from its sums and the count n of the entries that took part; work: CTK_POSE_SOLVE_DOUBLES -> the round stands
CTK_MM_HD bool ctk_pose_update(const CtkPose& cur, const int64_t* s, int n, double* work, CtkPose* next) {
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
  const double dn = (double)n;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double tt = cur.t[i] * cur.t[j];
      const double gt = tt * dn;
      N[(3 + i) * 8 + 3 + j] = N[(3 + i) * 8 + 3 + j] + gt;
    }
  N[6 * 8 + 6] = 1.0, N[7 * 8 + 7] = 1.0;
  for (int i = 0; i < 6; ++i) b[i] = -((double)s[21 + i] * CTK_PLANE_UNFIX);
  b[6] = 0.0, b[7] = 0.0;
  if (!ctk_plane_solve(N, b, L, D, v, z, h)) return false;
  double W[9];
  ctk_pose_skew_times(h, cur.R, W);
  for (int i = 0; i < 9; ++i) next->R[i] = cur.R[i] + W[i];
  const double det = ctk_pose_polar(next->R);
  const double u[3] = {cur.t[0] + h[3], cur.t[1] + h[4], cur.t[2] + h[5]};
  const double n2 = ctk_pose_dot(u, u);
  if (!(n2 > 0.0) || !ctk_plane_finite(n2)) return false;
  const double sc = ctk_pose_rsqrt(n2);
  for (int i = 0; i < 3; ++i) next->t[i] = u[i] * sc;
  return ctk_pose_valid(*next, det);
}

// the pose as it is written: float32 [3,4] = (R | t)
CTK_MM_HD void ctk_pose_out(const CtkPose& p, float* o) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) o[r * 4 + c] = (float)p.R[r * 3 + c];
    o[r * 4 + 3] = (float)p.t[r];
  }
}

CTK_MM_HD void ctk_pose_identity(float* o) {
  for (int i = 0; i < 12; ++i) o[i] = i % 5 == 0 ? 1.0f : 0.0f;
}
