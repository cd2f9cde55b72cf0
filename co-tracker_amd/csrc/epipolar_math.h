// The rules behind ctk_fit_epipolar (include/ctk.h, "fit epipolar"), restated ONCE for the device kernel (epipolar.hip) and for a host
// build of the same text (tests/test_epipolar_host.py compiles this header with g++ and compares it with the numpy restatement of
// tests/epipolar_reference.py -- no GPU needed to pin it).  Admissibility is INTEGER arithmetic; everything in double is ONE IEEE
// operation per step in the order written here (compile with -ffp-contract=off), there is no square root, and no sum depends on the
// order of accumulation: the device, the host build and numpy agree on every bit.  What is not named here is ctk_fit_motion's
// (motion_math.h) and ctk_fit_planes' (plane_math.h): positions in 1/16 pixel, mix, the pair rule with its three source forms, T from
// tol, the key, ctk_plane_reach, ctk_plane_bits, ctk_plane_fix and ctk_plane_solve, which is reused without change.
//
// P = source, Q = frame f, 1/16 pixel.  The matrix F satisfies (Q, 1)^T F (P, 1) = 0; its nine entries are numbered row major,
// f_{3r+c} = F[r][c].  A matrix always comes with the anchor pair it is centred on and a scale e: its coordinates are
// u = (P_m - P_{i_0}) 2^-e and w = (Q_m - Q_{i_0}) 2^-e, both exact.
//   fit list    the M correspondences that may be sampled and refitted on: every correspondence, or with a mask those whose mask
//               byte is nonzero, in ascending n.  Every correspondence, masked or not, is classified and gets an error.
//   sample      hypothesis k of K over M >= 8: h_t = mix(seed ^ mix(f * 0x9e3779b9 + 8k + t)), t = 0..7; i_t = h_t % (M - t), then for
//               every earlier index in ASCENDING order: i_t += (i_t >= that index).  Eight distinct indices.
//   admissible  p_t = P_{i_t} - P_{i_0}, q_t likewise, t = 1..7 (|.| <= 2^18).  Admissible iff every |p_t|^2 and every |q_t|^2 is
//               >= base2' and >= 1.  base2' = ctk_motion_base2(min_base) = b * b, b = (int64)rintf(min_base * 16): min_base is a length
//               in pixels, b is that length in 1/16 pixel, and |p_t|^2 is a squared length in 1/16 pixel already -- every sample
//               point lies at least min_base pixels from the anchor on both frames.  (ctk_fit_planes compares the same number with
//               twice a triangle's area, which is a squared length too.)
//   matrix      the anchor pair is a correspondence at both origins, so f8 = 0 exactly.  e = the bit length of the largest |component|
//               of the seven p_t, q_t, at least 1; (x, y) = p_t 2^-e, (X, Y) = q_t 2^-e.  Row t - 1 of the 7 x 8 system A is
//               (X x, X y, X, Y x, Y y, Y, x, y): one product each.  Its null vector by Gaussian elimination with COMPLETE pivoting:
//               step s = 0..6: the pivot is the largest |A[r][c]| over r = s..6, c = s..7, scanned row by row with a strict ">" (ties:
//               the lowest row, then the lowest column); rows s and the pivot's swap, columns s and the pivot's swap in ALL seven
//               rows, and the column permutation records it; a pivot that is 0 or not finite ends the hypothesis; then for r = s+1..6:
//               m = A[r][s] / A[s][s], and for c = s+1..7: A[r][c] = A[r][c] - m * A[s][c] (a product, then a difference).
//               Back substitution with z_7 = 1: for s = 6..0: acc = A[s][7]; for c = s+1..6 ascending: acc = acc + A[s][c] * z_c;
//               z_s = (-acc) / A[s][s].  f_{perm[c]} = z_c.  j* = the index of the largest |f_j|, j = 0..7, the lowest on ties; every
//               f_j is divided by f_{j*}, which so becomes exactly 1.  An entry that is then not finite ends the hypothesis.
//   inlier      the Sampson test without a division or a root, for a matrix F of scale e:
//               a0 = (f0 ux + f1 uy) + f2, a1 = (f3 ux + f4 uy) + f5, a2 = (f6 ux + f7 uy) + f8            a = F (u, 1)
//               b0 = (f0 wx + f3 wy) + f6, b1 = (f1 wx + f4 wy) + f7                                       b = F^T (w, 1)
//               r = (wx a0 + wy a1) + a2;  g = ((a0 a0 + a1 a1) + b0 b0) + b1 b1;  Ts = T 2^-e (exact)
//               inlier iff g > 0 and r r <= (Ts Ts) g.
//   refit       of a matrix (F, e) with a chosen j* over the inliers under it among the fit list: e' = ctk_plane_bits of the largest
//               ctk_plane_reach of those inliers; (x, y, X, Y) in the scale e'; a = (X x, X y, X, Y x, Y y, Y, x, y, 1); the 45 sums
//               S_ij, i <= j, of llrint((a_i a_j) 2^44) in int64 (|a_i a_j| <= 1, n <= 8192: below 2^58).  S = (double)sum 2^-44; row
//               and column j* are deleted: N is the 8 x 8 rest, b = -(column j* without its own row); N h = b by ctk_plane_solve;
//               f_{j*} = 1 and the other eight are h in order.  The result has the scale e'.
//   rounds      round 1 refits the best hypothesis (its own j*).  If the solve fails the hypothesis' matrix is moved to the scale e' by
//               exact powers of two, s = 2^(e' - e): f0, f1, f3, f4 times s s; f2, f5, f6, f7 times s; f8 as it is -- stats[3] bit 0.
//               Round 2 refits the result of round 1 with j* = the index of its largest |f_j|, j = 0..8, the lowest on ties.  If that
//               solve fails the matrix of round 1 stays -- stats[3] bit 1.
//   outputs     under the final (F, e), for EVERY correspondence: the label is the inlier test; error = (float)(((r r) / g) 2^(2e-8)),
//               one division and one exact scaling: the squared Sampson distance in pixels^2.  Where !(g > 0): label 0, error +inf.
//   pixels      s = 2^(4-e), c = P_{i_0} / 16, k = Q_{i_0} / 16 (exact).  G = F S_P: G[r][0] = f_{3r} s, G[r][1] = f_{3r+1} s (exact),
//               G[r][2] = f_{3r+2} - (G[r][0] cx + G[r][1] cy).  F_px = S_Q^T G: row 0 = s G[0], row 1 = s G[1] (exact),
//               row 2 = G[2][c] - (row0[c] kx + row1[c] ky).  The output is (float) of that; it is not renormalised.
//   no fit      M < 8, no admissible hypothesis, or fewer than min_points (8..8192) inliers of the best: the matrix is all zero, every
//               correspondence has label 0 and error -1, stats = (M, 0, -1, 0).  A slot without a correspondence: label -1, error -1.
#pragma once
#include <math.h>
#include <stdint.h>

#include "plane_math.h"

#define CTK_EPI_SAMPLE 8
#define CTK_EPI_SUMS 45
#define CTK_EPI_MIN_POINTS 8

#if defined(__HIPCC__)
#define CTK_EPI_UNROLL _Pragma("unroll")
#else
#define CTK_EPI_UNROLL
#endif

// the sample of hypothesis k on frame f among M >= 8 correspondences: eight distinct indices
CTK_MM_HD void ctk_epi_sample(uint32_t seed, int f, int k, int M, int* i) {
  const uint32_t base = (uint32_t)f * 0x9e3779b9u + 8u * (uint32_t)k;
  int s[CTK_EPI_SAMPLE];  // the indices so far, ascending
  CTK_EPI_UNROLL
  for (int t = 0; t < CTK_EPI_SAMPLE; ++t) {
    int v = (int)(ctk_motion_mix(seed ^ ctk_motion_mix(base + (uint32_t)t)) % (uint32_t)(M - t));
    CTK_EPI_UNROLL
    for (int j = 0; j < t; ++j) v += v >= s[j] ? 1 : 0;
    i[t] = v;
    s[t] = v;
    CTK_EPI_UNROLL
    for (int j = t; j > 0; --j) {
      const int lo = s[j - 1] < s[j] ? s[j - 1] : s[j], hi = s[j - 1] < s[j] ? s[j] : s[j - 1];
      s[j - 1] = lo, s[j] = hi;
    }
  }
}

// A matrix, ready to test points against: the anchor pair, the scale, the nine entries; jstar: where a hypothesis has its 1
struct CtkEpiFit {
  int px, py, qx, qy;  // P_{i_0}, Q_{i_0}
  int e, jstar;
  double f[9];
};

// the index of the largest |f_j| over j = 0..n-1, the lowest on ties
CTK_MM_HD int ctk_epi_largest(const double* f, int n) {
  int j = 0;
  double m = fabs(f[0]);
  for (int i = 1; i < n; ++i) {
    const double a = fabs(f[i]);
    if (a > m) m = a, j = i;
  }
  return j;
}

// the largest |component| of u, w of a point against the anchor pair of h (ctk_plane_reach)
CTK_MM_HD int ctk_epi_reach(const CtkEpiFit& h, int px, int py, int qx, int qy) {
  CtkPlaneHyp a;
  a.px = h.px, a.py = h.py, a.qx = h.qx, a.qy = h.qy;
  return ctk_plane_reach(a, px, py, qx, qy);
}

// pt[t] = (Px, Py, Qx, Qy) of sample point t -> admissible
CTK_MM_HD bool ctk_epi_hyp(const int (*pt)[4], int64_t base2, CtkEpiFit* h) {
  h->px = pt[0][0], h->py = pt[0][1], h->qx = pt[0][2], h->qy = pt[0][3];
  h->e = 1, h->jstar = 0;
  CTK_EPI_UNROLL
  for (int i = 0; i < 9; ++i) h->f[i] = 0.0;
  bool ok = true;
  int mx = 0;
  CTK_EPI_UNROLL
  for (int t = 1; t < CTK_EPI_SAMPLE; ++t) {
    const int64_t px = (int64_t)pt[t][0] - pt[0][0], py = (int64_t)pt[t][1] - pt[0][1];
    const int64_t qx = (int64_t)pt[t][2] - pt[0][2], qy = (int64_t)pt[t][3] - pt[0][3];
    const int64_t dp = px * px + py * py, dq = qx * qx + qy * qy;
    ok = ok && dp >= base2 && dp >= 1 && dq >= base2 && dq >= 1;
    const int r = ctk_epi_reach(*h, pt[t][0], pt[t][1], pt[t][2], pt[t][3]);
    mx = r > mx ? r : mx;
  }
  if (!ok) return false;
  const int e = ctk_plane_bits(mx);
  h->e = e;
  const double sc = ldexp(1.0, -e);
  double A[7][8];
  CTK_EPI_UNROLL
  for (int t = 1; t < CTK_EPI_SAMPLE; ++t) {
    const double x = (double)(pt[t][0] - pt[0][0]) * sc, y = (double)(pt[t][1] - pt[0][1]) * sc;
    const double X = (double)(pt[t][2] - pt[0][2]) * sc, Y = (double)(pt[t][3] - pt[0][3]) * sc;
    A[t - 1][0] = X * x, A[t - 1][1] = X * y, A[t - 1][2] = X, A[t - 1][3] = Y * x, A[t - 1][4] = Y * y, A[t - 1][5] = Y;
    A[t - 1][6] = x, A[t - 1][7] = y;
  }
  int perm[8];
  CTK_EPI_UNROLL
  for (int c = 0; c < 8; ++c) perm[c] = c;
  // every index below is a compile-time constant once the loops are unrolled; what depends on data moves by selects
  CTK_EPI_UNROLL
  for (int s = 0; s < 7; ++s) {
    double best = -1.0;
    int pr = s, pc = s;
    CTK_EPI_UNROLL
    for (int r = s; r < 7; ++r) {
      CTK_EPI_UNROLL
      for (int c = s; c < 8; ++c) {
        const double a = fabs(A[r][c]);
        const bool up = a > best;
        best = up ? a : best, pr = up ? r : pr, pc = up ? c : pc;
      }
    }
    CTK_EPI_UNROLL
    for (int r = s + 1; r < 7; ++r) {
      const bool hit = pr == r;
      CTK_EPI_UNROLL
      for (int c = s; c < 8; ++c) {  // (the columns before s of these rows are read no more)
        const double u = A[s][c], v = A[r][c];
        A[s][c] = hit ? v : u, A[r][c] = hit ? u : v;
      }
    }
    CTK_EPI_UNROLL
    for (int c = s + 1; c < 8; ++c) {
      const bool hit = pc == c;
      CTK_EPI_UNROLL
      for (int r = 0; r < 7; ++r) {
        const double u = A[r][s], v = A[r][c];
        A[r][s] = hit ? v : u, A[r][c] = hit ? u : v;
      }
      const int u = perm[s], v = perm[c];
      perm[s] = hit ? v : u, perm[c] = hit ? u : v;
    }
    const double piv = A[s][s];
    ok = ok && piv != 0.0 && ctk_plane_finite(piv);  // (a NaN anywhere in the block may hide behind the pivot; the result is checked)
    CTK_EPI_UNROLL
    for (int r = s + 1; r < 7; ++r) {
      const double m = A[r][s] / piv;
      CTK_EPI_UNROLL
      for (int c = s + 1; c < 8; ++c) {
        const double t = m * A[s][c];
        A[r][c] = A[r][c] - t;
      }
    }
  }
  double z[8];
  z[7] = 1.0;
  CTK_EPI_UNROLL
  for (int s = 6; s >= 0; --s) {
    double acc = A[s][7];
    CTK_EPI_UNROLL
    for (int c = s + 1; c < 7; ++c) {
      const double t = A[s][c] * z[c];
      acc = acc + t;
    }
    z[s] = (-acc) / A[s][s];
  }
  double f[8];
  CTK_EPI_UNROLL
  for (int j = 0; j < 8; ++j) {
    double v = 0.0;
    CTK_EPI_UNROLL
    for (int c = 0; c < 8; ++c) v = perm[c] == j ? z[c] : v;
    f[j] = v;
  }
  int js = 0;
  double m = fabs(f[0]);
  CTK_EPI_UNROLL
  for (int j = 1; j < 8; ++j) {
    const double a = fabs(f[j]);
    const bool up = a > m;
    m = up ? a : m, js = up ? j : js;
  }
  double den = f[0];
  CTK_EPI_UNROLL
  for (int j = 1; j < 8; ++j) den = js == j ? f[j] : den;
  CTK_EPI_UNROLL
  for (int j = 0; j < 8; ++j) {
    const double v = f[j] / den;
    ok = ok && ctk_plane_finite(v);
    h->f[j] = v;
  }
  h->f[8] = 0.0;
  h->jstar = js;
  return ok;
}

// r and g of a point under a matrix: the squared Sampson distance is r r / g in the matrix' own scale
CTK_MM_HD void ctk_epi_residual(const CtkEpiFit& h, int px, int py, int qx, int qy, double* r, double* g) {
  const double sc = ldexp(1.0, -h.e);
  const double ux = (double)(px - h.px) * sc, uy = (double)(py - h.py) * sc, wx = (double)(qx - h.qx) * sc, wy = (double)(qy - h.qy) * sc;
  const double* f = h.f;
  const double a00 = f[0] * ux, a01 = f[1] * uy, a10 = f[3] * ux, a11 = f[4] * uy, a20 = f[6] * ux, a21 = f[7] * uy;
  const double a0s = a00 + a01, a1s = a10 + a11, a2s = a20 + a21;
  const double a0 = a0s + f[2], a1 = a1s + f[5], a2 = a2s + f[8];
  const double b00 = f[0] * wx, b01 = f[3] * wy, b10 = f[1] * wx, b11 = f[4] * wy;
  const double b0s = b00 + b01, b1s = b10 + b11;
  const double b0 = b0s + f[6], b1 = b1s + f[7];
  const double r0 = wx * a0, r1 = wy * a1;
  const double rs = r0 + r1;
  *r = rs + a2;
  const double g0 = a0 * a0, g1 = a1 * a1, g2 = b0 * b0, g3 = b1 * b1;
  const double g01 = g0 + g1;
  const double g012 = g01 + g2;
  *g = g012 + g3;
}

CTK_MM_HD bool ctk_epi_test(double r, double g, int e, double T) {
  const double Ts = T * ldexp(1.0, -e);
  const double rr = r * r, TT = Ts * Ts;
  const double bound = TT * g;
  return g > 0.0 && rr <= bound;
}

CTK_MM_HD bool ctk_epi_inlier(const CtkEpiFit& h, double T, int px, int py, int qx, int qy) {
  double r, g;
  ctk_epi_residual(h, px, py, qx, qy, &r, &g);
  return ctk_epi_test(r, g, h.e, T);
}

// the squared Sampson distance in pixels^2 of a point with (r, g) under a matrix of scale e; +inf where !(g > 0)
CTK_MM_HD float ctk_epi_error(double r, double g, int e) {
  if (!(g > 0.0)) return INFINITY;
  const double rr = r * r;
  const double q = rr / g;
  return (float)(q * ldexp(1.0, 2 * e - 8));
}

// the place of S_ij, i <= j, among the 45 sums
CTK_MM_HD int ctk_epi_sum_index(int i, int j) { return i * 9 - i * (i - 1) / 2 + (j - i); }

// one inlier's terms added to s (45 sums, every index a compile-time constant); e: ctk_plane_bits of the inliers' reach
CTK_MM_HD void ctk_epi_terms(const CtkEpiFit& h, int e, int px, int py, int qx, int qy, int64_t* s) {
  const double sc = ldexp(1.0, -e);
  const double x = (double)(px - h.px) * sc, y = (double)(py - h.py) * sc, X = (double)(qx - h.qx) * sc, Y = (double)(qy - h.qy) * sc;
  const double a[9] = {X * x, X * y, X, Y * x, Y * y, Y, x, y, 1.0};
  int n = 0;
  CTK_EPI_UNROLL
  for (int i = 0; i < 9; ++i) {
    CTK_EPI_UNROLL
    for (int j = i; j < 9; ++j) {
      s[n] += ctk_plane_fix(a[i] * a[j]);
      ++n;
    }
  }
}

// the sums and j* -> N (8 x 8, row major, both triangles) and b (8)
CTK_MM_HD void ctk_epi_system(const int64_t* s, int jstar, double* N, double* b) {
  for (int i = 0, ri = 0; i < 9; ++i) {
    if (i == jstar) continue;
    for (int j = 0, cj = 0; j < 9; ++j) {
      if (j == jstar) continue;
      const int lo = i < j ? i : j, hi = i < j ? j : i;
      N[ri * 8 + cj] = (double)s[ctk_epi_sum_index(lo, hi)] * CTK_PLANE_UNFIX;
      ++cj;
    }
    const int lo = i < jstar ? i : jstar, hi = i < jstar ? jstar : i;
    b[ri] = -((double)s[ctk_epi_sum_index(lo, hi)] * CTK_PLANE_UNFIX);
    ++ri;
  }
}

// a refit from its sums: src gives the anchor pair and j*; e: the scale of the sums; work: 64 + 8 + 64 + 8 + 8 + 8 + 8 doubles
// (N, b, L, D, v, z, h) -> solved; then *out is the refitted matrix in the scale e
CTK_MM_HD bool ctk_epi_refit(const CtkEpiFit& src, int jstar, int e, const int64_t* s, double* work, CtkEpiFit* out) {
  double* N = work;
  double* b = N + 64;
  double* L = b + 8;
  double* D = L + 64;
  double* v = D + 8;
  double* z = v + 8;
  double* h = z + 8;
  ctk_epi_system(s, jstar, N, b);
  if (!ctk_plane_solve(N, b, L, D, v, z, h)) return false;
  out->px = src.px, out->py = src.py, out->qx = src.qx, out->qy = src.qy;
  out->e = e, out->jstar = jstar;
  for (int i = 0, k = 0; i < 9; ++i) out->f[i] = i == jstar ? 1.0 : h[k++];
  return true;
}

// a matrix moved to another scale by exact powers of two
CTK_MM_HD void ctk_epi_rescale(const CtkEpiFit& src, int e, CtkEpiFit* out) {
  const double s = ldexp(1.0, e - src.e);
  const double ss = s * s;
  *out = src;
  out->e = e;
  out->f[0] = src.f[0] * ss, out->f[1] = src.f[1] * ss, out->f[3] = src.f[3] * ss, out->f[4] = src.f[4] * ss;
  out->f[2] = src.f[2] * s, out->f[5] = src.f[5] * s, out->f[6] = src.f[6] * s, out->f[7] = src.f[7] * s;
}

// a matrix -> float32 3 x 3 in pixels
CTK_MM_HD void ctk_epi_pixels(const CtkEpiFit& h, float* out) {
  const double s = ldexp(1.0, 4 - h.e);
  const double cx = (double)h.px / 16.0, cy = (double)h.py / 16.0, kx = (double)h.qx / 16.0, ky = (double)h.qy / 16.0;
  double G[9], O[9];
  for (int r = 0; r < 3; ++r) {
    G[r * 3] = h.f[r * 3] * s, G[r * 3 + 1] = h.f[r * 3 + 1] * s;
    const double a = G[r * 3] * cx, c = G[r * 3 + 1] * cy;
    const double t = a + c;
    G[r * 3 + 2] = h.f[r * 3 + 2] - t;
  }
  for (int c = 0; c < 3; ++c) {
    O[c] = s * G[c], O[3 + c] = s * G[3 + c];
    const double a = O[c] * kx, d = O[3 + c] * ky;
    const double t = a + d;
    O[6 + c] = G[6 + c] - t;
  }
  for (int i = 0; i < 9; ++i) out[i] = (float)O[i];
}
