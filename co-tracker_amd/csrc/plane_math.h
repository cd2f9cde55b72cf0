// The rules behind ctk_fit_planes and ctk_warp_planes (include/ctk.h, "fit planes / warp planes"), restated ONCE for the device kernels
// (planes.hip, warp_planes.hip) and for a host build of the same text (tests/test_planes_host.py compiles this header with g++ and
// compares it with the numpy restatement of tests/planes_reference.py -- no GPU needed to pin it).  Admissibility is INTEGER arithmetic;
// everything in double is ONE IEEE operation per step in the order written here (compile with -ffp-contract=off): the device, the host
// build and numpy agree on every bit.  What is not named here is ctk_fit_objects' (objects_math.h) and ctk_fit_motion's
// (motion_math.h): positions, mix, the pair rule, the lists, the seed of a round, key, acceptance, the labels.
//
// Fit.  P = source, Q = frame f, 1/16 pixel; with inverse = 1 the two swap roles after staging (the matrix then maps frame f onto the
// source frame; no matrix is inverted anywhere).  The box is over the inliers' positions on frame f either way.
//   sample      hypothesis k of K over a list of M >= 4: h_t = mix(seed_r ^ mix(f * 0x9e3779b9 + 4k + t)), t = 0..3;
//               i_t = h_t % (M - t), then for every earlier index e in ASCENDING order: i_t += (i_t >= e).  Four distinct indices.
//   admissible  p_t = P_{i_t} - P_{i_0}, q_t likewise (|.| <= 2^18).  d_abc = (p_b - p_a) x (p_c - p_a) for abc = 123, 023, 013, 012
//               in int64 (|d| <= 2^37), e_abc of the q likewise.  Admissible iff every |d| and every |e| is >= base2 and >= 1 and every
//               d has the sign of its e: no three sample points near a line, and the quad keeps its orientation.
//   matrix      on centred homogeneous (x, y, 1): l = (d_023, -d_013, d_012); B_P[r][c] = (double)l_c * (double)(x_c, y_c, 1)_r for
//               the sample points c = 1, 2, 3; B_Q from the e and q likewise.  A = adj(B_P):
//               A[i][j] = B[j+1][i+1] B[j+2][i+2] - B[j+1][i+2] B[j+2][i+1] (indices mod 3; two products, one difference);
//               H'[i][j] = (B_Q[i][0] A[0][j] + B_Q[i][1] A[1][j]) + B_Q[i][2] A[2][j]; h = H' / H'[2][2], nine divisions.  The hypothesis
//               is inadmissible if an entry is then not finite.  No pivoting, no branch on data order.
//   inlier      u = P_m - P_{i_0}, w = Q_m - Q_{i_0} as doubles (exact): X = (h00 ux + h01 uy) + h02, Y and Z likewise;
//               inlier iff Z > 0 and |X - wx Z| <= T Z and |Y - wy Z| <= T Z, T = (double)ctk_motion_tol(tol).
//   refit       over the inliers of the best: mx = max |u|, |w| over their components (an integer max), e = bit length of mx, at least
//               1; x = ux 2^-e, y = uy 2^-e, X = wx 2^-e, Y = wy 2^-e (exact, inside (-1, 1)).  Least squares for (h00 .. h21) with
//               h22 = 1, two equations per point: x h00 + y h01 + h02 - xX h20 - yX h21 = X and its twin for Y.  The 23 sums of the
//               normal equations (ctk_plane_terms: the products in the order written there) are each sum llrint(t * 2^44) in int64
//               (|t| <= 2, n <= 8192: below 2^59), so their value does not depend on the order of accumulation.  Then S = (double)sum
//               * 2^-44, the 8 x 8 system N h = b (ctk_plane_system), solved by the square-root-free Cholesky N = L D L^T in the loop
//               order of ctk_plane_solve -- NOT the square-root form: a division is one IEEE operation everywhere, a square root is
//               not promised to be.  A pivot that is not > 0 or not finite, or a solution that is not finite, falls back to the best
//               hypothesis' own matrix (stats[3] = 1).
//   pixels      centred matrix Hc with sigma = 2^(4 - e) (the fall-back: sigma = 16, e = 0):
//               G = [[h00, h01, h02 / sigma], [h10, h11, h12 / sigma], [h20 sigma, h21 sigma, h22]] (exact);
//               c = P_{i_0} / 16, k = Q_{i_0} / 16 (exact); M[r][2] = G[r][2] - (G[r][0] cx + G[r][1] cy), columns 0 and 1 as in G;
//               out[0][c] = M[0][c] + kx M[2][c], out[1][c] = M[1][c] + ky M[2][c], out[2][c] = M[2][c]; the result is (float) of
//               that.  It is not re-normalised: it is the matrix whose centred form has h22 = 1.
//
// Warp.  matrices[j] (float32 3 x 3 -> double) maps an OUTPUT pixel to a SOURCE position:
//   coordinate  Xh = (m00 x + m01 y) + m02, Yh and Zh likewise.  The pixel is OUTSIDE iff the matrix has a non-finite entry, or
//               !(Zh > 0), or with r = 1.0 / Zh, sx = Xh r, sy = Yh r: !(|sx| <= 1048576 && |sy| <= 1048576).  Otherwise
//               X = llrint(sx * 256.0), ix = X >> 8, fx = X & 255 (Y likewise); the taps and the blend are ctk_warp_frames'.
//   borders     CTK_WARP_FILL, CTK_WARP_EDGE as in ctk_warp_frames; an outside pixel takes `fill` under both.  CTK_WARP_KEEP: a pixel
//               that is outside, or that has one of its four taps outside the source, is not written.
#pragma once
#include <math.h>
#include <stdint.h>

#include "objects_math.h"
#include "warp_math.h"

#define CTK_PLANES_MAX 16
#define CTK_WARP_KEEP 2
#define CTK_PLANE_FIX 17592186044416.0         // 2^44
#define CTK_PLANE_UNFIX 5.6843418860808015e-14  // 2^-44
#define CTK_PLANE_REACH 1048576.0
#define CTK_PLANE_DBL_MAX 1.7976931348623157e308

CTK_MM_HD bool ctk_plane_finite(double v) { return fabs(v) <= CTK_PLANE_DBL_MAX; }  // (a NaN fails the comparison)

// the sample of hypothesis k on frame f among M >= 4 correspondences: four distinct indices
CTK_MM_HD void ctk_plane_sample(uint32_t seed, int f, int k, int M, int* i) {
  const uint32_t base = (uint32_t)f * 0x9e3779b9u + 4u * (uint32_t)k;
  const int v0 = (int)(ctk_motion_mix(seed ^ ctk_motion_mix(base)) % (uint32_t)M);
  int v1 = (int)(ctk_motion_mix(seed ^ ctk_motion_mix(base + 1u)) % (uint32_t)(M - 1));
  v1 += v1 >= v0 ? 1 : 0;
  const int a1 = v0 < v1 ? v0 : v1, b1 = v0 < v1 ? v1 : v0;
  int v2 = (int)(ctk_motion_mix(seed ^ ctk_motion_mix(base + 2u)) % (uint32_t)(M - 2));
  v2 += v2 >= a1 ? 1 : 0;
  v2 += v2 >= b1 ? 1 : 0;
  const int a2 = v2 < a1 ? v2 : a1, c2 = v2 > b1 ? v2 : b1, b2 = a1 + b1 + v2 - a2 - c2;
  int v3 = (int)(ctk_motion_mix(seed ^ ctk_motion_mix(base + 3u)) % (uint32_t)(M - 3));
  v3 += v3 >= a2 ? 1 : 0;
  v3 += v3 >= b2 ? 1 : 0;
  v3 += v3 >= c2 ? 1 : 0;
  i[0] = v0, i[1] = v1, i[2] = v2, i[3] = v3;
}

// A hypothesis, ready to test points against: the anchor pair and the centred matrix (h[8] = 1), 1/16 pixel.
struct CtkPlaneHyp {
  int px, py, qx, qy;  // P_{i_0}, Q_{i_0}
  double h[9];
};

CTK_MM_HD int64_t ctk_plane_cross(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t cx, int64_t cy) {
  return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

// the four triangle determinants of the centred sample (x[0] = y[0] = 0): d[0..3] = d_123, d_023, d_013, d_012
CTK_MM_HD void ctk_plane_dets(const int64_t* x, const int64_t* y, int64_t* d) {
  d[0] = ctk_plane_cross(x[1], y[1], x[2], y[2], x[3], y[3]);
  d[1] = ctk_plane_cross(x[0], y[0], x[2], y[2], x[3], y[3]);
  d[2] = ctk_plane_cross(x[0], y[0], x[1], y[1], x[3], y[3]);
  d[3] = ctk_plane_cross(x[0], y[0], x[1], y[1], x[2], y[2]);
}

CTK_MM_HD void ctk_plane_basis(const int64_t* x, const int64_t* y, const int64_t* d, double* B) {
  const double l[3] = {(double)d[1], (double)-d[2], (double)d[3]};
  for (int c = 0; c < 3; ++c) {
    B[c] = l[c] * (double)x[c + 1];
    B[3 + c] = l[c] * (double)y[c + 1];
    B[6 + c] = l[c] * 1.0;
  }
}

// pt[t] = (Px, Py, Qx, Qy) of sample point t -> admissible
CTK_MM_HD bool ctk_plane_hyp(const int (*pt)[4], int64_t base2, CtkPlaneHyp* h) {
  h->px = pt[0][0], h->py = pt[0][1], h->qx = pt[0][2], h->qy = pt[0][3];
  int64_t px[4], py[4], qx[4], qy[4], d[4], e[4];
  for (int t = 0; t < 4; ++t) {
    px[t] = (int64_t)pt[t][0] - pt[0][0], py[t] = (int64_t)pt[t][1] - pt[0][1];
    qx[t] = (int64_t)pt[t][2] - pt[0][2], qy[t] = (int64_t)pt[t][3] - pt[0][3];
  }
  ctk_plane_dets(px, py, d);
  ctk_plane_dets(qx, qy, e);
  bool ok = true;
  for (int t = 0; t < 4; ++t) {
    const int64_t ad = d[t] < 0 ? -d[t] : d[t], ae = e[t] < 0 ? -e[t] : e[t];
    ok = ok && ad >= base2 && ad >= 1 && ae >= base2 && ae >= 1 && (d[t] > 0) == (e[t] > 0);
  }
  for (int i = 0; i < 9; ++i) h->h[i] = i % 4 == 0 ? 1.0 : 0.0;
  if (!ok) return false;
  double BP[9], BQ[9], A[9], H[9];
  ctk_plane_basis(px, py, d, BP);
  ctk_plane_basis(qx, qy, e, BQ);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const int j1 = (j + 1) % 3, j2 = (j + 2) % 3, i1 = (i + 1) % 3, i2 = (i + 2) % 3;
      const double t1 = BP[j1 * 3 + i1] * BP[j2 * 3 + i2], t2 = BP[j1 * 3 + i2] * BP[j2 * 3 + i1];
      A[i * 3 + j] = t1 - t2;
    }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double t0 = BQ[i * 3] * A[j], t1 = BQ[i * 3 + 1] * A[3 + j], t2 = BQ[i * 3 + 2] * A[6 + j];
      const double s01 = t0 + t1;
      H[i * 3 + j] = s01 + t2;
    }
  const double den = H[8];
  for (int i = 0; i < 9; ++i) {
    const double v = H[i] / den;
    ok = ok && ctk_plane_finite(v);
    h->h[i] = v;
  }
  return ok;
}

CTK_MM_HD bool ctk_plane_inlier(const CtkPlaneHyp& h, double T, int px, int py, int qx, int qy) {
  const double ux = (double)(px - h.px), uy = (double)(py - h.py), wx = (double)(qx - h.qx), wy = (double)(qy - h.qy);
  const double x0 = h.h[0] * ux, x1 = h.h[1] * uy, y0 = h.h[3] * ux, y1 = h.h[4] * uy, z0 = h.h[6] * ux, z1 = h.h[7] * uy;
  const double xs = x0 + x1, ys = y0 + y1, zs = z0 + z1;
  const double X = xs + h.h[2], Y = ys + h.h[5], Z = zs + h.h[8];
  if (!(Z > 0.0)) return false;
  const double TZ = T * Z, ax = wx * Z, ay = wy * Z;
  const double rx = X - ax, ry = Y - ay;
  return fabs(rx) <= TZ && fabs(ry) <= TZ;
}

// the largest |component| of u, w of a point against the anchor pair of h
CTK_MM_HD int ctk_plane_reach(const CtkPlaneHyp& h, int px, int py, int qx, int qy) {
  int m = 0;
  const int v[4] = {px - h.px, py - h.py, qx - h.qx, qy - h.qy};
  for (int i = 0; i < 4; ++i) {
    const int a = v[i] < 0 ? -v[i] : v[i];
    m = a > m ? a : m;
  }
  return m;
}

// the bit length of mx >= 0, at least 1: mx < 2^e
CTK_MM_HD int ctk_plane_bits(int mx) {
  int e = 1;
  while (((int64_t)1 << e) <= (int64_t)mx) ++e;
  return e;
}

// the 23 sums of the refit, in this order (U, V: the destination's X, Y; R = U^2 + V^2)
enum {
  CTK_PS_N = 0, CTK_PS_X, CTK_PS_Y, CTK_PS_XX, CTK_PS_XY, CTK_PS_YY, CTK_PS_U, CTK_PS_V, CTK_PS_XU, CTK_PS_YU, CTK_PS_XV, CTK_PS_YV,
  CTK_PS_XXU, CTK_PS_XYU, CTK_PS_YYU, CTK_PS_XXV, CTK_PS_XYV, CTK_PS_YYV, CTK_PS_XXR, CTK_PS_XYR, CTK_PS_YYR, CTK_PS_XR, CTK_PS_YR,
  CTK_PS_COUNT
};

CTK_MM_HD int64_t ctk_plane_fix(double t) { return (int64_t)llrint(t * CTK_PLANE_FIX); }

// one inlier's terms added to s; e: ctk_plane_bits of the inliers' reach
CTK_MM_HD void ctk_plane_terms(const CtkPlaneHyp& h, int e, int px, int py, int qx, int qy, int64_t* s) {
  const double sc = ldexp(1.0, -e);
  const double x = (double)(px - h.px) * sc, y = (double)(py - h.py) * sc, U = (double)(qx - h.qx) * sc, V = (double)(qy - h.qy) * sc;
  const double xx = x * x, xy = x * y, yy = y * y, uu = U * U, vv = V * V;
  const double R = uu + vv;
  s[CTK_PS_N] += ctk_plane_fix(1.0);
  s[CTK_PS_X] += ctk_plane_fix(x), s[CTK_PS_Y] += ctk_plane_fix(y);
  s[CTK_PS_XX] += ctk_plane_fix(xx), s[CTK_PS_XY] += ctk_plane_fix(xy), s[CTK_PS_YY] += ctk_plane_fix(yy);
  s[CTK_PS_U] += ctk_plane_fix(U), s[CTK_PS_V] += ctk_plane_fix(V);
  s[CTK_PS_XU] += ctk_plane_fix(x * U), s[CTK_PS_YU] += ctk_plane_fix(y * U);
  s[CTK_PS_XV] += ctk_plane_fix(x * V), s[CTK_PS_YV] += ctk_plane_fix(y * V);
  s[CTK_PS_XXU] += ctk_plane_fix(xx * U), s[CTK_PS_XYU] += ctk_plane_fix(xy * U), s[CTK_PS_YYU] += ctk_plane_fix(yy * U);
  s[CTK_PS_XXV] += ctk_plane_fix(xx * V), s[CTK_PS_XYV] += ctk_plane_fix(xy * V), s[CTK_PS_YYV] += ctk_plane_fix(yy * V);
  s[CTK_PS_XXR] += ctk_plane_fix(xx * R), s[CTK_PS_XYR] += ctk_plane_fix(xy * R), s[CTK_PS_YYR] += ctk_plane_fix(yy * R);
  s[CTK_PS_XR] += ctk_plane_fix(x * R), s[CTK_PS_YR] += ctk_plane_fix(y * R);
}

// the sums -> N (8 x 8, row major, both triangles) and b (8)
CTK_MM_HD void ctk_plane_system(const int64_t* s, double* N, double* b) {
  double S[CTK_PS_COUNT];
  for (int i = 0; i < CTK_PS_COUNT; ++i) S[i] = (double)s[i] * CTK_PLANE_UNFIX;
  for (int i = 0; i < 64; ++i) N[i] = 0.0;
  for (int o = 0; o < 6; o += 3) {
    N[(o + 0) * 8 + o + 0] = S[CTK_PS_XX], N[(o + 0) * 8 + o + 1] = S[CTK_PS_XY], N[(o + 0) * 8 + o + 2] = S[CTK_PS_X];
    N[(o + 1) * 8 + o + 1] = S[CTK_PS_YY], N[(o + 1) * 8 + o + 2] = S[CTK_PS_Y];
    N[(o + 2) * 8 + o + 2] = S[CTK_PS_N];
  }
  N[0 * 8 + 6] = -S[CTK_PS_XXU], N[0 * 8 + 7] = -S[CTK_PS_XYU];
  N[1 * 8 + 6] = -S[CTK_PS_XYU], N[1 * 8 + 7] = -S[CTK_PS_YYU];
  N[2 * 8 + 6] = -S[CTK_PS_XU], N[2 * 8 + 7] = -S[CTK_PS_YU];
  N[3 * 8 + 6] = -S[CTK_PS_XXV], N[3 * 8 + 7] = -S[CTK_PS_XYV];
  N[4 * 8 + 6] = -S[CTK_PS_XYV], N[4 * 8 + 7] = -S[CTK_PS_YYV];
  N[5 * 8 + 6] = -S[CTK_PS_XV], N[5 * 8 + 7] = -S[CTK_PS_YV];
  N[6 * 8 + 6] = S[CTK_PS_XXR], N[6 * 8 + 7] = S[CTK_PS_XYR], N[7 * 8 + 7] = S[CTK_PS_YYR];
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < i; ++j) N[i * 8 + j] = N[j * 8 + i];
  b[0] = S[CTK_PS_XU], b[1] = S[CTK_PS_YU], b[2] = S[CTK_PS_U], b[3] = S[CTK_PS_XV], b[4] = S[CTK_PS_YV], b[5] = S[CTK_PS_V];
  b[6] = -S[CTK_PS_XR], b[7] = -S[CTK_PS_YR];
}

// the doubles a caller keeps for one system and its solution: N, b, L, D, v, z, h
#define CTK_PLANE_SOLVE_DOUBLES (64 + 8 + 64 + 8 + 8 + 8 + 8)

// N h = b by N = L D L^T; L (8 x 8, the strict lower triangle is used), D, v, z: work space of 64 + 8 + 8 + 8 doubles -> solved
CTK_MM_HD bool ctk_plane_solve(const double* N, const double* b, double* L, double* D, double* v, double* z, double* h) {
  for (int j = 0; j < 8; ++j) {
    for (int k = 0; k < j; ++k) v[k] = L[j * 8 + k] * D[k];
    double d = N[j * 8 + j];
    for (int k = 0; k < j; ++k) {
      const double t = L[j * 8 + k] * v[k];
      d = d - t;
    }
    if (!(d > 0.0) || !ctk_plane_finite(d)) return false;
    D[j] = d;
    for (int i = j + 1; i < 8; ++i) {
      double s = N[i * 8 + j];
      for (int k = 0; k < j; ++k) {
        const double t = L[i * 8 + k] * v[k];
        s = s - t;
      }
      L[i * 8 + j] = s / d;
    }
  }
  for (int i = 0; i < 8; ++i) {
    double s = b[i];
    for (int k = 0; k < i; ++k) {
      const double t = L[i * 8 + k] * z[k];
      s = s - t;
    }
    z[i] = s;
  }
  for (int i = 7; i >= 0; --i) {
    double s = z[i] / D[i];
    for (int k = i + 1; k < 8; ++k) {
      const double t = L[k * 8 + i] * h[k];
      s = s - t;
    }
    h[i] = s;
  }
  bool ok = true;
  for (int i = 0; i < 8; ++i) ok = ok && ctk_plane_finite(h[i]);
  return ok;
}

// a centred matrix hc (9 doubles) whose coordinates are 2^e / 16 pixel -> out: float32 3 x 3 in pixels
CTK_MM_HD void ctk_plane_pixels(const double* hc, int e, int px, int py, int qx, int qy, float* out) {
  const double sig = ldexp(1.0, 4 - e), isig = ldexp(1.0, e - 4);
  const double cx = (double)px / 16.0, cy = (double)py / 16.0, kx = (double)qx / 16.0, ky = (double)qy / 16.0;
  double G[9], M[9];
  G[0] = hc[0], G[1] = hc[1], G[2] = hc[2] * isig;
  G[3] = hc[3], G[4] = hc[4], G[5] = hc[5] * isig;
  G[6] = hc[6] * sig, G[7] = hc[7] * sig, G[8] = hc[8];
  for (int r = 0; r < 3; ++r) {
    const double a = G[r * 3] * cx, c = G[r * 3 + 1] * cy;
    const double s = a + c;
    M[r * 3] = G[r * 3], M[r * 3 + 1] = G[r * 3 + 1], M[r * 3 + 2] = G[r * 3 + 2] - s;
  }
  for (int c = 0; c < 3; ++c) {
    const double tx = kx * M[6 + c], ty = ky * M[6 + c];
    out[c] = (float)(M[c] + tx);
    out[3 + c] = (float)(M[3 + c] + ty);
    out[6 + c] = (float)M[6 + c];
  }
}

CTK_MM_HD void ctk_plane_identity(float* m) {
  for (int i = 0; i < 9; ++i) m[i] = i % 4 == 0 ? 1.0f : 0.0f;
}

// ---- warp ---------------------------------------------------------------------------------------------------------------------------
// float32 3 x 3 -> doubles; -> every entry is finite
CTK_MM_HD bool ctk_plane_matrix(const float* m, double* md) {
  bool finite = true;
  for (int i = 0; i < 9; ++i) {
    md[i] = (double)m[i];
    finite = finite && fabsf(m[i]) <= 3.402823466e+38f;
  }
  return finite;
}

// the homogeneous position of output pixel (x, y): v[0..2] = Xh, Yh, Zh
CTK_MM_HD void ctk_plane_project(const double* m, int x, int y, double* v) {
  const double dx = (double)x, dy = (double)y;
  for (int r = 0; r < 3; ++r) {
    const double a = m[r * 3] * dx, c = m[r * 3 + 1] * dy;
    const double s = a + c;
    v[r] = s + m[r * 3 + 2];
  }
}

// homogeneous position -> inside; then (sx, sy) in pixels
CTK_MM_HD bool ctk_plane_position(const double* v, double* sx, double* sy) {
  if (!(v[2] > 0.0)) return false;
  const double r = 1.0 / v[2];
  *sx = v[0] * r, *sy = v[1] * r;
  return fabs(*sx) <= CTK_PLANE_REACH && fabs(*sy) <= CTK_PLANE_REACH;
}

// output pixel (x, y) under a matrix with finite entries -> inside; then X, Y in 1/256 pixel
CTK_MM_HD bool ctk_plane_coord(const double* m, int x, int y, int64_t* X, int64_t* Y) {
  double v[3], sx, sy;
  ctk_plane_project(m, x, y, v);
  if (!ctk_plane_position(v, &sx, &sy)) return false;
  *X = (int64_t)llrint(sx * 256.0), *Y = (int64_t)llrint(sy * 256.0);
  return true;
}
CTK_MM_HD int ctk_plane_whole(int64_t X) { return (int)(X >> 8); }
CTK_MM_HD int ctk_plane_frac(int64_t X) { return (int)(X & 255); }
