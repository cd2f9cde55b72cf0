// The rules behind ctk_fit_motion (include/ctk.h, "fit motion"), restated ONCE for the device kernel (motion.hip) and for a host build
// of the same text (tests/test_motion_host.py compiles this header with g++ and compares it with the numpy restatement of
// tests/motion_reference.py -- no GPU needed to pin it).  Everything between the quantisation of a position and the last four
// divisions is INTEGER arithmetic: the device, the host build and numpy agree bit for bit, there is no tolerance anywhere.
//
//   position    v = x * sx, one float32 multiplication (compile with -ffp-contract=off); valid iff finite and |v| <= 8192;
//               P = (int)rintf(v * 16.0f), 1/16 pixel, round half to even; the product by 16 is exact                     |P| <= 2^17
//   pair        P = source (frame f - lag), Q = destination (frame f); the M correspondences of a frame are numbered in ascending n
//   hypothesis  k of K: h0 = mix(seed ^ mix(f * 0x9e3779b9 + 2k)), h1 = mix(seed ^ mix(f * 0x9e3779b9 + 2k + 1)), uint32;
//               i = h0 % M;  j = h1 % (M - 1), j += (j >= i)   (similarity only)
//   similarity  d = P_j - P_i, e = Q_j - Q_i (components |.| <= 2^18), D = d.d, A = d.e, B = d x e:            D, |A|, |B| <= 2^37
//               admissible iff D >= base2 = b * b, b = (int64)rintf(min_base * 16) (<= 2^17), and D >= 1 (coincident sources define
//               no similarity; it matters for min_base = 0 only).  For point m, u = P_m - P_i, w = Q_m - Q_i (|.| <= 2^18):
//               rx = D w.x - (A u.x - B u.y), ry = D w.y - (B u.x + A u.y): every product <= 2^55, |rx|, |ry| < 2^57
//               inlier iff |rx| <= T D and |ry| <= T D, T = (int)rintf(tol * 16) in 1..4096:                          T D <= 2^49
//   translation only i; inlier iff |w.x - u.x| <= T and |w.y - u.y| <= T; always admissible
//   best        max of key = count << 32 | (K - 1 - k) over admissible hypotheses (count <= 8192, K <= 4096): most inliers, then
//               the lowest k; -1 = none
//   refit       over the inliers of the best: n, Spx, Spy, Sqx, Sqy, Spp = sum |P|^2, Sdot = sum P.Q, Scr = sum P x Q in int64.
//               n <= 2^13: |Sp.|, |Sq.| <= 2^30; Spp, |Sdot|, |Scr| <= 2^48; n Spp, Spx^2 + Spy^2 <= 2^61 and 0 <= den <= 2^61;
//               |n Sdot|, |Spx Sqx + Spy Sqy| <= 2^61 so |na|, |nb| <= 2^62 < 2^63.  den > 0: the inliers hold i and j, P_i != P_j.
//               Then in double, ONE IEEE operation per step: a = na / den, b = nb / den,
//               tx = (Sqx - (a Spx - b Spy)) / (n * 16), ty = (Sqy - (b Spx + a Spy)) / (n * 16); the row is (float) of
//               [[a, -b, tx], [b, a, ty]].  Translation: a = 1, b = 0, tx = (Sqx - Spx) / (n * 16).
#pragma once
#include <math.h>
#include <stdint.h>

#include "draw_math.h"  // ctk_draw_visible: ctk_stream_emit's visibility expression

#if defined(__HIPCC__)
#define CTK_MM_HD __host__ __device__ __forceinline__
#else
#define CTK_MM_HD static inline
#endif

#define CTK_MOTION_TRANSLATION 0
#define CTK_MOTION_SIMILARITY 1
#define CTK_MOTION_POINTS_MAX 8192
#define CTK_MOTION_HYPOTHESES_MAX 4096
#define CTK_MOTION_TOL_MAX 4096  // T, 1/16 pixel

// one component of a position: -> valid; *p = 1/16 pixel when valid
CTK_MM_HD bool ctk_motion_quant(float x, float s, int* p) {
  const float v = x * s;
  if (!(v >= -8192.0f && v <= 8192.0f)) return false;  // (NaN, +-inf: false)
  *p = (int)rintf(v * 16.0f);
  return true;
}

// tol -> T; 0 when tol is NaN or T lies outside 1..4096
CTK_MM_HD int ctk_motion_tol(float tol) {
  const float t = rintf(tol * 16.0f);
  return t >= 1.0f && t <= (float)CTK_MOTION_TOL_MAX ? (int)t : 0;
}

// min_base -> base2; -1 when min_base is NaN, negative or above 8192
CTK_MM_HD int64_t ctk_motion_base2(float min_base) {
  if (!(min_base >= 0.0f && min_base <= 8192.0f)) return -1;
  const int64_t b = (int64_t)rintf(min_base * 16.0f);
  return b * b;
}

CTK_MM_HD uint32_t ctk_motion_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// the sample of hypothesis k on frame f among M >= 1 (translation) / M >= 2 (similarity) correspondences
CTK_MM_HD void ctk_motion_sample(uint32_t seed, int f, int k, int M, int model, int* i, int* j) {
  const uint32_t base = (uint32_t)f * 0x9e3779b9u + 2u * (uint32_t)k;
  const uint32_t h0 = ctk_motion_mix(seed ^ ctk_motion_mix(base));
  *i = (int)(h0 % (uint32_t)M);
  *j = *i;
  if (model == CTK_MOTION_SIMILARITY) {
    const uint32_t h1 = ctk_motion_mix(seed ^ ctk_motion_mix(base + 1u));
    int jj = (int)(h1 % (uint32_t)(M - 1));
    jj += jj >= *i ? 1 : 0;
    *j = jj;
  }
}

// A hypothesis, ready to test points against: the anchor pair, and for a similarity D, A, B and the bound T D.
struct CtkMotionHyp {
  int px, py, qx, qy;  // P_i, Q_i
  int64_t D, A, B, TD;
};

// -> admissible
CTK_MM_HD bool ctk_motion_hyp(int model, int pix, int piy, int qix, int qiy, int pjx, int pjy, int qjx, int qjy, int T, int64_t base2,
                              CtkMotionHyp* h) {
  h->px = pix, h->py = piy, h->qx = qix, h->qy = qiy;
  h->D = 0, h->A = 0, h->B = 0, h->TD = (int64_t)T;
  if (model != CTK_MOTION_SIMILARITY) return true;
  const int64_t dx = pjx - pix, dy = pjy - piy, ex = qjx - qix, ey = qjy - qiy;
  h->D = dx * dx + dy * dy;
  h->A = dx * ex + dy * ey;
  h->B = dx * ey - dy * ex;
  h->TD = (int64_t)T * h->D;
  return h->D >= base2 && h->D >= 1;
}

CTK_MM_HD bool ctk_motion_inlier_similarity(const CtkMotionHyp& h, int px, int py, int qx, int qy) {
  const int64_t ux = px - h.px, uy = py - h.py, wx = qx - h.qx, wy = qy - h.qy;
  const int64_t rx = h.D * wx - (h.A * ux - h.B * uy);
  const int64_t ry = h.D * wy - (h.B * ux + h.A * uy);
  return rx <= h.TD && rx >= -h.TD && ry <= h.TD && ry >= -h.TD;
}

CTK_MM_HD bool ctk_motion_inlier_translation(const CtkMotionHyp& h, int px, int py, int qx, int qy) {
  const int T = (int)h.TD;
  const int rx = (qx - h.qx) - (px - h.px), ry = (qy - h.qy) - (py - h.py);  // (|.| <= 2^19)
  return rx <= T && rx >= -T && ry <= T && ry >= -T;
}

CTK_MM_HD bool ctk_motion_inlier(int model, const CtkMotionHyp& h, int px, int py, int qx, int qy) {
  return model == CTK_MOTION_SIMILARITY ? ctk_motion_inlier_similarity(h, px, py, qx, qy) : ctk_motion_inlier_translation(h, px, py, qx, qy);
}

// the selection key of an admissible hypothesis; an inadmissible one has -1
CTK_MM_HD int64_t ctk_motion_key(int count, int k, int K) { return ((int64_t)count << 32) | (int64_t)(K - 1 - k); }
CTK_MM_HD int ctk_motion_key_count(int64_t key) { return (int)(key >> 32); }
CTK_MM_HD int ctk_motion_key_k(int64_t key, int K) { return K - 1 - (int)(key & 0xffffffff); }

// the eight sums of the refit, in this order
enum { CTK_MS_N = 0, CTK_MS_PX, CTK_MS_PY, CTK_MS_QX, CTK_MS_QY, CTK_MS_PP, CTK_MS_DOT, CTK_MS_CR, CTK_MS_COUNT };

CTK_MM_HD void ctk_motion_accumulate(int64_t* s, int px, int py, int qx, int qy) {
  const int64_t Px = px, Py = py, Qx = qx, Qy = qy;
  s[CTK_MS_N] += 1;
  s[CTK_MS_PX] += Px, s[CTK_MS_PY] += Py, s[CTK_MS_QX] += Qx, s[CTK_MS_QY] += Qy;
  s[CTK_MS_PP] += Px * Px + Py * Py;
  s[CTK_MS_DOT] += Px * Qx + Py * Qy;
  s[CTK_MS_CR] += Px * Qy - Py * Qx;
}

CTK_MM_HD void ctk_motion_identity(float* row) {
  row[0] = 1.0f, row[1] = 0.0f, row[2] = 0.0f, row[3] = 0.0f, row[4] = 1.0f, row[5] = 0.0f;
}

// sums with n >= 1 (similarity: den > 0) -> the matrix row [a, -b, tx, b, a, ty]
CTK_MM_HD void ctk_motion_refit(int model, const int64_t* s, float* row) {
  const double n16 = (double)s[CTK_MS_N] * 16.0;
  const double spx = (double)s[CTK_MS_PX], spy = (double)s[CTK_MS_PY], sqx = (double)s[CTK_MS_QX], sqy = (double)s[CTK_MS_QY];
  double a = 1.0, b = 0.0, tx, ty;
  if (model == CTK_MOTION_SIMILARITY) {
    const int64_t n = s[CTK_MS_N];
    const int64_t den = n * s[CTK_MS_PP] - (s[CTK_MS_PX] * s[CTK_MS_PX] + s[CTK_MS_PY] * s[CTK_MS_PY]);
    const int64_t na = n * s[CTK_MS_DOT] - (s[CTK_MS_PX] * s[CTK_MS_QX] + s[CTK_MS_PY] * s[CTK_MS_QY]);
    const int64_t nb = n * s[CTK_MS_CR] - (s[CTK_MS_PX] * s[CTK_MS_QY] - s[CTK_MS_PY] * s[CTK_MS_QX]);
    a = (double)na / (double)den;
    b = (double)nb / (double)den;
    const double ax = a * spx, by = b * spy, bx = b * spx, ay = a * spy;
    const double mx = ax - by, my = bx + ay;
    const double rx = sqx - mx, ry = sqy - my;
    tx = rx / n16, ty = ry / n16;
  } else {
    const double rx = sqx - spx, ry = sqy - spy;
    tx = rx / n16, ty = ry / n16;
  }
  row[0] = (float)a, row[1] = (float)-b, row[2] = (float)tx, row[3] = (float)b, row[4] = (float)a, row[5] = (float)ty;
}
