// The rules behind ctk_lens_frames and ctk_lens_points (include/ctk.h, "lens"), restated ONCE for the device kernels (lens.hip) and for
// a host build of the same text (tests/test_lens_host.py compiles this header with g++ and compares it with the numpy restatement of
// tests/lens_reference.py -- no GPU needed to pin it).  Decisions are integers or single comparisons; everything in double is ONE
// IEEE operation per step, in the order written down here (compile with -ffp-contract=off): the device, the host build and numpy
// agree on every byte and on every float bit.  No root, no library call but rint.
//
// Camera.  Brown-Conrady, coefficients k = (k1, k2, p1, p2, k3).  The sensor's pinhole part is (fx, fy, cx, cy) in raw-video pixels,
// the ideal (pinhole) camera (fx', fy', cx', cy'); pixel centres are at integers (draw_math.h's convention).
//   valid       all 13 numbers finite, the four focal lengths in [1, 1e6], |centre| <= 32768, |coefficient| <= 64
//   forward     (ideal -> sensor), (x, y) normalised ideal coordinates; every line one operation per assignment, left to right:
//                 xx = x x;  yy = y y;  r2 = xx + yy;  txy = 2 (x y)
//                 rad = 1 + r2 (k1 + r2 (k2 + r2 k3))                            innermost product first
//                 xd  = (x rad + p1 txy) + p2 (r2 + 2 xx)
//                 yd  = (y rad + p1 (r2 + 2 yy)) + p2 txy
//   jacobian    of (xd, yd) by (x, y):
//                 dr = k1 + r2 (2 k2 + 3 (k3 r2))
//                 a = ((rad + (2 xx) dr) + (2 p1) y) + (6 p2) x       b = c = ((txy dr) + (2 p1) x) + (2 p2) y
//                 d = ((rad + (2 yy) dr) + (6 p1) y) + (2 p2) x       det = a d - b b
//   inverse     (sensor -> ideal): Newton from (x, y) = (xd, yd), CTK_LENS_ROUNDS = 8 rounds, always all of them:
//                 (ex, ey) = (xd, yd) - forward(x, y);  idet = 1 / det (the one division of a round)
//                 x += (d ex - b ey) idet;  y += (a ey - b ex) idet
//               then forward and jacobian ONCE more at the result: accepted iff det > 0 and e = (fx ex)^2 + (fy ey)^2 <= tol2, the
//               squared residual in sensor pixels against tol2 = (double)tol (double)tol.  A NaN fails both comparisons; a det of 0
//               makes one.  (Five rounds reach 3e-12 pixel on lenses from a mild barrel to a strong pincushion over a 1080p field
//               enlarged by 15 %; the plain fixed-point iteration is 0.6 pixel off after 8 rounds on an action camera.)
//   map         a position (px, py) in the pixels of camera A (focal lengths and centre `in`, iin = 1 / focal length: one division
//               per launch, made by ctk_lens_prepare on the host) -> (qx, qy) in the pixels of camera B (`out`):
//                 xn = (px - cx) ifx;  yn = (py - cy) ify;  (x, y) = forward or inverse of (xn, yn);  qx = fx_out x + cx_out
//               ok iff det > 0 at (xn, yn) (forward) or the inverse was accepted.
//
// Point rule (ctk_lens_points).  CTK_LENS_TO_IDEAL: A = sensor, B = ideal, the inverse.  CTK_LENS_TO_SENSOR: A = ideal, B = sensor,
// forward.  The position is read as two float32 widened to double; not finite or |p| > 32768 on either axis: (NaN, NaN) with the bits
// 0x7FC00000, label -1.  Otherwise the map: ok -> ((float)qx, (float)qy), label 1; not ok -> (NaN, NaN), label 0.
//
// Picture rule (ctk_lens_frames).  Output pixel (x, y) -> source position by the map in double, with the point rule of the OTHER
// direction: a CTK_LENS_TO_IDEAL picture is the pinhole picture, whose pixel (x, y) is an ideal position that forward carries onto the
// sensor; a CTK_LENS_TO_SENSOR picture needs the inverse.  The pixel is OUTSIDE when the map is not ok, or (qx, qy) is not finite, or
// |q| > 32768 on either axis; an outside pixel takes fill[c] under either border.  Otherwise X = llrint(qx * 256.0) (round half to
// even, as rint in ctk_warp_fix), ix = X >> 8 (arithmetic: a floor), fx = X & 255, Y likewise; the four taps, the CTK_WARP_FILL /
// CTK_WARP_EDGE borders and the blend are ctk_warp_frames' (warp_math.h: ctk_warp_clamp, ctk_warp_blend).
// With all coefficients 0 and the ideal camera equal to the sensor's the picture is copied bit for bit: rad = 1 and every tangential
// term is 0 exactly, so q = fx ((x - cx) ifx) + cx, three roundings after the exact x - cx, each below 2^-52 of a value below 2^17:
// q is within 1e-10 of the integer x, 256 q within 3e-8 of 256 x -- far less than the 1/512 pixel (0.5 after scaling) that would
// move llrint off 256 x, so fx = fy = 0 and the blend returns the tap.  A centre shifted by whole pixels gives a shifted copy.
#pragma once
#include <math.h>
#include <stdint.h>

#include "warp_math.h"

#if defined(__HIPCC__)
#define CTK_LM_HD __host__ __device__ __forceinline__
#else
#define CTK_LM_HD static inline
#endif

#ifndef CTK_LENS_TO_IDEAL  // (include/ctk.h has them too)
#define CTK_LENS_TO_IDEAL 0
#define CTK_LENS_TO_SENSOR 1
#define CTK_LENS_ROUNDS 8
#endif
#define CTK_LENS_FOCAL_MIN 1.0
#define CTK_LENS_FOCAL_MAX 1e6
#define CTK_LENS_REACH 32768.0
#define CTK_LENS_COEFF_MAX 64.0

// sensor, ideal: (fx, fy, cx, cy); k: (k1, k2, p1, p2, k3).  (A NaN fails every comparison; an infinity fails the bound.)
CTK_LM_HD bool ctk_lens_valid(const double* sensor, const double* ideal, const double* k) {
  bool ok = true;
  for (int c = 0; c < 2; ++c) {
    const double* cam = c == 0 ? sensor : ideal;
    ok = ok && cam[0] >= CTK_LENS_FOCAL_MIN && cam[0] <= CTK_LENS_FOCAL_MAX && cam[1] >= CTK_LENS_FOCAL_MIN && cam[1] <= CTK_LENS_FOCAL_MAX;
    ok = ok && fabs(cam[2]) <= CTK_LENS_REACH && fabs(cam[3]) <= CTK_LENS_REACH;
  }
  for (int i = 0; i < 5; ++i) ok = ok && fabs(k[i]) <= CTK_LENS_COEFF_MAX;
  return ok;
}

// What a launch needs of a lens, made once on the host (the divisions are here).
struct ctk_lens_rule {
  double k[5];
  double in[4], iin[2];  // the camera a position comes in: (fx, fy, cx, cy), and 1 / fx, 1 / fy
  double out[4];         // the camera the result is stated in
  double tol2;
  int invert;            // 1: the Newton inverse (`in` is the sensor), 0: forward (`in` is the ideal camera)
};

// direction: of the POINT rule (ctk_lens_frames passes the other one, see the picture rule)
CTK_LM_HD void ctk_lens_prepare(const double* sensor, const double* ideal, const double* k, int direction, float tol, ctk_lens_rule* r) {
  const double* in = direction == CTK_LENS_TO_IDEAL ? sensor : ideal;
  const double* out = direction == CTK_LENS_TO_IDEAL ? ideal : sensor;
  for (int i = 0; i < 5; ++i) r->k[i] = k[i];
  for (int i = 0; i < 4; ++i) r->in[i] = in[i], r->out[i] = out[i];
  r->iin[0] = 1.0 / in[0], r->iin[1] = 1.0 / in[1];
  r->tol2 = (double)tol * (double)tol;
  r->invert = direction == CTK_LENS_TO_IDEAL ? 1 : 0;
}

// forward and its jacobian at (x, y): j = (a, b, d, det)
CTK_LM_HD void ctk_lens_forward(const double* k, double x, double y, double* xd, double* yd, double* j) {
  const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4];
  const double xx = x * x, yy = y * y;
  const double r2 = xx + yy;
  const double xy = x * y;
  const double txy = 2.0 * xy;
  double t = r2 * k3;
  t = k2 + t;
  t = r2 * t;
  t = k1 + t;
  t = r2 * t;
  const double rad = 1.0 + t;
  const double txx = 2.0 * xx, tyy = 2.0 * yy;
  const double x1 = x * rad, x2 = p1 * txy;
  double x3 = r2 + txx;
  x3 = p2 * x3;
  const double xs = x1 + x2;
  *xd = xs + x3;
  const double y1 = y * rad, y3 = p2 * txy;
  double y2 = r2 + tyy;
  y2 = p1 * y2;
  const double ys = y1 + y2;
  *yd = ys + y3;
  double u = k3 * r2;
  u = 3.0 * u;
  const double v = 2.0 * k2;
  u = v + u;
  u = r2 * u;
  const double dr = k1 + u;
  const double tp1 = 2.0 * p1, tp2 = 2.0 * p2, sp1 = 6.0 * p1, sp2 = 6.0 * p2;
  const double a1 = txx * dr, a2 = tp1 * y, a3 = sp2 * x;
  double a = rad + a1;
  a = a + a2;
  a = a + a3;
  const double b1 = txy * dr, b2 = tp1 * x, b3 = tp2 * y;
  double b = b1 + b2;
  b = b + b3;
  const double d1 = tyy * dr, d2 = sp1 * y, d3 = tp2 * x;
  double d = rad + d1;
  d = d + d2;
  d = d + d3;
  const double ad = a * d, bb = b * b;
  j[0] = a, j[1] = b, j[2] = d, j[3] = ad - bb;
}

// Newton inverse of (xd, yd); fx, fy: the sensor's focal lengths, for the residual in pixels -> accepted
CTK_LM_HD bool ctk_lens_inverse(const double* k, double fx, double fy, double tol2, double xd, double yd, double* xo, double* yo) {
  double x = xd, y = yd, fxd, fyd, j[4];
  for (int round = 0; round < CTK_LENS_ROUNDS; ++round) {
    ctk_lens_forward(k, x, y, &fxd, &fyd, j);
    const double ex = xd - fxd, ey = yd - fyd;
    const double idet = 1.0 / j[3];
    const double n1 = j[2] * ex, n2 = j[1] * ey, n3 = j[0] * ey, n4 = j[1] * ex;
    double sx = n1 - n2, sy = n3 - n4;
    sx = sx * idet, sy = sy * idet;
    x = x + sx, y = y + sy;
  }
  ctk_lens_forward(k, x, y, &fxd, &fyd, j);
  const double ex = xd - fxd, ey = yd - fyd;
  double rx = fx * ex, ry = fy * ey;
  rx = rx * rx, ry = ry * ry;
  const double e = rx + ry;
  *xo = x, *yo = y;
  return j[3] > 0.0 && e <= tol2;
}

// the map: (px, py) in the pixels of r->in -> (qx, qy) in the pixels of r->out, and whether it holds there
CTK_LM_HD bool ctk_lens_map(const ctk_lens_rule* r, double px, double py, double* qx, double* qy) {
  const double dx = px - r->in[2], dy = py - r->in[3];
  const double xn = dx * r->iin[0], yn = dy * r->iin[1];
  double x, y;
  bool ok;
  if (r->invert) {
    ok = ctk_lens_inverse(r->k, r->in[0], r->in[1], r->tol2, xn, yn, &x, &y);
  } else {
    double j[4];
    ctk_lens_forward(r->k, xn, yn, &x, &y, j);
    ok = j[3] > 0.0;
  }
  const double ox = r->out[0] * x, oy = r->out[1] * y;
  *qx = ox + r->out[2], *qy = oy + r->out[3];
  return ok;
}

CTK_LM_HD bool ctk_lens_within(double px, double py) { return fabs(px) <= CTK_LENS_REACH && fabs(py) <= CTK_LENS_REACH; }

// the point rule: p -> q (two float32 each), -> label.  The NaN written has the bits 0x7FC00000 (out: two uint32).
CTK_LM_HD int ctk_lens_point(const ctk_lens_rule* r, float pxf, float pyf, uint32_t* out) {
  const double px = (double)pxf, py = (double)pyf;
  out[0] = out[1] = 0x7FC00000u;
  if (!ctk_lens_within(px, py)) return -1;
  double qx, qy;
  if (!ctk_lens_map(r, px, py, &qx, &qy)) return 0;
  const float fx = (float)qx, fy = (float)qy;
  union { float f; uint32_t u; } bx, by;
  bx.f = fx, by.f = fy;
  out[0] = bx.u, out[1] = by.u;
  return 1;
}

// the picture rule's coordinate: output pixel (x, y) -> inside, and X, Y in 1/256 pixel of the source
CTK_LM_HD bool ctk_lens_coord(const ctk_lens_rule* r, int x, int y, int64_t* X, int64_t* Y) {
  double qx, qy;
  const bool ok = ctk_lens_map(r, (double)x, (double)y, &qx, &qy);
  if (!(ok && ctk_lens_within(qx, qy))) {
    *X = 0, *Y = 0;
    return false;
  }
  *X = (int64_t)llrint(qx * 256.0), *Y = (int64_t)llrint(qy * 256.0);
  return true;
}
CTK_LM_HD int ctk_lens_whole(int64_t X) { return (int)(X >> 8); }
CTK_LM_HD int ctk_lens_frac(int64_t X) { return (int)(X & 255); }
