// The rules behind ctk_warp_frames and ctk_smooth_path (include/ctk.h, "warp frames"), restated ONCE for the device kernels (warp.hip)
// and for a host build of the same text (tests/test_warp_host.py compiles this header with g++ and compares it with the numpy
// restatement of tests/warp_reference.py -- no GPU needed to pin it).  Everything is integer arithmetic or ONE IEEE double operation
// per step (compile with -ffp-contract=off): the device, the host build and numpy agree on every byte and on every float bit.
//
// Picture warp.  matrices[j] (float32 2 x 3) maps an OUTPUT pixel to a SOURCE position of picture j: (sx, sy) = m (x, y, 1); pixel
// centres are at integers (draw_math.h's convention).
//   valid       all six entries finite, |m00|, |m01|, |m10|, |m11| <= 8, |m02|, |m12| <= 32768; an invalid matrix counts as the
//               identity: the picture is copied
//   fixed point c_k = (int64)rint((double)m_k * 16777216.0): Q24, the product is exact, round half to even        |c| <= 2^39
//   coordinate  X = c00 x + c01 y + c02 + 32768 (Y likewise) in int64, below 2^45 for sides up to 32768; ix = X >> 24 (arithmetic: a
//               floor), fx = (X >> 16) & 255: the position rounded to 1/256 pixel.  Exact, so X may be stepped by c00 per pixel.
//   taps        (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1).  CTK_WARP_FILL: a tap outside [0, W) x [0, H) has the value
//               fill[c]; CTK_WARP_EDGE: tap indices are clamped into range.  Nothing outside the picture is read.
//   blend       out = ((256 - fx)(256 - fy) p00 + fx (256 - fy) p01 + (256 - fx) fy p10 + fx fy p11 + 32768) >> 16 per channel, int32
//               (the weights sum to 65536: <= 2^24 + 2^15)
// The identity copies the source bit for bit, an integer translation is a shifted copy.
//
// Path step: a causal, leaky lock-on whose state stays bounded.  W (2 x 3, double) maps a stabilised pixel to a position in the
// current frame.  For frame f, M = the motion of frame f - 1 to frame f (float32 -> double; a matrix with a non-finite entry counts as
// the identity: the state persists and must never become NaN):
//   compose     P[r][0] = M[r][0] W[0][0] + M[r][1] W[1][0];  P[r][1] = M[r][0] W[0][1] + M[r][1] W[1][1];
//               P[r][2] = (M[r][0] W[0][2] + M[r][1] W[1][2]) + M[r][2]          one rounded operation per step, no contraction
//   blend       W' = k P elementwise, then W'[0][0] += a, W'[1][1] += a;  a = (double)alpha, k = 1.0 - a
//   output      (float)W', or (float)(W' o post) composed by the same three formulas (post: float32 2 x 3, not part of the state)
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CTK_WM_HD __host__ __device__ __forceinline__
#else
#define CTK_WM_HD static inline
#endif

#ifndef CTK_WARP_FILL  // (include/ctk.h has them too)
#define CTK_WARP_FILL 0
#define CTK_WARP_EDGE 1
#endif
#define CTK_WARP_LINEAR_MAX 8.0f
#define CTK_WARP_SHIFT_MAX 32768.0f

CTK_WM_HD bool ctk_warp_valid(const float* m) {
  // (a NaN fails every comparison; an infinity fails the bound)
  return fabsf(m[0]) <= CTK_WARP_LINEAR_MAX && fabsf(m[1]) <= CTK_WARP_LINEAR_MAX && fabsf(m[3]) <= CTK_WARP_LINEAR_MAX &&
         fabsf(m[4]) <= CTK_WARP_LINEAR_MAX && fabsf(m[2]) <= CTK_WARP_SHIFT_MAX && fabsf(m[5]) <= CTK_WARP_SHIFT_MAX;
}

// matrix row [m00, m01, m02, m10, m11, m12] -> Q24 coefficients; the identity's when the matrix is not valid
CTK_WM_HD void ctk_warp_fix(const float* m, int64_t* c) {
  if (!ctk_warp_valid(m)) {
    c[0] = 16777216, c[1] = 0, c[2] = 0, c[3] = 0, c[4] = 16777216, c[5] = 0;
    return;
  }
  for (int k = 0; k < 6; ++k) c[k] = (int64_t)rint((double)m[k] * 16777216.0);
}

// the coordinate of output pixel (x, y) along one axis: c = the axis' three coefficients
CTK_WM_HD int64_t ctk_warp_coord(const int64_t* c, int x, int y) { return c[0] * x + c[1] * y + c[2] + 32768; }
CTK_WM_HD int ctk_warp_whole(int64_t X) { return (int)(X >> 24); }
CTK_WM_HD int ctk_warp_frac(int64_t X) { return (int)((X >> 16) & 255); }

CTK_WM_HD int ctk_warp_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

CTK_WM_HD int ctk_warp_blend(int fx, int fy, int p00, int p01, int p10, int p11) {
  const int gx = 256 - fx, gy = 256 - fy;
  return (gx * gy * p00 + fx * gy * p01 + gx * fy * p10 + fx * fy * p11 + 32768) >> 16;
}

// P = A o B: the position B gives, then A
CTK_WM_HD void ctk_path_compose(const double* A, const double* B, double* P) {
  for (int r = 0; r < 2; ++r) {
    const double a0 = A[r * 3], a1 = A[r * 3 + 1], a2 = A[r * 3 + 2];
    const double p00 = a0 * B[0], p01 = a1 * B[3];
    const double p10 = a0 * B[1], p11 = a1 * B[4];
    const double p20 = a0 * B[2], p21 = a1 * B[5];
    const double s2 = p20 + p21;
    P[r * 3] = p00 + p01;
    P[r * 3 + 1] = p10 + p11;
    P[r * 3 + 2] = s2 + a2;
  }
}

// One frame: motion (float32 [6]) and the state W (double [6], updated in place) -> out (float32 [6]); post: float32 [6] or NULL
CTK_WM_HD void ctk_path_step(const float* motion, float alpha, const float* post, double* W, float* out) {
  double M[6], P[6];
  bool finite = true;
  for (int i = 0; i < 6; ++i) finite = finite && fabsf(motion[i]) <= 3.402823466e+38f;
  for (int i = 0; i < 6; ++i) M[i] = finite ? (double)motion[i] : (i == 0 || i == 4 ? 1.0 : 0.0);
  ctk_path_compose(M, W, P);
  const double a = (double)alpha, k = 1.0 - a;
  for (int i = 0; i < 6; ++i) W[i] = k * P[i];
  W[0] += a;
  W[4] += a;
  if (post != nullptr) {
    double B[6];
    for (int i = 0; i < 6; ++i) B[i] = (double)post[i];
    ctk_path_compose(W, B, P);
    for (int i = 0; i < 6; ++i) out[i] = (float)P[i];
  } else {
    for (int i = 0; i < 6; ++i) out[i] = (float)W[i];
  }
}
