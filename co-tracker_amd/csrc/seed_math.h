// The corner score behind ctk_seed_points (include/ctk.h, "seed points"), restated ONCE for the device kernel (seed.hip) and for a host
// build of the same text (tests/test_seed_host.py compiles this header with g++ and compares it with the numpy restatement of
// tests/seed_reference.py -- no GPU needed to pin it).  Everything past the quantisation of a pixel is INTEGER arithmetic: the
// device, the host build and numpy agree bit for bit, there is no tolerance anywhere.
//
//   luminance   q = (int)rintf(min(max(p, 0), 255)) per channel (a NaN gives 0);  L = (77 qR + 150 qG + 29 qB + 128) >> 8   in 0..255
//   gradient    central differences with replicated borders: gx = L(y, min(x+1, w-1)) - L(y, max(x-1, 0)), gy likewise      in -255..255
//   tensor      over the (2r+1)^2 window, pixels outside the image contributing nothing:
//               a = sum gx^2, b = sum gx gy, c = sum gy^2        (r <= 7: a, c <= 225 * 65025 < 2^24, |b| likewise -- int32)
//   score       a + c - ceil_sqrt((a - c)^2 + 4 b^2) = floor(2 lambda_min) of the tensor, >= 0, int32
//               (twice the smaller eigenvalue is a + c - sqrt(d); for an integer n and real s, floor(n - s) = n - ceil(s))
//   cell        one axis of the rule of health_cell (stream.hip): clamp((int)floorf((x - lo) * inv), 0, g - 1), two float32 operations:
//               compile with -ffp-contract=off.  A seed's cell is the cell ctk_stream_health counts it in.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CTK_SM_HD __host__ __device__ __forceinline__
#else
#define CTK_SM_HD static inline
#endif

#define CTK_SEED_RADIUS_MAX 7

CTK_SM_HD int ctk_seed_quant(float p) {
  float v = p > 0.0f ? p : 0.0f;  // (a NaN compares false: 0)
  v = v < 255.0f ? v : 255.0f;
  return (int)rintf(v);  // round half to even, as numpy's rint
}

CTK_SM_HD int ctk_seed_luma(float r, float g, float b) {
  return (77 * ctk_seed_quant(r) + 150 * ctk_seed_quant(g) + 29 * ctk_seed_quant(b) + 128) >> 8;
}

// the smallest t >= 0 with t * t >= d, 0 <= d < 2^62.  The double sqrt is a first guess only: the +-1 steps make the result exact
// whatever its rounding.
CTK_SM_HD int64_t ctk_seed_ceil_sqrt(int64_t d) {
  if (d <= 0) return 0;
  int64_t t = (int64_t)sqrt((double)d);
  while (t * t < d) ++t;
  while (t > 0 && (t - 1) * (t - 1) >= d) --t;
  return t;
}

CTK_SM_HD int ctk_seed_score(int a, int b, int c) {
  const int64_t m = (int64_t)a - (int64_t)c;
  const int64_t d = m * m + 4 * (int64_t)b * (int64_t)b;  // < 2^50
  return (int)((int64_t)a + (int64_t)c - ctk_seed_ceil_sqrt(d));
}

// one axis of the cell rule; the clamp is done on the float so that the conversion is defined for every finite operand
CTK_SM_HD int ctk_seed_cell_axis(float x, float lo, float inv, int g) {
  const float d = x - lo;
  float t = floorf(d * inv);
  t = t > 0.0f ? t : 0.0f;
  t = t < (float)(g - 1) ? t : (float)(g - 1);
  return (int)t;
}

// The pixels of [0, n) inside the inclusive bounds [lo, hi]: p0 .. p1 (empty when p0 > p1).  lo, hi finite.
CTK_SM_HD void ctk_seed_pixel_range(float lo, float hi, int n, int* p0, int* p1) {
  float a = ceilf(lo), b = floorf(hi);
  a = a > 0.0f ? a : 0.0f;
  a = a < (float)n ? a : (float)n;
  b = b > -1.0f ? b : -1.0f;
  b = b < (float)(n - 1) ? b : (float)(n - 1);
  *p0 = (int)a, *p1 = (int)b;
}

// The cell rule is monotone in the pixel (every step is), so the pixels p0 .. p1 of one cell are a run: the first pixel of [p0, p1 + 1]
// whose cell is >= c (p1 + 1 when there is none).  Cell c holds [first(c), first(c + 1) - 1].
CTK_SM_HD int ctk_seed_cell_first(int c, int p0, int p1, float lo, float inv, int g) {
  int a = p0, b = p1 + 1;
  while (a < b) {
    const int m = a + (b - a) / 2;
    if (ctk_seed_cell_axis((float)m, lo, inv, g) >= c) b = m;
    else a = m + 1;
  }
  return a;
}

// The candidate pixels of cell c along one axis of n pixels: the cell's run shrunk by `inset` at both ends, inside [margin, n-1-margin].
CTK_SM_HD void ctk_seed_candidates(int c, float lo, float hi, float inv, int g, int n, int margin, int inset, int* c0, int* c1) {
  int p0, p1;
  ctk_seed_pixel_range(lo, hi, n, &p0, &p1);
  const int f0 = ctk_seed_cell_first(c, p0, p1, lo, inv, g), f1 = ctk_seed_cell_first(c + 1, p0, p1, lo, inv, g) - 1;
  const int ins = inset < 65536 ? inset : 65536, mar = margin < 65536 ? margin : 65536;  // (sides are <= 32768: no sum overflows)
  const int lo_px = f0 + ins > mar ? f0 + ins : mar;
  const int hi_px = f1 - ins < n - 1 - mar ? f1 - ins : n - 1 - mar;
  *c0 = lo_px, *c1 = hi_px;
}

// The selection key: a higher score wins, then the lower py, then the lower px.  py, px < 65536; score >= 0.
CTK_SM_HD int64_t ctk_seed_key(int score, int py, int px) {
  return ((int64_t)score << 32) | (int64_t)((uint32_t)(65535 - py) << 16) | (int64_t)(uint32_t)(65535 - px);
}
CTK_SM_HD int ctk_seed_key_score(int64_t k) { return (int)(k >> 32); }
CTK_SM_HD int ctk_seed_key_py(int64_t k) { return 65535 - (int)((k >> 16) & 0xffff); }
CTK_SM_HD int ctk_seed_key_px(int64_t k) { return 65535 - (int)(k & 0xffff); }
