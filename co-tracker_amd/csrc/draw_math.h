// The drawing rules behind ctk_draw_tracks (include/ctk.h, "draw tracks"), restated ONCE for the device kernels (draw.hip) and for a
// host build of the same text (tests/test_draw_host.py compiles this header with g++ and compares it with the numpy restatement of
// tests/draw_reference.py -- no GPU needed to pin it).  Everything past the quantisation of a position is INTEGER arithmetic: the
// device, the host build and numpy agree bit for bit, there is no tolerance anywhere.
//
//   position   v = x * sx, one float32 multiplication (compile with -ffp-contract=off); valid iff -65536 <= v <= 65536 (a NaN or an
//              infinity compares false); pixel q = (int)rintf(v), round half to even                                |q| <= 65536
//   visible    from logits: sigmoid(vis) * sigmoid(conf) > thresh, sigmoid(x) = 1 / (1 + expf(-x)), every step one float32 operation
//              -- the expression of ctk_stream_emit; a NaN is not visible
//   mark       d2 = squared pixel distance to q.  disc (visible): d2 <= r*r + r;  ring (not visible): (r-1)*(r-1) + (r-1) < d2 <= r*r + r
//   segment    A -> B, d = B - A (|dx|, |dy| <= max_jump <= 4095), p = P - A, dd = d.d, t = p.d, w2 = hw*hw + hw (hw <= 16):
//              t <= 0: p.p <= w2;  t >= dd: |p - d|^2 <= w2;  otherwise cross(p, d)^2 <= w2 * dd in int64.  dd == 0 is the first case
//   blend      out = (v * (255 - a) + c * a + 127) / 255 per channel: a = 255 gives c, a = 0 gives v
//
// Both coverage tests begin with a per-axis reject -- a covered pixel lies within r (hw) of the mark's centre (the segment's
// bounding box) on each axis, because r*r + r < (r + 1)^2 -- after which every int32 product is small: |p| <= 4095 + 16 per axis,
// |t|, dd, |cross| < 2^26; the squares of the last case go through int64.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CTK_DM_HD __host__ __device__ __forceinline__
#else
#define CTK_DM_HD static inline
#endif

#define CTK_DRAW_TRAIL_MAX 64
#define CTK_DRAW_RADIUS_MAX 32
#define CTK_DRAW_HALF_WIDTH_MAX 16
#define CTK_DRAW_JUMP_MAX 4095

// one component of a position: -> valid; *q = the pixel when valid
CTK_DM_HD bool ctk_draw_quant(float x, float s, int* q) {
  const float v = x * s;
  if (!(v >= -65536.0f && v <= 65536.0f)) return false;  // (NaN, +-inf: false)
  *q = (int)rintf(v);
  return true;
}

// The device form is spelt with the round-to-nearest intrinsics of emit_sigmoid / emit_visible (stream.hip), operation for operation:
// it does not lean on the translation unit's contraction or division flags.  The host form is the same three float32 operations.
#if defined(__HIP_DEVICE_COMPILE__)
CTK_DM_HD float ctk_draw_sigmoid(float x) { return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-x))); }

CTK_DM_HD bool ctk_draw_visible(float v, float c, float thresh) { return __fmul_rn(ctk_draw_sigmoid(v), ctk_draw_sigmoid(c)) > thresh; }
#else
CTK_DM_HD float ctk_draw_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

CTK_DM_HD bool ctk_draw_visible(float v, float c, float thresh) { return ctk_draw_sigmoid(v) * ctk_draw_sigmoid(c) > thresh; }
#endif

// pixel offset (dx, dy) from the mark's centre
CTK_DM_HD bool ctk_draw_mark_covers(int dx, int dy, int r, bool visible) {
  if (dx < -r || dx > r || dy < -r || dy > r) return false;
  const int d2 = dx * dx + dy * dy;
  if (d2 > r * r + r) return false;
  return visible || d2 > (r - 1) * (r - 1) + (r - 1);
}

// pixel offset p = (px, py) from A; d = B - A, |dx|, |dy| <= CTK_DRAW_JUMP_MAX
CTK_DM_HD bool ctk_draw_segment_covers(int px, int py, int dx, int dy, int hw) {
  const int x_lo = dx < 0 ? dx : 0, x_hi = dx > 0 ? dx : 0, y_lo = dy < 0 ? dy : 0, y_hi = dy > 0 ? dy : 0;
  if (px < x_lo - hw || px > x_hi + hw || py < y_lo - hw || py > y_hi + hw) return false;
  const int w2 = hw * hw + hw;
  const int dd = dx * dx + dy * dy, t = px * dx + py * dy;
  if (t <= 0) return px * px + py * py <= w2;
  if (t >= dd) {
    const int qx = px - dx, qy = py - dy;
    return qx * qx + qy * qy <= w2;
  }
  const int64_t cr = (int64_t)(px * dy - py * dx);
  return cr * cr <= (int64_t)w2 * (int64_t)dd;
}

CTK_DM_HD int ctk_draw_blend(int v, int c, int a) { return (v * (255 - a) + c * a + 127) / 255; }
