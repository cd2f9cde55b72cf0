// Host build of co-tracker_amd/csrc/draw_math.h behind plain loops: the rules of ctk_draw_tracks (include/ctk.h, "draw tracks")
// without tiles, LDS or a GPU (tests/test_draw_host.py).  Compile with -ffp-contract=off, like the device unit.
#include <stdint.h>

#include "../../co-tracker_amd/csrc/draw_math.h"

// -> valid; *q = the pixel (untouched when not valid)
extern "C" int host_draw_quant(float x, float s, int* q) { return ctk_draw_quant(x, s, q) ? 1 : 0; }

extern "C" int host_draw_visible(float v, float c, float thresh) { return ctk_draw_visible(v, c, thresh) ? 1 : 0; }

// out [(2 span + 1)^2]: the offsets dy, dx = -span .. span, row-major
extern "C" void host_draw_mark_mask(int r, int visible, int span, uint8_t* out) {
  for (int dy = -span; dy <= span; ++dy)
    for (int dx = -span; dx <= span; ++dx) *out++ = ctk_draw_mark_covers(dx, dy, r, visible != 0) ? 1 : 0;
}

extern "C" int host_draw_mark_at(int dx, int dy, int r, int visible) { return ctk_draw_mark_covers(dx, dy, r, visible != 0) ? 1 : 0; }

// out [(y1 - y0 + 1) * (x1 - x0 + 1)]: the offsets p = (px, py) from A over [x0, x1] x [y0, y1], row-major
extern "C" void host_draw_segment_mask(int dx, int dy, int hw, int x0, int x1, int y0, int y1, uint8_t* out) {
  for (int py = y0; py <= y1; ++py)
    for (int px = x0; px <= x1; ++px) *out++ = ctk_draw_segment_covers(px, py, dx, dy, hw) ? 1 : 0;
}

// out [256 * 256]: blend(v, c, a) at [v * 256 + c]
extern "C" void host_draw_blend_table(int a, uint8_t* out) {
  for (int v = 0; v < 256; ++v)
    for (int c = 0; c < 256; ++c) *out++ = (uint8_t)ctk_draw_blend(v, c, a);
}
