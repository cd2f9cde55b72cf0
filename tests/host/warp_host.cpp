// Host build of co-tracker_amd/csrc/warp_math.h behind plain loops: the rules of ctk_warp_frames and ctk_smooth_path (include/ctk.h,
// "warp frames") without a GPU (tests/test_warp_host.py).  Compile with -ffp-contract=off, like the device unit.
#include <stdint.h>

#include "../../co-tracker_amd/csrc/warp_math.h"

extern "C" int host_warp_valid(const float* m) { return ctk_warp_valid(m) ? 1 : 0; }

extern "C" void host_warp_fix(const float* m, int64_t* c) { ctk_warp_fix(m, c); }

// The whole of ctk_warp_frames, one output pixel after the other from the closed form of the coordinate (the kernel steps it);
// layout 0: [F,H,W,3], 1: [F,3,H,W]; strides in elements as in ctk_warp_args.
extern "C" void host_warp_frames(int F, int H, int W, int layout, int border, const uint8_t* fill, int64_t src_frame, int64_t src_row,
                                 int64_t dst_frame, int64_t dst_row, const float* matrices, const uint8_t* src, uint8_t* dst) {
  const int64_t xs = layout == 0 ? 3 : 1;
  for (int j = 0; j < F; ++j) {
    int64_t c[6];
    ctk_warp_fix(matrices + j * 6, c);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const int64_t X = ctk_warp_coord(c, x, y), Y = ctk_warp_coord(c + 3, x, y);
        const int ix = ctk_warp_whole(X), iy = ctk_warp_whole(Y), fx = ctk_warp_frac(X), fy = ctk_warp_frac(Y);
        for (int ch = 0; ch < 3; ++ch) {
          const uint8_t* s = src + j * src_frame + (layout == 0 ? ch : (int64_t)ch * H * src_row);
          int p[4];
          for (int t = 0; t < 4; ++t) {
            const int tx = ix + (t & 1), ty = iy + (t >> 1);
            const bool in = tx >= 0 && tx < W && ty >= 0 && ty < H;
            if (border == CTK_WARP_FILL && !in) p[t] = fill[ch];
            else p[t] = s[(int64_t)ctk_warp_clamp(ty, H) * src_row + (int64_t)ctk_warp_clamp(tx, W) * xs];
          }
          dst[j * dst_frame + (layout == 0 ? ch : (int64_t)ch * H * dst_row) + y * dst_row + x * xs] =
              (uint8_t)ctk_warp_blend(fx, fy, p[0], p[1], p[2], p[3]);
        }
      }
  }
}

// The whole of ctk_smooth_path; post may be NULL
extern "C" void host_smooth_path(int G, int F, float alpha, const float* motion, const float* post, double* state, float* warp) {
  for (int64_t g = 0; g < G; ++g)
    for (int f = 0; f < F; ++f) ctk_path_step(motion + (g * F + f) * 6, alpha, post, state + g * 6, warp + (g * F + f) * 6);
}
