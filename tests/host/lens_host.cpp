// Host build of co-tracker_amd/csrc/lens_math.h behind plain loops: the rules of ctk_lens_frames and ctk_lens_points (include/ctk.h,
// "lens") without a GPU (tests/test_lens_host.py).  Compile with -ffp-contract=off, like the device unit.
#include <stdint.h>

#include "../../co-tracker_amd/csrc/lens_math.h"

// lens: 13 doubles, sensor (fx, fy, cx, cy), ideal (fx', fy', cx', cy'), k (k1, k2, p1, p2, k3)
extern "C" int host_lens_valid(const double* lens) { return ctk_lens_valid(lens, lens + 4, lens + 8) ? 1 : 0; }

// forward and jacobian of n normalised positions: out [n,6] = (xd, yd, a, b, d, det)
extern "C" void host_lens_forward(const double* k, int64_t n, const double* xy, double* out) {
  for (int64_t i = 0; i < n; ++i) ctk_lens_forward(k, xy[2 * i], xy[2 * i + 1], out + 6 * i, out + 6 * i + 1, out + 6 * i + 2);
}

// the Newton inverse of n normalised positions: out [n,2], accepted [n]
extern "C" void host_lens_inverse(const double* k, double fx, double fy, float tol, int64_t n, const double* xy, double* out, int8_t* accepted) {
  const double tol2 = (double)tol * (double)tol;
  for (int64_t i = 0; i < n; ++i) accepted[i] = ctk_lens_inverse(k, fx, fy, tol2, xy[2 * i], xy[2 * i + 1], out + 2 * i, out + 2 * i + 1) ? 1 : 0;
}

// The whole of ctk_lens_points over n dense positions; dst may be src; label may be NULL
extern "C" void host_lens_points(const double* lens, int direction, float tol, int64_t n, const float* src, float* dst, int8_t* label) {
  ctk_lens_rule r;
  ctk_lens_prepare(lens, lens + 4, lens + 8, direction, tol, &r);
  for (int64_t i = 0; i < n; ++i) {
    uint32_t* o = reinterpret_cast<uint32_t*>(dst) + 2 * i;
    uint32_t q[2];
    const int lab = ctk_lens_point(&r, src[2 * i], src[2 * i + 1], q);
    o[0] = q[0], o[1] = q[1];
    if (label) label[i] = (int8_t)lab;
  }
}

// The whole of ctk_lens_frames, one output pixel after the other; layout 0: [F,H,W,3], 1: [F,3,H,W]; strides in elements as in
// ctk_lens_frames_args.
extern "C" void host_lens_frames(const double* lens, int direction, float tol, int F, int H, int W, int Ho, int Wo, int layout, int border,
                                 const uint8_t* fill, int64_t src_frame, int64_t src_row, int64_t dst_frame, int64_t dst_row,
                                 const uint8_t* src, uint8_t* dst) {
  ctk_lens_rule r;
  ctk_lens_prepare(lens, lens + 4, lens + 8, direction == CTK_LENS_TO_IDEAL ? CTK_LENS_TO_SENSOR : CTK_LENS_TO_IDEAL, tol, &r);
  const int64_t xs = layout == 0 ? 3 : 1;
  for (int y = 0; y < Ho; ++y)
    for (int x = 0; x < Wo; ++x) {
      int64_t X, Y;
      const bool inside = ctk_lens_coord(&r, x, y, &X, &Y);
      const int ix = ctk_lens_whole(X), iy = ctk_lens_whole(Y), fx = ctk_lens_frac(X), fy = ctk_lens_frac(Y);
      for (int j = 0; j < F; ++j)
        for (int ch = 0; ch < 3; ++ch) {
          uint8_t* o = dst + j * dst_frame + (layout == 0 ? ch : (int64_t)ch * Ho * dst_row) + y * dst_row + x * xs;
          if (!inside) {
            *o = fill[ch];
            continue;
          }
          const uint8_t* s = src + j * src_frame + (layout == 0 ? ch : (int64_t)ch * H * src_row);
          int p[4];
          for (int t = 0; t < 4; ++t) {
            const int tx = ix + (t & 1), ty = iy + (t >> 1);
            const bool in = tx >= 0 && tx < W && ty >= 0 && ty < H;
            if (border == CTK_WARP_FILL && !in) p[t] = fill[ch];
            else p[t] = s[(int64_t)ctk_warp_clamp(ty, H) * src_row + (int64_t)ctk_warp_clamp(tx, W) * xs];
          }
          *o = (uint8_t)ctk_warp_blend(fx, fy, p[0], p[1], p[2], p[3]);
        }
    }
}
