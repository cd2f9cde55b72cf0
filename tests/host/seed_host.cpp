// Host build of co-tracker_amd/csrc/seed_math.h behind a plain loop: the rules of ctk_seed_points (include/ctk.h, "seed points")
// without tiles, LDS or a GPU (tests/test_seed_host.py).  Compile with -ffp-contract=off, like the device unit.
#include <stdint.h>

#include <vector>

#include "../../co-tracker_amd/csrc/seed_math.h"

namespace {
// the score of every pixel: luminance, gradients and the direct window sum, all through the header's functions
void scores_of(const float* frame, int h, int w, int r, std::vector<int>& sc) {
  const long plane = (long)h * w;
  std::vector<int> lum(plane), gx(plane), gy(plane);
  for (long i = 0; i < plane; ++i) lum[i] = ctk_seed_luma(frame[i], frame[plane + i], frame[2 * plane + i]);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const int xm = x > 0 ? x - 1 : 0, xp = x < w - 1 ? x + 1 : w - 1, ym = y > 0 ? y - 1 : 0, yp = y < h - 1 ? y + 1 : h - 1;
      gx[(long)y * w + x] = lum[(long)y * w + xp] - lum[(long)y * w + xm];
      gy[(long)y * w + x] = lum[(long)yp * w + x] - lum[(long)ym * w + x];
    }
  sc.assign(plane, 0);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      int a = 0, b = 0, c = 0;
      for (int v = y - r; v <= y + r; ++v)
        for (int u = x - r; u <= x + r; ++u) {
          if (v < 0 || v >= h || u < 0 || u >= w) continue;
          const int dx = gx[(long)v * w + u], dy = gy[(long)v * w + u];
          a += dx * dx, b += dx * dy, c += dy * dy;
        }
      sc[(long)y * w + x] = ctk_seed_score(a, b, c);
    }
}
}  // namespace

extern "C" long long host_seed_ceil_sqrt(long long d) { return (long long)ctk_seed_ceil_sqrt((int64_t)d); }

extern "C" int host_seed_cell_axis(float x, float lo, float inv, int g) { return ctk_seed_cell_axis(x, lo, inv, g); }

// scores: [h,w] int32, or NULL; seeds: [gh*gw,3] int32
extern "C" int host_seed_points(const float* frame, int h, int w, int radius, int margin, int inset, int min_score, float x_lo, float x_hi,
                                float y_lo, float y_hi, int gh, int gw, float inv_cw, float inv_ch, int32_t* scores, int32_t* seeds) {
  std::vector<int> sc;
  scores_of(frame, h, w, radius, sc);
  if (scores)
    for (long i = 0; i < (long)h * w; ++i) scores[i] = sc[i];
  for (int cy = 0; cy < gh; ++cy)
    for (int cx = 0; cx < gw; ++cx) {
      int X0, X1, Y0, Y1;
      ctk_seed_candidates(cx, x_lo, x_hi, inv_cw, gw, w, margin, inset, &X0, &X1);
      ctk_seed_candidates(cy, y_lo, y_hi, inv_ch, gh, h, margin, inset, &Y0, &Y1);
      int64_t best = -1;
      for (int y = Y1; y >= Y0; --y)  // (any order: the key decides)
        for (int x = X0; x <= X1; ++x) {
          const int64_t k = ctk_seed_key(sc[(long)y * w + x], y, x);
          if (k > best) best = k;
        }
      int32_t* out = seeds + ((long)cy * gw + cx) * 3;
      if (best < 0 || ctk_seed_key_score(best) < min_score) {
        out[0] = out[1] = out[2] = -1;
      } else {
        out[0] = ctk_seed_key_px(best), out[1] = ctk_seed_key_py(best), out[2] = ctk_seed_key_score(best);
      }
    }
  return 0;
}
