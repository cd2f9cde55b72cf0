// Host build of co-tracker_amd/csrc/ingest_math.h behind the loop of the device kernel (csrc/ingest.hip): the same index and stride
// rules, the same arithmetic text, no GPU (tests/test_ingest_host.py).  Compile with -ffp-contract=off, like the device unit.
#include <stdint.h>

#include "../../co-tracker_amd/csrc/ingest_math.h"

namespace {
template <typename T>
void run(const T* src, int hwc, int F, int H, int W, long frame_stride, long row_stride, float* dst, int h, int w, long* max_index) {
  const float ry = ctk_ingest_scale(H, h), rx = ctk_ingest_scale(W, w);
  const long plane = (long)H * row_stride;
  long top = 0;
  for (int f = 0; f < F; ++f)
    for (int oy = 0; oy < h; ++oy) {
      const CtkIngestAxis ay = ctk_ingest_axis(ry, oy, H);
      for (int ox = 0; ox < w; ++ox) {
        const CtkIngestAxis ax = ctk_ingest_axis(rx, ox, W);
        for (int c = 0; c < 3; ++c) {
          const int ys[2] = {ay.i0, ay.i1}, xs[2] = {ax.i0, ax.i1};
          float p[2][2];
          for (int j = 0; j < 2; ++j)
            for (int i = 0; i < 2; ++i) {
              const long at = (long)f * frame_stride + (hwc ? (long)ys[j] * row_stride + (long)xs[i] * 3 + c
                                                            : (long)c * plane + (long)ys[j] * row_stride + xs[i]);
              if (at > top) top = at;
              p[j][i] = (float)src[at];
            }
          dst[(((long)f * 3 + c) * h + oy) * w + ox] = ctk_ingest_blend(p[0][0], p[0][1], p[1][0], p[1][1], ax, ay);
        }
      }
    }
  if (max_index) *max_index = top;
}
}  // namespace

// dtype 0: uint8, 1: float32; hwc 1: channels-last, 0: planar.  max_index: the largest source element that was read.
extern "C" int host_ingest_frames(const void* src, int dtype, int hwc, int F, int H, int W, long frame_stride, long row_stride, float* dst,
                                  int h, int w, long* max_index) {
  if (dtype == 0) run(static_cast<const uint8_t*>(src), hwc, F, H, W, frame_stride, row_stride, dst, h, w, max_index);
  else run(static_cast<const float*>(src), hwc, F, H, W, frame_stride, row_stride, dst, h, w, max_index);
  return 0;
}
