// Decoder output -> encoder input in one launch (include/ctk.h, "frame ingest"): uint8 or float32 frames, channels-last or planar,
// strided, are resized to the model resolution with the arithmetic of F.interpolate(bilinear, align_corners=True) (ingest_math.h)
// and stored as the planar float32 [F,3,h,w] frames in 0..255 that ctk_enc_stem_im2col reads.
//
// A gather with nothing worth staging: every output pixel reads its own four taps (at 1080p -> 384x512 the taps of neighbouring
// outputs are 3.7 pixels apart).  One thread computes PX output pixels of one row for all three channels -- the row taps and weights
// once, the column taps once per pixel -- and stores one float4 per channel (PX == 4), so a wave writes 1 KB contiguous per channel
// plane.  No LDS, no atomics.  The blend is written with explicit fmaf where torch's kernel has an FMA and nowhere else: this
// translation unit is compiled with -ffp-contract=off (Makefile: NOFMA).
#include "ctk_common.h"
#include "ingest_math.h"

namespace {

template <typename T, int LAYOUT>
__device__ __forceinline__ float ingest_load(const T* __restrict__ frame, long row, int x, int c, long plane) {
  return LAYOUT == CTK_INGEST_HWC ? (float)frame[row + (long)x * 3 + c] : (float)frame[(long)c * plane + row + x];
}

// grid: x = ceil(h * (w / PX) / 256), y = frame
template <typename T, int LAYOUT, int PX>
__global__ __launch_bounds__(256) void ingest_kernel(const T* __restrict__ src, int H, int W, long frame_stride, long row_stride,
                                                     float* __restrict__ dst, int h, int w, float ry, float rx) {
  const int wq = w / PX;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h * wq) return;
  const int oy = i / wq, ox = (i - oy * wq) * PX;
  const CtkIngestAxis ay = ctk_ingest_axis(ry, oy, H);
  const T* frame = src + (long)blockIdx.y * frame_stride;
  const long plane = (long)H * row_stride;  // planar source: the channel planes of a frame lie H rows apart
  const long r0 = (long)ay.i0 * row_stride, r1 = (long)ay.i1 * row_stride;
  float o[3][PX];
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    const CtkIngestAxis ax = ctk_ingest_axis(rx, ox + k, W);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      o[c][k] = ctk_ingest_blend(ingest_load<T, LAYOUT>(frame, r0, ax.i0, c, plane), ingest_load<T, LAYOUT>(frame, r0, ax.i1, c, plane),
                                 ingest_load<T, LAYOUT>(frame, r1, ax.i0, c, plane), ingest_load<T, LAYOUT>(frame, r1, ax.i1, c, plane),
                                 ax, ay);
  }
  float* out = dst + (((long)blockIdx.y * 3) * h + oy) * w + ox;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float* q = out + (long)c * h * w;
    if (PX == 4) {
      *reinterpret_cast<float4*>(q) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
    } else {
#pragma unroll
      for (int k = 0; k < PX; ++k) q[k] = o[c][k];
    }
  }
}

template <typename T, int LAYOUT>
void ingest_launch(const ctk_ingest_args* a, hipStream_t stream) {
  const float ry = ctk_ingest_scale(a->H, a->h), rx = ctk_ingest_scale(a->W, a->w);
  const T* src = static_cast<const T*>(a->src);
  if (a->w % 4 == 0) {
    const unsigned blocks = (unsigned)(((long)a->h * (a->w / 4) + 255) / 256);
    hipLaunchKernelGGL((ingest_kernel<T, LAYOUT, 4>), dim3(blocks, (unsigned)a->F), dim3(256), 0, stream, src, a->H, a->W,
                       (long)a->frame_stride, (long)a->row_stride, a->dst, a->h, a->w, ry, rx);
  } else {
    const unsigned blocks = (unsigned)(((long)a->h * a->w + 255) / 256);
    hipLaunchKernelGGL((ingest_kernel<T, LAYOUT, 1>), dim3(blocks, (unsigned)a->F), dim3(256), 0, stream, src, a->H, a->W,
                       (long)a->frame_stride, (long)a->row_stride, a->dst, a->h, a->w, ry, rx);
  }
}

}  // namespace

extern "C" int ctk_ingest_frames(const ctk_ingest_args* a, void* stream) {
  if (!a || !a->src || !a->dst) return CTK_E_NULL;
  if (a->dtype != CTK_INGEST_U8 && a->dtype != CTK_INGEST_F32) return CTK_E_SHAPE;
  if (a->layout != CTK_INGEST_HWC && a->layout != CTK_INGEST_CHW) return CTK_E_SHAPE;
  if (a->F <= 0 || a->H <= 0 || a->W <= 0 || a->h <= 0 || a->w <= 0) return CTK_E_SHAPE;
  if (a->F > 65535 || a->H > CTK_INGEST_MAX_SIDE || a->W > CTK_INGEST_MAX_SIDE || a->h > CTK_INGEST_MAX_SIDE || a->w > CTK_INGEST_MAX_SIDE)
    return CTK_E_SHAPE;
  const bool hwc = a->layout == CTK_INGEST_HWC;
  if (a->row_stride < (int64_t)a->W * (hwc ? 3 : 1)) return CTK_E_SHAPE;
  if (a->row_stride > (int64_t)1 << 40 || a->frame_stride > (int64_t)1 << 40) return CTK_E_SHAPE;
  if (a->frame_stride < a->row_stride * a->H * (hwc ? 1 : 3)) return CTK_E_SHAPE;
  // vector path (w % 4 == 0): every row of every plane then starts on a 16-byte multiple of the base
  if (a->w % 4 == 0 ? !ctk_aligned16(a->dst) : (reinterpret_cast<uintptr_t>(a->dst) & 3u) != 0) return CTK_E_ALIGN;
  if (a->dtype == CTK_INGEST_F32 && (reinterpret_cast<uintptr_t>(a->src) & 3u) != 0) return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a->dtype == CTK_INGEST_U8) {
    if (hwc) ingest_launch<uint8_t, CTK_INGEST_HWC>(a, s);
    else ingest_launch<uint8_t, CTK_INGEST_CHW>(a, s);
  } else {
    if (hwc) ingest_launch<float, CTK_INGEST_HWC>(a, s);
    else ingest_launch<float, CTK_INGEST_CHW>(a, s);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
