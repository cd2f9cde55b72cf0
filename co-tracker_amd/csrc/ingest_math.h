// Arithmetic of F.interpolate(x, (h, w), mode="bilinear", align_corners=True) as the predictors call it (predictor.py:288-290 of the
// reference), restated ONCE for the device kernel (ingest.hip) and for a host build of the same text (tests/test_ingest_host.py
// compiles this header with g++ and compares it with a float64 evaluation and with torch on the CPU -- no GPU needed to pin it).
//
// ATen's upsample_bilinear2d_out_frame (aten/src/ATen/native/cuda/UpSampleBilinear2d.cu), all in float32:
//   r  = out > 1 ? (float)(in - 1) / (out - 1) : 0          area_pixel_compute_scale, align_corners
//   s  = r * o;  i0 = (int)s;  i1 = i0 + (i0 < in - 1);  l1 = s - i0;  l0 = 1 - l1
//   v  = l0y * (l0x * p00 + l1x * p01) + l1y * (l0x * p10 + l1x * p11)
// Which of these the GPU build of torch contracts was established on an MI355X against torch 2.10 (rocm 7.0): the coordinate
// steps are NOT contracted (l1 = s - i0 with s rounded), and the blend is
//   v  = fma(l0y, fma(l0x, p00, l1x * p01), l1y * fma(l0x, p10, l1x * p11))
// -- of each sum a*b + c*d the FIRST product is fused and the second is rounded.  With that form 0 of 589 824 outputs differ for
// 1080x1920 -> 384x512, 480x640 -> 384x512 and 100x100 -> 384x512 (torch's CPU kernel gives the same bits); every other placement
// of the FMAs differs in 17-28 % of the outputs.  Every operation below is one explicitly rounded operation: compile with
// -ffp-contract=off.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define CTK_IM_HD __host__ __device__ __forceinline__
#else
#define CTK_IM_HD static inline
#endif

struct CtkIngestAxis {
  int i0, i1;    // the two source indices: i1 == i0 on the last row / column, so nothing past the image is ever read
  float l0, l1;  // their weights
};

CTK_IM_HD float ctk_ingest_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f; }

CTK_IM_HD CtkIngestAxis ctk_ingest_axis(float scale, int o, int in) {
  const float s = scale * (float)o;
  CtkIngestAxis a;
  a.i0 = (int)s;
  if (a.i0 > in - 1) a.i0 = in - 1;  // defence only: r * (out - 1) rounds to at most in - 1 for every size the entry point admits
  a.i1 = a.i0 + (a.i0 < in - 1 ? 1 : 0);
  a.l1 = s - (float)a.i0;
  a.l0 = 1.0f - a.l1;
  return a;
}

CTK_IM_HD float ctk_ingest_blend(float p00, float p01, float p10, float p11, const CtkIngestAxis& x, const CtkIngestAxis& y) {
  const float top = fmaf(x.l0, p00, x.l1 * p01);
  const float bot = fmaf(x.l0, p10, x.l1 * p11);
  return fmaf(y.l0, top, y.l1 * bot);
}
