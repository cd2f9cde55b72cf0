// Device helpers shared by the robust-fit kernels: the wave reductions of a key and of a sum, and a hypothesis rebuilt from its number
// over a list of (Px, Py, Qx, Qy) points in LDS (motion.hip, objects.hip).  The rules themselves are motion_math.h's.  The kernels
// include fit_device.h, which includes this header and holds what else they share.
#pragma once
#include <hip/hip_runtime.h>

#include "motion_math.h"

__device__ __forceinline__ int64_t motion_wave_max(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t w = __shfl_xor((long long)v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

__device__ __forceinline__ int64_t motion_wave_sum(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor((long long)v, o, 64);
  return v;
}

// hypothesis k of frame f over the M points of pts, sampled with `seed`
template <int MODEL>
__device__ __forceinline__ bool motion_hyp_at(uint32_t seed, int T, int64_t base2, const int4* pts, int f, int k, int M, CtkMotionHyp* h) {
  int i, j;
  ctk_motion_sample(seed, f, k, M, MODEL, &i, &j);
  const int4 a = pts[i], b = pts[j];
  return ctk_motion_hyp(MODEL, a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, T, base2, h);
}
