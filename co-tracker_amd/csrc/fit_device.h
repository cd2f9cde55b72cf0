// What the robust-fit kernels share (motion.hip, objects.hip, planes.hip, epipolar.hip, pose.hip, resection.hip), stated once: which
// history a call reads and which slots of it are correspondences (CtkFitSource, fit_frame, fit_gather), the two-pass staging of a list
// in segments (fit_stage), the workgroup reductions, and on the host the checks of the source fields and the launch.  The rules
// themselves are the *_math.h headers'; the wave reductions of a key and of a sum and motion_hyp_at are motion_device.h's.
#pragma once
#include <math.h>

#include "ctk_common.h"
#include "motion_device.h"
#include "objects_math.h"

// The source of a call: the ring history of G groups, N slots a row, R rows, of which frames f0 .. f0 + F - 1 are fitted against
// exactly one of a fixed frame `to` >= 0, the frame f - lag, or an anchor (ac, av) taken on anchor_frame.
struct CtkFitSource {
  int G, N, N_out, R, f0, to, lag, anchor_frame;
  float sx, sy, thresh;
  const float* hc;
  const uint8_t* visible;
  const float* hv;
  const float* hf;
  const int32_t* first_row;
  const float* ac;
  const uint8_t* av;
};

// (the args structs with `to` and an anchor name these fields alike; ctk_fit_motion_args has neither and fills its source by hand)
template <class Args>
CtkFitSource fit_source_of(const Args* a) {
  CtkFitSource s;
  s.G = a->G, s.N = a->N, s.N_out = a->N_out, s.R = a->R, s.f0 = a->f0, s.to = a->to, s.lag = a->lag, s.anchor_frame = a->anchor_frame;
  s.sx = a->sx, s.sy = a->sy, s.thresh = a->thresh;
  s.hc = a->hist_coords, s.visible = a->visible, s.hv = a->hist_vis, s.hf = a->hist_conf, s.first_row = a->first_row;
  s.ac = a->anchor_coords, s.av = a->anchor_visible;
  return s;
}

// frame f of group g against its source frame fs (< 0: none): row_q of the history against row_p of the history, or of the anchor
struct FitFrame {
  long g;
  int f, fs;
  long row_p, row_q;
};

__device__ __forceinline__ FitFrame fit_frame(const CtkFitSource& s, long g, int f) {
  // (fit_check_source grants it.  Said here because a chunk loop that might run zero times leaves a path on which a scalar load of
  // the kernel arguments is still in flight behind it; scalar loads return out of order, so every LDS wait in the scoring loop
  // that follows became a wait for all reads instead of the oldest: fit_motion<0>, 1024 hypotheses, 0.174 -> 0.188 ms.)
  __builtin_assume(s.N_out > 0);
  const bool anchored = s.ac != nullptr;
  FitFrame fr;
  fr.g = g, fr.f = f, fr.fs = ctk_objects_source(f, s.to, s.lag, anchored, s.anchor_frame);
  fr.row_q = (g * s.R + f % s.R) * s.N;
  fr.row_p = anchored ? g * s.N : (fr.fs >= 0 ? (g * s.R + fr.fs % s.R) * s.N : 0);
  return fr;
}

// slot n -> a correspondence; *pt = (Px, Py, Qx, Qy).  The one place that decides it: both frames at or above the slot's first row,
// four coordinates the quantiser takes, and both ends visible (`visible`, or the logits against thresh, or the anchor's own flags).
__device__ __forceinline__ bool fit_gather(const CtkFitSource& s, const FitFrame& fr, int n, int4* pt) {
  if (n >= s.N_out || fr.fs < 0) return false;
  const int first = s.first_row != nullptr ? s.first_row[fr.g * s.N + n] : 0;
  if (fr.f < first || fr.fs < first) return false;
  const bool anchored = s.ac != nullptr;
  const float2 hp = *reinterpret_cast<const float2*>((anchored ? s.ac : s.hc) + (fr.row_p + n) * 2);
  const float2 hq = *reinterpret_cast<const float2*>(s.hc + (fr.row_q + n) * 2);
  int4 v;
  const bool ok0 = ctk_motion_quant(hp.x, s.sx, &v.x), ok1 = ctk_motion_quant(hp.y, s.sy, &v.y);
  const bool ok2 = ctk_motion_quant(hq.x, s.sx, &v.z), ok3 = ctk_motion_quant(hq.y, s.sy, &v.w);
  if (!(ok0 && ok1 && ok2 && ok3)) return false;
  *pt = v;
  const bool vq = s.visible != nullptr ? s.visible[fr.row_q + n] != 0 : ctk_draw_visible(s.hv[fr.row_q + n], s.hf[fr.row_q + n], s.thresh);
  bool vp;
  if (anchored) vp = s.av[fr.row_p + n] != 0;
  else if (s.visible != nullptr) vp = s.visible[fr.row_p + n] != 0;
  else vp = ctk_draw_visible(s.hv[fr.row_p + n], s.hf[fr.row_p + n], s.thresh);
  return vp && vq;
}

// ---- the staging of a list in NSEG segments, by a workgroup of 256 threads ---------------------------------------------------------------

template <int NSEG>
struct __attribute__((aligned(16))) FitStageLds {  // (a multiple of 16 bytes: a dynamic list behind the static part keeps its alignment)
  int wave_lab[4][NSEG];
  int run[2][NSEG];
  int seg[NSEG + 1];  // segment q of the list is [seg[q], seg[q + 1])
};

// Two passes over chunks of 256 slots, a slot per thread (the rows are gathered twice).  The first counts the correspondences of every
// segment by ballots, which gives L.seg; the second places each into its segment in ascending n -- the order is part of the rules --
// as (pts[place], slot[place] = n).  gather(n, &pt) -> slot n is a correspondence; classify(n) -> its segment, or -1 (asked of
// correspondences only); reject(n, hit) stores the outputs of a slot n < N_out that enters no segment.  L.seg is complete on return.
template <int NSEG, class Gather, class Classify, class Reject>
__device__ __forceinline__ void fit_stage(FitStageLds<NSEG>& L, int N_out, int4* pts, uint16_t* slot, Gather gather, Classify classify,
                                          Reject reject) {
  static_assert(NSEG <= 64, "a lane per segment publishes the wave's counts");
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  int cnt[NSEG];  // of this wave, per segment
#pragma unroll
  for (int q = 0; q < NSEG; ++q) cnt[q] = 0;
  for (int c0 = 0; c0 < N_out; c0 += 256) {
    const int n = c0 + tid;
    int4 pt;
    const int r = gather(n, &pt) ? classify(n) : -1;
#pragma unroll
    for (int q = 0; q < NSEG; ++q) cnt[q] += __popcll(__ballot(r == q));
  }
#pragma unroll
  for (int q = 0; q < NSEG; ++q)
    if (lane == q) L.wave_lab[wave][q] = cnt[q];
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int q = 0; q < NSEG; ++q) {
      L.seg[q] = s, L.run[0][q] = s;
      s += L.wave_lab[0][q] + L.wave_lab[1][q] + L.wave_lab[2][q] + L.wave_lab[3][q];
    }
    L.seg[NSEG] = s;
  }
  __syncthreads();
  // Two barriers a chunk suffice: the running segment ends are double-buffered, so a chunk reads run[cur] while run[cur ^ 1] is
  // written, and wave_lab is read between the chunk's barriers only.
  for (int c = 0, c0 = 0; c0 < N_out; c0 += 256, ++c) {
    const int n = c0 + tid, cur = c & 1;
    int4 pt = make_int4(0, 0, 0, 0);
    const bool hit = gather(n, &pt);
    const int r = hit ? classify(n) : -1;
    int rank = 0;
#pragma unroll
    for (int q = 0; q < NSEG; ++q) {
      const unsigned long long mask = __ballot(r == q);
      if (lane == q) L.wave_lab[wave][q] = __popcll(mask);
      if (r == q) rank = __popcll(mask & below);
    }
    __syncthreads();
    if (r >= 0) {
      int place = L.run[cur][r] + rank;
      for (int w = 0; w < wave; ++w) place += L.wave_lab[w][r];
      pts[place] = pt;  // (place < N_out: the segments partition the correspondences, of which there are at most N_out)
      slot[place] = (uint16_t)n;
    } else if (n < N_out) {
      reject(n, hit);
    }
    if (tid < NSEG) L.run[cur ^ 1][tid] = L.run[cur][tid] + L.wave_lab[0][tid] + L.wave_lab[1][tid] + L.wave_lab[2][tid] + L.wave_lab[3][tid];
    __syncthreads();  // the running ends of the next chunk are complete, and wave_lab is written again only behind it
  }
}

// ---- reductions over a wave and over the four waves of a workgroup ------------------------------------------------------------------------

__device__ __forceinline__ int fit_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

__device__ __forceinline__ int fit_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// the workgroup's best key, in every thread; holds a barrier: wave_key may be written again behind the caller's next one
__device__ __forceinline__ int64_t fit_block_best(int64_t best, int64_t* wave_key) {
  best = motion_wave_max(best);
  if ((threadIdx.x & 63) == 0) wave_key[threadIdx.x >> 6] = best;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 4; ++w) best = wave_key[w] > best ? wave_key[w] : best;
  return best;
}

// the wave's sum of every s[i] into wave_sum[wave][i]; the barrier and the total over the four waves are the caller's
template <int COUNT, int ROW>
__device__ __forceinline__ void fit_block_sums(const int64_t* s, int64_t (*wave_sum)[ROW]) {
  static_assert(COUNT <= ROW, "a row holds the sums");
#pragma unroll
  for (int i = 0; i < COUNT; ++i) {
    const int64_t t = motion_wave_sum(s[i]);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6][i] = t;
  }
}

// ---- the host side: what every entry point checks of its source, and the launch -----------------------------------------------------------

static inline bool fit_scale_ok(float s) { return s > 0.0f && s <= 3.402823466e+38f; }
static inline bool fit_finite(float s) { return fabsf(s) <= 3.402823466e+38f; }  // (a NaN fails the comparison)

// CTK_E_NULL: the history and one of its visibility forms, and an anchor's two pointers together
static inline bool fit_null_source(const CtkFitSource& s) {
  return !s.hc || (!s.visible && (!s.hv || !s.hf)) || (s.ac != nullptr) != (s.av != nullptr);
}

// CTK_E_SHAPE: everything of the source but the pointers (whether an anchor is given is looked at).  Exactly one source form, and
// the rows a call reads must be distinct rows of the ring.
static inline bool fit_check_source(const CtkFitSource& s, int F) {
  const long big = 1L << 30;
  if (s.G <= 0 || s.N <= 0 || s.N_out <= 0 || s.R <= 0 || F <= 0 || s.N_out > s.N || s.N_out > CTK_MOTION_POINTS_MAX) return false;
  if (s.f0 < 0 || (long)s.f0 + F > big || F > 65535 || s.G > 65535 || (long)s.G * s.N > (1L << 26)) return false;
  const bool anchored = s.ac != nullptr || s.av != nullptr;
  if (s.to < -1 || s.to > big || s.lag > big || s.lag < 0) return false;
  if ((s.to >= 0 ? 1 : 0) + (s.lag != 0 ? 1 : 0) + (anchored ? 1 : 0) != 1) return false;
  if (anchored) {
    if (s.anchor_frame < 0 || s.anchor_frame > big || F > s.R) return false;
  } else if (s.lag != 0) {
    if ((long)F + s.lag > s.R) return false;
  } else {
    const long lo = s.to < s.f0 ? s.to : s.f0, hi = s.to > (long)s.f0 + F - 1 ? s.to : (long)s.f0 + F - 1;
    if (hi - lo + 1 > s.R) return false;
  }
  if (!fit_scale_ok(s.sx) || !fit_scale_ok(s.sy)) return false;
  if (s.visible == nullptr && s.thresh != s.thresh) return false;
  return true;
}

// CTK_E_SHAPE: the pinhole camera of an args struct
template <class Args>
bool fit_check_camera(const Args* a) {
  return fit_scale_ok(a->fx) && fit_scale_ok(a->fy) && fit_finite(a->cx) && fit_finite(a->cy);
}

// CTK_E_ALIGN: positions are read two floats at a time
static inline bool fit_align_source(const CtkFitSource& s) {
  return ((reinterpret_cast<uintptr_t>(s.hc) | reinterpret_cast<uintptr_t>(s.ac)) & 7u) == 0;
}

// One workgroup of 256 threads per (frame, group) of F frames and G groups, with `lds` bytes of dynamic LDS, lds_max at the largest call.  Beyond 64 KiB of LDS a
// kernel has to say so once (not a stream operation).  Whether the static LDS beside the list counts towards the 64 KiB is not written
// down anywhere, and the kernels hold up to 9.5 KiB of it, so every one says so from 48 KiB of dynamic LDS on: early costs nothing.
template <class Params>
void fit_launch(void (*kernel)(Params), int F, int G, size_t lds, int lds_max, hipStream_t stream, const Params& p) {
  if (lds > 49152) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
  hipLaunchKernelGGL(kernel, dim3((unsigned)F, (unsigned)G), dim3(256), lds, stream, p);
}
