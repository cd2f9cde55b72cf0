// Camera motion per frame on the device (include/ctk.h, "fit motion"): a robust fit of a translation or a similarity to the motion of
// the tracked points from frame f - lag to frame f, and the points that do not follow it, by the integer rules stated once in
// motion_math.h.  One launch, no atomics, no fill; every output element is one plain store.
//
// One workgroup of 256 threads owns one (group, frame):
// 1. stage    the two history rows are gathered once, in chunks of 256 slots, one slot per thread.  The threads whose slot is a
//             correspondence take their place m in an LDS list by a wave ballot and a prefix count (wave totals through LDS), which
//             keeps the slots' order: the numbering m is part of the rule.  A point is (Px, Py, Qx, Qy) int32, 16 bytes: the list of
//             N_out <= 8192 slots is dynamic LDS, 128 KiB at most.  A thread remembers which of its slots (one per chunk, 32 at most)
//             are in the list as one bit each, and the list place of every (chunk, wave) stays in LDS for step 3.
// 2. score    a lane takes one hypothesis (K beyond 256: further rounds) and walks m = 0 .. M - 1, every lane reading the same LDS
//             address (a broadcast), counting inliers in a register; the keys are reduced by a wave shuffle and through LDS.
// 3. refit    every thread rebuilds the winner from its key, and the chunks are walked once more: a slot's list place comes from its
//             bit, a ballot and the kept (chunk, wave) place -- nothing is gathered twice.  `inlier` is written here, -1 included, and
//             the eight int64 sums are reduced by wave shuffles and through LDS (integer adds: the order does not matter).  Thread 0
//             divides and writes the matrix and the stats.
// Shared with the other fit kernels, from fit_device.h: the source and the slot gather (CtkFitSource, fit_gather; here always the
// `lag` form: to = -1, no anchor) and the reductions.  The single-pass staging with its `mine` bits and chunk_place stays here: it
// uses the shared gather only.
#include "ctk_common.h"
#include "ctk_profile.h"
#include "fit_device.h"  // and through it motion_device.h: the wave reductions, motion_hyp_at; motion_math.h

namespace {

constexpr int MOTION_CHUNK = 256;
constexpr int MOTION_CHUNKS_MAX = CTK_MOTION_POINTS_MAX / MOTION_CHUNK;  // 32: one bit each in a thread's register

struct MotionParams {
  CtkFitSource src;
  int K, T;
  uint32_t seed;
  int64_t base2;
  float* motion;
  int8_t* inlier;
  int32_t* stats;
};

// the winner (or any hypothesis) rebuilt from its number
template <int MODEL>
__device__ __forceinline__ bool motion_make_hyp(const MotionParams& p, const int4* pts, int f, int k, int M, CtkMotionHyp* h) {
  return motion_hyp_at<MODEL>(p.seed, p.T, p.base2, pts, f, k, M, h);
}

// grid: x = frame f0 + x, y = group; dynamic LDS: N_out * 16 bytes
template <int MODEL>
__global__ __launch_bounds__(256) void fit_motion_kernel(MotionParams p) {
  extern __shared__ int4 pts[];
  __shared__ int chunk_place[MOTION_CHUNKS_MAX][4];
  __shared__ int wave_hits[4];
  __shared__ int64_t wave_key[4];
  __shared__ int64_t wave_sum[4][CTK_MS_COUNT];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const CtkFitSource& src = p.src;
  const int F = (int)gridDim.x, pic = (int)blockIdx.x, f = src.f0 + pic;
  const long g = (long)blockIdx.y;
  const FitFrame fr = fit_frame(src, g, f);

  // 1. stage
  uint32_t mine = 0;
  int M = 0;
  for (int c = 0, c0 = 0; c0 < src.N_out; c0 += MOTION_CHUNK, ++c) {
    const int n = c0 + tid;
    int4 pt = make_int4(0, 0, 0, 0);
    const bool hit = fit_gather(src, fr, n, &pt);
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) wave_hits[wave] = __popcll(mask);
    __syncthreads();
    int before = M, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int h = wave_hits[w];
      before += w < wave ? h : 0;
      total += h;
    }
    if (lane == 0) chunk_place[c][wave] = before;
    if (hit) {
      pts[before + __popcll(mask & below)] = pt;
      mine |= 1u << c;
    }
    M += total;
    __syncthreads();  // the list is read, and wave_hits written again, only behind it
  }

  // 2. score
  int64_t best = -1;
  if (M >= (MODEL == CTK_MOTION_SIMILARITY ? 2 : 1)) {
    for (int k = tid; k < p.K; k += MOTION_CHUNK) {
      CtkMotionHyp h;
      if (!motion_make_hyp<MODEL>(p, pts, f, k, M, &h)) continue;
      int count = 0;
      for (int m = 0; m < M; ++m) {
        const int4 q = pts[m];
        count += ctk_motion_inlier(MODEL, h, q.x, q.y, q.z, q.w) ? 1 : 0;
      }
      const int64_t key = ctk_motion_key(count, k, p.K);
      best = key > best ? key : best;
    }
  }
  best = fit_block_best(best, wave_key);

  // 3. refit
  const bool have = best >= 0;
  CtkMotionHyp hb;
  hb.px = hb.py = hb.qx = hb.qy = 0, hb.D = hb.A = hb.B = hb.TD = 0;
  if (have) motion_make_hyp<MODEL>(p, pts, f, ctk_motion_key_k(best, p.K), M, &hb);
  int64_t s[CTK_MS_COUNT];
#pragma unroll
  for (int i = 0; i < CTK_MS_COUNT; ++i) s[i] = 0;
  int8_t* inl = p.inlier + (g * F + pic) * (long)src.N_out;
  for (int c = 0, c0 = 0; c0 < src.N_out; c0 += MOTION_CHUNK, ++c) {
    const int n = c0 + tid;
    const bool hit = (mine >> c) & 1u;
    const unsigned long long mask = __ballot(hit);
    if (n < src.N_out) {
      int8_t v = -1;
      if (hit) {
        const int4 q = pts[chunk_place[c][wave] + __popcll(mask & below)];
        const bool in = have && ctk_motion_inlier(MODEL, hb, q.x, q.y, q.z, q.w);
        if (in) ctk_motion_accumulate(s, q.x, q.y, q.z, q.w);
        v = in ? 1 : 0;
      }
      inl[n] = v;
    }
  }
  fit_block_sums<CTK_MS_COUNT>(s, wave_sum);
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < CTK_MS_COUNT; ++i) s[i] = wave_sum[0][i] + wave_sum[1][i] + wave_sum[2][i] + wave_sum[3][i];
    float row[6];
    if (have) ctk_motion_refit(MODEL, s, row);
    else ctk_motion_identity(row);
    float* mo = p.motion + (g * F + pic) * 6;
#pragma unroll
    for (int i = 0; i < 6; ++i) mo[i] = row[i];
    int32_t* st = p.stats + (g * F + pic) * 4;
    st[0] = M, st[1] = have ? (int)s[CTK_MS_N] : 0, st[2] = have ? ctk_motion_key_k(best, p.K) : -1, st[3] = 0;
  }
}

// the source of a call: f - lag alone, no fixed frame and no anchor
CtkFitSource motion_source_of(const ctk_fit_motion_args* a) {
  CtkFitSource s;
  s.G = a->G, s.N = a->N, s.N_out = a->N_out, s.R = a->R, s.f0 = a->f0, s.to = -1, s.lag = a->lag, s.anchor_frame = 0;
  s.sx = a->sx, s.sy = a->sy, s.thresh = a->thresh;
  s.hc = a->hist_coords, s.visible = a->visible, s.hv = a->hist_vis, s.hf = a->hist_conf, s.first_row = a->first_row;
  s.ac = nullptr, s.av = nullptr;
  return s;
}

// everything but the pointers  (the source rule leaves lag >= 1 as the one form)
int motion_check_shape(const ctk_fit_motion_args* a) {
  if (!fit_check_source(motion_source_of(a), a->F) || a->reserved != 0) return CTK_E_SHAPE;
  if (a->model != CTK_MOTION_TRANSLATION && a->model != CTK_MOTION_SIMILARITY) return CTK_E_SHAPE;
  if (a->K < 1 || a->K > CTK_MOTION_HYPOTHESES_MAX) return CTK_E_SHAPE;
  if (ctk_motion_tol(a->tol) == 0 || ctk_motion_base2(a->min_base) < 0) return CTK_E_SHAPE;
  return CTK_OK;
}

}  // namespace

extern "C" int ctk_fit_motion_workspace_bytes(const ctk_fit_motion_args* a, size_t* out_bytes) {
  if (!a || !out_bytes) return CTK_E_NULL;
  const int rc = motion_check_shape(a);
  if (rc != CTK_OK) return rc;
  *out_bytes = 0;  // the one-launch form keeps everything in LDS
  return CTK_OK;
}

extern "C" int ctk_fit_motion(const ctk_fit_motion_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  if (!a) return CTK_E_NULL;
  MotionParams p;
  p.src = motion_source_of(a);
  if (fit_null_source(p.src) || !a->motion || !a->inlier || !a->stats) return CTK_E_NULL;
  const int rc = motion_check_shape(a);
  if (rc != CTK_OK) return rc;
  size_t need = 0;
  ctk_fit_motion_workspace_bytes(a, &need);
  if (workspace_bytes < need || (need > 0 && !workspace)) return CTK_E_SHAPE;
  if (!fit_align_source(p.src)) return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);

  p.K = a->K;
  p.T = ctk_motion_tol(a->tol), p.base2 = ctk_motion_base2(a->min_base), p.seed = a->seed;
  p.motion = a->motion, p.inlier = a->inlier, p.stats = a->stats;
  {
    CtkProfScope prof("fit_motion", 0.0, (double)a->G * a->F * a->N_out * 33.0, s);
    fit_launch(a->model == CTK_MOTION_SIMILARITY ? fit_motion_kernel<CTK_MOTION_SIMILARITY> : fit_motion_kernel<CTK_MOTION_TRANSLATION>,
               a->F, a->G, (size_t)a->N_out * sizeof(int4), CTK_MOTION_POINTS_MAX * (int)sizeof(int4), s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
