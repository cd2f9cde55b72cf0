// Epipolar geometry on the device (include/ctk.h, "fit epipolar"): ONE robust fundamental matrix per (group, frame) over one staged list
// of correspondences, by the rules of epipolar_math.h (and, through it, plane_math.h, objects_math.h and motion_math.h).  The frame of
// the call is ctk_fit_planes' (planes.hip): the same workgroup layout, the same slot gather, the same two-pass staging -- its loops are
// copied here, as planes.hip keeps them in an anonymous namespace; only the model differs.  One launch, no atomics, no workspace; every
// output element is one plain store.
//
// One workgroup of 256 threads owns one (group, frame).  Dynamic LDS: the list of (Px, Py, Qx, Qy) int32 points, 16 bytes each, and
// next to it a uint16 side list that leads an entry back to its slot n: N_out * 18 bytes, 144 KiB at most.
// stage     two passes over chunks of 256 slots (the rows are gathered twice): the first counts the correspondences of the fit list
//           (mask nonzero, or no mask) and the others by ballots, which gives the two segments of the list: [0, M) the fit list,
//           [M, A) the masked-out correspondences; the second places every correspondence into its segment in ascending n.
// score     a lane per hypothesis (K beyond 256: further passes) draws eight points of the fit list, eliminates its 7 x 8 system in
//           registers (epipolar_math.h: unrolled loops, compile-time indices, swaps by selects) and walks the fit list, every lane
//           reading the same LDS address (a broadcast); the keys are reduced by a wave shuffle and through LDS.
// rounds    thread 0 rebuilds the best hypothesis into LDS.  Twice: the fit list is walked two times, an entry per thread: first the
//           integer reach of the inliers (a max), then their 45 fixed-point int64 terms; sums are reduced by wave shuffles and through
//           LDS; thread 0 solves the 8 x 8 system in LDS and publishes the round's matrix there.
// outputs   all A entries are walked once more under the final matrix: label, error, and the count of the fit list's inliers.
#include "ctk_common.h"
#include "ctk_profile.h"
#include "epipolar_math.h"
#include "motion_device.h"

namespace {

constexpr int EP_CHUNK = 256;
constexpr int EP_ENTRY_BYTES = (int)sizeof(int4) + (int)sizeof(uint16_t);  // a point and its slot
constexpr int EP_SOLVE_DOUBLES = 64 + 8 + 64 + 8 + 8 + 8 + 8;              // N, b, L, D, v, z, h

struct EpipolarParams {
  int G, N, N_out, R, f0, to, lag, anchor_frame, min_points, K, T;
  uint32_t seed;
  int64_t base2;
  float sx, sy, thresh;
  const float* hc;
  const uint8_t* visible;
  const float* hv;
  const float* hf;
  const int32_t* first_row;
  const float* ac;
  const uint8_t* av;
  const int8_t* mask;
  float* fundamental;
  int8_t* label;
  float* error;
  int32_t* stats;
};

// slot n of group g: frame f (row_q of the history) against the source frame fs (row_p of the history, or of the anchor)
// -> a correspondence; *pt = (Px, Py, Qx, Qy)
__device__ __forceinline__ bool epipolar_gather(const EpipolarParams& p, long g, int f, int fs, long row_p, long row_q, int n, int4* pt) {
  if (n >= p.N_out || fs < 0) return false;
  const int first = p.first_row != nullptr ? p.first_row[g * p.N + n] : 0;
  if (f < first || fs < first) return false;
  const bool anchored = p.ac != nullptr;
  const float2 hp = *reinterpret_cast<const float2*>((anchored ? p.ac : p.hc) + (row_p + n) * 2);
  const float2 hq = *reinterpret_cast<const float2*>(p.hc + (row_q + n) * 2);
  int4 v;
  const bool ok0 = ctk_motion_quant(hp.x, p.sx, &v.x), ok1 = ctk_motion_quant(hp.y, p.sy, &v.y);
  const bool ok2 = ctk_motion_quant(hq.x, p.sx, &v.z), ok3 = ctk_motion_quant(hq.y, p.sy, &v.w);
  if (!(ok0 && ok1 && ok2 && ok3)) return false;
  *pt = v;
  const bool vq = p.visible != nullptr ? p.visible[row_q + n] != 0 : ctk_draw_visible(p.hv[row_q + n], p.hf[row_q + n], p.thresh);
  bool vp;
  if (anchored) vp = p.av[row_p + n] != 0;
  else if (p.visible != nullptr) vp = p.visible[row_p + n] != 0;
  else vp = ctk_draw_visible(p.hv[row_p + n], p.hf[row_p + n], p.thresh);
  return vp && vq;
}

__device__ __forceinline__ int epipolar_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// hypothesis k of frame f over the M >= 8 points of `list`
__device__ __forceinline__ bool epipolar_hyp_at(uint32_t seed, int64_t base2, const int4* list, int f, int k, int M, CtkEpiFit* h) {
  int i[CTK_EPI_SAMPLE], pt[CTK_EPI_SAMPLE][4];
  ctk_epi_sample(seed, f, k, M, i);
#pragma unroll
  for (int t = 0; t < CTK_EPI_SAMPLE; ++t) {
    const int4 q = list[i[t]];  // (i[t] < M: the sample's indices are distinct values below M)
    pt[t][0] = q.x, pt[t][1] = q.y, pt[t][2] = q.z, pt[t][3] = q.w;
  }
  return ctk_epi_hyp(pt, base2, h);
}

// grid: x = frame f0 + x, y = group; dynamic LDS: N_out * 18 bytes
__global__ __launch_bounds__(256) void fit_epipolar_kernel(EpipolarParams p) {
  extern __shared__ __attribute__((aligned(16))) int4 pts[];
  uint16_t* slot = reinterpret_cast<uint16_t*>(pts + p.N_out);
  // (the static part is a multiple of 16 bytes, so that the dynamic list behind it keeps its 16-byte alignment)
  __shared__ __attribute__((aligned(16))) double solve[EP_SOLVE_DOUBLES];
  __shared__ __attribute__((aligned(16))) int64_t wave_sum[4][CTK_EPI_SUMS + 1];
  __shared__ __attribute__((aligned(16))) int64_t total[CTK_EPI_SUMS + 1];
  __shared__ __attribute__((aligned(16))) int64_t wave_key[4];
  __shared__ __attribute__((aligned(16))) CtkEpiFit fit;  // 96 bytes
  __shared__ __attribute__((aligned(16))) int wave_lab[4][2];
  __shared__ __attribute__((aligned(16))) int run[2][2];
  __shared__ __attribute__((aligned(16))) int seg[4];
  __shared__ __attribute__((aligned(16))) int wave_reach[4];
  __shared__ __attribute__((aligned(16))) int wave_count[4];
  __shared__ __attribute__((aligned(16))) int fell[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int F = (int)gridDim.x, pic = (int)blockIdx.x, f = p.f0 + pic;
  const long g = (long)blockIdx.y;
  const bool anchored = p.ac != nullptr;
  const int fs = ctk_objects_source(f, p.to, p.lag, anchored, p.anchor_frame);
  const long row_q = (g * p.R + f % p.R) * p.N;
  const long row_p = anchored ? g * p.N : (fs >= 0 ? (g * p.R + fs % p.R) * p.N : 0);
  int8_t* lab_out = p.label + (g * F + pic) * (long)p.N_out;
  float* err_out = p.error + (g * F + pic) * (long)p.N_out;
  const int8_t* mask = p.mask != nullptr ? p.mask + g * p.N : nullptr;
  const double T = (double)p.T;

  // 1. stage: segment 0 = the fit list, segment 1 = the correspondences the mask keeps out of it
  {
    int cnt0 = 0, cnt1 = 0;  // of this wave
    for (int c0 = 0; c0 < p.N_out; c0 += EP_CHUNK) {
      const int n = c0 + tid;
      int4 pt;
      const int r = epipolar_gather(p, g, f, fs, row_p, row_q, n, &pt) ? (mask != nullptr && mask[n] == 0 ? 1 : 0) : -1;
      cnt0 += __popcll(__ballot(r == 0)), cnt1 += __popcll(__ballot(r == 1));
    }
    if (lane == 0) wave_lab[wave][0] = cnt0, wave_lab[wave][1] = cnt1;
    __syncthreads();
    if (tid == 0) {
      const int M = wave_lab[0][0] + wave_lab[1][0] + wave_lab[2][0] + wave_lab[3][0];
      const int B = wave_lab[0][1] + wave_lab[1][1] + wave_lab[2][1] + wave_lab[3][1];
      seg[0] = 0, seg[1] = M, seg[2] = M + B, seg[3] = 0;
      run[0][0] = 0, run[0][1] = M;
    }
    __syncthreads();
    for (int c = 0, c0 = 0; c0 < p.N_out; c0 += EP_CHUNK, ++c) {
      const int n = c0 + tid, cur = c & 1;
      int4 pt = make_int4(0, 0, 0, 0);
      const int r = epipolar_gather(p, g, f, fs, row_p, row_q, n, &pt) ? (mask != nullptr && mask[n] == 0 ? 1 : 0) : -1;
      const unsigned long long m0 = __ballot(r == 0), m1 = __ballot(r == 1);
      if (lane == 0) wave_lab[wave][0] = __popcll(m0), wave_lab[wave][1] = __popcll(m1);
      const int rank = r == 0 ? __popcll(m0 & below) : __popcll(m1 & below);
      __syncthreads();
      if (r >= 0) {
        int place = run[cur][r] + rank;
        for (int w = 0; w < wave; ++w) place += wave_lab[w][r];
        pts[place] = pt;  // (place < N_out: the segments partition the correspondences, of which there are at most N_out)
        slot[place] = (uint16_t)n;
      } else if (n < p.N_out) {
        lab_out[n] = (int8_t)-1;
        err_out[n] = -1.0f;
      }
      if (tid < 2) run[cur ^ 1][tid] = run[cur][tid] + wave_lab[0][tid] + wave_lab[1][tid] + wave_lab[2][tid] + wave_lab[3][tid];
      __syncthreads();  // the running ends of the next chunk are complete, and wave_lab is written again only behind it
    }
  }
  const int M = seg[1], A = seg[2];

  // 2. score
  int64_t best = -1;
  if (M >= CTK_EPI_SAMPLE) {
    for (int k = tid; k < p.K; k += EP_CHUNK) {
      CtkEpiFit h;
      if (!epipolar_hyp_at(p.seed, p.base2, pts, f, k, M, &h)) continue;
      int count = 0;
      for (int m = 0; m < M; ++m) {
        const int4 q = pts[m];
        count += ctk_epi_inlier(h, T, q.x, q.y, q.z, q.w) ? 1 : 0;
      }
      const int64_t key = ctk_motion_key(count, k, p.K);
      best = key > best ? key : best;
    }
  }
  best = motion_wave_max(best);
  if (lane == 0) wave_key[wave] = best;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 4; ++w) best = wave_key[w] > best ? wave_key[w] : best;

  const long o = g * F + pic;
  if (!ctk_objects_accept(best, p.min_points)) {  // (the same in every thread) no fit
    for (int m = tid; m < A; m += EP_CHUNK) {
      const int n = slot[m];
      lab_out[n] = (int8_t)0;
      err_out[n] = -1.0f;
    }
    if (tid == 0) {
      float* mo = p.fundamental + o * 9;
#pragma unroll
      for (int i = 0; i < 9; ++i) mo[i] = 0.0f;
      int32_t* st = p.stats + o * 4;
      st[0] = M, st[1] = 0, st[2] = -1, st[3] = 0;
    }
    return;
  }

  // 3. the two rounds
  if (tid == 0) {
    CtkEpiFit hb;
    epipolar_hyp_at(p.seed, p.base2, pts, f, ctk_motion_key_k(best, p.K), M, &hb);
    fit = hb;
    fell[0] = 0;
  }
  __syncthreads();
  for (int round = 0; round < 2; ++round) {
    const CtkEpiFit cur = fit;
    int reach = 0;
    for (int m = tid; m < M; m += EP_CHUNK) {
      const int4 q = pts[m];
      if (ctk_epi_inlier(cur, T, q.x, q.y, q.z, q.w)) reach = max(reach, ctk_epi_reach(cur, q.x, q.y, q.z, q.w));
    }
    reach = epipolar_wave_max(reach);
    if (lane == 0) wave_reach[wave] = reach;
    __syncthreads();
    const int e = ctk_plane_bits(max(max(wave_reach[0], wave_reach[1]), max(wave_reach[2], wave_reach[3])));
    int64_t s[CTK_EPI_SUMS];
#pragma unroll
    for (int i = 0; i < CTK_EPI_SUMS; ++i) s[i] = 0;
    for (int m = tid; m < M; m += EP_CHUNK) {
      const int4 q = pts[m];
      if (ctk_epi_inlier(cur, T, q.x, q.y, q.z, q.w)) ctk_epi_terms(cur, e, q.x, q.y, q.z, q.w, s);
    }
#pragma unroll
    for (int i = 0; i < CTK_EPI_SUMS; ++i) {
      const int64_t t = motion_wave_sum(s[i]);
      if (lane == 0) wave_sum[wave][i] = t;
    }
    __syncthreads();
    if (tid == 0) {
      for (int i = 0; i < CTK_EPI_SUMS; ++i) total[i] = wave_sum[0][i] + wave_sum[1][i] + wave_sum[2][i] + wave_sum[3][i];
      const int jstar = round == 0 ? cur.jstar : ctk_epi_largest(fit.f, 9);
      CtkEpiFit next;
      if (ctk_epi_refit(cur, jstar, e, total, solve, &next)) {
        fit = next;
      } else {
        fell[0] |= 1 << round;
        if (round == 0) {
          ctk_epi_rescale(cur, e, &next);
          fit = next;
        }
      }
    }
    __syncthreads();  // the round's matrix is published; wave_reach and wave_sum are written again only behind the next round's barriers
  }

  // 4. the outputs under the final matrix
  const CtkEpiFit fin = fit;
  int count = 0;
  for (int m = tid; m < A; m += EP_CHUNK) {
    const int4 q = pts[m];
    double r, gg;
    ctk_epi_residual(fin, q.x, q.y, q.z, q.w, &r, &gg);
    const bool in = ctk_epi_test(r, gg, fin.e, T);
    const int n = slot[m];
    lab_out[n] = in ? (int8_t)1 : (int8_t)0;
    err_out[n] = ctk_epi_error(r, gg, fin.e);
    count += (in && m < M) ? 1 : 0;
  }
  count = (int)motion_wave_sum((int64_t)count);
  if (lane == 0) wave_count[wave] = count;
  __syncthreads();
  if (tid == 0) {
    float m9[9];
    ctk_epi_pixels(fin, m9);
    float* mo = p.fundamental + o * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) mo[i] = m9[i];
    int32_t* st = p.stats + o * 4;
    st[0] = M, st[1] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3], st[2] = ctk_motion_key_k(best, p.K), st[3] = fell[0];
  }
}

bool epipolar_scale_ok(float s) { return s > 0.0f && s <= 3.402823466e+38f; }

// everything but the pointers (whether an anchor is given is looked at)
int epipolar_check_shape(const ctk_fit_epipolar_args* a) {
  const long big = 1L << 30;
  if (a->G <= 0 || a->N <= 0 || a->N_out <= 0 || a->R <= 0 || a->F <= 0 || a->N_out > a->N || a->N_out > CTK_MOTION_POINTS_MAX) return CTK_E_SHAPE;
  if (a->f0 < 0 || (long)a->f0 + a->F > big || a->F > 65535 || a->G > 65535 || (long)a->G * a->N > (1L << 26) || a->reserved != 0) return CTK_E_SHAPE;
  if (a->min_points < CTK_EPI_MIN_POINTS || a->min_points > CTK_MOTION_POINTS_MAX) return CTK_E_SHAPE;
  if (a->K < 1 || a->K > CTK_MOTION_HYPOTHESES_MAX) return CTK_E_SHAPE;
  if (ctk_motion_tol(a->tol) == 0 || ctk_motion_base2(a->min_base) < 0) return CTK_E_SHAPE;
  const bool anchored = a->anchor_coords != nullptr || a->anchor_visible != nullptr;
  if (a->to < -1 || a->to > big || a->lag > big || a->lag < 0) return CTK_E_SHAPE;
  if ((a->to >= 0 ? 1 : 0) + (a->lag != 0 ? 1 : 0) + (anchored ? 1 : 0) != 1) return CTK_E_SHAPE;
  if (anchored) {
    if (a->anchor_frame < 0 || a->anchor_frame > big || a->F > a->R) return CTK_E_SHAPE;
  } else if (a->lag != 0) {
    if ((long)a->F + a->lag > a->R) return CTK_E_SHAPE;
  } else {
    const long lo = a->to < a->f0 ? a->to : a->f0, hi = a->to > (long)a->f0 + a->F - 1 ? a->to : (long)a->f0 + a->F - 1;
    if (hi - lo + 1 > a->R) return CTK_E_SHAPE;
  }
  if (!epipolar_scale_ok(a->sx) || !epipolar_scale_ok(a->sy)) return CTK_E_SHAPE;
  if (a->visible == nullptr && a->thresh != a->thresh) return CTK_E_SHAPE;
  return CTK_OK;
}

}  // namespace

extern "C" int ctk_fit_epipolar_workspace_bytes(const ctk_fit_epipolar_args* a, size_t* out_bytes) {
  if (!a || !out_bytes) return CTK_E_NULL;
  const int rc = epipolar_check_shape(a);
  if (rc != CTK_OK) return rc;
  *out_bytes = 0;  // the one-launch form keeps everything in LDS
  return CTK_OK;
}

extern "C" int ctk_fit_epipolar(const ctk_fit_epipolar_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  if (!a) return CTK_E_NULL;
  if (!a->hist_coords || !a->fundamental || !a->label || !a->error || !a->stats) return CTK_E_NULL;
  if (!a->visible && (!a->hist_vis || !a->hist_conf)) return CTK_E_NULL;
  if ((a->anchor_coords != nullptr) != (a->anchor_visible != nullptr)) return CTK_E_NULL;
  const int rc = epipolar_check_shape(a);
  if (rc != CTK_OK) return rc;
  (void)workspace, (void)workspace_bytes;  // the query answers 0: nothing is too small
  if (((reinterpret_cast<uintptr_t>(a->hist_coords) | reinterpret_cast<uintptr_t>(a->anchor_coords)) & 7u) != 0) return CTK_E_ALIGN;
  if (((reinterpret_cast<uintptr_t>(a->fundamental) | reinterpret_cast<uintptr_t>(a->error) | reinterpret_cast<uintptr_t>(a->stats)) & 3u) != 0)
    return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);

  EpipolarParams p;
  p.G = a->G, p.N = a->N, p.N_out = a->N_out, p.R = a->R, p.f0 = a->f0, p.to = a->to, p.lag = a->lag, p.anchor_frame = a->anchor_frame;
  p.min_points = a->min_points, p.K = a->K;
  p.T = ctk_motion_tol(a->tol), p.base2 = ctk_motion_base2(a->min_base), p.seed = a->seed;
  p.sx = a->sx, p.sy = a->sy, p.thresh = a->thresh;
  p.hc = a->hist_coords, p.visible = a->visible, p.hv = a->hist_vis, p.hf = a->hist_conf, p.first_row = a->first_row;
  p.ac = a->anchor_coords, p.av = a->anchor_visible, p.mask = a->mask;
  p.fundamental = a->fundamental, p.label = a->label, p.error = a->error, p.stats = a->stats;
  {
    CtkProfScope prof("fit_epipolar", 0.0, (double)a->G * a->F * (a->N_out * 71.0 + 52.0), s);
    const size_t lds = (size_t)p.N_out * EP_ENTRY_BYTES;
    // (Beyond 64 KiB of LDS a kernel has to say so once; not a stream operation.  As planes.hip, which has the reason, from 48 KiB of
    // dynamic LDS on: this kernel holds 3.3 KiB of static LDS beside it.)
    if (lds > 49152) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fit_epipolar_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               CTK_MOTION_POINTS_MAX * EP_ENTRY_BYTES);
    hipLaunchKernelGGL(fit_epipolar_kernel, dim3((unsigned)a->F, (unsigned)p.G), dim3(256), lds, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
