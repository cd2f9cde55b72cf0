// Planes on the device (include/ctk.h, "fit planes / warp planes"): up to L robust homography fits per (group, frame) over sub-lists
// of ONE staged list of correspondences, by the rules of plane_math.h (and, through it, objects_math.h and motion_math.h).  The frame
// of the call is ctk_fit_objects' labels mode (objects.hip): the same workgroup layout, the same slot gather, the same staging -- its
// loops are copied here, as objects.hip keeps them in an anonymous namespace; only the model differs.  One launch, no atomics, no
// workspace; every output element is one plain store.
//
// One workgroup of 256 threads owns one (group, frame).  Dynamic LDS: the list of (Px, Py, Qx, Qy) int32 points, 16 bytes each, and
// next to it a uint16 side list that leads an entry back to its slot n: N_out * 18 bytes, 144 KiB at most.
// stage     two passes over chunks of 256 slots (the rows are gathered twice): the first counts the correspondences of every label by
//           per-label ballots, which gives each label's segment of the list; the second places every correspondence into its label's
//           segment in ascending n.  Without labels every correspondence has label 0.  inverse = 1 swaps P and Q as a point is gathered.
// round r   score: a lane per hypothesis (K beyond 256: further passes) builds its matrix from four points of the list and walks the
//           list, every lane reading the same LDS address (a broadcast); the keys are reduced by a wave shuffle and through LDS.
//           refit: the list is walked twice more, an entry per thread: first the integer reach of the inliers (a max), then their 23
//           fixed-point int64 terms, the box and the labels.  Sums and box are reduced by wave shuffles and through LDS; thread 0
//           solves the 8 x 8 system in LDS and writes the round's matrix, stats and box.
#include "ctk_common.h"
#include "ctk_profile.h"
#include "motion_device.h"
#include "plane_math.h"

namespace {

constexpr int PL_CHUNK = 256;
constexpr int PL_ENTRY_BYTES = (int)sizeof(int4) + (int)sizeof(uint16_t);  // a point and its slot
constexpr int PL_SOLVE_DOUBLES = 64 + 8 + 64 + 8 + 8 + 8 + 8;              // N, b, L, D, v, z, h

struct PlanesParams {
  int G, N, N_out, R, f0, to, lag, anchor_frame, L, min_points, K, T, inverse;
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
  const int8_t* labels;
  float* homography;
  int8_t* label;
  int32_t* stats;
  int32_t* box;
};

// slot n of group g: frame f (row_q of the history) against the source frame fs (row_p of the history, or of the anchor)
// -> a correspondence; *pt = (Px, Py, Qx, Qy), the two swapped when inverse is set
__device__ __forceinline__ bool planes_gather(const PlanesParams& p, long g, int f, int fs, long row_p, long row_q, int n, int4* pt) {
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
  *pt = p.inverse ? make_int4(v.z, v.w, v.x, v.y) : v;
  const bool vq = p.visible != nullptr ? p.visible[row_q + n] != 0 : ctk_draw_visible(p.hv[row_q + n], p.hf[row_q + n], p.thresh);
  bool vp;
  if (anchored) vp = p.av[row_p + n] != 0;
  else if (p.visible != nullptr) vp = p.visible[row_p + n] != 0;
  else vp = ctk_draw_visible(p.hv[row_p + n], p.hf[row_p + n], p.thresh);
  return vp && vq;
}

__device__ __forceinline__ int planes_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

__device__ __forceinline__ int planes_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// hypothesis k of frame f over the M >= 4 points of `list`, sampled with `seed`
__device__ __forceinline__ bool planes_hyp_at(uint32_t seed, int64_t base2, const int4* list, int f, int k, int M, CtkPlaneHyp* h) {
  int i[4], pt[4][4];
  ctk_plane_sample(seed, f, k, M, i);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int4 q = list[i[t]];
    pt[t][0] = q.x, pt[t][1] = q.y, pt[t][2] = q.z, pt[t][3] = q.w;
  }
  return ctk_plane_hyp(pt, base2, h);
}

// grid: x = frame f0 + x, y = group; dynamic LDS: N_out * 18 bytes
__global__ __launch_bounds__(256) void fit_planes_kernel(PlanesParams p) {
  extern __shared__ int4 pts[];
  uint16_t* slot = reinterpret_cast<uint16_t*>(pts + p.N_out);
  __shared__ int wave_lab[4][CTK_PLANES_MAX];
  __shared__ int run[2][CTK_PLANES_MAX];
  __shared__ int seg[CTK_PLANES_MAX + 1];
  __shared__ int64_t wave_key[4];
  __shared__ int64_t wave_sum[4][CTK_PS_COUNT];
  __shared__ int wave_box[4][4];
  __shared__ int wave_reach[4];
  __shared__ double solve[PL_SOLVE_DOUBLES];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int F = (int)gridDim.x, pic = (int)blockIdx.x, f = p.f0 + pic;
  const long g = (long)blockIdx.y;
  const bool anchored = p.ac != nullptr;
  const int fs = ctk_objects_source(f, p.to, p.lag, anchored, p.anchor_frame);
  const long row_q = (g * p.R + f % p.R) * p.N;
  const long row_p = anchored ? g * p.N : (fs >= 0 ? (g * p.R + fs % p.R) * p.N : 0);
  int8_t* lab_out = p.label + (g * F + pic) * (long)p.N_out;
  const int8_t* labels = p.labels != nullptr ? p.labels + g * p.N : nullptr;
  const double T = (double)p.T;

  // 1. stage
  {
    int cnt[CTK_PLANES_MAX];  // of this wave, per label
#pragma unroll
    for (int q = 0; q < CTK_PLANES_MAX; ++q) cnt[q] = 0;
    for (int c0 = 0; c0 < p.N_out; c0 += PL_CHUNK) {
      const int n = c0 + tid;
      int4 pt;
      const int r = planes_gather(p, g, f, fs, row_p, row_q, n, &pt) ? (labels != nullptr ? ctk_objects_round(labels[n], p.L) : 0) : -1;
#pragma unroll
      for (int q = 0; q < CTK_PLANES_MAX; ++q) cnt[q] += __popcll(__ballot(r == q));
    }
#pragma unroll
    for (int q = 0; q < CTK_PLANES_MAX; ++q)
      if (lane == q) wave_lab[wave][q] = cnt[q];
    __syncthreads();
    if (tid == 0) {
      int s = 0;
      for (int q = 0; q < CTK_PLANES_MAX; ++q) {
        seg[q] = s, run[0][q] = s;
        s += wave_lab[0][q] + wave_lab[1][q] + wave_lab[2][q] + wave_lab[3][q];
      }
      seg[CTK_PLANES_MAX] = s;
    }
    __syncthreads();
    for (int c = 0, c0 = 0; c0 < p.N_out; c0 += PL_CHUNK, ++c) {
      const int n = c0 + tid, cur = c & 1;
      int4 pt = make_int4(0, 0, 0, 0);
      const bool hit = planes_gather(p, g, f, fs, row_p, row_q, n, &pt);
      const int r = hit ? (labels != nullptr ? ctk_objects_round(labels[n], p.L) : 0) : -1;
      int rank = 0;
#pragma unroll
      for (int q = 0; q < CTK_PLANES_MAX; ++q) {
        const unsigned long long mask = __ballot(r == q);
        if (lane == q) wave_lab[wave][q] = __popcll(mask);
        if (r == q) rank = __popcll(mask & below);
      }
      __syncthreads();
      if (r >= 0) {
        int place = run[cur][r] + rank;
        for (int w = 0; w < wave; ++w) place += wave_lab[w][r];
        pts[place] = pt;  // (place < N_out: the segments partition the correspondences, of which there are at most N_out)
        slot[place] = (uint16_t)n;
      } else if (n < p.N_out) {
        lab_out[n] = hit ? (int8_t)CTK_OBJECT_NONE : (int8_t)-1;
      }
      if (tid < CTK_PLANES_MAX) run[cur ^ 1][tid] = run[cur][tid] + wave_lab[0][tid] + wave_lab[1][tid] + wave_lab[2][tid] + wave_lab[3][tid];
      __syncthreads();  // the running ends of the next chunk are complete, and wave_lab is written again only behind it
    }
  }

  // 2. the rounds, each over its own segment
  for (int r = 0; r < p.L; ++r) {
    const int lo = seg[r], Mr = seg[r + 1] - seg[r];
    const int4* list = pts + lo;
    const uint32_t seed_r = ctk_objects_seed(p.seed, r);
    int64_t best = -1;
    if (Mr >= 4) {
      for (int k = tid; k < p.K; k += PL_CHUNK) {
        CtkPlaneHyp h;
        if (!planes_hyp_at(seed_r, p.base2, list, f, k, Mr, &h)) continue;
        int count = 0;
        for (int m = 0; m < Mr; ++m) {
          const int4 q = list[m];
          count += ctk_plane_inlier(h, T, q.x, q.y, q.z, q.w) ? 1 : 0;
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

    const bool have = ctk_objects_accept(best, p.min_points);
    CtkPlaneHyp hb;
    hb.px = hb.py = hb.qx = hb.qy = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) hb.h[i] = 0.0;
    if (have) planes_hyp_at(seed_r, p.base2, list, f, ctk_motion_key_k(best, p.K), Mr, &hb);
    // the reach of the inliers
    int reach = 0;
    if (have)
      for (int m = tid; m < Mr; m += PL_CHUNK) {
        const int4 q = list[m];
        if (ctk_plane_inlier(hb, T, q.x, q.y, q.z, q.w)) reach = max(reach, ctk_plane_reach(hb, q.x, q.y, q.z, q.w));
      }
    reach = planes_wave_max(reach);
    if (lane == 0) wave_reach[wave] = reach;
    __syncthreads();
    const int e = ctk_plane_bits(max(max(wave_reach[0], wave_reach[1]), max(wave_reach[2], wave_reach[3])));
    int64_t s[CTK_PS_COUNT];
#pragma unroll
    for (int i = 0; i < CTK_PS_COUNT; ++i) s[i] = 0;
    int bx[4];
    ctk_objects_box_empty(bx);
    for (int m = tid; m < Mr; m += PL_CHUNK) {
      const int4 q = list[m];
      const bool in = have && ctk_plane_inlier(hb, T, q.x, q.y, q.z, q.w);
      if (in) {
        ctk_plane_terms(hb, e, q.x, q.y, q.z, q.w, s);
        if (p.inverse) ctk_objects_box_add(bx, q.x, q.y);
        else ctk_objects_box_add(bx, q.z, q.w);
      }
      lab_out[slot[lo + m]] = in ? (int8_t)r : (int8_t)CTK_OBJECT_NONE;
    }
#pragma unroll
    for (int i = 0; i < CTK_PS_COUNT; ++i) {
      const int64_t t = motion_wave_sum(s[i]);
      if (lane == 0) wave_sum[wave][i] = t;
    }
    {
      const int b0 = planes_wave_min(bx[0]), b1 = planes_wave_min(bx[1]), b2 = planes_wave_max(bx[2]), b3 = planes_wave_max(bx[3]);
      if (lane == 0) wave_box[wave][0] = b0, wave_box[wave][1] = b1, wave_box[wave][2] = b2, wave_box[wave][3] = b3;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < CTK_PS_COUNT; ++i) s[i] = wave_sum[0][i] + wave_sum[1][i] + wave_sum[2][i] + wave_sum[3][i];
      float m9[9];
      int fell = 0;
      if (have) {
        double* Nm = solve;
        double* bv = Nm + 64;
        double* Lm = bv + 8;
        double* Dv = Lm + 64;
        double* vv = Dv + 8;
        double* zv = vv + 8;
        double* hv = zv + 8;
        ctk_plane_system(s, Nm, bv);
        double hc[9];
        if (ctk_plane_solve(Nm, bv, Lm, Dv, vv, zv, hv)) {
#pragma unroll
          for (int i = 0; i < 8; ++i) hc[i] = hv[i];
          hc[8] = 1.0;
          ctk_plane_pixels(hc, e, hb.px, hb.py, hb.qx, hb.qy, m9);
        } else {
          fell = 1;
          ctk_plane_pixels(hb.h, 0, hb.px, hb.py, hb.qx, hb.qy, m9);
        }
        bx[0] = min(min(wave_box[0][0], wave_box[1][0]), min(wave_box[2][0], wave_box[3][0]));
        bx[1] = min(min(wave_box[0][1], wave_box[1][1]), min(wave_box[2][1], wave_box[3][1]));
        bx[2] = max(max(wave_box[0][2], wave_box[1][2]), max(wave_box[2][2], wave_box[3][2]));
        bx[3] = max(max(wave_box[0][3], wave_box[1][3]), max(wave_box[2][3], wave_box[3][3]));
      } else {
        ctk_plane_identity(m9);
        ctk_objects_box_none(bx);
      }
      const long o = ((g * F + pic) * p.L + r);
      float* mo = p.homography + o * 9;
#pragma unroll
      for (int i = 0; i < 9; ++i) mo[i] = m9[i];
      int32_t* st = p.stats + o * 4;
      st[0] = Mr, st[1] = have ? ctk_motion_key_count(best) : 0, st[2] = have ? ctk_motion_key_k(best, p.K) : -1, st[3] = fell;
      int32_t* bo = p.box + o * 4;
      bo[0] = bx[0], bo[1] = bx[1], bo[2] = bx[2], bo[3] = bx[3];
    }
    // (wave_key, wave_reach, wave_sum and wave_box are written again only behind the next round's first barrier, which every thread
    // reaches after it has read them here; thread 0 reads wave_sum and wave_box before it gets there)
  }
}

bool planes_scale_ok(float s) { return s > 0.0f && s <= 3.402823466e+38f; }

// everything but the pointers (whether an anchor or labels are given is looked at)
int planes_check_shape(const ctk_fit_planes_args* a) {
  const long big = 1L << 30;
  if (a->G <= 0 || a->N <= 0 || a->N_out <= 0 || a->R <= 0 || a->F <= 0 || a->N_out > a->N || a->N_out > CTK_MOTION_POINTS_MAX) return CTK_E_SHAPE;
  if (a->f0 < 0 || (long)a->f0 + a->F > big || a->F > 65535 || a->G > 65535 || (long)a->G * a->N > (1L << 26) || a->reserved != 0) return CTK_E_SHAPE;
  if (a->L < 1 || a->L > CTK_PLANES_MAX || a->min_points < 1 || a->min_points > CTK_MOTION_POINTS_MAX) return CTK_E_SHAPE;
  if (a->inverse != 0 && a->inverse != 1) return CTK_E_SHAPE;
  if (a->labels == nullptr && a->L != 1) return CTK_E_SHAPE;
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
  if (!planes_scale_ok(a->sx) || !planes_scale_ok(a->sy)) return CTK_E_SHAPE;
  if (a->visible == nullptr && a->thresh != a->thresh) return CTK_E_SHAPE;
  return CTK_OK;
}

}  // namespace

extern "C" int ctk_fit_planes_workspace_bytes(const ctk_fit_planes_args* a, size_t* out_bytes) {
  if (!a || !out_bytes) return CTK_E_NULL;
  const int rc = planes_check_shape(a);
  if (rc != CTK_OK) return rc;
  *out_bytes = 0;  // the one-launch form keeps everything in LDS
  return CTK_OK;
}

extern "C" int ctk_fit_planes(const ctk_fit_planes_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  if (!a) return CTK_E_NULL;
  if (!a->hist_coords || !a->homography || !a->label || !a->stats || !a->box) return CTK_E_NULL;
  if (!a->visible && (!a->hist_vis || !a->hist_conf)) return CTK_E_NULL;
  if ((a->anchor_coords != nullptr) != (a->anchor_visible != nullptr)) return CTK_E_NULL;
  const int rc = planes_check_shape(a);
  if (rc != CTK_OK) return rc;
  (void)workspace, (void)workspace_bytes;  // the query answers 0: nothing is too small
  if (((reinterpret_cast<uintptr_t>(a->hist_coords) | reinterpret_cast<uintptr_t>(a->anchor_coords)) & 7u) != 0) return CTK_E_ALIGN;
  if (((reinterpret_cast<uintptr_t>(a->homography) | reinterpret_cast<uintptr_t>(a->stats) | reinterpret_cast<uintptr_t>(a->box)) & 3u) != 0)
    return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);

  PlanesParams p;
  p.G = a->G, p.N = a->N, p.N_out = a->N_out, p.R = a->R, p.f0 = a->f0, p.to = a->to, p.lag = a->lag, p.anchor_frame = a->anchor_frame;
  p.L = a->L, p.min_points = a->min_points, p.K = a->K, p.inverse = a->inverse;
  p.T = ctk_motion_tol(a->tol), p.base2 = ctk_motion_base2(a->min_base), p.seed = a->seed;
  p.sx = a->sx, p.sy = a->sy, p.thresh = a->thresh;
  p.hc = a->hist_coords, p.visible = a->visible, p.hv = a->hist_vis, p.hf = a->hist_conf, p.first_row = a->first_row;
  p.ac = a->anchor_coords, p.av = a->anchor_visible, p.labels = a->labels;
  p.homography = a->homography, p.label = a->label, p.stats = a->stats, p.box = a->box;
  {
    CtkProfScope prof("fit_planes", 0.0, (double)a->G * a->F * (a->N_out * 67.0 + a->L * 68.0), s);
    const size_t lds = (size_t)p.N_out * PL_ENTRY_BYTES;
    // (Beyond 64 KiB of LDS a kernel has to say so once; not a stream operation.  objects.hip says so from 64 KiB of DYNAMIC LDS on; this
    // kernel also holds 1.3 KiB of static LDS -- the 23 sums per wave --, and whether that counts towards the 64 KiB is not written
    // down anywhere, so it says so from 48 KiB on: early costs nothing.  tests/test_gpu_planes.py runs N_out = 3600, 63.3 KiB dynamic.)
    if (lds > 49152) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fit_planes_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               CTK_MOTION_POINTS_MAX * PL_ENTRY_BYTES);
    hipLaunchKernelGGL(fit_planes_kernel, dim3((unsigned)a->F, (unsigned)p.G), dim3(256), lds, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
