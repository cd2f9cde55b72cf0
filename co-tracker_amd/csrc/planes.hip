// Planes on the device (include/ctk.h, "fit planes / warp planes"): up to L robust homography fits per (group, frame) over sub-lists
// of ONE staged list of correspondences, by the rules of plane_math.h (and, through it, objects_math.h and motion_math.h).  The frame
// of the call is ctk_fit_objects' labels mode (objects.hip): the same workgroup layout, and from fit_device.h the same source and slot
// gather (CtkFitSource, fit_gather), the same two-pass staging (fit_stage, a segment per label) and the same reductions; only the
// model differs.  One launch, no atomics, no workspace; every output element is one plain store.
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
#include "fit_device.h"
#include "plane_math.h"

namespace {

constexpr int PL_CHUNK = 256;
constexpr int PL_ENTRY_BYTES = (int)sizeof(int4) + (int)sizeof(uint16_t);  // a point and its slot

struct PlanesParams {
  CtkFitSource src;
  int L, min_points, K, T, inverse;
  uint32_t seed;
  int64_t base2;
  const int8_t* labels;
  float* homography;
  int8_t* label;
  int32_t* stats;
  int32_t* box;
};

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
  uint16_t* slot = reinterpret_cast<uint16_t*>(pts + p.src.N_out);
  __shared__ FitStageLds<CTK_PLANES_MAX> stage;
  __shared__ int64_t wave_key[4];
  __shared__ int64_t wave_sum[4][CTK_PS_COUNT];
  __shared__ int wave_box[4][4];
  __shared__ int wave_reach[4];
  __shared__ double solve[CTK_PLANE_SOLVE_DOUBLES];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const CtkFitSource& src = p.src;
  const int F = (int)gridDim.x, pic = (int)blockIdx.x, f = src.f0 + pic;
  const long g = (long)blockIdx.y;
  const FitFrame fr = fit_frame(src, g, f);
  int8_t* lab_out = p.label + (g * F + pic) * (long)src.N_out;
  const int8_t* labels = p.labels != nullptr ? p.labels + g * src.N : nullptr;
  const double T = (double)p.T;

  // 1. stage: a segment per label (without labels every correspondence has label 0); inverse = 1 swaps P and Q as a point is gathered
  fit_stage(
      stage, src.N_out, pts, slot,
      [&](int n, int4* pt) {
        const bool hit = fit_gather(src, fr, n, pt);
        if (hit && p.inverse) *pt = make_int4(pt->z, pt->w, pt->x, pt->y);
        return hit;
      },
      [&](int n) { return labels != nullptr ? ctk_objects_round(labels[n], p.L) : 0; },
      [&](int n, bool hit) { lab_out[n] = hit ? (int8_t)CTK_OBJECT_NONE : (int8_t)-1; });

  // 2. the rounds, each over its own segment
  for (int r = 0; r < p.L; ++r) {
    const int lo = stage.seg[r], Mr = stage.seg[r + 1] - stage.seg[r];
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
    best = fit_block_best(best, wave_key);

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
    reach = fit_wave_max(reach);
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
    fit_block_sums<CTK_PS_COUNT>(s, wave_sum);
    {
      const int b0 = fit_wave_min(bx[0]), b1 = fit_wave_min(bx[1]), b2 = fit_wave_max(bx[2]), b3 = fit_wave_max(bx[3]);
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

// everything but the pointers (whether an anchor or labels are given is looked at)
int planes_check_shape(const ctk_fit_planes_args* a) {
  if (!fit_check_source(fit_source_of(a), a->F) || a->reserved != 0) return CTK_E_SHAPE;
  if (a->L < 1 || a->L > CTK_PLANES_MAX || a->min_points < 1 || a->min_points > CTK_MOTION_POINTS_MAX) return CTK_E_SHAPE;
  if (a->inverse != 0 && a->inverse != 1) return CTK_E_SHAPE;
  if (a->labels == nullptr && a->L != 1) return CTK_E_SHAPE;
  if (a->K < 1 || a->K > CTK_MOTION_HYPOTHESES_MAX) return CTK_E_SHAPE;
  if (ctk_motion_tol(a->tol) == 0 || ctk_motion_base2(a->min_base) < 0) return CTK_E_SHAPE;
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
  PlanesParams p;
  p.src = fit_source_of(a);
  if (fit_null_source(p.src) || !a->homography || !a->label || !a->stats || !a->box) return CTK_E_NULL;
  const int rc = planes_check_shape(a);
  if (rc != CTK_OK) return rc;
  (void)workspace, (void)workspace_bytes;  // the query answers 0: nothing is too small
  if (!fit_align_source(p.src)) return CTK_E_ALIGN;
  if (((reinterpret_cast<uintptr_t>(a->homography) | reinterpret_cast<uintptr_t>(a->stats) | reinterpret_cast<uintptr_t>(a->box)) & 3u) != 0)
    return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);

  p.L = a->L, p.min_points = a->min_points, p.K = a->K, p.inverse = a->inverse;
  p.T = ctk_motion_tol(a->tol), p.base2 = ctk_motion_base2(a->min_base), p.seed = a->seed;
  p.labels = a->labels;
  p.homography = a->homography, p.label = a->label, p.stats = a->stats, p.box = a->box;
  {
    CtkProfScope prof("fit_planes", 0.0, (double)a->G * a->F * (a->N_out * 67.0 + a->L * 68.0), s);
    // (tests/test_gpu_planes.py runs N_out = 3600, 63.3 KiB of dynamic LDS beside 1.3 KiB of static)
    fit_launch(fit_planes_kernel, a->F, a->G, (size_t)a->N_out * PL_ENTRY_BYTES, CTK_MOTION_POINTS_MAX * PL_ENTRY_BYTES, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
