// Epipolar geometry on the device (include/ctk.h, "fit epipolar"): ONE robust fundamental matrix per (group, frame) over one staged list
// of correspondences, by the rules of epipolar_math.h (and, through it, plane_math.h, objects_math.h and motion_math.h).  The frame of
// the call is ctk_fit_planes' (planes.hip): the same workgroup layout, and from fit_device.h the same source and slot gather
// (CtkFitSource, fit_gather), the same two-pass staging (fit_stage, two segments here) and the same reductions; only the model
// differs.  One launch, no atomics, no workspace; every output element is one plain store.
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
#include "fit_device.h"

namespace {

constexpr int EP_CHUNK = 256;
constexpr int EP_ENTRY_BYTES = (int)sizeof(int4) + (int)sizeof(uint16_t);  // a point and its slot

struct EpipolarParams {
  CtkFitSource src;
  int min_points, K, T;
  uint32_t seed;
  int64_t base2;
  const int8_t* mask;
  float* fundamental;
  int8_t* label;
  float* error;
  int32_t* stats;
};

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
  uint16_t* slot = reinterpret_cast<uint16_t*>(pts + p.src.N_out);
  // (the static part is a multiple of 16 bytes, so that the dynamic list behind it keeps its 16-byte alignment)
  __shared__ __attribute__((aligned(16))) double solve[CTK_PLANE_SOLVE_DOUBLES];
  __shared__ __attribute__((aligned(16))) int64_t wave_sum[4][CTK_EPI_SUMS + 1];
  __shared__ __attribute__((aligned(16))) int64_t total[CTK_EPI_SUMS + 1];
  __shared__ __attribute__((aligned(16))) int64_t wave_key[4];
  __shared__ __attribute__((aligned(16))) CtkEpiFit fit;  // 96 bytes
  __shared__ FitStageLds<2> stage;
  __shared__ __attribute__((aligned(16))) int wave_reach[4];
  __shared__ __attribute__((aligned(16))) int wave_count[4];
  __shared__ __attribute__((aligned(16))) int fell[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const CtkFitSource& src = p.src;
  const int F = (int)gridDim.x, pic = (int)blockIdx.x, f = src.f0 + pic;
  const long g = (long)blockIdx.y;
  const FitFrame fr = fit_frame(src, g, f);
  int8_t* lab_out = p.label + (g * F + pic) * (long)src.N_out;
  float* err_out = p.error + (g * F + pic) * (long)src.N_out;
  const int8_t* mask = p.mask != nullptr ? p.mask + g * src.N : nullptr;
  const double T = (double)p.T;

  // 1. stage: segment 0 = the fit list, segment 1 = the correspondences the mask keeps out of it
  fit_stage(
      stage, src.N_out, pts, slot, [&](int n, int4* pt) { return fit_gather(src, fr, n, pt); },
      [&](int n) { return mask != nullptr && mask[n] == 0 ? 1 : 0; }, [&](int n, bool) { lab_out[n] = (int8_t)-1, err_out[n] = -1.0f; });
  const int M = stage.seg[1], A = stage.seg[2];

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
  best = fit_block_best(best, wave_key);

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
    reach = fit_wave_max(reach);
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
    fit_block_sums<CTK_EPI_SUMS>(s, wave_sum);
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

// everything but the pointers (whether an anchor is given is looked at)
int epipolar_check_shape(const ctk_fit_epipolar_args* a) {
  if (!fit_check_source(fit_source_of(a), a->F) || a->reserved != 0) return CTK_E_SHAPE;
  if (a->min_points < CTK_EPI_MIN_POINTS || a->min_points > CTK_MOTION_POINTS_MAX) return CTK_E_SHAPE;
  if (a->K < 1 || a->K > CTK_MOTION_HYPOTHESES_MAX) return CTK_E_SHAPE;
  if (ctk_motion_tol(a->tol) == 0 || ctk_motion_base2(a->min_base) < 0) return CTK_E_SHAPE;
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
  EpipolarParams p;
  p.src = fit_source_of(a);
  if (fit_null_source(p.src) || !a->fundamental || !a->label || !a->error || !a->stats) return CTK_E_NULL;
  const int rc = epipolar_check_shape(a);
  if (rc != CTK_OK) return rc;
  (void)workspace, (void)workspace_bytes;  // the query answers 0: nothing is too small
  if (!fit_align_source(p.src)) return CTK_E_ALIGN;
  if (((reinterpret_cast<uintptr_t>(a->fundamental) | reinterpret_cast<uintptr_t>(a->error) | reinterpret_cast<uintptr_t>(a->stats)) & 3u) != 0)
    return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);

  p.min_points = a->min_points, p.K = a->K;
  p.T = ctk_motion_tol(a->tol), p.base2 = ctk_motion_base2(a->min_base), p.seed = a->seed;
  p.mask = a->mask;
  p.fundamental = a->fundamental, p.label = a->label, p.error = a->error, p.stats = a->stats;
  {
    CtkProfScope prof("fit_epipolar", 0.0, (double)a->G * a->F * (a->N_out * 71.0 + 52.0), s);
    fit_launch(fit_epipolar_kernel, a->F, a->G, (size_t)a->N_out * EP_ENTRY_BYTES, CTK_MOTION_POINTS_MAX * EP_ENTRY_BYTES, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
