// Focal length from the tracks on the device (include/ctk.h, "fit focal"): K candidate focal lengths are swept through ctk_fit_pose's
// rules over the fundamental matrices and labels that ctk_fit_epipolar wrote, every (frame, candidate) gets an integer cost in pixels,
// and per group the candidate with the smallest total is taken and refined, by the rules of focal_math.h (and, through it,
// pose_math.h).  The frame of the call is ctk_fit_pose's (pose.hip): from fit_device.h the same source and slot gather (CtkFitSource,
// fit_gather) and the same two-pass staging (fit_stage).  One entry, two launches, no atomics, no workspace; every output element is
// one plain store; `fundamental`, `label`, `focals` and `curve_in` are only read.
//
// sweep   grid (frame, group, block of four candidates), 256 threads.  Dynamic LDS: the fit list of (Px, Py, Qx, Qy) int32 points, 16
//         bytes each, and the uint16 side list fit_stage writes: N_out * 18 bytes, 144 KiB at most.  A workgroup stages its frame's fit
//         list once (one segment: label 1, and mask nonzero or no mask); thread k < K then asks whether candidate k's camera is
//         accepted, which tells every workgroup of the frame alike whether the frame takes part.  Behind that each of the four waves
//         owns one candidate: lane 0 decomposes into the wave's block of LDS, the wave votes, runs the rounds (sums by wave shuffles,
//         lane 0 solves in the wave's own CTK_POSE_SOLVE_DOUBLES of LDS) and scores; lane 0 stores cost[frame][k].  The barriers are
//         the workgroup's: a wave without a candidate walks an empty list through the same barriers.
// choose  one workgroup of 256 threads per group.  Thread k < K adds cost[.][k] over the frames to curve_in[k]; the waves walk the
//         frames, one each at a time, and count by the sweep's own rule the frames that took part and their entries (the slots are
//         gathered once more, which is cheaper than a workspace and a third launch); thread 0 chooses and refines.
#include "ctk_common.h"
#include "ctk_profile.h"
#include "fit_device.h"
#include "focal_math.h"

namespace {

constexpr int FO_ENTRY_BYTES = (int)sizeof(int4) + (int)sizeof(uint16_t);  // a point and its slot
constexpr int FO_SLOTS = CTK_POSE_SUMS + 2;                                // the sums, the count, and one to keep rows 16-byte multiples
constexpr int FO_WAVES = 4;

struct FocalParams {
  CtkFitSource src;
  int F, K, min_points, min_frames;
  float cx, cy, tol, contrast;
  const int8_t* mask;
  const float* fundamental;
  const int8_t* label;
  const float* focals;
  const int64_t* curve_in;
  float* focal;
  int64_t* curve;
  int64_t* cost;
  int32_t* stats;
};

// whether slot n of the frame is on the fit list
__device__ __forceinline__ bool focal_listed(const FocalParams& p, const FitFrame& fr, const int8_t* lab, const int8_t* mask, int n, int4* pt) {
  return fit_gather(p.src, fr, n, pt) && lab[n] == 1 && (mask == nullptr || mask[n] != 0);
}

// grid: x = frame f0 + x, y = group, z = candidates 4 z .. 4 z + 3; dynamic LDS: N_out * 18 bytes
__global__ __launch_bounds__(256) void fit_focal_sweep_kernel(FocalParams p) {
  extern __shared__ __attribute__((aligned(16))) int4 pts[];
  uint16_t* slot = reinterpret_cast<uint16_t*>(pts + p.src.N_out);
  // (the static part is a multiple of 16 bytes, so that the dynamic list behind it keeps its 16-byte alignment)
  __shared__ __attribute__((aligned(16))) double solve[FO_WAVES][CTK_POSE_SOLVE_DOUBLES];
  __shared__ __attribute__((aligned(16))) int64_t total[FO_WAVES][FO_SLOTS];
  __shared__ __attribute__((aligned(16))) CtkPose cand[FO_WAVES][4];  // 96 bytes each
  __shared__ __attribute__((aligned(16))) CtkPose fit[FO_WAVES];
  __shared__ FitStageLds<1> stage;
  __shared__ __attribute__((aligned(16))) int cand_ok[FO_WAVES][4];
  __shared__ __attribute__((aligned(16))) int stands[FO_WAVES];
  __shared__ __attribute__((aligned(16))) int accept[FO_WAVES];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const CtkFitSource& src = p.src;
  const int F = (int)gridDim.x, pic = (int)blockIdx.x, f = src.f0 + pic;
  const long g = (long)blockIdx.y;
  const FitFrame fr = fit_frame(src, g, f);
  const long o = g * F + pic;
  const int8_t* lab = p.label + o * (long)src.N_out;
  const int8_t* mask = p.mask != nullptr ? p.mask + g * src.N : nullptr;
  const float* Fm = p.fundamental + o * 9;
  const int K = p.K, k = (int)blockIdx.z * FO_WAVES + wave;
  const bool mine = k < K;  // (the same in every lane of a wave)

  // 1. stage the fit list
  fit_stage(
      stage, src.N_out, pts, slot, [&](int n, int4* pt) { return fit_gather(src, fr, n, pt); },
      [&](int n) { return lab[n] == 1 && (mask == nullptr || mask[n] != 0) ? 0 : -1; }, [&](int, bool) {});
  const int M = stage.seg[1];

  // 2. does the frame take part: thread j asks for candidate j
  {
    const bool yes = tid < K && ctk_focal_accepts(Fm, p.focals[tid], p.cx, p.cy);
    const unsigned long long any = __ballot(yes);
    if (lane == 0) accept[wave] = any != 0ull ? 1 : 0;
  }
  // 3. E and the four poses of the wave's candidate
  const float fk = mine ? p.focals[k] : 0.0f;
  const CtkPoseCam cam = ctk_focal_cam(mine ? fk : 1.0f, p.cx, p.cy);
  if (lane == 0) {
    bool ok = false;
    if (mine && M >= p.min_points && ctk_focal_stands(fk)) {
      double E[9];
      CtkPose c4[4];
      bool ok4[4] = {false, false, false, false};
      ok = ctk_pose_essential(Fm, cam, E) && ctk_pose_decompose(E, c4, ok4);
      if (ok) {
        for (int i = 0; i < 4; ++i) cand[wave][i] = c4[i], cand_ok[wave][i] = ok4[i] ? 1 : 0;
      }
    }
    stands[wave] = ok ? 1 : 0;
  }
  __syncthreads();
  const bool takes = M >= p.min_points && (accept[0] | accept[1] | accept[2] | accept[3]) != 0;  // (the same in every thread)
  int64_t* out = p.cost + o * (long)K + k;
  if (!takes) {
    if (mine && lane == 0) *out = 0;
    return;
  }

  // 4. the vote, the wave's own
  int chosen = -1;
  if (stands[wave] != 0) {
    int cnt[4] = {0, 0, 0, 0};
    for (int m = lane; m < M; m += 64) {
      const int4 q = pts[m];
      double x[3], y[3];
      ctk_pose_ray(cam, q.x, q.y, x);
      ctk_pose_ray(cam, q.z, q.w, y);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double zs, zf;
        ctk_pose_depths(cand[wave][i], x, y, &zs, &zf);
        cnt[i] += ctk_pose_front(zs, zf) ? 1 : 0;
      }
    }
    int count[4];
    bool ok4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) count[i] = (int)motion_wave_sum((int64_t)cnt[i]), ok4[i] = cand_ok[wave][i] != 0;
    chosen = ctk_pose_choose(count, ok4);  // (every lane holds the four sums)
    if (chosen >= 0 && lane == 0) fit[wave] = cand[wave][chosen];
  }
  __syncthreads();
  const int Mw = chosen >= 0 ? M : 0;  // a wave without a pose walks nothing, through the same barriers

  // 5. the rounds
  for (int round = 0; round < CTK_POSE_ROUNDS; ++round) {
    const CtkPose cur = fit[wave];
    int64_t s[CTK_POSE_SUMS];
#pragma unroll
    for (int i = 0; i < CTK_POSE_SUMS; ++i) s[i] = 0;
    int took = 0;
    for (int m = lane; m < Mw; m += 64) {
      const int4 q = pts[m];
      double x[3], y[3], v[7], gg;
      ctk_pose_ray(cam, q.x, q.y, x);
      ctk_pose_ray(cam, q.z, q.w, y);
      if (ctk_pose_entry(cur, x, y, v, &gg)) {
        ctk_pose_terms(v, gg, s);
        ++took;
      }
    }
#pragma unroll
    for (int i = 0; i < CTK_POSE_SUMS; ++i) {
      const int64_t t = motion_wave_sum(s[i]);
      if (lane == 0) total[wave][i] = t;
    }
    const int n = (int)motion_wave_sum((int64_t)took);
    __syncthreads();  // every wave has read its pose; lane 0 sees its own stores to total
    if (lane == 0 && chosen >= 0) {
      CtkPose next;
      if (ctk_pose_update(cur, total[wave], n, solve[wave], &next)) fit[wave] = next;
    }
    __syncthreads();  // the round's pose is published
  }

  // 6. the score under the final pose
  if (!mine) return;
  int64_t sum = ctk_focal_worst(M);
  if (chosen >= 0) {
    const CtkPose fin = fit[wave];
    const double fd = (double)fk;
    const double ff = fd * fd, T = ctk_focal_tol2(p.tol);
    int64_t part = 0;
    for (int m = lane; m < M; m += 64) {
      const int4 q = pts[m];
      double x[3], y[3];
      ctk_pose_ray(cam, q.x, q.y, x);
      ctk_pose_ray(cam, q.z, q.w, y);
      part += ctk_focal_term(fin, x, y, ff, T);
    }
    sum = motion_wave_sum(part);
  }
  if (lane == 0) *out = sum;
}

// grid: x = group
__global__ __launch_bounds__(256) void fit_focal_choose_kernel(FocalParams p) {
  __shared__ __attribute__((aligned(16))) int64_t total[CTK_FOCAL_K_MAX];
  __shared__ __attribute__((aligned(16))) float cands[CTK_FOCAL_K_MAX];
  __shared__ __attribute__((aligned(16))) int64_t counted[FO_WAVES][2];
  __shared__ __attribute__((aligned(16))) int wave_bad[FO_WAVES];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const CtkFitSource& src = p.src;
  const int F = p.F, K = p.K;
  const long g = (long)blockIdx.x;
  const int8_t* mask = p.mask != nullptr ? p.mask + g * src.N : nullptr;
  const int64_t* in = p.curve_in != nullptr ? p.curve_in + g * (long)(K + 2) : nullptr;
  int64_t* curve = p.curve + g * (long)(K + 2);

  // 1. the totals, a candidate per thread
  bool bad = false;
  if (tid < K) {
    int64_t t = in != nullptr ? in[tid] : 0;
    const int64_t* c = p.cost + g * (long)F * K + tid;
    for (int pic = 0; pic < F; ++pic) t += c[(long)pic * K];
    const float fk = p.focals[tid];
    total[tid] = t, cands[tid] = fk, curve[tid] = t;
    bad = !ctk_focal_stands(fk);
  }
  {
    const unsigned long long any = __ballot(bad);
    if (lane == 0) wave_bad[wave] = any != 0ull ? 1 : 0;
  }

  // 2. the frames that took part and their entries, a frame per wave at a time
  int64_t frames = 0, entries = 0;
  for (int pic = wave; pic < F; pic += FO_WAVES) {
    const FitFrame fr = fit_frame(src, g, src.f0 + pic);
    const long o = g * F + pic;
    const int8_t* lab = p.label + o * (long)src.N_out;
    const float* Fm = p.fundamental + o * 9;
    int cnt = 0;
    for (int n = lane; n < src.N_out; n += 64) {
      int4 pt;
      cnt += focal_listed(p, fr, lab, mask, n, &pt) ? 1 : 0;
    }
    const int M = (int)motion_wave_sum((int64_t)cnt);
    bool yes = false;
    for (int j = lane; j < K; j += 64) yes = yes || ctk_focal_accepts(Fm, p.focals[j], p.cx, p.cy);
    const bool takes = M >= p.min_points && __ballot(yes) != 0ull;
    frames += takes ? 1 : 0, entries += takes ? M : 0;
  }
  if (lane == 0) counted[wave][0] = frames, counted[wave][1] = entries;
  __syncthreads();

  // 3. the choice
  if (tid == 0) {
    int64_t fr_all = in != nullptr ? in[K] : 0, en_all = in != nullptr ? in[K + 1] : 0;
    bool any_bad = false;
    for (int w = 0; w < FO_WAVES; ++w) fr_all += counted[w][0], en_all += counted[w][1], any_bad = any_bad || wave_bad[w] != 0;
    float focal;
    int index;
    const int bits = ctk_focal_choose(total, cands, K, fr_all, p.min_frames, p.contrast, any_bad, &focal, &index);
    curve[K] = fr_all, curve[K + 1] = en_all;
    p.focal[g] = focal;
    int32_t* st = p.stats + g * 4;
    st[0] = ctk_focal_clamp(fr_all), st[1] = index, st[2] = ctk_focal_clamp(en_all), st[3] = bits;
  }
}

// everything but the pointers (whether an anchor is given is looked at)
int focal_check_shape(const ctk_fit_focal_args* a) {
  if (!fit_check_source(fit_source_of(a), a->F) || a->reserved != 0) return CTK_E_SHAPE;
  if (a->F > CTK_FOCAL_FRAMES_MAX) return CTK_E_SHAPE;
  if (a->min_points < CTK_POSE_MIN_POINTS || a->min_points > CTK_MOTION_POINTS_MAX) return CTK_E_SHAPE;
  if (a->K < 1 || a->K > CTK_FOCAL_K_MAX || a->min_frames < 1) return CTK_E_SHAPE;
  if (!fit_finite(a->cx) || !fit_finite(a->cy) || !fit_scale_ok(a->tol)) return CTK_E_SHAPE;
  if (!(a->contrast >= 1.0f) || !fit_finite(a->contrast)) return CTK_E_SHAPE;
  return CTK_OK;
}

}  // namespace

extern "C" int ctk_fit_focal_workspace_bytes(const ctk_fit_focal_args* a, size_t* out_bytes) {
  if (!a || !out_bytes) return CTK_E_NULL;
  const int rc = focal_check_shape(a);
  if (rc != CTK_OK) return rc;
  *out_bytes = 0;  // the sweep keeps everything in LDS, and `cost` carries its result to the choice
  return CTK_OK;
}

extern "C" int ctk_fit_focal(const ctk_fit_focal_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  if (!a) return CTK_E_NULL;
  FocalParams p;
  p.src = fit_source_of(a);
  if (fit_null_source(p.src) || !a->fundamental || !a->label || !a->focals || !a->focal || !a->curve || !a->cost || !a->stats) return CTK_E_NULL;
  const int rc = focal_check_shape(a);
  if (rc != CTK_OK) return rc;
  (void)workspace, (void)workspace_bytes;  // the query answers 0: nothing is too small
  if (!fit_align_source(p.src)) return CTK_E_ALIGN;
  if (((reinterpret_cast<uintptr_t>(a->fundamental) | reinterpret_cast<uintptr_t>(a->focals) | reinterpret_cast<uintptr_t>(a->focal) |
        reinterpret_cast<uintptr_t>(a->stats)) & 3u) != 0)
    return CTK_E_ALIGN;
  if (((reinterpret_cast<uintptr_t>(a->curve_in) | reinterpret_cast<uintptr_t>(a->curve) | reinterpret_cast<uintptr_t>(a->cost)) & 7u) != 0)
    return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);

  p.F = a->F, p.K = a->K, p.min_points = a->min_points, p.min_frames = a->min_frames;
  p.cx = a->cx, p.cy = a->cy, p.tol = a->tol, p.contrast = a->contrast;
  p.mask = a->mask, p.fundamental = a->fundamental, p.label = a->label, p.focals = a->focals, p.curve_in = a->curve_in;
  p.focal = a->focal, p.curve = a->curve, p.cost = a->cost, p.stats = a->stats;
  const size_t lds = (size_t)a->N_out * FO_ENTRY_BYTES;
  const unsigned blocks = (unsigned)((a->K + FO_WAVES - 1) / FO_WAVES);
  {
    CtkProfScope prof("fit_focal_sweep", 0.0, (double)a->G * a->F * blocks * (a->N_out * 23.0 + 100.0), s);
    if (lds > 49152)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fit_focal_sweep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                CTK_MOTION_POINTS_MAX * FO_ENTRY_BYTES);
    hipLaunchKernelGGL(fit_focal_sweep_kernel, dim3((unsigned)a->F, (unsigned)a->G, blocks), dim3(256), lds, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  {
    CtkProfScope prof("fit_focal_choose", 0.0, (double)a->G * a->F * (a->K * 8.0 + a->N_out * 23.0), s);
    hipLaunchKernelGGL(fit_focal_choose_kernel, dim3((unsigned)a->G), dim3(256), 0, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
