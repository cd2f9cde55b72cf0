// Camera pose and point depths on the device (include/ctk.h, "fit pose"): per (group, frame) the fundamental matrix and the labels that
// ctk_fit_epipolar wrote become a rotation, a unit translation and two depths per correspondence, by the rules of pose_math.h (and,
// through it, epipolar_math.h, plane_math.h, objects_math.h and motion_math.h).  The frame of the call is ctk_fit_epipolar's
// (epipolar.hip): the same workgroup layout, and from fit_device.h the same source and slot gather (CtkFitSource, fit_gather), the
// same two-pass staging (fit_stage, two segments); only what is done with the list differs.  One launch, no atomics, no workspace;
// every output element is one plain store; `fundamental` and `label` are only read.
//
// One workgroup of 256 threads owns one (group, frame).  Dynamic LDS: the list of (Px, Py, Qx, Qy) int32 points, 16 bytes each, and
// next to it a uint16 side list that leads an entry back to its slot n: N_out * 18 bytes, 144 KiB at most.
// stage     two passes over chunks of 256 slots (the rows are gathered twice): the first counts the correspondences of the fit list
//           (label 1, and mask nonzero or no mask) and the others by ballots, which gives the two segments of the list: [0, M) the fit
//           list, [M, A) every other correspondence; the second places every correspondence into its segment in ascending n and
//           writes the NaN depths of the slots without one.
// decompose thread 0 builds E and the four candidates into LDS.
// vote      the fit list is walked once, an entry per thread: four integer counts, reduced by wave shuffles and through LDS.
// rounds    twice: the fit list is walked, an entry per thread: its 28 fixed-point int64 terms and the count of the entries that take
//           part; sums are reduced by wave shuffles and through LDS; thread 0 solves the 8 x 8 system in LDS and publishes the pose.
// outputs   all A entries are walked once more under the final pose: the depths, and the count of the fit list's entries in front.
#include "ctk_common.h"
#include "ctk_profile.h"
#include "fit_device.h"
#include "pose_math.h"

namespace {

constexpr int PO_CHUNK = 256;
constexpr int PO_ENTRY_BYTES = (int)sizeof(int4) + (int)sizeof(uint16_t);  // a point and its slot
constexpr int PO_SLOTS = CTK_POSE_SUMS + 2;                                // the sums, the count, and one to keep rows 16-byte multiples

struct PoseParams {
  CtkFitSource src;
  int min_points;
  CtkPoseCam cam;
  const int8_t* mask;
  const float* fundamental;
  const int8_t* label;
  float* pose;
  float* depth;
  int32_t* stats;
};

// grid: x = frame f0 + x, y = group; dynamic LDS: N_out * 18 bytes
__global__ __launch_bounds__(256) void fit_pose_kernel(PoseParams p) {
  extern __shared__ __attribute__((aligned(16))) int4 pts[];
  uint16_t* slot = reinterpret_cast<uint16_t*>(pts + p.src.N_out);
  // (the static part is a multiple of 16 bytes, so that the dynamic list behind it keeps its 16-byte alignment)
  __shared__ __attribute__((aligned(16))) double solve[CTK_POSE_SOLVE_DOUBLES];
  __shared__ __attribute__((aligned(16))) int64_t wave_sum[4][PO_SLOTS];
  __shared__ __attribute__((aligned(16))) int64_t total[PO_SLOTS];
  __shared__ __attribute__((aligned(16))) CtkPose cand[4];  // 96 bytes each
  __shared__ __attribute__((aligned(16))) CtkPose fit;
  __shared__ __attribute__((aligned(16))) int wave_vote[4][4];
  __shared__ FitStageLds<2> stage;
  __shared__ __attribute__((aligned(16))) int cand_ok[4];
  __shared__ __attribute__((aligned(16))) int wave_count[4];
  __shared__ __attribute__((aligned(16))) int state[4];  // [0]: the decomposition stands; [1]: the chosen k; [2]: the bits
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const CtkFitSource& src = p.src;
  const int F = (int)gridDim.x, pic = (int)blockIdx.x, f = src.f0 + pic;
  const long g = (long)blockIdx.y;
  const FitFrame fr = fit_frame(src, g, f);
  const long o = g * F + pic;
  const int8_t* lab = p.label + o * (long)src.N_out;
  float* dep_out = p.depth + o * (long)src.N_out * 2;
  const int8_t* mask = p.mask != nullptr ? p.mask + g * src.N : nullptr;
  const CtkPoseCam cam = p.cam;

  // 1. stage: segment 0 = the fit list (label 1, and mask nonzero or no mask), segment 1 = every other correspondence
  fit_stage(
      stage, src.N_out, pts, slot, [&](int n, int4* pt) { return fit_gather(src, fr, n, pt); },
      [&](int n) { return lab[n] == 1 && (mask == nullptr || mask[n] != 0) ? 0 : 1; },
      [&](int n, bool) { dep_out[n * 2L] = ctk_pose_nan(), dep_out[n * 2L + 1] = ctk_pose_nan(); });
  const int M = stage.seg[1], A = stage.seg[2];

  // 2. E and the four candidates
  if (tid == 0) {
    double E[9];
    CtkPose c4[4];
    bool ok4[4] = {false, false, false, false};
    const bool stands = ctk_pose_essential(p.fundamental + o * 9, cam, E) && M >= p.min_points && ctk_pose_decompose(E, c4, ok4);
    state[0] = stands ? 1 : 0, state[1] = -1, state[2] = 0;
    if (stands) {
      for (int k = 0; k < 4; ++k) cand[k] = c4[k], cand_ok[k] = ok4[k] ? 1 : 0;
    }
  }
  __syncthreads();

  // 3. the vote
  if (state[0] != 0) {  // (the same in every thread)
    int cnt[4] = {0, 0, 0, 0};
    for (int m = tid; m < M; m += PO_CHUNK) {
      const int4 q = pts[m];
      double x[3], y[3];
      ctk_pose_ray(cam, q.x, q.y, x);
      ctk_pose_ray(cam, q.z, q.w, y);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        double zs, zf;
        ctk_pose_depths(cand[k], x, y, &zs, &zf);
        cnt[k] += ctk_pose_front(zs, zf) ? 1 : 0;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int t = (int)motion_wave_sum((int64_t)cnt[k]);
      if (lane == 0) wave_vote[wave][k] = t;
    }
    __syncthreads();
    if (tid == 0) {
      int count[4];
      bool ok4[4];
      for (int k = 0; k < 4; ++k) count[k] = wave_vote[0][k] + wave_vote[1][k] + wave_vote[2][k] + wave_vote[3][k], ok4[k] = cand_ok[k] != 0;
      const int k = ctk_pose_choose(count, ok4);
      state[1] = k;
      if (k >= 0) fit = cand[k];
    }
    __syncthreads();
  }
  const int chosen = state[1];
  if (chosen < 0) {  // (the same in every thread) no fit
    for (int m = tid; m < A; m += PO_CHUNK) {
      const int n = slot[m];
      dep_out[n * 2L] = ctk_pose_nan(), dep_out[n * 2L + 1] = ctk_pose_nan();
    }
    if (tid == 0) {
      float m12[12];
      ctk_pose_identity(m12);
      float* po = p.pose + o * 12;
#pragma unroll
      for (int i = 0; i < 12; ++i) po[i] = m12[i];
      int32_t* st = p.stats + o * 4;
      st[0] = M, st[1] = 0, st[2] = -1, st[3] = 0;
    }
    return;
  }

  // 4. the two rounds
  for (int round = 0; round < CTK_POSE_ROUNDS; ++round) {
    const CtkPose cur = fit;
    int64_t s[CTK_POSE_SUMS];
#pragma unroll
    for (int i = 0; i < CTK_POSE_SUMS; ++i) s[i] = 0;
    int took = 0;
    for (int m = tid; m < M; m += PO_CHUNK) {
      const int4 q = pts[m];
      double x[3], y[3], v[7], gg;
      ctk_pose_ray(cam, q.x, q.y, x);
      ctk_pose_ray(cam, q.z, q.w, y);
      if (ctk_pose_entry(cur, x, y, v, &gg)) {
        ctk_pose_terms(v, gg, s);
        ++took;
      }
    }
    // (fit_block_sums' loop, written out: called as a function the same loop compiles to 216 VGPRs here, against 160 -- one wave a SIMD less)
#pragma unroll
    for (int i = 0; i < CTK_POSE_SUMS; ++i) {
      const int64_t t = motion_wave_sum(s[i]);
      if (lane == 0) wave_sum[wave][i] = t;
    }
    {
      const int64_t t = motion_wave_sum((int64_t)took);
      if (lane == 0) wave_sum[wave][CTK_POSE_SUMS] = t;
    }
    __syncthreads();
    if (tid == 0) {
      for (int i = 0; i <= CTK_POSE_SUMS; ++i) total[i] = wave_sum[0][i] + wave_sum[1][i] + wave_sum[2][i] + wave_sum[3][i];
      const int n = (int)total[CTK_POSE_SUMS];
      if (n < M) state[2] |= 4;
      CtkPose next;
      if (ctk_pose_update(cur, total, n, solve, &next)) fit = next;
      else state[2] |= 1 << round;
    }
    __syncthreads();  // the round's pose is published; wave_sum is written again only behind the next round's barrier
  }

  // 5. the outputs under the final pose
  const CtkPose fin = fit;
  int count = 0;
  for (int m = tid; m < A; m += PO_CHUNK) {
    const int4 q = pts[m];
    double x[3], y[3], zs, zf;
    ctk_pose_ray(cam, q.x, q.y, x);
    ctk_pose_ray(cam, q.z, q.w, y);
    ctk_pose_depths(fin, x, y, &zs, &zf);
    const int n = slot[m];
    dep_out[n * 2L] = ctk_pose_depth_out(zs), dep_out[n * 2L + 1] = ctk_pose_depth_out(zf);
    count += (m < M && ctk_pose_front(zs, zf)) ? 1 : 0;
  }
  count = (int)motion_wave_sum((int64_t)count);
  if (lane == 0) wave_count[wave] = count;
  __syncthreads();
  if (tid == 0) {
    float m12[12];
    ctk_pose_out(fin, m12);
    float* po = p.pose + o * 12;
#pragma unroll
    for (int i = 0; i < 12; ++i) po[i] = m12[i];
    int32_t* st = p.stats + o * 4;
    st[0] = M, st[1] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3], st[2] = chosen, st[3] = state[2];
  }
}

// everything but the pointers (whether an anchor is given is looked at)
int pose_check_shape(const ctk_fit_pose_args* a) {
  if (!fit_check_source(fit_source_of(a), a->F) || a->reserved != 0) return CTK_E_SHAPE;
  if (a->min_points < CTK_POSE_MIN_POINTS || a->min_points > CTK_MOTION_POINTS_MAX) return CTK_E_SHAPE;
  if (!fit_check_camera(a)) return CTK_E_SHAPE;
  return CTK_OK;
}

}  // namespace

extern "C" int ctk_fit_pose_workspace_bytes(const ctk_fit_pose_args* a, size_t* out_bytes) {
  if (!a || !out_bytes) return CTK_E_NULL;
  const int rc = pose_check_shape(a);
  if (rc != CTK_OK) return rc;
  *out_bytes = 0;  // the one-launch form keeps everything in LDS
  return CTK_OK;
}

extern "C" int ctk_fit_pose(const ctk_fit_pose_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  if (!a) return CTK_E_NULL;
  PoseParams p;
  p.src = fit_source_of(a);
  if (fit_null_source(p.src) || !a->fundamental || !a->label || !a->pose || !a->depth || !a->stats) return CTK_E_NULL;
  const int rc = pose_check_shape(a);
  if (rc != CTK_OK) return rc;
  (void)workspace, (void)workspace_bytes;  // the query answers 0: nothing is too small
  if (!fit_align_source(p.src)) return CTK_E_ALIGN;
  if (((reinterpret_cast<uintptr_t>(a->fundamental) | reinterpret_cast<uintptr_t>(a->pose) | reinterpret_cast<uintptr_t>(a->depth) |
        reinterpret_cast<uintptr_t>(a->stats)) & 3u) != 0)
    return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);

  p.min_points = a->min_points;
  p.cam.fx = (double)a->fx, p.cam.fy = (double)a->fy, p.cam.cx = (double)a->cx, p.cam.cy = (double)a->cy;
  p.mask = a->mask, p.fundamental = a->fundamental, p.label = a->label;
  p.pose = a->pose, p.depth = a->depth, p.stats = a->stats;
  {
    CtkProfScope prof("fit_pose", 0.0, (double)a->G * a->F * (a->N_out * 46.0 + 100.0), s);
    fit_launch(fit_pose_kernel, a->F, a->G, (size_t)a->N_out * PO_ENTRY_BYTES, CTK_MOTION_POINTS_MAX * PO_ENTRY_BYTES, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
