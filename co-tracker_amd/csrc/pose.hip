// Camera pose and point depths on the device (include/ctk.h, "fit pose"): per (group, frame) the fundamental matrix and the labels that
// ctk_fit_epipolar wrote become a rotation, a unit translation and two depths per correspondence, by the rules of pose_math.h (and,
// through it, epipolar_math.h, plane_math.h, objects_math.h and motion_math.h).  The frame of the call is ctk_fit_epipolar's
// (epipolar.hip): the same workgroup layout, the same slot gather, the same two-pass staging -- its loops are copied here, as
// epipolar.hip copied planes.hip's; only what is done with the list differs.  One launch, no atomics, no workspace; every output
// element is one plain store; `fundamental` and `label` are only read.
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
#include "motion_device.h"
#include "pose_math.h"

namespace {

constexpr int PO_CHUNK = 256;
constexpr int PO_ENTRY_BYTES = (int)sizeof(int4) + (int)sizeof(uint16_t);  // a point and its slot
constexpr int PO_SLOTS = CTK_POSE_SUMS + 2;                                // the sums, the count, and one to keep rows 16-byte multiples

struct PoseParams {
  int G, N, N_out, R, f0, to, lag, anchor_frame, min_points;
  float sx, sy, thresh;
  CtkPoseCam cam;
  const float* hc;
  const uint8_t* visible;
  const float* hv;
  const float* hf;
  const int32_t* first_row;
  const float* ac;
  const uint8_t* av;
  const int8_t* mask;
  const float* fundamental;
  const int8_t* label;
  float* pose;
  float* depth;
  int32_t* stats;
};

// slot n of group g: frame f (row_q of the history) against the source frame fs (row_p of the history, or of the anchor)
// -> a correspondence; *pt = (Px, Py, Qx, Qy)
__device__ __forceinline__ bool pose_gather(const PoseParams& p, long g, int f, int fs, long row_p, long row_q, int n, int4* pt) {
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

// -1: no correspondence; 0: on the fit list; 1: a correspondence off it  (n < N_out wherever lab and mask are read)
__device__ __forceinline__ int pose_segment(const PoseParams& p, long g, int f, int fs, long row_p, long row_q, int n, const int8_t* lab,
                                            const int8_t* mask, int4* pt) {
  if (!pose_gather(p, g, f, fs, row_p, row_q, n, pt)) return -1;
  return lab[n] == 1 && (mask == nullptr || mask[n] != 0) ? 0 : 1;
}

// grid: x = frame f0 + x, y = group; dynamic LDS: N_out * 18 bytes
__global__ __launch_bounds__(256) void fit_pose_kernel(PoseParams p) {
  extern __shared__ __attribute__((aligned(16))) int4 pts[];
  uint16_t* slot = reinterpret_cast<uint16_t*>(pts + p.N_out);
  // (the static part is a multiple of 16 bytes, so that the dynamic list behind it keeps its 16-byte alignment)
  __shared__ __attribute__((aligned(16))) double solve[CTK_POSE_SOLVE_DOUBLES];
  __shared__ __attribute__((aligned(16))) int64_t wave_sum[4][PO_SLOTS];
  __shared__ __attribute__((aligned(16))) int64_t total[PO_SLOTS];
  __shared__ __attribute__((aligned(16))) CtkPose cand[4];  // 96 bytes each
  __shared__ __attribute__((aligned(16))) CtkPose fit;
  __shared__ __attribute__((aligned(16))) int wave_vote[4][4];
  __shared__ __attribute__((aligned(16))) int wave_lab[4][2];
  __shared__ __attribute__((aligned(16))) int run[2][2];
  __shared__ __attribute__((aligned(16))) int seg[4];
  __shared__ __attribute__((aligned(16))) int cand_ok[4];
  __shared__ __attribute__((aligned(16))) int wave_count[4];
  __shared__ __attribute__((aligned(16))) int state[4];  // [0]: the decomposition stands; [1]: the chosen k; [2]: the bits
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int F = (int)gridDim.x, pic = (int)blockIdx.x, f = p.f0 + pic;
  const long g = (long)blockIdx.y;
  const bool anchored = p.ac != nullptr;
  const int fs = ctk_objects_source(f, p.to, p.lag, anchored, p.anchor_frame);
  const long row_q = (g * p.R + f % p.R) * p.N;
  const long row_p = anchored ? g * p.N : (fs >= 0 ? (g * p.R + fs % p.R) * p.N : 0);
  const long o = g * F + pic;
  const int8_t* lab = p.label + o * (long)p.N_out;
  float* dep_out = p.depth + o * (long)p.N_out * 2;
  const int8_t* mask = p.mask != nullptr ? p.mask + g * p.N : nullptr;
  const CtkPoseCam cam = p.cam;

  // 1. stage: segment 0 = the fit list, segment 1 = every other correspondence
  {
    int cnt0 = 0, cnt1 = 0;  // of this wave
    for (int c0 = 0; c0 < p.N_out; c0 += PO_CHUNK) {
      int4 pt;
      const int r = pose_segment(p, g, f, fs, row_p, row_q, c0 + tid, lab, mask, &pt);
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
    for (int c = 0, c0 = 0; c0 < p.N_out; c0 += PO_CHUNK, ++c) {
      const int n = c0 + tid, cur = c & 1;
      int4 pt = make_int4(0, 0, 0, 0);
      const int r = pose_segment(p, g, f, fs, row_p, row_q, n, lab, mask, &pt);
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
        dep_out[n * 2L] = ctk_pose_nan(), dep_out[n * 2L + 1] = ctk_pose_nan();
      }
      if (tid < 2) run[cur ^ 1][tid] = run[cur][tid] + wave_lab[0][tid] + wave_lab[1][tid] + wave_lab[2][tid] + wave_lab[3][tid];
      __syncthreads();  // the running ends of the next chunk are complete, and wave_lab is written again only behind it
    }
  }
  const int M = seg[1], A = seg[2];

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

bool pose_scale_ok(float s) { return s > 0.0f && s <= 3.402823466e+38f; }
bool pose_finite(float s) { return fabsf(s) <= 3.402823466e+38f; }

// everything but the pointers (whether an anchor is given is looked at)
int pose_check_shape(const ctk_fit_pose_args* a) {
  const long big = 1L << 30;
  if (a->G <= 0 || a->N <= 0 || a->N_out <= 0 || a->R <= 0 || a->F <= 0 || a->N_out > a->N || a->N_out > CTK_MOTION_POINTS_MAX) return CTK_E_SHAPE;
  if (a->f0 < 0 || (long)a->f0 + a->F > big || a->F > 65535 || a->G > 65535 || (long)a->G * a->N > (1L << 26) || a->reserved != 0) return CTK_E_SHAPE;
  if (a->min_points < CTK_POSE_MIN_POINTS || a->min_points > CTK_MOTION_POINTS_MAX) return CTK_E_SHAPE;
  if (!pose_scale_ok(a->fx) || !pose_scale_ok(a->fy) || !pose_finite(a->cx) || !pose_finite(a->cy)) return CTK_E_SHAPE;
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
  if (!pose_scale_ok(a->sx) || !pose_scale_ok(a->sy)) return CTK_E_SHAPE;
  if (a->visible == nullptr && a->thresh != a->thresh) return CTK_E_SHAPE;
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
  if (!a->hist_coords || !a->fundamental || !a->label || !a->pose || !a->depth || !a->stats) return CTK_E_NULL;
  if (!a->visible && (!a->hist_vis || !a->hist_conf)) return CTK_E_NULL;
  if ((a->anchor_coords != nullptr) != (a->anchor_visible != nullptr)) return CTK_E_NULL;
  const int rc = pose_check_shape(a);
  if (rc != CTK_OK) return rc;
  (void)workspace, (void)workspace_bytes;  // the query answers 0: nothing is too small
  if (((reinterpret_cast<uintptr_t>(a->hist_coords) | reinterpret_cast<uintptr_t>(a->anchor_coords)) & 7u) != 0) return CTK_E_ALIGN;
  if (((reinterpret_cast<uintptr_t>(a->fundamental) | reinterpret_cast<uintptr_t>(a->pose) | reinterpret_cast<uintptr_t>(a->depth) |
        reinterpret_cast<uintptr_t>(a->stats)) & 3u) != 0)
    return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);

  PoseParams p;
  p.G = a->G, p.N = a->N, p.N_out = a->N_out, p.R = a->R, p.f0 = a->f0, p.to = a->to, p.lag = a->lag, p.anchor_frame = a->anchor_frame;
  p.min_points = a->min_points;
  p.sx = a->sx, p.sy = a->sy, p.thresh = a->thresh;
  p.cam.fx = (double)a->fx, p.cam.fy = (double)a->fy, p.cam.cx = (double)a->cx, p.cam.cy = (double)a->cy;
  p.hc = a->hist_coords, p.visible = a->visible, p.hv = a->hist_vis, p.hf = a->hist_conf, p.first_row = a->first_row;
  p.ac = a->anchor_coords, p.av = a->anchor_visible, p.mask = a->mask;
  p.fundamental = a->fundamental, p.label = a->label;
  p.pose = a->pose, p.depth = a->depth, p.stats = a->stats;
  {
    CtkProfScope prof("fit_pose", 0.0, (double)a->G * a->F * (a->N_out * 46.0 + 100.0), s);
    const size_t lds = (size_t)p.N_out * PO_ENTRY_BYTES;
    // (Beyond 64 KiB of LDS a kernel has to say so once; not a stream operation.  As epipolar.hip, from 48 KiB of dynamic LDS on:
    // this kernel holds less than 4 KiB of static LDS beside it, 148 KiB of the CU's 160 KiB at most.)
    if (lds > 49152) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fit_pose_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               CTK_MOTION_POINTS_MAX * PO_ENTRY_BYTES);
    hipLaunchKernelGGL(fit_pose_kernel, dim3((unsigned)a->F, (unsigned)p.G), dim3(256), lds, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
