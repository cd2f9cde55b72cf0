// Camera pose from three points on the device (include/ctk.h, "fit p3p"): per (group, frame) the tracked positions of the points of a
// 3-D structure become the camera's pose in the structure's unit and coordinates WITHOUT a seed pose, by the rules of p3p_math.h (and,
// through it, resection_math.h and what that one names).  The frame of the call is ctk_fit_resection's (resection.hip): the same
// workgroup layout, from fit_device.h the same source and slot gather (CtkFitSource, fit_gather), the same sums and launch, the same
// two-pass staging of a capped list and the same output walk.  One launch, no atomics, no workspace; every output element is one plain
// store; `structure` and `valid` are only read.
//
// One workgroup of 256 threads owns one (group, frame).  Dynamic LDS: the fit list, at most CTK_RESECTION_LIST_MAX entries of X (three
// doubles, one array per component), Q (two int32) and the slot n (uint16): 34 bytes each, 136 KiB at most.
// stage     two passes over chunks of 256 slots (the rows are gathered twice): the first counts the entries of the fit list by
//           ballots; the second places them in ascending n, the first 4096 of them.
// score     wave w owns the candidates k = w, w + 4, ..., 64 of them at a time: lane l of the wave MAKES candidate b + 4 l + w of the
//           batch that starts at b (a few hundred dependent double operations, one candidate a lane; a whole wave on one candidate
//           would pay them once per candidate, which is what scoring it costs).  The twelve doubles stay in the lane's registers: no
//           LDS beside the list is needed for them, 1024 poses would not fit there.  The wave then takes the candidates that stand one
//           after the other, lowest k first: the pose is read from its lane (v_readlane, the lane index is uniform) and counted over
//           the whole list by __ballot / __popcll.  Every wave keeps its best (count, k, pose); the four are reduced through LDS behind
//           ONE barrier.  The (I, 0) candidate k = K needs no making: wave K % 4 counts it last.
// rounds    three times: the list is walked, an entry per thread: the 28 fixed-point int64 sums of the entries within tol and their
//           count; reduced by wave shuffles and through LDS; thread 0 solves the 8 x 8 system.
// outputs   ALL N_out slots are gathered once more from global memory and labelled under the final pose.
#include "ctk_common.h"
#include "ctk_profile.h"
#include "fit_device.h"
#include "p3p_math.h"

namespace {

constexpr int P3_CHUNK = 256;
constexpr int P3_ENTRY_BYTES = 3 * (int)sizeof(double) + (int)sizeof(int2) + (int)sizeof(uint16_t);  // X, Q and the slot
constexpr int P3_SLOTS = CTK_POSE_SUMS + 2;  // the sums, the count, and one to keep rows 16-byte multiples

struct P3pParams {
  CtkFitSource src;
  int min_points, K, cap;
  uint32_t seed;
  float tol;
  CtkPoseCam cam;
  const float* structure;
  const int8_t* valid;
  float* pose;
  int8_t* label;
  float* error;
  int32_t* stats;
};

// -1: no correspondence, or the point is not in the structure; 0: a structure point with a correspondence  (*q = (Qx, Qy); *same:
// P = Q -- the source position decides with the frame's; X: the point's doubles)
__device__ __forceinline__ int p3p_segment(const P3pParams& p, const FitFrame& fr, int n, int2* q, double* X, bool* same) {
  *same = false;
  int4 v;
  if (!fit_gather(p.src, fr, n, &v)) return -1;
  *q = make_int2(v.z, v.w);
  *same = v.x == v.z && v.y == v.w;
  const float* s = p.structure + (fr.g * p.src.N + n) * 3;
  const float s3[3] = {s[0], s[1], s[2]};
  return ctk_resection_point(s3, p.valid[fr.g * p.src.N + n], X) ? 0 : -1;
}

// the double that lane j of the wave holds (j is the same in every lane)
__device__ __forceinline__ double p3p_from_lane(double v, int j) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
  return __hiloint2double(hi, lo);
}

// grid: x = frame f0 + x, y = group; dynamic LDS: cap * 34 bytes, cap = min(N_out, CTK_RESECTION_LIST_MAX)
__global__ __launch_bounds__(256) void fit_p3p_kernel(P3pParams p) {
  extern __shared__ __attribute__((aligned(16))) double list_x[];
  double* ax = list_x;
  double* ay = ax + p.cap;
  double* az = ay + p.cap;
  int2* qs = reinterpret_cast<int2*>(az + p.cap);
  uint16_t* slot = reinterpret_cast<uint16_t*>(qs + p.cap);
  __shared__ __attribute__((aligned(16))) double solve[CTK_POSE_SOLVE_DOUBLES];
  __shared__ __attribute__((aligned(16))) int64_t wave_sum[4][P3_SLOTS];
  __shared__ __attribute__((aligned(16))) int64_t total[P3_SLOTS];
  __shared__ __attribute__((aligned(16))) CtkPose wave_pose[4];  // 96 bytes each
  __shared__ __attribute__((aligned(16))) CtkPose fit;
  __shared__ __attribute__((aligned(16))) int wave_best[4][2];
  __shared__ __attribute__((aligned(16))) int wave_lab[4];
  __shared__ __attribute__((aligned(16))) int run[2];
  __shared__ __attribute__((aligned(16))) int wave_count[4];
  __shared__ __attribute__((aligned(16))) int state[4];  // [0]: every entry of the fit list; [1]: the winning k; [2]: the bits; [3]: still
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int N_out = p.src.N_out;
  const int F = (int)gridDim.x, pic = (int)blockIdx.x, f = p.src.f0 + pic;
  const long g = (long)blockIdx.y;
  const FitFrame fr = fit_frame(p.src, g, f);
  const long o = g * F + pic;
  int8_t* lab_out = p.label + o * (long)N_out;
  float* err_out = p.error + o * (long)N_out;
  const CtkPoseCam cam = p.cam;
  const double tol2 = ctk_resection_tol2(p.tol);
  const int K = p.K;

  // 1. stage the fit list
  {
    if (tid == 0) run[0] = 0, run[1] = 0;
    int cnt = 0, cnt_same = 0;  // of this wave
    for (int c0 = 0; c0 < N_out; c0 += P3_CHUNK) {
      int2 q;
      double X[3];
      bool same;
      const int r = p3p_segment(p, fr, c0 + tid, &q, X, &same);
      cnt += __popcll(__ballot(r == 0)), cnt_same += __popcll(__ballot(r == 0 && same));
    }
    if (lane == 0) wave_lab[wave] = cnt, wave_count[wave] = cnt_same;
    __syncthreads();
    if (tid == 0) {
      const int all = wave_lab[0] + wave_lab[1] + wave_lab[2] + wave_lab[3];
      const int same = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
      const bool still = all > 0 && same == all;
      state[0] = all, state[1] = -1, state[2] = (all > p.cap ? CTK_RESECTION_BIT_CAP : 0) | (still ? CTK_RESECTION_BIT_STILL : 0), state[3] = still ? 1 : 0;
    }
    __syncthreads();
    for (int c = 0, c0 = 0; c0 < N_out; c0 += P3_CHUNK, ++c) {
      const int n = c0 + tid, cur = c & 1;
      int2 q = make_int2(0, 0);
      double X[3] = {0.0, 0.0, 0.0};
      bool same;
      const int r = p3p_segment(p, fr, n, &q, X, &same);
      const unsigned long long m0 = __ballot(r == 0);
      if (lane == 0) wave_lab[wave] = __popcll(m0);
      const int rank = __popcll(m0 & below);
      __syncthreads();
      if (r == 0) {
        int place = run[cur] + rank;
        for (int w = 0; w < wave; ++w) place += wave_lab[w];
        if (place < p.cap) {  // (the list holds cap entries; what comes later is classified by the output walk only)
          ax[place] = X[0], ay[place] = X[1], az[place] = X[2];
          qs[place] = q;
          slot[place] = (uint16_t)n;
        }
      }
      if (tid == 0) run[cur ^ 1] = run[cur] + wave_lab[0] + wave_lab[1] + wave_lab[2] + wave_lab[3];
      __syncthreads();  // the running end of the next chunk is complete, and wave_lab is written again only behind it
    }
  }
  const int M = state[0] < p.cap ? state[0] : p.cap;
  const bool still = state[3] != 0;

  if (M >= p.min_points) {  // (the same in every thread)
    // 2. the candidates, made a lane each and counted a wave each
    int best = -1, best_k = -1;
    CtkPose bestp;
    ctk_resection_eye(&bestp);
    // (two entries a lane and step: the wave is alone on its SIMD, so the second projection is what hides the first one's latency)
    auto count = [&](const CtkPose& c) {
      auto within = [&](int m) {
        if (m >= M) return false;
        const double X[3] = {ax[m], ay[m], az[m]};
        double Xc[3], uvd[5];
        ctk_resection_apply(c, X, Xc);
        const int2 q = qs[m];
        return ctk_resection_within(ctk_resection_error(cam, Xc, q.x, q.y, uvd), tol2);
      };
      int cnt = 0;
      for (int m0 = 0; m0 < M; m0 += 128) {
        const bool in0 = within(m0 + lane), in1 = within(m0 + 64 + lane);
        cnt += __popcll(__ballot(in0)) + __popcll(__ballot(in1));
      }
      return cnt;
    };
    for (int b0 = 0; b0 < K && !still; b0 += 4 * 64) {  // (the same in every thread; a still frame is the source frame: (I, 0) alone)
      const int k = b0 + 4 * lane + wave;
      CtkPose mine;
      bool ok = false;
      if (k < K) {
        int idx[4], q[6];
        double X[9];
        ctk_plane_sample(p.seed, f, k, M, idx);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const int m = idx[i];
          X[i * 3] = ax[m], X[i * 3 + 1] = ay[m], X[i * 3 + 2] = az[m];
          const int2 qq = qs[m];
          q[i * 2] = qq.x, q[i * 2 + 1] = qq.y;
        }
        ok = ctk_p3p_candidate(cam, X, q, &mine);
      } else {
        ctk_resection_eye(&mine);
      }
      unsigned long long live = __ballot(ok);
      while (live != 0ull) {  // (the same in the whole wave) ascending lanes are ascending k
        const int j = __ffsll((long long)live) - 1;
        live &= live - 1ull;
        CtkPose c;
#pragma unroll
        for (int i = 0; i < 9; ++i) c.R[i] = p3p_from_lane(mine.R[i], j);
#pragma unroll
        for (int i = 0; i < 3; ++i) c.t[i] = p3p_from_lane(mine.t[i], j);
        const int cnt = count(c), kj = b0 + 4 * j + wave;
        if (ctk_resection_better(cnt, kj, best, best_k < 0 ? 0x7fffffff : best_k)) best = cnt, best_k = kj, bestp = c;
      }
    }
    if (wave == (K & 3)) {  // the fixed candidate (I, 0), k = K
      CtkPose c;
      ctk_resection_eye(&c);
      const int cnt = count(c);
      if (ctk_resection_better(cnt, K, best, best_k < 0 ? 0x7fffffff : best_k)) best = cnt, best_k = K, bestp = c;
    }
    if (lane == 0) wave_best[wave][0] = best, wave_best[wave][1] = best_k, wave_pose[wave] = bestp;
    __syncthreads();
    if (tid == 0) {
      int b = -1, bk = -1, bw = 0;
      for (int w = 0; w < 4; ++w)
        if (wave_best[w][1] >= 0 && ctk_resection_better(wave_best[w][0], wave_best[w][1], b, bk < 0 ? 0x7fffffff : bk))
          b = wave_best[w][0], bk = wave_best[w][1], bw = w;
      if (b >= p.min_points) {
        state[1] = bk;
        fit = wave_pose[bw];
      }
    }
    __syncthreads();
  }
  const int chosen = state[1];

  if (chosen >= 0 && !still) {  // (the same in every thread)
    // 3. the three rounds
    const double c2 = ctk_resection_c2(cam), ic2 = ctk_resection_ic2(c2);
    for (int round = 0; round < CTK_RESECTION_ROUNDS; ++round) {
      const CtkPose cur = fit;
      int64_t s[CTK_POSE_SUMS];
#pragma unroll
      for (int i = 0; i < CTK_POSE_SUMS; ++i) s[i] = 0;
      int took = 0, left = 0;
      for (int m = tid; m < M; m += P3_CHUNK) {
        const double X[3] = {ax[m], ay[m], az[m]};
        const int2 q = qs[m];
        double Xc[3], uvd[5], vx[7], vy[7];
        ctk_resection_apply(cur, X, Xc);
        if (ctk_resection_within(ctk_resection_error(cam, Xc, q.x, q.y, uvd), tol2)) {
          if (ctk_resection_entry(cam, c2, Xc, uvd, vx, vy)) {
            ctk_resection_terms(vx, ic2, s);
            ctk_resection_terms(vy, ic2, s);
            ++took;
          } else {
            ++left;
          }
        }
      }
      fit_block_sums<CTK_POSE_SUMS>(s, wave_sum);
      {
        const int64_t t = motion_wave_sum((int64_t)took), u = motion_wave_sum((int64_t)left);
        if (lane == 0) wave_sum[wave][CTK_POSE_SUMS] = t, wave_sum[wave][CTK_POSE_SUMS + 1] = u;
      }
      __syncthreads();
      if (tid == 0) {
        for (int i = 0; i < P3_SLOTS; ++i) total[i] = wave_sum[0][i] + wave_sum[1][i] + wave_sum[2][i] + wave_sum[3][i];
        const int n = (int)total[CTK_POSE_SUMS];
        if (total[CTK_POSE_SUMS + 1] != 0) state[2] |= 4;
        CtkPose next;
        if (ctk_resection_update(cur, total, n, solve, &next)) fit = next;
        else state[2] |= round == 0 ? 1 : (round == 1 ? 2 : 16);
      }
      __syncthreads();  // the round's pose is published; wave_sum is written again only behind the next round's barrier
    }
  }

  // 4. the outputs: every slot, gathered again
  CtkPose fin;
  if (chosen >= 0) fin = fit;
  else ctk_resection_eye(&fin);
  int count = 0;
  for (int c0 = 0; c0 < N_out; c0 += P3_CHUNK) {
    const int n = c0 + tid;
    int2 q = make_int2(0, 0);
    double X[3] = {0.0, 0.0, 0.0};
    bool same;
    const int r = p3p_segment(p, fr, n, &q, X, &same);
    if (n < N_out) {
      int8_t lab = -1;
      float err = -1.0f;
      if (r == 0) {
        lab = 0;
        if (chosen >= 0) {
          double Xc[3], uvd[5];
          ctk_resection_apply(fin, X, Xc);
          const double e = ctk_resection_error(cam, Xc, q.x, q.y, uvd);
          lab = ctk_resection_within(e, tol2) ? 1 : 0;
          err = (float)e;
        }
      }
      lab_out[n] = lab, err_out[n] = err;
      count += lab == 1 ? 1 : 0;
    }
  }
  count = (int)motion_wave_sum((int64_t)count);
  if (lane == 0) wave_count[wave] = count;
  __syncthreads();
  if (tid == 0) {
    float m12[12];
    if (chosen >= 0) ctk_pose_out(fin, m12);
    else ctk_pose_identity(m12);
    float* po = p.pose + o * 12;
#pragma unroll
    for (int i = 0; i < 12; ++i) po[i] = m12[i];
    int32_t* st = p.stats + o * 4;
    st[0] = M, st[1] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3], st[2] = chosen, st[3] = state[2];
  }
}

// everything but the pointers (whether an anchor is given is looked at)
int p3p_check_shape(const ctk_fit_p3p_args* a) {
  if (!fit_check_source(fit_source_of(a), a->F)) return CTK_E_SHAPE;
  if (a->min_points < CTK_RESECTION_MIN_POINTS || a->min_points > CTK_MOTION_POINTS_MAX) return CTK_E_SHAPE;
  if (a->hypotheses < 1 || a->hypotheses > CTK_RESECTION_HYPOTHESES_MAX) return CTK_E_SHAPE;
  if (!fit_scale_ok(a->tol) || !fit_check_camera(a)) return CTK_E_SHAPE;
  return CTK_OK;
}

}  // namespace

extern "C" int ctk_fit_p3p_workspace_bytes(const ctk_fit_p3p_args* a, size_t* out_bytes) {
  if (!a || !out_bytes) return CTK_E_NULL;
  const int rc = p3p_check_shape(a);
  if (rc != CTK_OK) return rc;
  *out_bytes = 0;  // the one-launch form keeps everything in LDS and registers
  return CTK_OK;
}

extern "C" int ctk_fit_p3p(const ctk_fit_p3p_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  if (!a) return CTK_E_NULL;
  P3pParams p;
  p.src = fit_source_of(a);
  if (fit_null_source(p.src) || !a->structure || !a->valid || !a->pose || !a->label || !a->error || !a->stats) return CTK_E_NULL;
  const int rc = p3p_check_shape(a);
  if (rc != CTK_OK) return rc;
  (void)workspace, (void)workspace_bytes;  // the query answers 0: nothing is too small
  if (!fit_align_source(p.src)) return CTK_E_ALIGN;
  if (((reinterpret_cast<uintptr_t>(a->structure) | reinterpret_cast<uintptr_t>(a->pose) | reinterpret_cast<uintptr_t>(a->error) |
        reinterpret_cast<uintptr_t>(a->stats)) & 3u) != 0)
    return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);

  p.min_points = a->min_points, p.K = a->hypotheses, p.seed = a->seed;
  p.cap = a->N_out < CTK_RESECTION_LIST_MAX ? a->N_out : CTK_RESECTION_LIST_MAX;
  p.tol = a->tol;
  p.cam.fx = (double)a->fx, p.cam.fy = (double)a->fy, p.cam.cx = (double)a->cx, p.cam.cy = (double)a->cy;
  p.structure = a->structure, p.valid = a->valid;
  p.pose = a->pose, p.label = a->label, p.error = a->error, p.stats = a->stats;
  {
    CtkProfScope prof("fit_p3p", 0.0, (double)a->G * a->F * (a->N_out * 50.0 + 100.0), s);
    fit_launch(fit_p3p_kernel, a->F, a->G, (size_t)p.cap * P3_ENTRY_BYTES, CTK_RESECTION_LIST_MAX * P3_ENTRY_BYTES, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
