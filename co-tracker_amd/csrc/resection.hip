// Camera resection on the device (include/ctk.h, "fit resection"): per (group, frame) the tracked positions of the points of a 3-D
// structure become the camera's pose in the structure's unit and coordinates, by the rules of resection_math.h (and, through it,
// pose_math.h, epipolar_math.h, plane_math.h, objects_math.h and motion_math.h).  The frame of the call is ctk_fit_pose's (pose.hip):
// the same workgroup layout, and from fit_device.h the same source and slot gather (CtkFitSource, fit_gather) and the same sums.  The
// staging stays here, with its capped list, its own entry layout and its `same` count: it uses the shared gather only.  One launch, no
// atomics, no workspace; every output element is one plain store; `structure`, `valid` and `seed_pose` are only read.
//
// One workgroup of 256 threads owns one (group, frame).  Dynamic LDS: the fit list, at most CTK_RESECTION_LIST_MAX entries of
// a = R0 X (three doubles, one array per component), Q (two int32) and the slot n (uint16): 34 bytes each, 136 KiB at most.
// seed      thread 0 reads the seed pose, orthogonalises it and publishes (R0 | t0).
// stage     two passes over chunks of 256 slots (the rows are gathered twice): the first counts the entries of the fit list by
//           ballots; the second places them in ascending n, the first 4096 of them.
// scalars   hypothesis k's entry gives its scale s_k into LDS, a thread per hypothesis (none on a frame that is `still`).
// score     candidates outer, entries inner: wave w walks the candidates k = w, w + 4, ... and counts each over the whole list by
//           __ballot / __popcll; every wave keeps its best (count, k), the four are reduced through LDS.  The (I, 0) candidate reads
//           X from global memory through the slot list.
// rounds    three times: the list is walked, an entry per thread (X again from global memory): the 28 fixed-point int64 sums of the
//           entries within tol and their count; reduced by wave shuffles and through LDS; thread 0 solves the 8 x 8 system.
// outputs   ALL N_out slots are gathered once more from global memory and labelled under the final pose.
#include "ctk_common.h"
#include "ctk_profile.h"
#include "fit_device.h"
#include "resection_math.h"

namespace {

constexpr int RS_CHUNK = 256;
constexpr int RS_ENTRY_BYTES = 3 * (int)sizeof(double) + (int)sizeof(int2) + (int)sizeof(uint16_t);  // a, Q and the slot
constexpr int RS_SLOTS = CTK_POSE_SUMS + 2;  // the sums, the count, and one to keep rows 16-byte multiples

struct ResectionParams {
  CtkFitSource src;
  int min_points, K, cap;
  uint32_t seed;
  float tol;
  CtkPoseCam cam;
  const float* structure;
  const int8_t* valid;
  const float* seed_pose;
  float* pose;
  int8_t* label;
  float* error;
  int32_t* stats;
};

// -1: no correspondence, or the point is not in the structure; 0: a structure point with a correspondence  (*q = (Qx, Qy); *same:
// P = Q -- the source position decides with the frame's; X: the point's doubles)
__device__ __forceinline__ int resection_segment(const ResectionParams& p, const FitFrame& fr, int n, int2* q, double* X, bool* same) {
  *same = false;
  int4 v;
  if (!fit_gather(p.src, fr, n, &v)) return -1;
  *q = make_int2(v.z, v.w);
  *same = v.x == v.z && v.y == v.w;
  const float* s = p.structure + (fr.g * p.src.N + n) * 3;
  const float s3[3] = {s[0], s[1], s[2]};
  return ctk_resection_point(s3, p.valid[fr.g * p.src.N + n], X) ? 0 : -1;
}

// grid: x = frame f0 + x, y = group; dynamic LDS: cap * 34 bytes, cap = min(N_out, CTK_RESECTION_LIST_MAX)
__global__ __launch_bounds__(256) void fit_resection_kernel(ResectionParams p) {
  extern __shared__ __attribute__((aligned(16))) double list_a[];
  double* ax = list_a;
  double* ay = ax + p.cap;
  double* az = ay + p.cap;
  int2* qs = reinterpret_cast<int2*>(az + p.cap);
  uint16_t* slot = reinterpret_cast<uint16_t*>(qs + p.cap);
  __shared__ __attribute__((aligned(16))) double scal[CTK_RESECTION_HYPOTHESES_MAX];
  __shared__ __attribute__((aligned(16))) double solve[CTK_POSE_SOLVE_DOUBLES];
  __shared__ __attribute__((aligned(16))) int64_t wave_sum[4][RS_SLOTS];
  __shared__ __attribute__((aligned(16))) int64_t total[RS_SLOTS];
  __shared__ __attribute__((aligned(16))) CtkPose seed0;  // 96 bytes
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
  const float* str = p.structure + g * p.src.N * 3;
  const CtkPoseCam cam = p.cam;
  const double tol2 = ctk_resection_tol2(p.tol);
  const int K = p.K;

  // 1. the seed
  if (tid == 0) {
    float m12[12];
    const float* sp = p.seed_pose + o * 12;
#pragma unroll
    for (int i = 0; i < 12; ++i) m12[i] = sp[i];
    CtkPose s;
    ctk_resection_seed(m12, &s);
    seed0 = s;
    run[0] = 0, run[1] = 0;
  }

  // 2. stage the fit list
  {
    int cnt = 0, cnt_same = 0;  // of this wave
    for (int c0 = 0; c0 < N_out; c0 += RS_CHUNK) {
      int2 q;
      double X[3];
      bool same;
      const int r = resection_segment(p, fr, c0 + tid, &q, X, &same);
      cnt += __popcll(__ballot(r == 0)), cnt_same += __popcll(__ballot(r == 0 && same));
    }
    if (lane == 0) wave_lab[wave] = cnt, wave_count[wave] = cnt_same;
    __syncthreads();  // (the seed is published behind this barrier too)
    if (tid == 0) {
      const int all = wave_lab[0] + wave_lab[1] + wave_lab[2] + wave_lab[3];
      const int same = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
      const bool still = all > 0 && same == all;
      state[0] = all, state[1] = -1, state[2] = (all > p.cap ? CTK_RESECTION_BIT_CAP : 0) | (still ? CTK_RESECTION_BIT_STILL : 0), state[3] = still ? 1 : 0;
    }
    __syncthreads();
    const CtkPose s0 = seed0;
    for (int c = 0, c0 = 0; c0 < N_out; c0 += RS_CHUNK, ++c) {
      const int n = c0 + tid, cur = c & 1;
      int2 q = make_int2(0, 0);
      double X[3] = {0.0, 0.0, 0.0};
      bool same;
      const int r = resection_segment(p, fr, n, &q, X, &same);
      const unsigned long long m0 = __ballot(r == 0);
      if (lane == 0) wave_lab[wave] = __popcll(m0);
      const int rank = __popcll(m0 & below);
      __syncthreads();
      if (r == 0) {
        int place = run[cur] + rank;
        for (int w = 0; w < wave; ++w) place += wave_lab[w];
        if (place < p.cap) {  // (the list holds cap entries; what comes later is classified by the output walk only)
          ax[place] = ctk_pose_dot(s0.R, X), ay[place] = ctk_pose_dot(s0.R + 3, X), az[place] = ctk_pose_dot(s0.R + 6, X);
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
  const CtkPose s0 = seed0;

  if (M >= p.min_points) {  // (the same in every thread)
    // 3. the candidates' scalars
    for (int k = tid; k < K && !still; k += RS_CHUNK) {
      int i, j;
      ctk_motion_sample(p.seed, f, k, M, CTK_MOTION_TRANSLATION, &i, &j);
      const double a[3] = {ax[i], ay[i], az[i]};
      const int2 q = qs[i];
      const double s = ctk_resection_scale(cam, a, q.x, q.y, s0.t);
      scal[k] = ctk_resection_scale_ok(s) ? s : -1.0;
    }
    __syncthreads();

    // 4. the score: wave w owns the candidates k = w, w + 4, ...
    int best = -1, best_k = -1;
    for (int k = wave; k < K + 3; k += 4) {
      if (still && k != K + 2) continue;  // (the same in every thread) the frame is the source frame: (I, 0) alone
      double s = k == K ? 1.0 : 0.0;
      if (k < K) {
        s = scal[k];
        if (!(s > 0.0)) continue;  // (the same in the whole wave) skipped
      }
      const bool eye = k == K + 2;
      // (two entries a lane and step: the wave is alone on its SIMD, so the second projection is what hides the first one's latency)
      auto within = [&](int m) {
        if (m >= M) return false;
        double Xc[3], uvd[5];
        if (eye) {
          const float* sp = str + (long)slot[m] * 3;
          Xc[0] = (double)sp[0], Xc[1] = (double)sp[1], Xc[2] = (double)sp[2];
        } else {
          const double a[3] = {ax[m], ay[m], az[m]};
          ctk_resection_shift(a, s, s0.t, Xc);
        }
        const int2 q = qs[m];
        return ctk_resection_within(ctk_resection_error(cam, Xc, q.x, q.y, uvd), tol2);
      };
      int cnt = 0;
      for (int m0 = 0; m0 < M; m0 += 128) {
        const bool in0 = within(m0 + lane), in1 = within(m0 + 64 + lane);
        cnt += __popcll(__ballot(in0)) + __popcll(__ballot(in1));
      }
      if (ctk_resection_better(cnt, k, best, best_k < 0 ? 0x7fffffff : best_k)) best = cnt, best_k = k;
    }
    if (lane == 0) wave_best[wave][0] = best, wave_best[wave][1] = best_k;
    __syncthreads();
    if (tid == 0) {
      int b = -1, bk = -1;
      for (int w = 0; w < 4; ++w)
        if (wave_best[w][1] >= 0 && ctk_resection_better(wave_best[w][0], wave_best[w][1], b, bk < 0 ? 0x7fffffff : bk))
          b = wave_best[w][0], bk = wave_best[w][1];
      if (b >= p.min_points) {
        state[1] = bk;
        CtkPose w;
        ctk_resection_eye(&w);
        if (bk != K + 2) {
          const double s = bk < K ? scal[bk] : (bk == K ? 1.0 : 0.0);
          for (int i = 0; i < 9; ++i) w.R[i] = s0.R[i];
          for (int i = 0; i < 3; ++i) w.t[i] = s * s0.t[i];
        }
        fit = w;
      }
    }
    __syncthreads();
  }
  const int chosen = state[1];

  if (chosen >= 0 && !still) {  // (the same in every thread)
    // 5. the three rounds
    const double c2 = ctk_resection_c2(cam), ic2 = ctk_resection_ic2(c2);
    for (int round = 0; round < CTK_RESECTION_ROUNDS; ++round) {
      const CtkPose cur = fit;
      int64_t s[CTK_POSE_SUMS];
#pragma unroll
      for (int i = 0; i < CTK_POSE_SUMS; ++i) s[i] = 0;
      int took = 0, left = 0;
      for (int m = tid; m < M; m += RS_CHUNK) {
        const float* sp = str + (long)slot[m] * 3;
        const double X[3] = {(double)sp[0], (double)sp[1], (double)sp[2]};
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
        for (int i = 0; i < RS_SLOTS; ++i) total[i] = wave_sum[0][i] + wave_sum[1][i] + wave_sum[2][i] + wave_sum[3][i];
        const int n = (int)total[CTK_POSE_SUMS];
        if (total[CTK_POSE_SUMS + 1] != 0) state[2] |= 4;
        CtkPose next;
        if (ctk_resection_update(cur, total, n, solve, &next)) fit = next;
        else state[2] |= round == 0 ? 1 : (round == 1 ? 2 : 16);
      }
      __syncthreads();  // the round's pose is published; wave_sum is written again only behind the next round's barrier
    }
  }

  // 6. the outputs: every slot, gathered again
  CtkPose fin;
  if (chosen >= 0) fin = fit;
  else ctk_resection_eye(&fin);
  int count = 0;
  for (int c0 = 0; c0 < N_out; c0 += RS_CHUNK) {
    const int n = c0 + tid;
    int2 q = make_int2(0, 0);
    double X[3] = {0.0, 0.0, 0.0};
    bool same;
    const int r = resection_segment(p, fr, n, &q, X, &same);
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
int resection_check_shape(const ctk_fit_resection_args* a) {
  if (!fit_check_source(fit_source_of(a), a->F)) return CTK_E_SHAPE;
  if (a->min_points < CTK_RESECTION_MIN_POINTS || a->min_points > CTK_MOTION_POINTS_MAX) return CTK_E_SHAPE;
  if (a->hypotheses < 1 || a->hypotheses > CTK_RESECTION_HYPOTHESES_MAX) return CTK_E_SHAPE;
  if (!fit_scale_ok(a->tol) || !fit_check_camera(a)) return CTK_E_SHAPE;
  return CTK_OK;
}

}  // namespace

extern "C" int ctk_fit_resection_workspace_bytes(const ctk_fit_resection_args* a, size_t* out_bytes) {
  if (!a || !out_bytes) return CTK_E_NULL;
  const int rc = resection_check_shape(a);
  if (rc != CTK_OK) return rc;
  *out_bytes = 0;  // the one-launch form keeps everything in LDS
  return CTK_OK;
}

extern "C" int ctk_fit_resection(const ctk_fit_resection_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  if (!a) return CTK_E_NULL;
  ResectionParams p;
  p.src = fit_source_of(a);
  if (fit_null_source(p.src) || !a->structure || !a->valid || !a->seed_pose || !a->pose || !a->label || !a->error || !a->stats) return CTK_E_NULL;
  const int rc = resection_check_shape(a);
  if (rc != CTK_OK) return rc;
  (void)workspace, (void)workspace_bytes;  // the query answers 0: nothing is too small
  if (!fit_align_source(p.src)) return CTK_E_ALIGN;
  if (((reinterpret_cast<uintptr_t>(a->structure) | reinterpret_cast<uintptr_t>(a->seed_pose) | reinterpret_cast<uintptr_t>(a->pose) |
        reinterpret_cast<uintptr_t>(a->error) | reinterpret_cast<uintptr_t>(a->stats)) & 3u) != 0)
    return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);

  p.min_points = a->min_points, p.K = a->hypotheses, p.seed = a->seed;
  p.cap = a->N_out < CTK_RESECTION_LIST_MAX ? a->N_out : CTK_RESECTION_LIST_MAX;
  p.tol = a->tol;
  p.cam.fx = (double)a->fx, p.cam.fy = (double)a->fy, p.cam.cx = (double)a->cx, p.cam.cy = (double)a->cy;
  p.structure = a->structure, p.valid = a->valid, p.seed_pose = a->seed_pose;
  p.pose = a->pose, p.label = a->label, p.error = a->error, p.stats = a->stats;
  {
    CtkProfScope prof("fit_resection", 0.0, (double)a->G * a->F * (a->N_out * 50.0 + 100.0), s);
    fit_launch(fit_resection_kernel, a->F, a->G, (size_t)p.cap * RS_ENTRY_BYTES, CTK_RESECTION_LIST_MAX * RS_ENTRY_BYTES, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
