// Two 3-D point sets aligned on the device (include/ctk.h, "fit align"): per pair g the similarity Y ~ s R X + t between the points
// a[g] and b[g] that share slots, by the rules of align_math.h (and, through it, p3p_math.h and what that one names).  The frame of
// the call is ctk_fit_p3p's (p3p.hip): the same workgroup layout, the same two-pass staging of a capped list, a lane a candidate, the
// same reductions (motion_wave_sum, fit_block_sums, fit_wave_max) and the same output walk.  There is no stream history in this call,
// so no CtkFitSource: a correspondence is decided from the two sets alone (ctk_align_point).  fit_stage places int4 entries without a
// cap, which neither holds six floats nor stops at 4096, so the capped staging is p3p.hip's form.  One launch, no atomics, no
// workspace; every output element is one plain store; the inputs are only read.
//
// One workgroup of 256 threads owns one pair.  Dynamic LDS: the fit list, at most CTK_RESECTION_LIST_MAX entries of X and Y as floats
// (one array per component; they are widened where they are read, as the rules widen them): 24 bytes each, 96 KiB at most, inside the
// 136 KiB of ctk_fit_resection's list.  The slot of an entry is not kept: the output walk gathers every slot again.
// stage     two passes over chunks of 256 slots: the first counts the entries of the fit list and the correspondences that are the
//           same in both sets by ballots; the second places the entries in ascending n, the first 4096 of them.
// score     as p3p.hip: lane l of wave w MAKES candidate b + 4 l + w of the batch that starts at b and keeps its thirteen doubles in
//           registers; the wave takes the candidates that stand one after the other, lowest k first, by v_readlane, and counts each
//           over the whole list by __ballot / __popcll.  Every wave keeps its best; the four are reduced through LDS behind ONE
//           barrier.  The fixed candidate k = K needs no making: wave K % 4 counts it last.
// rounds    three times: the reach of the entries within the round's gates (an integer maximum), then their 36 fixed-point int64
//           sums and their count; reduced by wave shuffles and through LDS; thread 0 solves the 8 x 8 system in LDS.
// outputs   ALL N slots are gathered once more from global memory and labelled under the final transform.
#include "ctk_common.h"
#include "ctk_profile.h"
#include "fit_device.h"
#include "align_math.h"

namespace {

constexpr int AL_CHUNK = 256;
constexpr int AL_ENTRY_BYTES = 6 * (int)sizeof(float);
constexpr int AL_SLOTS = CTK_ALIGN_SUMS + 2;  // the sums, the entries that took part and those left out

struct AlignParams {
  int N, min_points, K, cap;
  uint32_t seed;
  float tol, depth_tol;
  CtkPoseCam cam;
  const float* a;
  const int8_t* valid_a;
  const float* b;
  const int8_t* valid_b;
  const uint8_t* mask;
  float* sim;
  float* scale;
  int8_t* label;
  float* error;
  int32_t* stats;
};

// -1: no correspondence; 0: a correspondence on the fit list; 1: a correspondence the mask keeps off it  (*same: a[n] == b[n])
__device__ __forceinline__ int align_segment(const AlignParams& p, long g, int n, double* X, double* Y, bool* same) {
  *same = false;
  if (n >= p.N) return -1;
  const long o = g * p.N + n;
  const float* pa = p.a + o * 3;
  const float* pb = p.b + o * 3;
  const float a3[3] = {pa[0], pa[1], pa[2]}, b3[3] = {pb[0], pb[1], pb[2]};
  if (!ctk_align_point(a3, p.valid_a[o], b3, p.valid_b[o], X, Y, same)) return -1;
  return p.mask == nullptr || p.mask[o] != 0 ? 0 : 1;
}

// the double that lane j of the wave holds (j is the same in every lane)
__device__ __forceinline__ double align_from_lane(double v, int j) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
  return __hiloint2double(hi, lo);
}

// grid: y = pair; dynamic LDS: cap * 24 bytes, cap = min(N, CTK_RESECTION_LIST_MAX)
__global__ __launch_bounds__(256) void fit_align_kernel(AlignParams p) {
  extern __shared__ __attribute__((aligned(16))) float list_f[];
  float* ax = list_f;
  float* ay = ax + p.cap;
  float* az = ay + p.cap;
  float* bx = az + p.cap;
  float* by = bx + p.cap;
  float* bz = by + p.cap;
  __shared__ __attribute__((aligned(16))) double solve[CTK_POSE_SOLVE_DOUBLES];
  __shared__ __attribute__((aligned(16))) int64_t wave_sum[4][AL_SLOTS];
  __shared__ __attribute__((aligned(16))) int64_t total[AL_SLOTS];
  __shared__ __attribute__((aligned(16))) CtkAlign wave_fit[4];  // 104 bytes each
  __shared__ __attribute__((aligned(16))) CtkAlign fit;
  __shared__ __attribute__((aligned(16))) int wave_best[4];    // (the count and the k of a wave's best in arrays of their own: as one
  __shared__ __attribute__((aligned(16))) int wave_best_k[4];  // pair the compiler swaps them by a packed move right in front of the store)
  __shared__ __attribute__((aligned(16))) int wave_lab[4];
  __shared__ __attribute__((aligned(16))) int run[2];
  __shared__ __attribute__((aligned(16))) int wave_count[4];
  __shared__ __attribute__((aligned(16))) int wave_all[4];
  __shared__ __attribute__((aligned(16))) int wave_reach[4];
  __shared__ __attribute__((aligned(16))) int state[4];  // [0]: every entry of the fit list; [1]: the winning k; [2]: the bits; [3]: identical
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int N = p.N;
  __builtin_assume(N > 0);
  const long g = (long)blockIdx.y;
  int8_t* lab_out = p.label + g * (long)N;
  float* err_out = p.error + g * (long)N;
  const CtkPoseCam cam = p.cam;
  const double tol2 = ctk_resection_tol2(p.tol), dtol = (double)p.depth_tol;
  const int K = p.K;
  const CtkAlignWeights weights = ctk_align_weights(cam, p.tol, p.depth_tol);

  // 1. stage the fit list
  {
    if (tid == 0) run[0] = 0, run[1] = 0;
    int cnt = 0, cnt_all = 0, cnt_same = 0;  // of this wave
    for (int c0 = 0; c0 < N; c0 += AL_CHUNK) {
      double X[3], Y[3];
      bool same;
      const int r = align_segment(p, g, c0 + tid, X, Y, &same);
      cnt += __popcll(__ballot(r == 0)), cnt_all += __popcll(__ballot(r >= 0)), cnt_same += __popcll(__ballot(r >= 0 && same));
    }
    if (lane == 0) wave_lab[wave] = cnt, wave_all[wave] = cnt_all, wave_count[wave] = cnt_same;
    __syncthreads();
    if (tid == 0) {
      const int listed = wave_lab[0] + wave_lab[1] + wave_lab[2] + wave_lab[3];
      const int all = wave_all[0] + wave_all[1] + wave_all[2] + wave_all[3];
      const int same = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
      const bool identical = all > 0 && same == all;
      state[0] = listed, state[1] = -1, state[3] = identical ? 1 : 0;
      state[2] = (listed > p.cap ? CTK_RESECTION_BIT_CAP : 0) | (identical ? CTK_RESECTION_BIT_STILL : 0);
    }
    __syncthreads();
    for (int c = 0, c0 = 0; c0 < N; c0 += AL_CHUNK, ++c) {
      const int cur = c & 1;
      double X[3] = {0.0, 0.0, 0.0}, Y[3] = {0.0, 0.0, 0.0};
      bool same;
      const int r = align_segment(p, g, c0 + tid, X, Y, &same);
      const unsigned long long m0 = __ballot(r == 0);
      if (lane == 0) wave_lab[wave] = __popcll(m0);
      const int rank = __popcll(m0 & below);
      __syncthreads();
      if (r == 0) {
        int place = run[cur] + rank;
        for (int w = 0; w < wave; ++w) place += wave_lab[w];
        if (place < p.cap) {  // (the list holds cap entries; what comes later is classified by the output walk only)
          ax[place] = (float)X[0], ay[place] = (float)X[1], az[place] = (float)X[2];  // (the doubles are widened floats: exact)
          bx[place] = (float)Y[0], by[place] = (float)Y[1], bz[place] = (float)Y[2];
        }
      }
      if (tid == 0) run[cur ^ 1] = run[cur] + wave_lab[0] + wave_lab[1] + wave_lab[2] + wave_lab[3];
      __syncthreads();  // the running end of the next chunk is complete, and wave_lab is written again only behind it
    }
  }
  const int M = state[0] < p.cap ? state[0] : p.cap;
  const bool identical = state[3] != 0;
  auto entry = [&](int m, double* X, double* Y) {
    X[0] = (double)ax[m], X[1] = (double)ay[m], X[2] = (double)az[m];
    Y[0] = (double)bx[m], Y[1] = (double)by[m], Y[2] = (double)bz[m];
  };

  if (M >= CTK_ALIGN_MIN_POINTS) {  // (the same in every thread)
    // 2. the candidates, made a lane each and counted a wave each
    int best = -1, best_k = -1;
    CtkAlign bestc;
    ctk_align_eye(&bestc);
    auto count = [&](const CtkAlign& c) {
      auto within = [&](int m) {
        if (m >= M) return false;
        double X[3], Y[3], Z[3];
        entry(m, X, Y);
        ctk_align_apply(c, X, Z);
        return ctk_align_within(cam, Z, Y, tol2, dtol);
      };
      int cnt = 0;
      for (int m0 = 0; m0 < M; m0 += 128) {
        const bool in0 = within(m0 + lane), in1 = within(m0 + 64 + lane);
        cnt += __popcll(__ballot(in0)) + __popcll(__ballot(in1));
      }
      return cnt;
    };
    for (int b0 = 0; b0 < K && !identical; b0 += 4 * 64) {  // (the same in every thread)
      const int k = b0 + 4 * lane + wave;
      CtkAlign mine;
      bool ok = false;
      if (k < K) {
        int idx[3];
        double X[9], Y[9];
        ctk_align_sample(p.seed, k, M, idx);
#pragma unroll
        for (int i = 0; i < 3; ++i) entry(idx[i], X + i * 3, Y + i * 3);
        ok = ctk_align_candidate(X, Y, &mine);
      } else {
        ctk_align_eye(&mine);
      }
      unsigned long long live = __ballot(ok);
      while (live != 0ull) {  // (the same in the whole wave) ascending lanes are ascending k
        const int j = __ffsll((long long)live) - 1;
        live &= live - 1ull;
        CtkAlign c;
        c.s = align_from_lane(mine.s, j);
#pragma unroll
        for (int i = 0; i < 9; ++i) c.R[i] = align_from_lane(mine.R[i], j);
#pragma unroll
        for (int i = 0; i < 3; ++i) c.t[i] = align_from_lane(mine.t[i], j);
        const int cnt = count(c), kj = b0 + 4 * j + wave;
        if (ctk_resection_better(cnt, kj, best, best_k < 0 ? 0x7fffffff : best_k)) best = cnt, best_k = kj, bestc = c;
      }
    }
    if (wave == (K & 3)) {  // the fixed candidate (1, I, 0), k = K
      CtkAlign c;
      ctk_align_eye(&c);
      const int cnt = count(c);
      if (ctk_resection_better(cnt, K, best, best_k < 0 ? 0x7fffffff : best_k)) best = cnt, best_k = K, bestc = c;
    }
    if (lane == 0) wave_best[wave] = best, wave_best_k[wave] = best_k, wave_fit[wave] = bestc;
    __syncthreads();
    if (tid == 0) {
      int b = -1, bk = -1, bw = 0;
      for (int w = 0; w < 4; ++w)
        if (wave_best_k[w] >= 0 && ctk_resection_better(wave_best[w], wave_best_k[w], b, bk < 0 ? 0x7fffffff : bk))
          b = wave_best[w], bk = wave_best_k[w], bw = w;
      if (b >= p.min_points) {
        state[1] = bk;
        fit = wave_fit[bw];
      }
    }
    __syncthreads();
  }
  const int chosen = state[1];

  if (chosen >= 0) {  // (the same in every thread)
    // 3. the three rounds
    for (int round = 0; round < CTK_ALIGN_ROUNDS; ++round) {
      const CtkAlign cur = fit;
      const double gate2 = ctk_structure_gate2(p.tol, round), dgate = ctk_align_dgate(p.depth_tol, round);
      int reach = CTK_ALIGN_NO_REACH;
      for (int m = tid; m < M; m += AL_CHUNK) {
        double X[3], Y[3], Z[3];
        entry(m, X, Y);
        ctk_align_apply(cur, X, Z);
        if (ctk_align_within(cam, Z, Y, gate2, dgate)) {
          const int e = ctk_align_reach(Y);
          reach = e > reach ? e : reach;
        }
      }
      reach = fit_wave_max(reach);
      if (lane == 0) wave_reach[wave] = reach;
      __syncthreads();
#pragma unroll
      for (int w = 0; w < 4; ++w) reach = wave_reach[w] > reach ? wave_reach[w] : reach;
      int64_t s[CTK_ALIGN_SUMS];
#pragma unroll
      for (int i = 0; i < CTK_ALIGN_SUMS; ++i) s[i] = 0;
      int took = 0, left = 0;
      for (int m = tid; m < M; m += AL_CHUNK) {
        double X[3], Y[3], Z[3], v[24];
        entry(m, X, Y);
        ctk_align_apply(cur, X, Z);
        if (ctk_align_within(cam, Z, Y, gate2, dgate)) {
          if (ctk_align_entry(weights, Z, Y, reach, v)) {
            ctk_align_terms(v, s);
            ctk_align_terms(v + 8, s);
            ctk_align_terms(v + 16, s);
            ++took;
          } else {
            ++left;
          }
        }
      }
      fit_block_sums<CTK_ALIGN_SUMS>(s, wave_sum);
      {
        const int64_t t = motion_wave_sum((int64_t)took), u = motion_wave_sum((int64_t)left);
        if (lane == 0) wave_sum[wave][CTK_ALIGN_SUMS] = t, wave_sum[wave][CTK_ALIGN_SUMS + 1] = u;
      }
      __syncthreads();
      if (tid == 0) {
        for (int i = 0; i < AL_SLOTS; ++i) total[i] = wave_sum[0][i] + wave_sum[1][i] + wave_sum[2][i] + wave_sum[3][i];
        const int n = (int)total[CTK_ALIGN_SUMS];
        if (total[CTK_ALIGN_SUMS + 1] != 0) state[2] |= CTK_ALIGN_BIT_LEFT;
        CtkAlign next;
        if (ctk_align_update(cur, total, n, reach, solve, &next)) fit = next;
        else state[2] |= CTK_ALIGN_BIT_ROUND;
      }
      __syncthreads();  // the round's transform is published; wave_sum and wave_reach are written again only behind the next barrier
    }
  }

  // 4. the outputs: every slot, gathered again
  CtkAlign fin;
  if (chosen >= 0) fin = fit;
  else ctk_align_eye(&fin);
  int count = 0;
  for (int c0 = 0; c0 < N; c0 += AL_CHUNK) {
    const int n = c0 + tid;
    double X[3] = {0.0, 0.0, 0.0}, Y[3] = {0.0, 0.0, 0.0};
    bool same;
    const int r = align_segment(p, g, n, X, Y, &same);
    if (n < N) {
      int8_t lab = -1;
      float err = -1.0f;
      if (r >= 0) {
        lab = 0;
        if (chosen >= 0) {
          double Z[3];
          ctk_align_apply(fin, X, Z);
          lab = ctk_align_within(cam, Z, Y, tol2, dtol) ? 1 : 0;
          err = ctk_align_error(cam, Z, Y);
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
    float m12[12], sc = 0.0f;
#pragma unroll
    for (int i = 0; i < 12; ++i) m12[i] = 0.0f;
    if (chosen >= 0) ctk_align_out(fin, m12, &sc);
    float* so = p.sim + g * 12;
#pragma unroll
    for (int i = 0; i < 12; ++i) so[i] = m12[i];
    p.scale[g] = sc;
    int32_t* st = p.stats + g * 4;
    st[0] = M, st[1] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3], st[2] = chosen, st[3] = state[2];
  }
}

// everything but the pointers
int align_check_shape(const ctk_fit_align_args* a) {
  if (a->G < 1 || a->G > 65535 || a->N < 1 || a->N > CTK_MOTION_POINTS_MAX || a->reserved != 0) return CTK_E_SHAPE;
  if (a->min_points < CTK_ALIGN_MIN_POINTS || a->min_points > CTK_MOTION_POINTS_MAX) return CTK_E_SHAPE;
  if (a->hypotheses < 1 || a->hypotheses > CTK_RESECTION_HYPOTHESES_MAX) return CTK_E_SHAPE;
  if (!fit_scale_ok(a->tol) || !fit_scale_ok(a->depth_tol) || !fit_check_camera(a)) return CTK_E_SHAPE;
  return CTK_OK;
}

}  // namespace

extern "C" int ctk_fit_align_workspace_bytes(const ctk_fit_align_args* a, size_t* out_bytes) {
  if (!a || !out_bytes) return CTK_E_NULL;
  const int rc = align_check_shape(a);
  if (rc != CTK_OK) return rc;
  *out_bytes = 0;  // the one-launch form keeps everything in LDS and registers
  return CTK_OK;
}

extern "C" int ctk_fit_align(const ctk_fit_align_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  if (!a) return CTK_E_NULL;
  if (!a->a || !a->valid_a || !a->b || !a->valid_b || !a->sim || !a->scale || !a->label || !a->error || !a->stats) return CTK_E_NULL;
  const int rc = align_check_shape(a);
  if (rc != CTK_OK) return rc;
  (void)workspace, (void)workspace_bytes;  // the query answers 0: nothing is too small
  if (((reinterpret_cast<uintptr_t>(a->a) | reinterpret_cast<uintptr_t>(a->b) | reinterpret_cast<uintptr_t>(a->sim) |
        reinterpret_cast<uintptr_t>(a->scale) | reinterpret_cast<uintptr_t>(a->error) | reinterpret_cast<uintptr_t>(a->stats)) & 3u) != 0)
    return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);

  AlignParams p;
  p.N = a->N, p.min_points = a->min_points, p.K = a->hypotheses, p.seed = a->seed;
  p.cap = a->N < CTK_RESECTION_LIST_MAX ? a->N : CTK_RESECTION_LIST_MAX;
  p.tol = a->tol, p.depth_tol = a->depth_tol;
  p.cam.fx = (double)a->fx, p.cam.fy = (double)a->fy, p.cam.cx = (double)a->cx, p.cam.cy = (double)a->cy;
  p.a = a->a, p.valid_a = a->valid_a, p.b = a->b, p.valid_b = a->valid_b, p.mask = a->mask;
  p.sim = a->sim, p.scale = a->scale, p.label = a->label, p.error = a->error, p.stats = a->stats;
  {
    CtkProfScope prof("fit_align", 0.0, (double)a->G * (a->N * 50.0 + 100.0), s);
    fit_launch(fit_align_kernel, 1, a->G, (size_t)p.cap * AL_ENTRY_BYTES, CTK_RESECTION_LIST_MAX * AL_ENTRY_BYTES, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
