// Objects by motion on the device (include/ctk.h, "fit objects"): up to L robust fits per (group, frame) over sub-lists of ONE staged list
// of correspondences, by the integer rules of objects_math.h (and, through it, motion_math.h).  The sub-lists are the regions a caller
// labelled (labels mode) or what is left after the earlier fits took their inliers (split mode).  One launch, no atomics, no
// workspace; every output element is one plain store.
//
// One workgroup of 256 threads owns one (group, frame).  Dynamic LDS: the list of (Px, Py, Qx, Qy) int32 points, 16 bytes each, and
// next to it a uint16 side list that leads an entry back to its slot n: N_out * 18 bytes, 144 KiB at most.
// stage, split   as motion.hip: the two rows are gathered once, in chunks of 256 slots, one slot per thread; the correspondences take
//                their place by a wave ballot and a prefix count (wave totals through LDS), which keeps the slots' order.  A slot
//                that is no correspondence gets its label -1 here.
// stage, labels  two passes over the chunks (the rows are gathered twice): the first counts the correspondences of every label by
//                per-label ballots, which gives each label's segment of the list; the second places every correspondence into its
//                label's segment in ascending n (per-label ballots again, the running segment ends double-buffered in LDS: two
//                barriers per chunk).  A correspondence whose label names no round gets CTK_OBJECT_NONE here and never enters the list.
// round r        score: motion.hip's -- a lane per hypothesis (K beyond 256: further passes) walks the round's list, every lane
//                reading the same LDS address (a broadcast); the keys are reduced by a wave shuffle and through LDS.
//                refit: the list is walked once more, an entry per thread: the inliers of an accepted best add to the eight int64
//                sums and to the box and write their label; in labels mode every other entry of the segment writes CTK_OBJECT_NONE.
//                In split mode the same walk removes the inliers by a stable in-place compaction: chunks of 256, a barrier between a
//                chunk's reads and its writes, and the writes never pass the read position, so one list is enough.  Sums and box are
//                reduced by wave shuffles and through LDS; thread 0 divides and writes the round's matrix, stats and box.
// end, split     a round that fits nothing ends the rounds: the later ones report the same M_r; what is left in the list gets
//                CTK_OBJECT_NONE.
// Every slot is written once: at the stage (no correspondence, no round), by the round that visits it (labels mode), by the round that
// takes it or at the end (split mode).
// Shared with the other fit kernels, from fit_device.h: the source and the slot gather (CtkFitSource, fit_gather), the labels mode's
// two-pass staging (fit_stage, a segment per label) and the reductions.  The single-pass staging of split mode stays here: it uses the
// shared gather only.
#include "ctk_common.h"
#include "ctk_profile.h"
#include "fit_device.h"
#include "objects_math.h"

namespace {

constexpr int OBJ_CHUNK = 256;
constexpr int OBJ_ENTRY_BYTES = (int)sizeof(int4) + (int)sizeof(uint16_t);  // a point and its slot

struct ObjectsParams {
  CtkFitSource src;
  int L, min_points, K, T;
  uint32_t seed;
  int64_t base2;
  const int8_t* labels;
  float* motion;
  int8_t* label;
  int32_t* stats;
  int32_t* box;
};

// grid: x = frame f0 + x, y = group; dynamic LDS: N_out * 18 bytes
template <int MODEL>
__global__ __launch_bounds__(256) void fit_objects_kernel(ObjectsParams p) {
  extern __shared__ int4 pts[];
  uint16_t* slot = reinterpret_cast<uint16_t*>(pts + p.src.N_out);
  __shared__ int wave_hits[4];
  __shared__ FitStageLds<CTK_OBJECTS_MAX> stage;
  __shared__ int64_t wave_key[4];
  __shared__ int64_t wave_sum[4][CTK_MS_COUNT];
  __shared__ int wave_box[4][4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const CtkFitSource& src = p.src;
  const int F = (int)gridDim.x, pic = (int)blockIdx.x, f = src.f0 + pic;
  const long g = (long)blockIdx.y;
  const bool by_labels = p.labels != nullptr;
  const FitFrame fr = fit_frame(src, g, f);
  int8_t* lab_out = p.label + (g * F + pic) * (long)src.N_out;

  // 1. stage
  int M = 0;
  if (!by_labels) {
    for (int c0 = 0; c0 < src.N_out; c0 += OBJ_CHUNK) {
      const int n = c0 + tid;
      int4 pt = make_int4(0, 0, 0, 0);
      const bool hit = fit_gather(src, fr, n, &pt);
      const unsigned long long mask = __ballot(hit);
      if (lane == 0) wave_hits[wave] = __popcll(mask);
      __syncthreads();
      int before = M, total = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int h = wave_hits[w];
        before += w < wave ? h : 0;
        total += h;
      }
      if (hit) {
        const int place = before + __popcll(mask & below);
        pts[place] = pt;
        slot[place] = (uint16_t)n;
      } else if (n < src.N_out) {
        lab_out[n] = -1;
      }
      M += total;
      __syncthreads();  // the list is read, and wave_hits written again, only behind it
    }
  } else {
    const int8_t* labels = p.labels + g * src.N;
    fit_stage(
        stage, src.N_out, pts, slot, [&](int n, int4* pt) { return fit_gather(src, fr, n, pt); },
        [&](int n) { return ctk_objects_round(labels[n], p.L); },
        [&](int n, bool hit) { lab_out[n] = hit ? (int8_t)CTK_OBJECT_NONE : (int8_t)-1; });
  }

  // 2. the rounds
  int lo = 0, Mr = M, r = 0;
  for (; r < p.L; ++r) {
    if (by_labels) lo = stage.seg[r], Mr = stage.seg[r + 1] - stage.seg[r];
    const int4* list = pts + lo;
    const uint32_t seed_r = ctk_objects_seed(p.seed, r);
    int64_t best = -1;
    if (Mr >= (MODEL == CTK_MOTION_SIMILARITY ? 2 : 1)) {
      for (int k = tid; k < p.K; k += OBJ_CHUNK) {
        CtkMotionHyp h;
        if (!motion_hyp_at<MODEL>(seed_r, p.T, p.base2, list, f, k, Mr, &h)) continue;
        int count = 0;
        for (int m = 0; m < Mr; ++m) {
          const int4 q = list[m];
          count += ctk_motion_inlier(MODEL, h, q.x, q.y, q.z, q.w) ? 1 : 0;
        }
        const int64_t key = ctk_motion_key(count, k, p.K);
        best = key > best ? key : best;
      }
    }
    best = fit_block_best(best, wave_key);

    const bool have = ctk_objects_accept(best, p.min_points);
    CtkMotionHyp hb;
    hb.px = hb.py = hb.qx = hb.qy = 0, hb.D = hb.A = hb.B = hb.TD = 0;
    if (have) motion_hyp_at<MODEL>(seed_r, p.T, p.base2, list, f, ctk_motion_key_k(best, p.K), Mr, &hb);
    int64_t s[CTK_MS_COUNT];
#pragma unroll
    for (int i = 0; i < CTK_MS_COUNT; ++i) s[i] = 0;
    int bx[4];
    ctk_objects_box_empty(bx);
    int left = Mr;  // split mode: what the next round fits
    if (by_labels) {
      for (int m = tid; m < Mr; m += OBJ_CHUNK) {
        const int4 q = list[m];
        const bool in = have && ctk_motion_inlier(MODEL, hb, q.x, q.y, q.z, q.w);
        if (in) ctk_motion_accumulate(s, q.x, q.y, q.z, q.w), ctk_objects_box_add(bx, q.z, q.w);
        lab_out[slot[lo + m]] = in ? (int8_t)r : (int8_t)CTK_OBJECT_NONE;
      }
    } else if (have) {
      left = 0;
      for (int c0 = 0; c0 < Mr; c0 += OBJ_CHUNK) {
        const int m = c0 + tid;
        int4 q = make_int4(0, 0, 0, 0);
        uint16_t sn = 0;
        bool keep = false;
        if (m < Mr) {
          q = pts[m], sn = slot[m];
          const bool in = ctk_motion_inlier(MODEL, hb, q.x, q.y, q.z, q.w);
          if (in) {
            ctk_motion_accumulate(s, q.x, q.y, q.z, q.w), ctk_objects_box_add(bx, q.z, q.w);
            lab_out[sn] = (int8_t)r;
          }
          keep = !in;
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wave_hits[wave] = __popcll(mask);
        __syncthreads();  // the chunk has been read by everyone: its places, and those below, may be written
        int before = left, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int h = wave_hits[w];
          before += w < wave ? h : 0;
          total += h;
        }
        if (keep) {
          const int place = before + __popcll(mask & below);  // <= m
          pts[place] = q;
          slot[place] = sn;
        }
        left += total;
        __syncthreads();
      }
    }
    fit_block_sums<CTK_MS_COUNT>(s, wave_sum);
    {
      const int b0 = fit_wave_min(bx[0]), b1 = fit_wave_min(bx[1]), b2 = fit_wave_max(bx[2]), b3 = fit_wave_max(bx[3]);
      if (lane == 0) wave_box[wave][0] = b0, wave_box[wave][1] = b1, wave_box[wave][2] = b2, wave_box[wave][3] = b3;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < CTK_MS_COUNT; ++i) s[i] = wave_sum[0][i] + wave_sum[1][i] + wave_sum[2][i] + wave_sum[3][i];
      float row[6];
      if (have) {
        ctk_motion_refit(MODEL, s, row);
        bx[0] = min(min(wave_box[0][0], wave_box[1][0]), min(wave_box[2][0], wave_box[3][0]));
        bx[1] = min(min(wave_box[0][1], wave_box[1][1]), min(wave_box[2][1], wave_box[3][1]));
        bx[2] = max(max(wave_box[0][2], wave_box[1][2]), max(wave_box[2][2], wave_box[3][2]));
        bx[3] = max(max(wave_box[0][3], wave_box[1][3]), max(wave_box[2][3], wave_box[3][3]));
      } else {
        ctk_motion_identity(row);
        ctk_objects_box_none(bx);
      }
      const long o = ((g * F + pic) * p.L + r);
      float* mo = p.motion + o * 6;
#pragma unroll
      for (int i = 0; i < 6; ++i) mo[i] = row[i];
      int32_t* st = p.stats + o * 4;
      st[0] = Mr, st[1] = have ? (int)s[CTK_MS_N] : 0, st[2] = have ? ctk_motion_key_k(best, p.K) : -1, st[3] = 0;
      int32_t* bo = p.box + o * 4;
      bo[0] = bx[0], bo[1] = bx[1], bo[2] = bx[2], bo[3] = bx[3];
    }
    if (!by_labels) {
      if (!have) break;  // (uniform: `best` is the workgroup's)
      Mr = left;
    }
  }

  // 3. split mode: the rounds behind one that fitted nothing, and the correspondences no round took
  if (!by_labels) {
    for (int q = r + 1 + tid; q < p.L; q += OBJ_CHUNK) {
      const long o = ((g * F + pic) * p.L + q);
      float row[6];
      ctk_motion_identity(row);
      float* mo = p.motion + o * 6;
#pragma unroll
      for (int i = 0; i < 6; ++i) mo[i] = row[i];
      int32_t* st = p.stats + o * 4;
      st[0] = Mr, st[1] = 0, st[2] = -1, st[3] = 0;
      int32_t* bo = p.box + o * 4;
      bo[0] = 0, bo[1] = 0, bo[2] = -1, bo[3] = -1;
    }
    for (int m = tid; m < Mr; m += OBJ_CHUNK) lab_out[slot[m]] = (int8_t)CTK_OBJECT_NONE;
  }
}

// everything but the pointers (whether an anchor is given is looked at, as in ctk_track_field)
int objects_check_shape(const ctk_fit_objects_args* a) {
  if (!fit_check_source(fit_source_of(a), a->F) || a->reserved != 0) return CTK_E_SHAPE;
  if (a->L < 1 || a->L > CTK_OBJECTS_MAX || a->min_points < 1 || a->min_points > CTK_MOTION_POINTS_MAX) return CTK_E_SHAPE;
  if (a->model != CTK_MOTION_TRANSLATION && a->model != CTK_MOTION_SIMILARITY) return CTK_E_SHAPE;
  if (a->K < 1 || a->K > CTK_MOTION_HYPOTHESES_MAX) return CTK_E_SHAPE;
  if (ctk_motion_tol(a->tol) == 0 || ctk_motion_base2(a->min_base) < 0) return CTK_E_SHAPE;
  return CTK_OK;
}

}  // namespace

extern "C" int ctk_fit_objects_workspace_bytes(const ctk_fit_objects_args* a, size_t* out_bytes) {
  if (!a || !out_bytes) return CTK_E_NULL;
  const int rc = objects_check_shape(a);
  if (rc != CTK_OK) return rc;
  *out_bytes = 0;  // the one-launch form keeps everything in LDS
  return CTK_OK;
}

extern "C" int ctk_fit_objects(const ctk_fit_objects_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  if (!a) return CTK_E_NULL;
  ObjectsParams p;
  p.src = fit_source_of(a);
  if (fit_null_source(p.src) || !a->motion || !a->label || !a->stats || !a->box) return CTK_E_NULL;
  const int rc = objects_check_shape(a);
  if (rc != CTK_OK) return rc;
  size_t need = 0;
  ctk_fit_objects_workspace_bytes(a, &need);
  if (workspace_bytes < need || (need > 0 && !workspace)) return CTK_E_SHAPE;
  if (!fit_align_source(p.src)) return CTK_E_ALIGN;
  if (((reinterpret_cast<uintptr_t>(a->motion) | reinterpret_cast<uintptr_t>(a->stats) | reinterpret_cast<uintptr_t>(a->box)) & 3u) != 0) return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);

  p.L = a->L, p.min_points = a->min_points, p.K = a->K;
  p.T = ctk_motion_tol(a->tol), p.base2 = ctk_motion_base2(a->min_base), p.seed = a->seed;
  p.labels = a->labels;
  p.motion = a->motion, p.label = a->label, p.stats = a->stats, p.box = a->box;
  {
    CtkProfScope prof("fit_objects", 0.0, (double)a->G * a->F * (a->N_out * (a->labels ? 67.0 : 33.0) + a->L * 56.0), s);
    fit_launch(a->model == CTK_MOTION_SIMILARITY ? fit_objects_kernel<CTK_MOTION_SIMILARITY> : fit_objects_kernel<CTK_MOTION_TRANSLATION>,
               a->F, a->G, (size_t)a->N_out * OBJ_ENTRY_BYTES, CTK_MOTION_POINTS_MAX * OBJ_ENTRY_BYTES, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
