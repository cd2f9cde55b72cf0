// Device-resident stream state of G query groups over one live video (include/ctk.h, "stream state step").
//
// Three byte-moving kernels, each launched ONCE per streaming call for all G*N points.  They replace the per-stream torch glue of
// the host model (carry-over + masks, support sampling + masked accumulation, write-back + finiteness reductions) and keep its
// arithmetic operation for operation -- the acceptance test is bit equality with streams that still run that glue -- so every
// float step is an explicit IEEE intrinsic and this translation unit is compiled with -ffp-contract=off (Makefile: NOFMA).
//   begin    cotracker3_online.py:457-484   window state + point mask from the queries and the history
//   support  cotracker3_online.py:411-440   trilinear support patches of the points whose query frame entered this window, added
//                                           into the persistent accumulators
//   commit   cotracker3_online.py:498-510   finished window -> history rows, optional non-finite flag
// A fourth kernel, assign, runs BETWEEN two calls and does no float arithmetic at all: it hands slots of the resident query table
// to new queries (or empties them) and clears what their previous occupants left.
// Its resident form (ctk_stream_assign_resident) admits query frames of the window just tracked, whose features the resident pyramid
// still holds: it samples the slot's support patch then and there and lays the carry-over rows the next begin reads.
// Ring forms (ctk_stream_*_ring): the history holds R = T_cap rows and frame f lives in row f % R.  begin and commit are the same
// kernel bodies under RING = true, with t and g on grid axes so that the row of a frame is wave-uniform arithmetic; the RING = false
// instantiations are the linear kernels, instruction for instruction.  support touches no history and assign clears every row of
// a slot, so their ring forms are the linear kernels behind the ring's capacity rule.
// A fifth kernel, emit, runs AFTER a call: history frames [f0, f1) of the first N_out points of every group -> contiguous,
// frame-ordered outputs (tracks scaled to the caller's pixels, the logits, thresholded visibility), in one launch.
// A sixth, health, judges the slots over the newest frames of the history with emit's visibility expression: frames lost per slot,
// the slot's cell of a coverage grid, points per cell (integer counts in LDS, stored with plain stores).
// No LDS and no atomics except the one flag OR and health's LDS counts; no device-side globals.
#include "ctk_common.h"

namespace {

// torch divides a tensor by a host scalar as a multiplication with the scalar's float reciprocal (queries / stride, / 2^l, history /
// stride): the kernels take 1 / stride, rounded once on the host, and multiply.
// float -> integer frame index as torch's .long() does it (truncation toward zero); NaN / out-of-range frames match no window:
// a frame that is NaN or outside [-2^31, 2^31) becomes QFRAME_NONE, which lies beyond every ind + S (<= 2^31) and leaves room
// for the long arithmetic of its readers.  (The bare conversion is no such rule: it takes NaN to frame 0.)
constexpr long QFRAME_NONE = 1L << 62;
__device__ __forceinline__ long qframe_of(float f) {
  if (!(f >= -2147483648.0f && f < 2147483648.0f)) return QFRAME_NONE;
  return (long)f;
}

// ---- begin: one thread per (g, t, n) of the window state ------------------------------------------------------------------
// the history row of frame f in a ring of R rows; every use below has wave-uniform operands (block indices, kernel arguments)
__device__ __forceinline__ long ring_row(int f, long R) { return (long)((unsigned)f % (unsigned)R); }

template <bool RING>
__global__ __launch_bounds__(256) void stream_begin_kernel(int G, int N, int S, int step, int ind, long T_cap, float inv_stride,
                                                           const float* __restrict__ queries, const float* __restrict__ hc,
                                                           const float* __restrict__ hv, const float* __restrict__ hf,
                                                           float* __restrict__ coords, float* __restrict__ vis,
                                                           float* __restrict__ conf, uint8_t* __restrict__ mask) {
  // RING: grid (n blocks, S, G), so t and g -- and with them the history row -- are wave-uniform; a thread past N has nothing to do
  if (RING && (int)(blockIdx.x * blockDim.x + threadIdx.x) >= N) return;
  const long i = RING ? ((long)blockIdx.z * S + blockIdx.y) * N + (blockIdx.x * blockDim.x + threadIdx.x)
                      : (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)G * S * N;
  if (i >= total) return;
  const int n = RING ? (int)(blockIdx.x * blockDim.x + threadIdx.x) : (int)(i % N);
  const int t = RING ? (int)blockIdx.y : (int)((i / N) % S);
  const long g = RING ? (long)blockIdx.z : i / ((long)N * S);
  const float* q = queries + (g * N + n) * 3;
  const long qf = qframe_of(q[0]);
  const int overlap = S - step;
  float2 c;
  float v = 0.0f, f = 0.0f;
  if (ind > 0 && qf < (long)ind + overlap) {
    // carry-over: rows ind .. ind+overlap-1 of the history, the last of them repeated `step` times
    const long row = RING ? (g * T_cap + ring_row(ind + min(t, overlap - 1), T_cap)) * N + n
                          : (g * T_cap + ind + min(t, overlap - 1)) * N + n;
    const float2 h = *reinterpret_cast<const float2*>(hc + row * 2);
    c.x = __fmul_rn(h.x, inv_stride);
    c.y = __fmul_rn(h.y, inv_stride);
    v = hv[row];
    f = hf[row];
  } else {
    c.x = __fmul_rn(q[1], inv_stride);
    c.y = __fmul_rn(q[2], inv_stride);
  }
  *reinterpret_cast<float2*>(coords + i * 2) = c;
  vis[i] = v;
  conf[i] = f;
  if (t == 0) mask[g * N + n] = qf < (long)ind + S ? 1 : 0;
}

// ---- support: one wave per (level, point, tap) row of 128 channels, float2 per lane ----------------------------------------
struct StreamLevels {
  const float* fm[CTK_LEVELS];
  float* acc[CTK_LEVELS];
  int H[CTK_LEVELS], W[CTK_LEVELS];
  float sx[CTK_LEVELS], sy[CTK_LEVELS];
};

// One (level, point, tap) row: the trilinear patch of (z, x, y) -- z a frame of the pyramid lv.fm[l], (x, y) the query position in
// pixels -- for channels 2 * lane, 2 * lane + 1.  The one copy of this arithmetic: support adds it into the accumulator, the resident
// assign stores it.
__device__ __forceinline__ float2 support_row(const StreamLevels& lv, int l, int pp, int lane, long z, float qx, float qy, int S,
                                              float sz, float inv_stride) {
  const int hx = pp / 7, wy = pp - hx * 7;
  const int H = lv.H[l], W = lv.W[l];
  // (queries / stride) / 2^l, then the tap arithmetic of sample_support_kernel (corr.hip)
  const float linv = 1.0f / (float)(1 << l);
  const float cx = __fmul_rn(__fmul_rn(qx, inv_stride), linv), cy = __fmul_rn(__fmul_rn(qy, inv_stride), linv);
  const CtkTap tx = ctk_tap(__fadd_rn(cx, (float)(hx - 3)), W, lv.sx[l]);
  const CtkTap ty = ctk_tap(__fadd_rn(cy, (float)(wy - 3)), H, lv.sy[l]);
  const CtkTap tz = ctk_tap(__fadd_rn((float)z, 0.0f), S, sz);
  const float* fm = lv.fm[l];
  float2 o = make_float2(0.f, 0.f);
  const int zi[2] = {tz.i0, tz.i1};
  const float zw[2] = {tz.w0, tz.w1};
  const int yi[2] = {ty.i0, ty.i1};
  const float yw[2] = {ty.w0, ty.w1};
  const int xi[2] = {tx.i0, tx.i1};
  const float xw[2] = {tx.w0, tx.w1};
#pragma unroll
  for (int dz = 0; dz < 2; ++dz)
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const float w = __fmul_rn(__fmul_rn(xw[dx], yw[dy]), zw[dz]);
        const float2 v = *reinterpret_cast<const float2*>(fm + (((long)zi[dz] * H + yi[dy]) * W + xi[dx]) * CTK_C + lane * 2);
        o.x = __fadd_rn(o.x, __fmul_rn(v.x, w));
        o.y = __fadd_rn(o.y, __fmul_rn(v.y, w));
      }
  return o;
}

__global__ __launch_bounds__(256) void stream_support_kernel(StreamLevels lv, long P /* G*N */, int S, float sz, int left, int right,
                                                             int ind, float inv_stride, const float* __restrict__ queries) {
  const long wid = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wid >= P * CTK_TAPS) return;
  const long n = wid / CTK_TAPS;
  const float* q = queries + n * 3;
  const long qf = qframe_of(q[0]);
  if (qf < left || qf >= right) return;  // not this window's point: its accumulator row is neither read nor written
  const int l = blockIdx.y;
  const float2 o = support_row(lv, l, (int)(wid - n * CTK_TAPS), lane, qf - ind, q[1], q[2], S, sz, inv_stride);
  float2* dst = reinterpret_cast<float2*>(lv.acc[l] + wid * CTK_C + lane * 2);
  float2 a = *dst;  // acc + s: the accumulation of the host glue (zeros + s * 1 on the one call that samples this point)
  a.x = __fadd_rn(a.x, o.x);
  a.y = __fadd_rn(a.y, o.y);
  *dst = a;
}

// ---- commit: one thread per (g, t < T_valid, n) ------------------------------------------------------------------------------
template <bool RING>
__global__ __launch_bounds__(256) void stream_commit_kernel(int G, int N, int S, int T_valid, int ind, long T_cap, float stride,
                                                            const float* __restrict__ coords, const float* __restrict__ vis,
                                                            const float* __restrict__ conf, float* __restrict__ hc,
                                                            float* __restrict__ hv, float* __restrict__ hf,
                                                            int32_t* __restrict__ flag) {
  long i = 0, total = 1;
  if constexpr (RING) {  // grid (n blocks, T_valid, G): a thread past N has nothing to do
    if ((int)(blockIdx.x * blockDim.x + threadIdx.x) >= N) i = 1;
  } else {
    i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    total = (long)G * T_valid * N;
  }
  bool bad = false;
  if (i < total) {
    const int n = RING ? (int)(blockIdx.x * blockDim.x + threadIdx.x) : (int)(i % N);
    const int t = RING ? (int)blockIdx.y : (int)((i / N) % T_valid);
    const long g = RING ? (long)blockIdx.z : i / ((long)N * T_valid);
    const long src = (g * S + t) * N + n;
    const long row = RING ? (g * T_cap + ring_row(ind + t, T_cap)) * N + n : (g * T_cap + ind + t) * N + n;
    const float2 c = *reinterpret_cast<const float2*>(coords + src * 2);
    float2 o;
    o.x = __fmul_rn(c.x, stride);
    o.y = __fmul_rn(c.y, stride);
    const float v = vis[src], f = conf[src];
    *reinterpret_cast<float2*>(hc + row * 2) = o;
    hv[row] = v;
    hf[row] = f;
    bad = !(isfinite(o.x) && isfinite(o.y) && isfinite(v) && isfinite(f));
  }
  if (flag != nullptr && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// ---- assign: blockIdx.x = listed slot m; the y blocks stride over the slot's accumulator floats, then over its history rows ----
struct AssignLevels {
  float* acc[CTK_LEVELS];
};
constexpr int ASSIGN_ACC4 = CTK_TAPS * CTK_C / 4;  // float4 stores per slot and level: the slot's 49 x 128 floats are one run

__global__ __launch_bounds__(256) void stream_assign_kernel(AssignLevels lv, int G, int N, long T_cap, int rows,
                                                            const int32_t* __restrict__ slots, const float* __restrict__ newq,
                                                            float* __restrict__ queries, float* __restrict__ hc,
                                                            float* __restrict__ hv, float* __restrict__ hf) {
  const long m = blockIdx.x;
  const long slot = slots[m];
  if (slot < 0 || slot >= (long)G * N) return;  // defence only: the host checks the list before it is copied over
  const long tid = (long)blockIdx.y * blockDim.x + threadIdx.x;
  const long nthreads = (long)gridDim.y * blockDim.x;
  if (tid < 3) queries[slot * 3 + tid] = newq[m * 3 + tid];
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long i = tid; i < (long)CTK_LEVELS * ASSIGN_ACC4; i += nthreads) {
    const int l = (int)(i / ASSIGN_ACC4);
    const long j = i - (long)l * ASSIGN_ACC4;
    reinterpret_cast<float4*>(lv.acc[l] + slot * (CTK_TAPS * CTK_C))[j] = z4;  // (a slot's run starts on a 25088-byte multiple)
  }
  const long g = slot / N, n = slot - g * N;
  for (long t = tid; t < rows; t += nthreads) {
    const long row = (g * T_cap + t) * N + n;
    *reinterpret_cast<float2*>(hc + row * 2) = make_float2(0.f, 0.f);
    hv[row] = 0.0f;
    hf[row] = 0.0f;
  }
}

// ---- resident assign: the assign for query frames the resident pyramid still holds ------------------------------------------
// grid (M, 2 * CTK_LEVELS): blockIdx.x = listed slot m, blockIdx.y >> 1 = the level whose accumulator rows this block writes (two
// blocks of four waves per level); all the y blocks together stride over the slot's history rows.  `ind` is the first frame of the
// NEXT call's window: the pyramid holds frames [ind - step, ind - step + S), row z = frame - (ind - step).
//   resident  ind - step <= qframe < ind + overlap: the accumulator rows get the trilinear patch (one wave per tap row, as support:
//             0 + s, what "cleared accumulator plus sample" leaves), and the history rows of frames [ind, ind + overlap) -- the rows the
//             next begin carries over -- get (x, y) and zero logits, so that begin starts the point from its query as it starts a
//             fresh one: fmul(x, 1 / stride) at every t
//   else      the plain assign: accumulators and history rows zero
// Every accumulator float and every history row has one writer, which stores its final value.
template <bool RING>
__global__ __launch_bounds__(256) void stream_assign_resident_kernel(StreamLevels lv, int G, int N, int S, int step, int ind, float sz,
                                                                     float inv_stride, long T_cap, int rows,
                                                                     const int32_t* __restrict__ slots, const float* __restrict__ newq,
                                                                     float* __restrict__ queries, float* __restrict__ hc,
                                                                     float* __restrict__ hv, float* __restrict__ hf) {
  const long m = blockIdx.x;
  const long slot = slots[m];
  if (slot < 0 || slot >= (long)G * N) return;  // defence only: the host checks the list before it is copied over
  const long tid = (long)blockIdx.y * blockDim.x + threadIdx.x;
  const long nthreads = (long)gridDim.y * blockDim.x;
  const float q0 = newq[m * 3], qx = newq[m * 3 + 1], qy = newq[m * 3 + 2];
  if (tid < 3) queries[slot * 3 + tid] = newq[m * 3 + tid];
  const long qf = qframe_of(q0);
  const int overlap = S - step;
  const bool resident = qf >= (long)ind - step && qf < (long)ind + overlap;
  const int l = blockIdx.y >> 1;
  float* acc = lv.acc[l] + slot * (CTK_TAPS * CTK_C);  // (a slot's run starts on a 25088-byte multiple)
  if (resident) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(((blockIdx.y & 1) * blockDim.x + threadIdx.x) >> 6));
    const int lane = threadIdx.x & 63;
    for (int pp = wave; pp < CTK_TAPS; pp += 8) {
      const float2 o = support_row(lv, l, pp, lane, qf - ((long)ind - step), qx, qy, S, sz, inv_stride);
      float2 a;
      a.x = __fadd_rn(0.0f, o.x);
      a.y = __fadd_rn(0.0f, o.y);
      *reinterpret_cast<float2*>(acc + pp * CTK_C + lane * 2) = a;
    }
  } else {
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = (int)((blockIdx.y & 1) * blockDim.x + threadIdx.x); j < ASSIGN_ACC4; j += 2 * (int)blockDim.x)
      reinterpret_cast<float4*>(acc)[j] = z4;
  }
  const long g = slot / N, n = slot - g * N;
  // linear: rows [0, rows) and, resident, the carry rows [ind, ind + overlap) wherever they lie; ring: all T_cap rows
  const long nrows = RING ? T_cap : (resident ? max((long)rows, (long)ind + overlap) : (long)rows);
  const long first = RING ? (long)ring_row(ind, T_cap) : (long)ind;  // the row of frame ind
  for (long t = tid; t < nrows; t += nthreads) {
    if (!RING && t >= rows && t < ind) continue;  // between the cleared rows and the carry rows: not this call's
    const long d = RING ? (t >= first ? t - first : t - first + T_cap) : t - first;  // frame of row t, minus ind
    const bool carry = resident && d >= 0 && d < overlap;
    const long row = (g * T_cap + t) * N + n;
    *reinterpret_cast<float2*>(hc + row * 2) = carry ? make_float2(qx, qy) : make_float2(0.f, 0.f);
    hv[row] = 0.0f;
    hf[row] = 0.0f;
  }
}

// ---- emit: one thread per (g, frame, n < N_out); grid (n blocks, f1 - f0, G): the frame's row is wave-uniform arithmetic ---------
// sigmoid as 1 / (1 + expf(-x)), every step a float32 operation
__device__ __forceinline__ float emit_sigmoid(float x) { return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-x))); }

// the predictor's visibility rule; a NaN compares false: not visible.  Emit thresholds with it, health judges with it; draw_math.h
// (ctk_draw_visible) restates it operation for operation for the draw kernels and their host build
__device__ __forceinline__ bool emit_visible(float v, float c, float thresh) {
  return __fmul_rn(emit_sigmoid(v), emit_sigmoid(c)) > thresh;
}

__global__ __launch_bounds__(256) void stream_emit_kernel(int N, int N_out, long R, int f0, int F, float sx, float sy, float thresh,
                                                          const float* __restrict__ hc, const float* __restrict__ hv,
                                                          const float* __restrict__ hf, const int32_t* __restrict__ first_row,
                                                          float* __restrict__ tracks, float* __restrict__ vis_logit,
                                                          float* __restrict__ conf_logit, uint8_t* __restrict__ visible) {
  const int n = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (n >= N_out) return;
  const int t = (int)blockIdx.y;
  const long g = (long)blockIdx.z;
  const int f = f0 + t;
  const long row = (g * R + ring_row(f, R)) * N + n;
  const long dst = (g * F + t) * N_out + n;
  const float2 h = *reinterpret_cast<const float2*>(hc + row * 2);
  float2 o;
  o.x = __fmul_rn(h.x, sx);
  o.y = __fmul_rn(h.y, sy);
  *reinterpret_cast<float2*>(tracks + dst * 2) = o;
  if (vis_logit == nullptr && conf_logit == nullptr && visible == nullptr) return;
  const float v = hv[row], c = hf[row];
  if (vis_logit != nullptr) vis_logit[dst] = v;
  if (conf_logit != nullptr) conf_logit[dst] = c;
  if (visible != nullptr) {
    bool on = emit_visible(v, c, thresh);
    if (first_row != nullptr) on = on && f >= first_row[g * N + n];
    visible[dst] = on ? 1 : 0;
  }
}

// ---- health: grid (n blocks, G); one thread per slot n < N_out walks the history backwards from frame f1 - 1 -------------------
constexpr int HEALTH_CELLS_MAX = 4096;

struct HealthParams {
  int N, N_out;
  long R;
  int f1, look, ind_next;
  float thresh, x_lo, x_hi, y_lo, y_hi;
  int gh, gw;
  float inv_cw, inv_ch;
  const float* queries;
  const float* hc;
  const float* hv;
  const float* hf;
  const int32_t* first_row;
};

// inclusive bounds; a NaN coordinate is outside
__device__ __forceinline__ bool health_inside(const HealthParams& p, float x, float y) {
  return x >= p.x_lo && x <= p.x_hi && y >= p.y_lo && y <= p.y_hi;
}

// the cell of a position inside the bounds (x_hi and y_hi are clamped into the last column and row)
__device__ __forceinline__ int health_cell(const HealthParams& p, float x, float y) {
  const int cx = min(max((int)floorf(__fmul_rn(__fsub_rn(x, p.x_lo), p.inv_cw)), 0), p.gw - 1);
  const int cy = min(max((int)floorf(__fmul_rn(__fsub_rn(y, p.y_lo), p.inv_ch)), 0), p.gh - 1);
  return cy * p.gw + cx;
}

// Slot (g, n) judged over the last `look` frames -> its cell, and through `lost` the frames lost.  The cell depends on frame f1 - 1
// (or the query) only: look = 1 yields the same cell as any longer look.
__device__ __forceinline__ int health_judge(const HealthParams& p, long g, int n, int look, int& lost) {
  const long s = g * p.N + n;
  const int fr = p.first_row[s];
  const float* q = p.queries + s * 3;
  const float q0 = q[0];
  lost = -1;
  if (fr == INT32_MAX || q0 == CTK_STREAM_EMPTY_FRAME) return -1;  // an empty slot
  lost = 0;
  const long start = max((long)fr, qframe_of(q0));
  if (fr >= p.ind_next || start >= (long)p.f1) {  // pending: no row of the history is this occupant's track yet
    const float x = q[1], y = q[2];
    return health_inside(p, x, y) ? health_cell(p, x, y) : -1;
  }
  const int stop = (int)max((long)(p.f1 - look), start);  // (0 <= f1 - look: checked on the host)
  for (int f = p.f1 - 1; f >= stop; --f) {
    const long row = (g * p.R + ring_row(f, p.R)) * p.N + n;
    const float2 h = *reinterpret_cast<const float2*>(p.hc + row * 2);
    if (emit_visible(p.hv[row], p.hf[row], p.thresh) && health_inside(p, h.x, h.y))
      return f == p.f1 - 1 ? health_cell(p, h.x, h.y) : -1;
    ++lost;
  }
  return -1;
}

// Block b of group g judges slots [256 b, 256 b + 256) and owns the cells [c0, c1) of the group's cover: it counts them in LDS over
// ALL slots of the group -- its own from the judgement it has just made, the others judged again at look = 1 (one history row each) --
// and stores the counts with plain stores.  Integer counting: the order of the LDS adds does not show in the result.
__global__ __launch_bounds__(256) void stream_health_kernel(HealthParams p, int32_t* __restrict__ lost, int32_t* __restrict__ cell,
                                                            int32_t* __restrict__ cover) {
  __shared__ int counts[HEALTH_CELLS_MAX];
  const long g = (long)blockIdx.y;
  const int tid = (int)threadIdx.x;
  const int cells = p.gh * p.gw;
  const int per = (cells + (int)gridDim.x - 1) / (int)gridDim.x;
  const int c0 = min((int)blockIdx.x * per, cells), c1 = min(c0 + per, cells);
  for (int c = c0 + tid; c < c1; c += 256) counts[c - c0] = 0;
  __syncthreads();
  const int n0 = (int)blockIdx.x * 256;
  const int n = n0 + tid;
  if (n < p.N_out) {
    int l;
    const int c = health_judge(p, g, n, p.look, l);
    lost[g * p.N_out + n] = l;
    cell[g * p.N_out + n] = c;
    if (c >= c0 && c < c1) atomicAdd(&counts[c - c0], 1);
  }
  if (c0 < c1) {
    for (int m = tid; m < p.N_out; m += 256) {
      if (m >= n0 && m < n0 + 256) continue;  // (wave-uniform: m - tid is a multiple of 256)
      int l;
      const int c = health_judge(p, g, m, 1, l);
      if (c >= c0 && c < c1) atomicAdd(&counts[c - c0], 1);
    }
  }
  __syncthreads();
  for (int c = c0 + tid; c < c1; c += 256) cover[g * cells + c] = counts[c - c0];
}

constexpr int GRID_YZ_MAX = 65535;  // grid axes y and z

int check_common(const ctk_stream_args* a, bool ring) {
  if (!a) return CTK_E_NULL;
  if (a->G <= 0 || a->N <= 0 || a->S <= 0 || a->step <= 0 || a->step >= a->S || a->ind < 0 || a->ind % a->step != 0)
    return CTK_E_SHAPE;
  if (ring ? a->T_cap < a->S : (long)a->T_cap < (long)a->ind + a->S) return CTK_E_SHAPE;
  if (!(a->stride > 0.0f) || !(a->stride <= 65536.0f)) return CTK_E_SHAPE;
  if ((long)a->G * a->N > (1L << 26) || (long)a->G * a->N * a->S > (1L << 30)) return CTK_E_SHAPE;
  // ring forms: g and t ride on grid axes, and ind + S must not overflow the 32-bit frame arithmetic
  if (ring && (a->G > GRID_YZ_MAX || a->S > GRID_YZ_MAX || (long)a->ind + a->S > (1L << 30))) return CTK_E_SHAPE;
  return CTK_OK;
}

int stream_begin(const ctk_stream_args* a, void* stream, bool ring) {
  const int rc = check_common(a, ring);
  if (rc != CTK_OK) return rc;
  if (!a->queries || !a->hist_coords || !a->hist_vis || !a->hist_conf || !a->coords || !a->vis || !a->conf || !a->point_mask)
    return CTK_E_NULL;
  if (ring) {
    hipLaunchKernelGGL(stream_begin_kernel<true>, dim3((unsigned)((a->N + 255) / 256), (unsigned)a->S, (unsigned)a->G), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a->G, a->N, a->S, a->step, a->ind, (long)a->T_cap, 1.0f / a->stride,
                       a->queries, a->hist_coords, a->hist_vis, a->hist_conf, a->coords, a->vis, a->conf, a->point_mask);
  } else {
    const long total = (long)a->G * a->S * a->N;
    hipLaunchKernelGGL(stream_begin_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a->G, a->N, a->S, a->step, a->ind, (long)a->T_cap, 1.0f / a->stride,
                       a->queries, a->hist_coords, a->hist_vis, a->hist_conf, a->coords, a->vis, a->conf, a->point_mask);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}

int stream_support(const ctk_stream_args* a, void* stream, bool ring) {
  const int rc = check_common(a, ring);
  if (rc != CTK_OK) return rc;
  if (!a->queries) return CTK_E_NULL;
  StreamLevels lv;
  for (int l = 0; l < CTK_LEVELS; ++l) {
    if (!a->fmaps[l] || !a->support[l]) return CTK_E_NULL;
    if (a->H[l] <= 0 || a->W[l] <= 0) return CTK_E_SHAPE;
    lv.fm[l] = a->fmaps[l];
    lv.acc[l] = a->support[l];
    lv.H[l] = a->H[l];
    lv.W[l] = a->W[l];
    lv.sx[l] = ctk_sampler_scale(a->W[l]);
    lv.sy[l] = ctk_sampler_scale(a->H[l]);
  }
  const long P = (long)a->G * a->N;
  const long waves = P * CTK_TAPS;
  const int left = a->ind == 0 ? 0 : a->ind + a->step;  // cotracker3_online.py:411-414
  const int right = a->ind + a->S;
  hipLaunchKernelGGL(stream_support_kernel, dim3((unsigned)((waves + 3) / 4), CTK_LEVELS), dim3(256), 0,
                     static_cast<hipStream_t>(stream), lv, P, a->S, ctk_sampler_scale(a->S), left, right, a->ind, 1.0f / a->stride,
                     a->queries);
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}

int stream_commit(const ctk_stream_args* a, void* stream, bool ring) {
  const int rc = check_common(a, ring);
  if (rc != CTK_OK) return rc;
  if (a->T_valid <= 0 || a->T_valid > a->S) return CTK_E_SHAPE;
  if (!a->hist_coords || !a->hist_vis || !a->hist_conf || !a->coords || !a->vis || !a->conf) return CTK_E_NULL;
  if (ring) {
    hipLaunchKernelGGL(stream_commit_kernel<true>, dim3((unsigned)((a->N + 255) / 256), (unsigned)a->T_valid, (unsigned)a->G),
                       dim3(256), 0, static_cast<hipStream_t>(stream), a->G, a->N, a->S, a->T_valid, a->ind, (long)a->T_cap,
                       a->stride, a->coords, a->vis, a->conf, a->hist_coords, a->hist_vis, a->hist_conf, a->nonfinite);
  } else {
    const long total = (long)a->G * a->T_valid * a->N;
    hipLaunchKernelGGL(stream_commit_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a->G, a->N, a->S, a->T_valid, a->ind, (long)a->T_cap, a->stride, a->coords,
                       a->vis, a->conf, a->hist_coords, a->hist_vis, a->hist_conf, a->nonfinite);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}

int stream_assign(const ctk_stream_args* a, const int32_t* slots, const float* new_queries, int32_t M, int32_t rows, void* stream,
                  bool ring) {
  const int rc = check_common(a, ring);
  if (rc != CTK_OK) return rc;
  if (!slots || !new_queries || !a->queries || !a->hist_coords || !a->hist_vis || !a->hist_conf) return CTK_E_NULL;
  AssignLevels lv;
  for (int l = 0; l < CTK_LEVELS; ++l) {
    if (!a->support[l]) return CTK_E_NULL;
    if (!ctk_aligned16(a->support[l])) return CTK_E_SHAPE;  // cleared with 16-byte stores
    lv.acc[l] = a->support[l];
  }
  if (M <= 0 || (long)M > (long)a->G * a->N || rows < 0 || rows > a->T_cap) return CTK_E_SHAPE;
  // 4 x 1568 float4 stores per slot: 8 blocks of 256 threads take them in about three rounds each, a long history in a few more
  hipLaunchKernelGGL(stream_assign_kernel, dim3((unsigned)M, 8), dim3(256), 0, static_cast<hipStream_t>(stream), lv, a->G, a->N,
                     (long)a->T_cap, rows, slots, new_queries, const_cast<float*>(a->queries), a->hist_coords, a->hist_vis,
                     a->hist_conf);
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}

int stream_assign_resident(const ctk_stream_args* a, const int32_t* slots, const float* new_queries, int32_t M, int32_t rows,
                           void* stream, bool ring) {
  const int rc = check_common(a, ring);  // a->ind: the first frame of the NEXT call's window (linear: T_cap >= ind + S holds its rows)
  if (rc != CTK_OK) return rc;
  if (!slots || !new_queries || !a->queries || !a->hist_coords || !a->hist_vis || !a->hist_conf) return CTK_E_NULL;
  StreamLevels lv;
  for (int l = 0; l < CTK_LEVELS; ++l) {
    if (!a->support[l] || !a->fmaps[l]) return CTK_E_NULL;
    if (!ctk_aligned16(a->support[l])) return CTK_E_SHAPE;  // cleared with 16-byte stores
    if (a->H[l] <= 0 || a->W[l] <= 0) return CTK_E_SHAPE;
    lv.fm[l] = a->fmaps[l];
    lv.acc[l] = a->support[l];
    lv.H[l] = a->H[l];
    lv.W[l] = a->W[l];
    lv.sx[l] = ctk_sampler_scale(a->W[l]);
    lv.sy[l] = ctk_sampler_scale(a->H[l]);
  }
  if (a->ind < a->step) return CTK_E_SHAPE;  // no window has been tracked yet: the pyramid holds nothing to sample
  if (M <= 0 || (long)M > (long)a->G * a->N || rows < 0 || rows > a->T_cap) return CTK_E_SHAPE;
  const dim3 grid((unsigned)M, 2 * CTK_LEVELS);
  if (ring) {
    hipLaunchKernelGGL(stream_assign_resident_kernel<true>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), lv, a->G, a->N, a->S,
                       a->step, a->ind, ctk_sampler_scale(a->S), 1.0f / a->stride, (long)a->T_cap, rows, slots, new_queries,
                       const_cast<float*>(a->queries), a->hist_coords, a->hist_vis, a->hist_conf);
  } else {
    hipLaunchKernelGGL(stream_assign_resident_kernel<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), lv, a->G, a->N, a->S,
                       a->step, a->ind, ctk_sampler_scale(a->S), 1.0f / a->stride, (long)a->T_cap, rows, slots, new_queries,
                       const_cast<float*>(a->queries), a->hist_coords, a->hist_vis, a->hist_conf);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}

}  // namespace

extern "C" int ctk_stream_begin(const ctk_stream_args* a, void* stream) { return stream_begin(a, stream, false); }
extern "C" int ctk_stream_support(const ctk_stream_args* a, void* stream) { return stream_support(a, stream, false); }
extern "C" int ctk_stream_commit(const ctk_stream_args* a, void* stream) { return stream_commit(a, stream, false); }
extern "C" int ctk_stream_assign(const ctk_stream_args* a, const int32_t* slots, const float* new_queries, int32_t M, int32_t rows,
                                 void* stream) {
  return stream_assign(a, slots, new_queries, M, rows, stream, false);
}

// ring forms: T_cap is the ring size R, the history row of frame f is f % R, and the capacity rule is R >= S
extern "C" int ctk_stream_begin_ring(const ctk_stream_args* a, void* stream) { return stream_begin(a, stream, true); }
extern "C" int ctk_stream_support_ring(const ctk_stream_args* a, void* stream) { return stream_support(a, stream, true); }
extern "C" int ctk_stream_commit_ring(const ctk_stream_args* a, void* stream) { return stream_commit(a, stream, true); }
extern "C" int ctk_stream_assign_ring(const ctk_stream_args* a, const int32_t* slots, const float* new_queries, int32_t M,
                                      void* stream) {
  if (!a) return CTK_E_NULL;
  return stream_assign(a, slots, new_queries, M, a->T_cap, stream, true);  // every row of the ring: whatever frame it holds
}

// resident forms of the assign: a->ind is the first frame of the NEXT call's window, a->fmaps / H / W the resident pyramid
extern "C" int ctk_stream_assign_resident(const ctk_stream_args* a, const int32_t* slots, const float* new_queries, int32_t M,
                                          int32_t rows, void* stream) {
  return stream_assign_resident(a, slots, new_queries, M, rows, stream, false);
}
extern "C" int ctk_stream_assign_resident_ring(const ctk_stream_args* a, const int32_t* slots, const float* new_queries, int32_t M,
                                               void* stream) {
  if (!a) return CTK_E_NULL;
  return stream_assign_resident(a, slots, new_queries, M, a->T_cap, stream, true);
}

extern "C" int ctk_stream_emit(const ctk_stream_emit_args* a, void* stream) {
  if (!a) return CTK_E_NULL;
  if (a->G <= 0 || a->N <= 0 || a->N_out <= 0 || a->N_out > a->N || a->R <= 0 || a->reserved != 0) return CTK_E_SHAPE;
  if (a->f0 < 0 || a->f1 <= a->f0 || (long)a->f1 - a->f0 > a->R || a->f1 > (1 << 30)) return CTK_E_SHAPE;
  if (a->G > GRID_YZ_MAX || a->f1 - a->f0 > GRID_YZ_MAX || (long)a->G * a->N > (1L << 26)) return CTK_E_SHAPE;
  if (!a->hist_coords || !a->tracks) return CTK_E_NULL;
  const bool logits = a->vis_logit || a->conf_logit || a->visible;
  if (logits && (!a->hist_vis || !a->hist_conf)) return CTK_E_NULL;
  if (a->first_row && !a->visible) return CTK_E_NULL;  // the mask has nothing to act on
  if (a->visible && !(a->thresh == a->thresh)) return CTK_E_SHAPE;
  const int F = a->f1 - a->f0;
  hipLaunchKernelGGL(stream_emit_kernel, dim3((unsigned)((a->N_out + 255) / 256), (unsigned)F, (unsigned)a->G), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a->N, a->N_out, (long)a->R, a->f0, F, a->sx, a->sy, a->thresh, a->hist_coords,
                     a->hist_vis, a->hist_conf, a->first_row, a->tracks, a->vis_logit, a->conf_logit, a->visible);
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}

extern "C" int ctk_stream_health(const ctk_stream_health_args* a, void* stream) {
  if (!a) return CTK_E_NULL;
  if (!a->queries || !a->hist_coords || !a->hist_vis || !a->hist_conf || !a->first_row || !a->lost || !a->cell || !a->cover)
    return CTK_E_NULL;
  if (a->G <= 0 || a->N <= 0 || a->N_out <= 0 || a->N_out > a->N || a->R <= 0 || a->reserved != 0) return CTK_E_SHAPE;
  if (a->gh <= 0 || a->gw <= 0 || (long)a->gh * a->gw > HEALTH_CELLS_MAX) return CTK_E_SHAPE;
  if (a->f1 <= 0 || a->f1 > (1 << 30) || a->look < 1 || a->look > a->R || a->look > a->f1 || a->ind_next < 0) return CTK_E_SHAPE;
  if (a->G > GRID_YZ_MAX || (long)a->G * a->N > (1L << 26)) return CTK_E_SHAPE;
  if (!(a->thresh == a->thresh)) return CTK_E_SHAPE;
  if (!std::isfinite(a->x_lo) || !std::isfinite(a->x_hi) || !std::isfinite(a->y_lo) || !std::isfinite(a->y_hi)) return CTK_E_SHAPE;
  if (a->x_hi <= a->x_lo || a->y_hi <= a->y_lo) return CTK_E_SHAPE;
  if (!std::isfinite(a->inv_cw) || !std::isfinite(a->inv_ch) || !(a->inv_cw > 0.0f) || !(a->inv_ch > 0.0f)) return CTK_E_SHAPE;
  HealthParams p;
  p.N = a->N, p.N_out = a->N_out, p.R = (long)a->R;
  p.f1 = a->f1, p.look = a->look, p.ind_next = a->ind_next;
  p.thresh = a->thresh, p.x_lo = a->x_lo, p.x_hi = a->x_hi, p.y_lo = a->y_lo, p.y_hi = a->y_hi;
  p.gh = a->gh, p.gw = a->gw, p.inv_cw = a->inv_cw, p.inv_ch = a->inv_ch;
  p.queries = a->queries, p.hc = a->hist_coords, p.hv = a->hist_vis, p.hf = a->hist_conf, p.first_row = a->first_row;
  hipLaunchKernelGGL(stream_health_kernel, dim3((unsigned)((a->N_out + 255) / 256), (unsigned)a->G), dim3(256), 0,
                     static_cast<hipStream_t>(stream), p, a->lost, a->cell, a->cover);
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
