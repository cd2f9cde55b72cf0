// C-ABI orchestration: one update iteration = corr_embed -> assemble_tokens -> update_former
// -> heads + state update, all enqueued on the caller's stream (no host sync, capturable).
#include "ctk_common.h"
#include "ctk_profile.h"
#include "gemm_params.h"
#include "ctk_options.h"
#include <cstdlib>
#include <mutex>
#include <new>

int ctk_launch_corr_volume(const ctk_window_args* a, int n0, int ncount, float* out, long level_stride, int ld,
                           hipStream_t s, bool groups = false);
int ctk_launch_pyramid_split(const float* fmap, long pixels, void* out, int version, hipStream_t s);
int ctk_launch_corr_volume_sh(const ctk_window_args* a, const void* const* fm_sh, int n0, int ncount, void* out,
                              long level_stride_halves, int version, hipStream_t s, bool groups = false);
int ctk_launch_virtual_init(const float* vt, int S, float* dst, int B, hipStream_t s);
int ctk_launch_layernorm2(const float* x, void* y, long R, const float* gamma, const float* beta, float eps, void* y2, float eps2,
                          int out_split, hipStream_t s);
int ctk_launch_heads(const float* tokens, const float* hw, const float* hb, int S, int N, float* delta, float* coords,
                     float* vis, float* conf, hipStream_t s);
int ctk_launch_assemble(const ctk_window_args* a, void* x, int x_split, int ld, int base, hipStream_t s);
int ctk_launch_assemble_batch(const CtkBatchState& st, int B, int S, int N, float scale_x, float scale_y, void* x, int x_split,
                              int ld, int base, hipStream_t s);
int ctk_launch_heads_batch(const float* tokens, const float* hw, const float* hb, const CtkBatchState& st, int B, int S, int N,
                           hipStream_t s);

namespace {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

#define CTK_TRY(expr)        \
  do {                       \
    int rc__ = (expr);       \
    if (rc__) return rc__;   \
  } while (0)

// ---- two-stream overlap (ctk_window_args.aux_stream) --------------------------------------------------------
// Fork / join between the caller's stream and its auxiliary stream use timing-less events from a small ring.  An event
// may be re-recorded as soon as the hipStreamWaitEvent that consumes its previous record has been ENQUEUED (the wait
// binds to the record that precedes it), so a ring far longer than one fork/join sequence needs no host synchronisation.
// The events are host objects created on first use and kept for the life of the process (the second exception, after
// the profiler, to "no mutable global state"); both calls are legal during stream capture, where they become graph edges
// and pull the auxiliary stream into the capture.
// One ring per device (an event belongs to the device that was current when it was created: recording it on another
// device's stream is an invalid-handle error), creation errors are reported to the caller.
class EventRing {
 public:
  int next(hipEvent_t* out) {
    int dev = 0;
    hipError_t rc = hipGetDevice(&dev);
    if (rc != hipSuccess) return (int)rc;
    if (dev < 0 || dev >= kMaxDev) return CTK_E_STATE;
    std::lock_guard<std::mutex> g(m_);
    PerDev& d = d_[dev];
    if (!d.ready) {
      for (int i = 0; i < kN; ++i) {
        rc = hipEventCreateWithFlags(&d.ev[i], hipEventDisableTiming);
        if (rc != hipSuccess) {
          for (int j = 0; j < i; ++j) (void)hipEventDestroy(d.ev[j]);
          return (int)rc;
        }
      }
      d.ready = true;
    }
    *out = d.ev[d.i];
    d.i = (d.i + 1) % kN;
    return CTK_OK;
  }

 private:
  static constexpr int kN = 256, kMaxDev = 64;
  struct PerDev {
    hipEvent_t ev[kN];
    int i = 0;
    bool ready = false;
  };
  std::mutex m_;
  PerDev d_[kMaxDev];
};
EventRing g_events;

// `to` waits for everything enqueued on `from` so far
int stream_follow(hipStream_t from, hipStream_t to) {
  hipEvent_t e;
  CTK_TRY(g_events.next(&e));
  hipError_t rc = hipEventRecord(e, from);
  if (rc != hipSuccess) return (int)rc;
  rc = hipStreamWaitEvent(to, e, 0);
  return rc == hipSuccess ? CTK_OK : (int)rc;
}

// CTK_OPT_OVERLAP (ctk_set_option; initial value from CTK_OVERLAP when the library is loaded): 0 = ignore aux_stream (everything on
// the caller's stream), bit 0 = software pipeline sampler || corr_mlp, bit 1 = points<-virtual query projection beside the
// virtual-track chain.  DEFAULT 0: measured on MI355X at C3 (profiles/r02_overlap_and_time_attention_ab.txt) the sampler and the
// corr_mlp GEMM do NOT complement each other -- run side by side each slows down by more than the other gains (sampler 2.70 -> 4 x
// 1.21 ms, fc1 2.24 -> 4 x 0.77 ms per iteration; step 1528.5 -> 1547.3 ms) -- and the side query projection is worth 0.15 %
// (1526.1 ms), inside run-to-run noise.  Results are bit-identical in every mode (tests), so the code stays as an opt-in for
// other shapes.  Two more placements were measured in round 4 and removed in round 6 (both +-0: the time blocks' q projection
// beside their kv projection, profiles/r04_overlap_qkv_ab.txt; the side projection on a limited number of CUs beside the small
// launches of the virtual-track chain, profiles/r04_overlap8_trace.txt).
int overlap_mode() { return ctk_opt(CTK_OPT_OVERLAP); }

// Joins `aux` back into `main` when a fork is still open at scope exit (an error return between fork and join would
// otherwise leave the auxiliary stream unjoined -- inside ctk_window_graph_create: stuck in a broken capture).
struct JoinGuard {
  hipStream_t main, aux;
  bool open = false;
  int fork() {
    const int rc = stream_follow(main, aux);
    open = rc == CTK_OK;
    return rc;
  }
  int join() {
    open = false;
    return stream_follow(aux, main);
  }
  ~JoinGuard() {
    if (open) (void)stream_follow(aux, main);
  }
};

// A Linear's weight [N][K]: torch-layout f32 and/or the ctk_pack_weight blob (preferred when present).
struct WRef {
  const float* w;
  const void* p;
};

// One nn.Linear, y[M][N] = x[M][K] W^T + bias.  The constructor takes what every Linear has and assumes dense rows (x rows K
// floats apart, y rows N); a call site then names only what distinguishes it.  run() is the one place that finishes
// ctk_gemm_args: leading dimensions and batch strides are given in f32 ELEMENTS of the logical matrix, and an SH operand
// stores two halves per element, so its strides double there (a row of K columns = 2K halves).
struct Linear {
  ctk_gemm_args g{};
  Linear(const float* x, long M, WRef W, int N, int K, float* y, const float* bias) {
    g.A = x; g.lda = K; g.M = (int)M; g.W = W.w; g.Wp = W.p; g.ldw = K; g.N = N; g.K = K; g.C = y; g.ldc = N; g.bias = bias;
    g.act = CTK_ACT_NONE; g.batch = 1;
  }
  Linear& act(int a) { g.act = a; return *this; }
  Linear& ldy(long ld) { g.ldc = ld; return *this; }                  // y is a column block of a wider matrix
  Linear& add(const float* resid) { g.resid = resid; return *this; }  // y = ... + resid, resid laid out as y
  Linear& bias_rows(const float* rows, int period) { g.bias_rows = rows; g.bias_period = period; return *this; }  // + rows[m % period]
  Linear& k_valid(int k) { g.k_valid = k; return *this; }             // non-padding columns of K (flop accounting only)
  Linear& batched(int n, long x_bs, long y_bs) { g.batch = n; g.a_bs = x_bs; g.c_bs = y_bs; return *this; }  // n Linears, one W
  Linear& sh(bool in, bool out) { g.a_split = in; g.c_split = out; return *this; }  // x / y in SH format
  int run(hipStream_t s) {
    if (g.resid) g.ldr = g.ldc;
    if (g.a_split) { g.lda *= 2; g.a_bs *= 2; }
    if (g.c_split) { g.ldc *= 2; g.c_bs *= 2; }
    return ctk_gemm(&g, s);
  }
};

bool split_mode(const ctk_model_weights* w) { return w->in_p != nullptr; }
// corr_mlp.fc2 folded into the input projection (include/ctk.h, ctk_model_weights): in_w / in_p are [384, CTK_XF_LD]
bool folded(const ctk_model_weights* w) { return !w->corr_fc2_w && !w->corr_fc2_p; }

// ---- update-former workspace carve -------------------------------------------------------
// B videos (joint window): R = B*(N+64)*S rows, the B*N*S point rows first, then the B*64*S virtual rows
struct UfWs {
  float* tokens;  // [R,384]
  float* xn;      // [R,384]
  float* xn2;     // [N*S,384]  norm1(points) of the points<-virtual block, produced on the auxiliary stream
  float* qkv;     // [R,1152]
  float* att;     // [R,384]
  float* hid;     // [R,1536]
  float* partial; // attention split-K partials
  size_t bytes;
};

int v2p_splits(int N) {
  int s = (N + 1023) / 1024;  // ~1024 keys (32 tiles of 32, 8 per wave) per 4-wave workgroup of attention_q64_kernel
  if (s < 1) s = 1;
  if (s > 32) s = 32;
  return s;
}

UfWs carve_uf(int S, int N, void* base, int B = 1) {
  const size_t R = (size_t)B * (N + CTK_VIRT) * S;
  UfWs w;
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t nfloat) {
    float* r = reinterpret_cast<float*>(p + off);
    off += align256(nfloat * sizeof(float));
    return r;
  };
  w.tokens = take(R * CTK_HID);
  w.xn = take(R * CTK_HID);
  w.xn2 = take((size_t)B * N * S * CTK_HID);
  w.qkv = take(R * 3 * CTK_HID);
  w.att = take(R * CTK_HID);
  w.hid = take(R * CTK_MLP);
  w.partial = take((size_t)v2p_splits(N) * B * S * CTK_HEADS * CTK_VIRT * (CTK_HEAD_DIM + 2));
  w.bytes = off;
  return w;
}

int attn(const float* q, long q_ld, long q_bs, long q_is, const float* k, const float* v, long kv_ld, long kv_bs,
         long kv_is, float* out, long o_bs, long o_is, int nbatch, int n1, int n2, int splits, float* partial,
         hipStream_t s, bool o_split, const uint8_t* key_mask = nullptr, const uint8_t* query_mask = nullptr,
         const ctk_attn_batch2* b2 = nullptr) {
  ctk_attn_args a;
  a.key_mask = key_mask; a.query_mask = query_mask;
  a.q = q; a.q_ld = q_ld; a.q_bs = q_bs; a.q_is = q_is;
  a.k = k; a.v = v; a.kv_ld = kv_ld; a.kv_bs = kv_bs; a.kv_is = kv_is;
  a.out = out; a.o_ld = o_split ? 2 * CTK_HID : CTK_HID; a.o_bs = o_bs; a.o_is = o_is; a.o_split = o_split;
  a.nbatch = nbatch; a.n1 = n1; a.n2 = n2; a.splits = splits; a.partial = partial;
  return ctk_attention_ex(&a, b2, s);
}

// residual MLP: x += fc2(gelu_tanh(fc1(LN(x))))  on rows [r0, r0+R)   (blocks.py:437 / cotracker.py:576)
// In split mode (sp) the GEMM inputs xn / att / hid live in SH format (same bytes, same row offsets).
int mlp_block(const UfWs& ws, long r0, long R, const ctk_block_weights& b, hipStream_t s, bool sp) {
  float* tok = ws.tokens + r0 * CTK_HID;
  float* xn = ws.xn + r0 * CTK_HID;
  float* hid = ws.hid + r0 * CTK_MLP;
  CTK_TRY(ctk_layernorm(tok, xn, R, nullptr, nullptr, 1e-6f, sp, s));
  CTK_TRY(Linear(xn, R, {b.w1, b.w1_p}, CTK_MLP, CTK_HID, hid, b.b1).act(CTK_ACT_GELU_TANH).sh(sp, sp).run(s));
  CTK_TRY(Linear(hid, R, {b.w2, b.w2_p}, CTK_HID, CTK_MLP, tok, b.b2).add(tok).sh(sp, false).run(s));
  return CTK_OK;
}

// What run_transformer needs of a model: CoTracker3 (ctk_model_weights: 3 layers, no mask) and CoTracker2
// (ctk_former_weights: 6 layers, per-point attention mask) share the block structure.
struct FormerRef {
  int depth;
  const ctk_block_weights* time_blocks;
  const ctk_block_weights* virtual2point;
  const ctk_block_weights* virtual_self;
  const ctk_block_weights* point2virtual;
  const float* virtual_tokens;
  const uint8_t* point_mask;  // CoTracker2 attention_mask per point (cotracker.py:343-345) or null
  bool split;                 // xn / att / hid are SH-format (split-half back end)
  hipStream_t aux;            // optional second stream (ctk_window_args.aux_stream) or null
  bool space_attn = true;     // false: add_space_attn=False (cotracker.py:496-502): the three space blocks are skipped
  int B = 1;                  // videos of a joint window (CoTracker3 only: point_mask must be null when B > 1)
};

FormerRef former_of(const ctk_model_weights* w) {
  return FormerRef{CTK_DEPTH, w->time_blocks, w->virtual2point, w->virtual_self, w->point2virtual, w->virtual_tokens, nullptr,
                   w->in_p != nullptr, nullptr};
}

// EfficientUpdateFormer.forward (cotracker.py:483-531) on tokens already holding the input
// projection in rows [0, B*N*S).  B = fr.B videos share every row-wise launch: point row (b*N + j)*S + t, virtual row
// P + (b*64 + i)*S + t.  The tracks of all videos are ONE linear batch of the time attention; the space attentions batch over
// (video, frame) with the two outer strides N*S (point rows) and 64*S (virtual rows) -- a single level when B == 1.
int run_transformer(int S, int N, const FormerRef& fr, const UfWs& ws, hipStream_t s) {
  const FormerRef* w = &fr;
  const bool sp = fr.split;
  const int B = fr.B;
  const long P = (long)B * N * S;             // point rows
  const long V = (long)B * CTK_VIRT * S;      // virtual rows
  const long PS = (long)N * S, VS = (long)CTK_VIRT * S;  // rows of one video
  const bool joint = B > 1;
  if (joint && fr.point_mask) return CTK_E_STATE;
  const ctk_attn_batch2 v2p_b{S, 0, VS, PS, VS, 0, 0};   // queries / out: virtual rows, keys: point rows
  const ctk_attn_batch2 vself_b{S, 0, VS, VS, VS, 0, 0};
  const ctk_attn_batch2 p2v_b{S, 0, PS, VS, PS, 0, 0};   // queries / out: point rows, keys: virtual rows
  const long R = P + V;
  const long QL = 3 * CTK_HID;  // leading dimension of qkv: q | k | v columns
  // the per-row buffers from one row on: point rows (and "all rows") start at row 0, the virtual rows behind them at row P
  struct Rows { float *tok, *xn, *att, *q, *k, *v; };
  auto rows_from = [&](long r) {
    return Rows{ws.tokens + r * CTK_HID, ws.xn + r * CTK_HID, ws.att + r * CTK_HID, ws.qkv + r * QL, ws.qkv + r * QL + CTK_HID, ws.qkv + r * QL + 2 * CTK_HID};
  };
  const Rows pt = rows_from(0), vt = rows_from(P);
  // The three projections of an attention block.  The four blocks below stay written out: they differ in which rows are
  // normalised how, where q comes from and on which stream -- more than a shared helper would have parameters for.
  auto to_q = [&](const ctk_block_weights& b, const float* xn, long rows, const Rows& q, hipStream_t st) {  // q columns of q.q
    return Linear(xn, rows, {b.wq, b.wq_p}, CTK_HID, CTK_HID, q.q, b.bq).ldy(QL).sh(sp, false).run(st);
  };
  auto to_kv = [&](const ctk_block_weights& b, const Rows& kv, long rows) {  // k | v columns of kv.q from kv.xn
    return Linear(kv.xn, rows, {b.wkv, b.wkv_p}, 2 * CTK_HID, CTK_HID, kv.k, b.bkv).ldy(QL).sh(sp, false).run(s);
  };
  auto to_out = [&](const ctk_block_weights& b, const Rows& q, long rows) {  // q.tok += to_out(q.att)
    return Linear(q.att, rows, {b.wo, b.wo_p}, CTK_HID, CTK_HID, q.tok, b.bo).add(q.tok).sh(sp, false).run(s);
  };
  CTK_TRY(ctk_launch_virtual_init(w->virtual_tokens, S, vt.tok, B, s));  // cotracker.py:487-488

  for (int i = 0; i < fr.depth; ++i) {
    // ---- time attention over S for every track (incl. virtual)      cotracker.py:494-497
    {
      const ctk_block_weights& b = w->time_blocks[i];
      CTK_TRY(ctk_layernorm(pt.tok, pt.xn, R, nullptr, nullptr, 1e-6f, sp, s));
      CTK_TRY(to_q(b, pt.xn, R, pt, s));
      CTK_TRY(to_kv(b, pt, R));
      CTK_TRY(attn(pt.q, QL, S, 1, pt.k, pt.v, QL, S, 1, pt.att, S, 1, B * (N + CTK_VIRT), S, S, 1, nullptr, s, sp));
      CTK_TRY(to_out(b, pt, R));
      CTK_TRY(mlp_block(ws, 0, R, b, s, sp));
    }
    // The points<-virtual block's query side -- norm1(points) and to_q(points) -- depends only on the point tokens the
    // time block just produced, not on the virtual tracks: with an auxiliary stream it runs BESIDE the virtual-track
    // chain below (virtual<-points attention, two 1024-row MLPs, virtual self attention: ~16 launches that occupy a
    // fraction of the chip), into its own xn2 buffer and the (otherwise unused) q columns of the point rows of qkv.
    if (!fr.space_attn) continue;
    // (bit-identical to the single-stream order: same launches, same inputs; measured useless at C3 -- the side stream's persistent
    // to_q kernel and the main stream's persistent to_kv kernel each want every CU's whole LDS and serialise)
    const bool side_q = fr.aux != nullptr && (overlap_mode() & 2) != 0;
    JoinGuard side{s, fr.aux};
    if (side_q) {
      CTK_TRY(side.fork());
      CTK_TRY(ctk_layernorm(pt.tok, ws.xn2, P, nullptr, nullptr, 1e-6f, sp, fr.aux));  // norm1(points)
      CTK_TRY(to_q(w->point2virtual[i], ws.xn2, P, pt, fr.aux));
    }
    // ---- virtual <- points cross attention                          cotracker.py:510-512
    {
      const ctk_block_weights& b = w->virtual2point[i];
      CTK_TRY(ctk_layernorm(vt.tok, vt.xn, V, nullptr, nullptr, 1e-6f, sp, s));   // norm1(virtual)
      // norm_context(points) -- and, from the same read of the point tokens (the virtual-track chain below does not touch them),
      // norm1(points) of this depth's points<-virtual block into xn2 (round 5: one pass, two norms)
      if (!side_q) CTK_TRY(ctk_launch_layernorm2(pt.tok, pt.xn, P, b.ctx_gamma, b.ctx_beta, 1e-5f, ws.xn2, 1e-6f, sp, s));
      else CTK_TRY(ctk_layernorm(pt.tok, pt.xn, P, b.ctx_gamma, b.ctx_beta, 1e-5f, sp, s));                   // norm_context(points)
      CTK_TRY(to_q(b, vt.xn, V, vt, s));
      CTK_TRY(to_kv(b, pt, P));
      // batch = frame t; query i = virtual track (row P + i*S + t); key j = point (row j*S + t)
      CTK_TRY(attn(vt.q, QL, 1, S, pt.k, pt.v, QL, 1, S, vt.att, 1, S, B * S, CTK_VIRT, N,
                   v2p_splits(N), ws.partial, s, sp, fr.point_mask, nullptr, joint ? &v2p_b : nullptr));  // mask over KEYS (cotracker.py:566-569)
      CTK_TRY(to_out(b, vt, V));
      CTK_TRY(mlp_block(ws, P, V, b, s, sp));
    }
    // ---- virtual self attention (AttnBlock over 64 virtual tracks per frame)  cotracker.py:514
    {
      const ctk_block_weights& b = w->virtual_self[i];
      CTK_TRY(ctk_layernorm(vt.tok, vt.xn, V, nullptr, nullptr, 1e-6f, sp, s));
      CTK_TRY(to_q(b, vt.xn, V, vt, s));
      CTK_TRY(to_kv(b, vt, V));
      CTK_TRY(attn(vt.q, QL, 1, S, vt.k, vt.v, QL, 1, S, vt.att, 1, S, B * S,
                   CTK_VIRT, CTK_VIRT, 1, nullptr, s, sp, nullptr, nullptr, joint ? &vself_b : nullptr));
      CTK_TRY(to_out(b, vt, V));
      CTK_TRY(mlp_block(ws, P, V, b, s, sp));
    }
    // ---- points <- virtual cross attention                          cotracker.py:515-517
    {
      const ctk_block_weights& b = w->point2virtual[i];
      CTK_TRY(ctk_layernorm(vt.tok, vt.xn, V, b.ctx_gamma, b.ctx_beta, 1e-5f, sp, s));           // norm_context(virtual)
      if (!side_q) CTK_TRY(to_q(b, ws.xn2, P, pt, s));  // xn2 = norm1(points), written beside norm_context(points) above
      else CTK_TRY(side.join());  // join: q(points) is ready
      CTK_TRY(to_kv(b, vt, V));
      CTK_TRY(attn(pt.q, QL, 1, S, vt.k, vt.v, QL, 1, S, pt.att, 1, S, B * S, N, CTK_VIRT, 1, nullptr, s, sp,
                   nullptr, fr.point_mask, joint ? &p2v_b : nullptr));  // mask over QUERIES (cotracker.py:561-564)
      CTK_TRY(to_out(b, pt, P));
      CTK_TRY(mlp_block(ws, 0, P, b, s, sp));
    }
  }
  return CTK_OK;
}

// Every block of a former: the pointers its launches read; packed blobs all-or-nothing (fr.split: the SH activation pipeline
// needs every Linear of the transformer split, the f32 pipeline none)
int check_former(const FormerRef& fr) {
  auto check_block = [&](const ctk_block_weights& b, bool cross) {
    if (!b.bq || !b.bkv || !b.bo || !b.b1 || !b.b2) return CTK_E_NULL;
    if ((!b.wq && !b.wq_p) || (!b.wkv && !b.wkv_p) || (!b.wo && !b.wo_p) || (!b.w1 && !b.w1_p) || (!b.w2 && !b.w2_p)) return CTK_E_NULL;
    if (cross && (!b.ctx_gamma || !b.ctx_beta)) return CTK_E_NULL;
    const bool all_p = b.wq_p && b.wkv_p && b.wo_p && b.w1_p && b.w2_p, any_p = b.wq_p || b.wkv_p || b.wo_p || b.w1_p || b.w2_p;
    return (fr.split ? !all_p : any_p) ? CTK_E_NULL : CTK_OK;
  };
  for (int i = 0; i < fr.depth; ++i) {
    CTK_TRY(check_block(fr.time_blocks[i], false));
    CTK_TRY(check_block(fr.virtual2point[i], true));
    CTK_TRY(check_block(fr.virtual_self[i], false));
    CTK_TRY(check_block(fr.point2virtual[i], true));
  }
  // what the row kernels read with 16-byte loads (rowops.hip): the virtual tokens and norm_context's gamma / beta.  (The Linears'
  // weights and biases are checked by ctk_gemm.)  Here, so that a window refuses them before an iteration has updated anything.
  if (!ctk_aligned16(fr.virtual_tokens)) return CTK_E_ALIGN;
  for (int i = 0; i < fr.depth; ++i)
    for (const ctk_block_weights* b : {&fr.virtual2point[i], &fr.point2virtual[i]})
      if (!ctk_aligned16(b->ctx_gamma) || !ctk_aligned16(b->ctx_beta)) return CTK_E_ALIGN;
  return CTK_OK;
}

// window: the caller is a window entry point, which takes the folded form of the weights too (the stage entry points read
// in_w as [384, CTK_X_LD] or need fc2, and keep answering CTK_E_NULL to it)
int check_weights(const ctk_model_weights* w, bool window = false) {
  if (!w) return CTK_E_NULL;
  if ((!w->in_w && !w->in_p) || !w->in_bias_t || !w->virtual_tokens || !w->head_w || !w->head_b) return CTK_E_NULL;
  if (folded(w)) {
    if (!window || (!w->corr_fc1_w && !w->corr_fc1_p) || !w->corr_fc1_b) return CTK_E_NULL;
    if (split_mode(w) != (w->corr_fc1_p != nullptr)) return CTK_E_NULL;
  } else if (split_mode(w) != (w->corr_fc1_p && w->corr_fc2_p)) {
    return CTK_E_NULL;  // (corr_mlp belongs to the same pipeline)
  }
  CTK_TRY(check_former(former_of(w)));
  return ctk_aligned16(w->head_w) ? CTK_OK : CTK_E_ALIGN;  // heads_kernel holds the 4 x 384 weights as f32x4
}

// N = point tracks of ALL videos of the call (the per-frame bias is indexed by row % S: rows are track-major in every video)
// fold: x is the folded input xf [N*S, CTK_XF_LD] and in_w / in_p carry corr_mlp.fc2 (include/ctk.h)
int input_projection(int S, int N, const float* x, bool x_split, const ctk_model_weights* w, const UfWs& ws, hipStream_t s,
                     bool fold = false) {
  // tokens = input_transform(x + time_emb)   (cotracker3_online.py:247, cotracker.py:484)
  return Linear(x, N * S, {w->in_w, w->in_p}, CTK_HID, fold ? CTK_XF_LD : CTK_X_LD, ws.tokens, nullptr)
      .bias_rows(w->in_bias_t, S).k_valid(fold ? CTK_XF_DIM : CTK_X_DIM).sh(x_split, false).run(s);
}

// ---- corr_embed workspace -------------------------------------------------------------------
struct CorrWs {
  float* vol;  // [4][chunk*S][2432]   (SH format in split mode: same bytes)
  float* h1;   // [4*chunk*S][384]     (SH format in split mode); null on the folded path, where fc1 writes into xf
  void* fm_sh[CTK_MAX_BATCH][CTK_LEVELS];  // split mode: SH copy of every video's pyramid (scaled by 2^8), [S*H*W][4][2][32] halves
                                           // (query groups of one video, CTK_BATCH_SHARED_FMAPS: ONE copy, every fm_sh[b] = fm_sh[0])
  size_t bytes;
  int chunk;
  int corr_version;  // CTK_OPT_CORR_VERSION as read ONCE per entry-point call: the layout of fm_sh and the sampler kernel must agree
};

// points of the STACKED list (B*N) that go through the correlation stage at a time
int corr_chunk_points(const ctk_window_args* a, int B = 1) {
  const long all = (long)B * a->N;
  long c = a->points_per_chunk > 0 ? a->points_per_chunk : all;
  if (c > all) c = all;
  return (int)c;
}

// a = videos[0] of a joint window (the videos agree in every size); shared: the B windows are query groups of one video
CorrWs carve_corr(const ctk_window_args* a, void* base, int B = 1, bool shared = false, bool fold = false) {
  CorrWs w;
  w.corr_version = ctk_opt(CTK_OPT_CORR_VERSION);
  w.chunk = corr_chunk_points(a, B);
  const size_t rows = (size_t)w.chunk * a->S;
  char* p = static_cast<char*>(base);
  size_t off = 0;
  w.vol = reinterpret_cast<float*>(p + off);
  off += align256(rows * CTK_LEVELS * CTK_CORR_LD * sizeof(float));
  w.h1 = fold ? nullptr : reinterpret_cast<float*>(p + off);
  if (!fold) off += align256(rows * CTK_LEVELS * CTK_HID * sizeof(float));
  for (int b = 0; b < B; ++b)
    for (int l = 0; l < CTK_LEVELS; ++l) {  // always carved (the size query does not know the weights' mode): ~8 MB per frame
      if (shared && b > 0) {
        w.fm_sh[b][l] = w.fm_sh[0][l];
        continue;
      }
      w.fm_sh[b][l] = p + off;
      off += align256((size_t)a->S * (a->H[l] > 0 ? a->H[l] : 0) * (a->W[l] > 0 ? a->W[l] : 0) * CTK_C * sizeof(float));
    }
  w.bytes = off;
  return w;
}

// split mode, once per window: SH copy of the pyramid for the correlation sampler's footprint DMA (B = 1 for query groups of
// one video: the copy is shared)
int prepare_pyramid_sh(const ctk_window_args* videos, const CorrWs& ws, hipStream_t s, int B = 1) {
  for (int b = 0; b < B; ++b) {
    const ctk_window_args* a = videos + b;
    for (int l = 0; l < CTK_LEVELS; ++l) {
      if (!a->fmaps[l]) return CTK_E_NULL;
      if (a->H[l] <= 0 || a->W[l] <= 0) return CTK_E_SHAPE;
      CTK_TRY(ctk_launch_pyramid_split(a->fmaps[l], (long)a->S * a->H[l] * a->W[l], ws.fm_sh[b][l], ws.corr_version, s));
    }
  }
  return CTK_OK;
}

// x is f32 [B*N*S, CTK_X_LD] or, when x_split, the same matrix in SH format.  In split mode the hidden h1 is SH
// (fc1's epilogue writes it, fc2 streams it) and so is the correlation volume (corr_sh.hip); the caller has run
// prepare_pyramid_sh for this window.
// B videos (`videos[0..B)`, equal sizes): the chunk loop walks the STACKED point list g = b*N + n, so corr_mlp is one fc1 and one
// fc2 launch per chunk over the rows of every video in it; the sampler is launched once per video that owns points of the chunk,
// into that video's rows of the volume (its grid is already 4 workgroups per point: the single-video kernel, unchanged).
// shared (CTK_BATCH_SHARED_FMAPS, validated by check_batch): the B windows are query groups of ONE video whose coords / support /
// point_mask are consecutive slices of one allocation each -- the sampler is then launched ONCE per chunk piece over the
// stacked points [g0, g0 + pc), in its grouped instantiation (point g reads group g / N's coordinates).
// fold (window path with folded weights): x is xf [B*N*S, CTK_XF_LD] and fc1, one batch per level, writes GELU(fc1) of level l
// into its columns [384 l, 384 l + 384) -- there is no fc2 launch and no hidden buffer (ws.h1 is null).
int run_corr_embed(const ctk_window_args* videos, int B, const ctk_model_weights* w, float* x, bool x_split, const CorrWs& ws,
                   hipStream_t s, bool shared = false, bool fold = false) {
  const ctk_window_args* a = videos;
  const bool sp = split_mode(w);
  if (x_split && !sp) return CTK_E_SHAPE;
  if ((!w->corr_fc1_w && !w->corr_fc1_p) || !w->corr_fc1_b) return CTK_E_NULL;
  if (fold != folded(w) || (!fold && !w->corr_fc2_b)) return CTK_E_NULL;
  hipStream_t aux = B == 1 ? static_cast<hipStream_t>(a->aux_stream) : nullptr;  // a joint window ignores aux_stream
  const bool pipelined = sp && aux != nullptr && (overlap_mode() & 1) != 0;
  const int NT = B * a->N;
  for (int n0 = 0; n0 < NT; n0 += ws.chunk) {
    const int cnt = (NT - n0 < ws.chunk) ? NT - n0 : ws.chunk;
    // Software pipeline over point pieces: the sampler (VALU / LDS bound, MFMA pipe ~11 % busy) of piece j+1 runs on the
    // caller's stream while corr_mlp of piece j (MFMA bound) runs on the auxiliary stream; one workgroup of each kind
    // fits on a CU (77 KiB + 64 KiB of LDS).  Each piece has its own slice of the volume / hidden buffers.
    const int pieces = pipelined ? ((cnt >= 4096) ? 4 : (cnt >= 1024 ? 2 : 1)) : 1;
    const int per = (cnt + pieces - 1) / pieces;
    JoinGuard pipe{s, aux};
    for (int j = 0; j < pieces; ++j) {
      const int p0 = j * per;
      const int pc = (cnt - p0 < per) ? cnt - p0 : per;
      if (pc <= 0) break;
      const long rows = (long)pc * a->S;
      float* vol = ws.vol + (size_t)p0 * a->S * CTK_LEVELS * CTK_CORR_LD;
      float* h1 = fold ? nullptr : ws.h1 + (size_t)p0 * a->S * CTK_LEVELS * CTK_HID;
      hipStream_t gs = s;
      // stacked points [g0, g0 + pc) -> per video b: its points [m0, m0 + mc), rows (g - g0)*S + t of every level of the volume
      const int g0 = n0 + p0;
      if (shared && B > 1) {  // one grouped launch over the stacked points of every group in the piece
        if (sp) CTK_TRY(ctk_launch_corr_volume_sh(a, ws.fm_sh[0], g0, pc, vol, rows * CTK_CORR_LD * 2, ws.corr_version, s, true));
        else CTK_TRY(ctk_launch_corr_volume(a, g0, pc, vol, rows * CTK_CORR_LD, CTK_CORR_LD, s, true));
      } else {
        for (int b = g0 / a->N; b < B && b * a->N < g0 + pc; ++b) {
          const int lo = g0 > b * a->N ? g0 : b * a->N;
          const int hi = g0 + pc < (b + 1) * a->N ? g0 + pc : (b + 1) * a->N;
          const int m0 = lo - b * a->N, mc = hi - lo;
          float* vb = vol + (size_t)(lo - g0) * a->S * CTK_CORR_LD;  // (an SH row has the bytes of an f32 row)
          if (sp) CTK_TRY(ctk_launch_corr_volume_sh(videos + b, ws.fm_sh[b], m0, mc, vb, rows * CTK_CORR_LD * 2, ws.corr_version, s));
          else CTK_TRY(ctk_launch_corr_volume(videos + b, m0, mc, vb, rows * CTK_CORR_LD, CTK_CORR_LD, s));
        }
      }
      if (pipelined && pieces > 1) {
        CTK_TRY(pipe.fork());
        gs = aux;
      }
      if (fold) {
        // corr_mlp.fc1 + exact GELU, one batch per level, written into xf[g*S+t][l*384 ...]: fc2 lives in the projection
        CTK_TRY(Linear(vol, rows, {w->corr_fc1_w, w->corr_fc1_p}, CTK_HID, CTK_CORR_LD, x + (long)g0 * a->S * CTK_XF_LD, w->corr_fc1_b)
                    .act(CTK_ACT_GELU_ERF).k_valid(CTK_CORR_K).ldy(CTK_XF_LD).batched(CTK_LEVELS, rows * CTK_CORR_LD, CTK_HID)
                    .sh(sp, x_split).run(gs));
      } else {
        // corr_mlp.fc1 + exact GELU over all 4 levels at once        cotracker3_online.py:205, blocks.py:71-72
        CTK_TRY(Linear(vol, rows * CTK_LEVELS, {w->corr_fc1_w, w->corr_fc1_p}, CTK_HID, CTK_CORR_LD, h1, w->corr_fc1_b)
                    .act(CTK_ACT_GELU_ERF).k_valid(CTK_CORR_K).sh(sp, sp).run(gs));
        // corr_mlp.fc2, one batch per level, written into x[g*S+t][l*256 ...]   (torch.cat :209)
        CTK_TRY(Linear(h1, rows, {w->corr_fc2_w, w->corr_fc2_p}, 256, CTK_HID, x + (long)g0 * a->S * CTK_X_LD + CTK_X_CORR, w->corr_fc2_b)
                    .ldy(CTK_X_LD).batched(CTK_LEVELS, rows * CTK_HID, 256).sh(sp, x_split).run(gs));
      }
    }
    if (pipelined && pieces > 1) CTK_TRY(pipe.join());  // join before the next chunk reuses the buffers / x is consumed
  }
  return CTK_OK;
}

int check_window(const ctk_window_args* a) {
  if (!a) return CTK_E_NULL;
  if (a->S <= 0 || a->N <= 0 || a->iters < 0) return CTK_E_SHAPE;
  if ((long)(a->N + CTK_VIRT) * a->S > 2000000000L / CTK_MLP * 64) return CTK_E_SHAPE;
  if (a->flags & ~CTK_WINDOW_NO_SPACE_ATTN) return CTK_E_SHAPE;  // unknown flag bits: a caller built the pre-v6 struct (no `flags`)
  return CTK_OK;
}

// Host-only validation of a joint window: no HIP call is made before this has passed.
int check_batch(const ctk_window_batch* bt) {
  if (!bt) return CTK_E_NULL;
  if (bt->B < 1 || bt->B > CTK_MAX_BATCH) return CTK_E_SHAPE;
  if (bt->flags & ~CTK_BATCH_SHARED_FMAPS) return CTK_E_SHAPE;  // unknown flag bits
  if (!bt->videos) return CTK_E_NULL;
  const ctk_window_args* a = bt->videos;
  for (int b = 0; b < bt->B; ++b) CTK_TRY(check_window(a + b));
  for (int b = 1; b < bt->B; ++b) {
    const ctk_window_args* v = a + b;
    if (v->S != a->S || v->N != a->N || v->iters != a->iters || v->flags != a->flags) return CTK_E_SHAPE;
    if (v->scale_x != a->scale_x || v->scale_y != a->scale_y) return CTK_E_SHAPE;
    for (int l = 0; l < CTK_LEVELS; ++l)
      if (v->H[l] != a->H[l] || v->W[l] != a->W[l]) return CTK_E_SHAPE;
    if ((v->point_mask == nullptr) != (a->point_mask == nullptr)) return CTK_E_NULL;
  }
  if ((long)bt->B * (a->N + CTK_VIRT) * a->S > 2000000000L / CTK_MLP * 64) return CTK_E_SHAPE;  // (row counts travel as int)
  if ((bt->flags & CTK_BATCH_SHARED_FMAPS) && bt->B > 1) {
    // query groups of one video: the same pyramid, and state / support as consecutive slices of one allocation each -- what
    // the grouped sampler launch addresses with g = b*N + n (include/ctk.h)
    const size_t SN = (size_t)a->S * a->N;
    if (!a->coords || !a->vis || !a->conf) return CTK_E_NULL;
    for (int l = 0; l < CTK_LEVELS; ++l)
      if (!a->fmaps[l] || !a->support[l]) return CTK_E_NULL;
    for (int b = 1; b < bt->B; ++b) {
      const ctk_window_args* v = a + b;
      if (!v->coords || !v->vis || !v->conf) return CTK_E_NULL;
      if (v->coords != a->coords + b * SN * 2 || v->vis != a->vis + b * SN || v->conf != a->conf + b * SN) return CTK_E_SHAPE;
      for (int l = 0; l < CTK_LEVELS; ++l) {
        if (!v->support[l]) return CTK_E_NULL;
        if (v->fmaps[l] != a->fmaps[l]) return CTK_E_SHAPE;
        if (v->support[l] != a->support[l] + (size_t)b * a->N * CTK_TAPS * CTK_C) return CTK_E_SHAPE;
      }
      if (a->point_mask && v->point_mask != a->point_mask + (size_t)b * a->N) return CTK_E_SHAPE;
    }
  }
  return CTK_OK;
}

// the window state every video of a call updates in place
bool has_state(const ctk_window_args* videos, int B) {
  for (int b = 0; b < B; ++b)
    if (!videos[b].coords || !videos[b].vis || !videos[b].conf) return false;
  return true;
}

bool shared_fmaps(const ctk_window_batch* bt) { return (bt->flags & CTK_BATCH_SHARED_FMAPS) != 0 && bt->B > 1; }

// Workspace of a window: x | update-former buffers | correlation buffers.  With folded weights x is xf (CTK_XF_LD columns) and
// the correlation buffers have no hidden h1; the size queries do not know the weights, so they answer for the larger of the two
// (the unfolded one, x + h1, unless points_per_chunk is below a third of the points).
size_t x_bytes(const ctk_window_args* a, int B, bool fold) {
  return align256((size_t)B * a->N * a->S * (fold ? CTK_XF_LD : CTK_X_LD) * sizeof(float));
}

size_t window_bytes(const ctk_window_args* a, int B, bool shared = false) {
  size_t need[2];
  for (int fold = 0; fold < 2; ++fold) need[fold] = x_bytes(a, B, fold != 0) + carve_corr(a, nullptr, B, shared, fold != 0).bytes;
  return carve_uf(a->S, a->N, nullptr, B).bytes + (need[0] > need[1] ? need[0] : need[1]);
}

// One window of B videos (validated by the caller): ctk_forward_window is the B == 1 call.  shared: B query groups of one video.
// tokens_out (ctk_window_tokens_batch): the first half of ONE iteration only -- the tokens the update former would start from
int forward_windows(const ctk_window_args* videos, int B, const ctk_model_weights* w, void* workspace, size_t workspace_bytes,
                    hipStream_t s, bool shared = false, float* tokens_out = nullptr) {
  const ctk_window_args* a = videos;
  if (!has_state(videos, B) || !workspace) return CTK_E_NULL;
  if (!ctk_aligned16(workspace)) return CTK_E_ALIGN;
  if (window_bytes(a, B, shared) > workspace_bytes) return CTK_E_WORKSPACE;
  char* base = static_cast<char*>(workspace);
  float* x = reinterpret_cast<float*>(base);
  const bool fold = folded(w);    // x is xf: fc1's hidden features | small features, and the projection carries fc2
  size_t off = x_bytes(a, B, fold);
  const UfWs uws = carve_uf(a->S, a->N, base + off, B);
  off += uws.bytes;
  const CorrWs cws = carve_corr(a, base + off, B, shared, fold);
  const bool sp = split_mode(w);  // split mode: the transformer input x is kept in SH format
  const int x_ld = fold ? CTK_XF_LD : CTK_X_LD, x_small = fold ? CTK_XF_SMALL : CTK_X_VIS;
  const int iters = tokens_out ? 1 : a->iters;
  CtkBatchState st{};
  for (int b = 0; b < B; ++b) {
    st.coords[b] = videos[b].coords; st.vis[b] = videos[b].vis; st.conf[b] = videos[b].conf;
  }
  if (sp && iters > 0) CTK_TRY(prepare_pyramid_sh(videos, cws, s, shared ? 1 : B));
  for (int it = 0; it < iters; ++it) {                             // cotracker3_online.py:187
    CTK_TRY(run_corr_embed(videos, B, w, x, sp, cws, s, shared, fold));  // :190-210
    if (B == 1) CTK_TRY(ctk_launch_assemble(a, x, sp, x_ld, x_small, s));  // :212-245
    else CTK_TRY(ctk_launch_assemble_batch(st, B, a->S, a->N, a->scale_x, a->scale_y, x, sp, x_ld, x_small, s));
    CTK_TRY(input_projection(a->S, B * a->N, x, sp, w, uws, s, fold));  // :247 + cotracker.py:484
    if (tokens_out) {
      const hipError_t e = hipMemcpyAsync(tokens_out, uws.tokens, (size_t)B * a->N * a->S * CTK_HID * sizeof(float), hipMemcpyDeviceToDevice, s);
      return e == hipSuccess ? CTK_OK : (int)e;
    }
    FormerRef fr = former_of(w);
    fr.aux = B == 1 ? static_cast<hipStream_t>(a->aux_stream) : nullptr;
    fr.space_attn = (a->flags & CTK_WINDOW_NO_SPACE_ATTN) == 0;
    fr.B = B;
    // (CoTracker3's point_mask acts through the sampler alone -- it zeroes the support features of not-yet-queried tracks,
    // cotracker3_online.py:493-496 -- and the sampler reads every point's own mask byte: fr.point_mask stays null)
    CTK_TRY(run_transformer(a->S, a->N, fr, uws, s));              // :250
    if (B == 1) CTK_TRY(ctk_launch_heads(uws.tokens, w->head_w, w->head_b, a->S, a->N, nullptr, a->coords, a->vis, a->conf, s));  // :252-259
    else CTK_TRY(ctk_launch_heads_batch(uws.tokens, w->head_w, w->head_b, st, B, a->S, a->N, s));
  }
  return CTK_OK;
}

}  // namespace

extern "C" int ctk_abi_version(void) { return CTK_ABI_VERSION; }

extern "C" const char* ctk_error_string(int code) {
  switch (code) {
    case CTK_OK: return "ok";
    case CTK_E_NULL: return "required pointer is NULL";
    case CTK_E_SHAPE: return "unsupported shape";
    case CTK_E_ALIGN: return "pointer or leading dimension not aligned";
    case CTK_E_WORKSPACE: return "workspace too small";
    case CTK_E_STATE: return "call not allowed in the current state";
    default: return code > 0 ? hipGetErrorString(static_cast<hipError_t>(code)) : "unknown error";
  }
}

extern "C" int ctk_update_former_workspace_bytes(int32_t S, int32_t N, size_t* out_bytes) {
  if (!out_bytes) return CTK_E_NULL;
  if (S <= 0 || N <= 0) return CTK_E_SHAPE;
  *out_bytes = carve_uf(S, N, nullptr).bytes;
  return CTK_OK;
}

extern "C" int ctk_update_former(int32_t S, int32_t N, const float* x, const ctk_model_weights* w, float* delta,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !delta || !workspace) return CTK_E_NULL;
  if (S <= 0 || N <= 0) return CTK_E_SHAPE;
  CTK_TRY(check_weights(w));
  if (!ctk_aligned16(workspace) || !ctk_aligned16(delta)) return CTK_E_ALIGN;  // (delta: one 16-byte store per row)
  const UfWs ws = carve_uf(S, N, workspace);
  if (ws.bytes > workspace_bytes) return CTK_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  CTK_TRY(input_projection(S, N, x, false, w, ws, s));
  CTK_TRY(run_transformer(S, N, former_of(w), ws, s));
  return ctk_launch_heads(ws.tokens, w->head_w, w->head_b, S, N, delta, nullptr, nullptr, nullptr, s);
}

// ---- general update former (CoTracker2: 6 + 6 layers, 456 -> 130, attention mask) ---------------------------
extern "C" int ctk_update_former_ex(int32_t S, int32_t N, const void* x, int32_t x_split, const ctk_former_weights* w,
                                    const uint8_t* point_mask, float* delta, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (!x || !delta || !workspace || !w) return CTK_E_NULL;
  if (S <= 0 || N <= 0 || w->depth <= 0 || w->depth > 64) return CTK_E_SHAPE;
  if (w->in_ld <= 0 || (w->in_ld % 32) || w->out_ld <= 0 || (w->out_ld % 64)) return CTK_E_SHAPE;
  if ((!w->in_w && !w->in_p) || !w->virtual_tokens || (!w->head_w && !w->head_p) || !w->head_b) return CTK_E_NULL;
  if (!w->time_blocks || !w->virtual2point || !w->virtual_self || !w->point2virtual) return CTK_E_NULL;
  const bool sp = w->in_p != nullptr;
  if (x_split && !sp) return CTK_E_SHAPE;
  const FormerRef fr{w->depth, w->time_blocks, w->virtual2point, w->virtual_self, w->point2virtual, w->virtual_tokens, point_mask, sp, nullptr};
  CTK_TRY(check_former(fr));
  if (!ctk_aligned16(workspace)) return CTK_E_ALIGN;
  const UfWs ws = carve_uf(S, N, workspace);
  if (ws.bytes > workspace_bytes) return CTK_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // tokens = input_transform(x) (+ per-frame bias rows = W e_t + b when in_bias_t is given, else + in_b)
  CTK_TRY(Linear(static_cast<const float*>(x), N * S, {w->in_w, w->in_p}, CTK_HID, w->in_ld, ws.tokens, w->in_bias_t ? nullptr : w->in_b)
              .bias_rows(w->in_bias_t, S).k_valid(w->in_dim).sh(x_split != 0, false).run(s));
  CTK_TRY(run_transformer(S, N, fr, ws, s));
  // heads: delta[n*S+t][0..out_ld) = tokens @ head_w^T + head_b   (flow_head, cotracker.py:526)
  return Linear(ws.tokens, N * S, {w->head_w, w->head_p}, w->out_ld, CTK_HID, delta, w->head_b).run(s);
}

extern "C" int ctk_corr_embed_workspace_bytes(const ctk_window_args* a, size_t* out_bytes) {
  if (!out_bytes) return CTK_E_NULL;
  CTK_TRY(check_window(a));
  *out_bytes = carve_corr(a, nullptr).bytes;
  return CTK_OK;
}

extern "C" int ctk_corr_embed(const ctk_window_args* a, const ctk_model_weights* w, float* x, void* workspace,
                              size_t workspace_bytes, void* stream) {
  CTK_TRY(check_window(a));
  if (!w || !x || !workspace) return CTK_E_NULL;
  if (!ctk_aligned16(workspace) || !ctk_aligned16(x)) return CTK_E_ALIGN;
  const CorrWs ws = carve_corr(a, workspace);
  if (ws.bytes > workspace_bytes) return CTK_E_WORKSPACE;
  if (split_mode(w)) CTK_TRY(prepare_pyramid_sh(a, ws, static_cast<hipStream_t>(stream)));
  return run_corr_embed(a, 1, w, x, false, ws, static_cast<hipStream_t>(stream));
}

extern "C" int ctk_corr_volume_sh_workspace_bytes(const ctk_window_args* a, size_t* out_bytes) {
  return ctk_corr_embed_workspace_bytes(a, out_bytes);
}

extern "C" int ctk_corr_volume_sh(const ctk_window_args* a, void* out, void* workspace, size_t workspace_bytes, void* stream) {
  CTK_TRY(check_window(a));
  if (!out || !workspace) return CTK_E_NULL;
  if (!ctk_aligned16(workspace) || !ctk_aligned16(out)) return CTK_E_ALIGN;
  const CorrWs ws = carve_corr(a, workspace);
  if (ws.bytes > workspace_bytes) return CTK_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  CTK_TRY(prepare_pyramid_sh(a, ws, s));
  return ctk_launch_corr_volume_sh(a, ws.fm_sh[0], 0, a->N, out, (long)a->N * a->S * CTK_CORR_LD * 2, ws.corr_version, s);
}

// Workspace of a whole window: x | update-former buffers | correlation buffers
extern "C" int ctk_forward_window_workspace_bytes(const ctk_window_args* a, size_t* out_bytes) {
  if (!out_bytes) return CTK_E_NULL;
  CTK_TRY(check_window(a));
  *out_bytes = window_bytes(a, 1);
  return CTK_OK;
}

extern "C" int ctk_forward_window(const ctk_window_args* a, const ctk_model_weights* w, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  CTK_TRY(check_window(a));
  CTK_TRY(check_weights(w, true));
  return forward_windows(a, 1, w, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

// ---- joint window of B videos --------------------------------------------------------------------------------
extern "C" int ctk_forward_window_batch_workspace_bytes(const ctk_window_batch* batch, size_t* out_bytes) {
  if (!out_bytes) return CTK_E_NULL;
  CTK_TRY(check_batch(batch));
  *out_bytes = window_bytes(batch->videos, batch->B, shared_fmaps(batch));
  return CTK_OK;
}

extern "C" int ctk_forward_window_batch(const ctk_window_batch* batch, const ctk_model_weights* w, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  CTK_TRY(check_batch(batch));
  CTK_TRY(check_weights(w, true));
  return forward_windows(batch->videos, batch->B, w, workspace, workspace_bytes, static_cast<hipStream_t>(stream), shared_fmaps(batch));
}

extern "C" int ctk_window_tokens_batch(const ctk_window_batch* batch, const ctk_model_weights* w, float* tokens, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  CTK_TRY(check_batch(batch));
  CTK_TRY(check_weights(w, true));
  if (!tokens) return CTK_E_NULL;
  if (!ctk_aligned16(tokens)) return CTK_E_ALIGN;
  return forward_windows(batch->videos, batch->B, w, workspace, workspace_bytes, static_cast<hipStream_t>(stream), shared_fmaps(batch),
                         tokens);
}

extern "C" int ctk_corr_embed_batch_workspace_bytes(const ctk_window_batch* batch, size_t* out_bytes) {
  if (!out_bytes) return CTK_E_NULL;
  CTK_TRY(check_batch(batch));
  *out_bytes = carve_corr(batch->videos, nullptr, batch->B, shared_fmaps(batch)).bytes;
  return CTK_OK;
}

extern "C" int ctk_corr_embed_batch(const ctk_window_batch* batch, const ctk_model_weights* w, float* x, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  CTK_TRY(check_batch(batch));
  if (!w || !x || !workspace) return CTK_E_NULL;
  if (!ctk_aligned16(workspace) || !ctk_aligned16(x)) return CTK_E_ALIGN;
  const bool shared = shared_fmaps(batch);
  const CorrWs ws = carve_corr(batch->videos, workspace, batch->B, shared);
  if (ws.bytes > workspace_bytes) return CTK_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (split_mode(w)) CTK_TRY(prepare_pyramid_sh(batch->videos, ws, s, shared ? 1 : batch->B));
  return run_corr_embed(batch->videos, batch->B, w, x, false, ws, s, shared);
}

// ---- hipGraph of one window (BASELINE.json configs[3]) ------------------------------------------------------
struct ctk_window_graph {
  hipGraph_t graph;
  hipGraphExec_t exec;
  int64_t nodes;
};

namespace {
// Capture `enqueue(stream)` on a private stream into an instantiated graph.
template <typename F>
int capture_graph(F enqueue, ctk_window_graph** out) {
  hipStream_t cs = nullptr;
  hipError_t e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
  if (e != hipSuccess) return (int)e;
  // thread-local mode: allocations made by other host threads (e.g. torch's caching allocator) stay legal
  e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) {
    (void)hipStreamDestroy(cs);
    return (int)e;
  }
  const int rc = enqueue(cs);
  hipGraph_t graph = nullptr;
  e = hipStreamEndCapture(cs, &graph);
  (void)hipStreamDestroy(cs);
  if (rc != CTK_OK || e != hipSuccess || !graph) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc != CTK_OK ? rc : (e != hipSuccess ? (int)e : (int)hipErrorUnknown);
  }
  hipGraphExec_t exec = nullptr;
  e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    (void)hipGraphDestroy(graph);
    return (int)e;
  }
  size_t n = 0;
  (void)hipGraphGetNodes(graph, nullptr, &n);
  ctk_window_graph* g = new (std::nothrow) ctk_window_graph{graph, exec, (int64_t)n};
  if (!g) {
    (void)hipGraphExecDestroy(exec);
    (void)hipGraphDestroy(graph);
    return (int)hipErrorOutOfMemory;
  }
  *out = g;
  return CTK_OK;
}

// The three *_graph_create entry points.  valid(): the call's host-only validation -- everything its forward call would refuse
// is said before the capture machinery is touched; bytes(): its workspace size; enqueue(stream): that forward call.
template <typename V, typename B, typename F>
int graph_create(void* workspace, size_t workspace_bytes, ctk_window_graph** out, V valid, B bytes, F enqueue) {
  if (!out) return CTK_E_NULL;
  *out = nullptr;
  if (ctk_profile_is_on()) return CTK_E_STATE;
  CTK_TRY(valid());
  if (!workspace) return CTK_E_NULL;
  if (bytes() > workspace_bytes) return CTK_E_WORKSPACE;
  return capture_graph(enqueue, out);
}
}  // namespace

extern "C" int ctk_window_graph_create(const ctk_window_args* a, const ctk_model_weights* w, void* workspace,
                                       size_t workspace_bytes, ctk_window_graph** out) {
  auto valid = [&]() -> int { CTK_TRY(check_window(a)); CTK_TRY(check_weights(w, true)); return has_state(a, 1) ? CTK_OK : CTK_E_NULL; };
  auto bytes = [&] { return window_bytes(a, 1); };
  auto enqueue = [&](hipStream_t cs) { return ctk_forward_window(a, w, workspace, workspace_bytes, cs); };
  return graph_create(workspace, workspace_bytes, out, valid, bytes, enqueue);
}

extern "C" int ctk_window_batch_graph_create(const ctk_window_batch* batch, const ctk_model_weights* w, void* workspace,
                                             size_t workspace_bytes, ctk_window_graph** out) {
  auto valid = [&]() -> int { CTK_TRY(check_batch(batch)); CTK_TRY(check_weights(w, true)); return has_state(batch->videos, batch->B) ? CTK_OK : CTK_E_NULL; };
  auto bytes = [&] { return window_bytes(batch->videos, batch->B, shared_fmaps(batch)); };
  auto enqueue = [&](hipStream_t cs) { return ctk_forward_window_batch(batch, w, workspace, workspace_bytes, cs); };
  return graph_create(workspace, workspace_bytes, out, valid, bytes, enqueue);
}

// ---- CoTracker2 window driver (cotracker.py:86-173): one capture-safe call per window --------------------------
namespace {
struct V2Ws {
  float* pos;     // [N,456]
  float* fcorrs;  // [N,S,196]
  float* x;       // [N*S,in_ld]  (f32 or SH: same bytes)
  float* delta;   // [N*S,out_ld]
  float* normed;  // [S*N,128]
  void* former;   // update-former workspace
  size_t former_bytes;
  size_t bytes;
};

V2Ws carve_v2(const ctk_v2_window_args* a, const ctk_v2_weights* w, void* base) {
  V2Ws r;
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t nfloat) {
    float* q = reinterpret_cast<float*>(p + off);
    off += align256(nfloat * sizeof(float));
    return q;
  };
  const size_t rows = (size_t)a->N * a->S;
  r.pos = take((size_t)a->N * w->former.in_dim);
  r.fcorrs = take(rows * CTK_LEVELS * CTK_TAPS);
  r.x = take(rows * w->former.in_ld);
  r.delta = take(rows * w->former.out_ld);
  r.normed = take(rows * CTK_C);
  r.former = p + off;
  r.former_bytes = carve_uf(a->S, a->N, nullptr).bytes;
  off += r.former_bytes;
  r.bytes = off;
  return r;
}

int check_v2(const ctk_v2_window_args* a, const ctk_v2_weights* w) {
  if (!a || !w) return CTK_E_NULL;
  if (a->S <= 0 || a->N <= 0 || a->iters < 0) return CTK_E_SHAPE;
  if (w->former.in_dim != 456 || w->former.out_dim != CTK_C + 2 || w->former.in_ld < 456 || (w->former.in_ld % 32) ||
      w->former.out_ld < CTK_C + 2 || (w->former.out_ld % 64))
    return CTK_E_SHAPE;
  if (!a->coords || !a->track_feat || !a->vis || !a->track_mask || !a->vis_out) return CTK_E_NULL;
  if (!w->pos_hwc || !w->norm_w || !w->norm_b || (!w->upd_w && !w->upd_p) || !w->upd_b || !w->vis_w || !w->vis_b) return CTK_E_NULL;
  if (w->pos_h <= 0 || w->pos_w <= 0) return CTK_E_SHAPE;
  for (int l = 0; l < CTK_LEVELS; ++l) {
    if (!a->fmaps[l]) return CTK_E_NULL;
    if (a->H[l] <= 0 || a->W[l] <= 0) return CTK_E_SHAPE;
  }
  // what ctk_v2_vis_head, the LAST call of the window, would refuse (float2 loads): said here, before the iterations have
  // updated coords and track_feat in place
  if ((reinterpret_cast<uintptr_t>(a->track_feat) & 7u) || (reinterpret_cast<uintptr_t>(w->vis_w) & 7u)) return CTK_E_ALIGN;
  return CTK_OK;
}
}  // namespace

extern "C" int ctk_forward_window_v2_workspace_bytes(const ctk_v2_window_args* a, const ctk_v2_weights* w, size_t* out_bytes) {
  if (!out_bytes) return CTK_E_NULL;
  CTK_TRY(check_v2(a, w));
  *out_bytes = carve_v2(a, w, nullptr).bytes;
  return CTK_OK;
}

extern "C" int ctk_forward_window_v2(const ctk_v2_window_args* a, const ctk_v2_weights* w, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  CTK_TRY(check_v2(a, w));
  if (!workspace) return CTK_E_NULL;
  if (!ctk_aligned16(workspace)) return CTK_E_ALIGN;
  const V2Ws ws = carve_v2(a, w, workspace);
  if (ws.bytes > workspace_bytes) return CTK_E_WORKSPACE;
  const ctk_former_weights* fw = &w->former;
  const int x_split = fw->in_p != nullptr;
  const int S = a->S, N = a->N;
  // sampled_pos_emb: pos_emb at the FIRST frame's coordinates of the window (cotracker.py:126-130), fixed over the iterations
  CTK_TRY(ctk_sample_features4d(w->pos_hwc, w->pos_h, w->pos_w, fw->in_dim, a->coords, N, ws.pos, stream));
  for (int it = 0; it < a->iters; ++it) {                                                             // cotracker.py:132
    CTK_TRY(ctk_corrblock_sample(a->fmaps, a->H, a->W, S, N, a->track_feat, a->coords, ws.fcorrs, stream));   // :134-137
    CTK_TRY(ctk_v2_assemble(S, N, a->coords, ws.fcorrs, a->track_feat, a->track_mask, a->vis, ws.pos, fw->in_ld, ws.x, x_split,
                            stream));                                                                  // :139-150
    CTK_TRY(ctk_update_former_ex(S, N, ws.x, x_split, fw, a->point_mask, ws.delta, ws.former, ws.former_bytes, stream));  // :152-155
    CTK_TRY(ctk_v2_apply_delta(S, N, ws.delta, fw->out_ld, a->coords, w->norm_w, w->norm_b, 1e-5f, ws.normed, stream));  // :157-159,167
    // track_feat += GELU(Linear(GroupNorm(delta_feats)))   (track_feat_updater, cotracker.py:162-170), rows t*N+n
    CTK_TRY(Linear(ws.normed, S * N, {w->upd_w, w->upd_p}, CTK_C, CTK_C, a->track_feat, w->upd_b)
                .act(CTK_ACT_GELU_ERF).add(a->track_feat).run(static_cast<hipStream_t>(stream)));
  }
  return ctk_v2_vis_head(a->track_feat, (int64_t)S * N, w->vis_w, w->vis_b, a->vis_out, stream);   // :172
}

extern "C" int ctk_v2_window_graph_create(const ctk_v2_window_args* a, const ctk_v2_weights* w, void* workspace,
                                          size_t workspace_bytes, ctk_window_graph** out) {
  auto valid = [&]() -> int { return check_v2(a, w); };
  auto bytes = [&] { return carve_v2(a, w, nullptr).bytes; };
  auto enqueue = [&](hipStream_t cs) { return ctk_forward_window_v2(a, w, workspace, workspace_bytes, cs); };
  return graph_create(workspace, workspace_bytes, out, valid, bytes, enqueue);
}

extern "C" int ctk_window_graph_launch(ctk_window_graph* g, void* stream) {
  if (!g) return CTK_E_NULL;
  const hipError_t e = hipGraphLaunch(g->exec, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? CTK_OK : (int)e;
}

extern "C" int ctk_window_graph_nodes(const ctk_window_graph* g, int64_t* out_nodes) {
  if (!g || !out_nodes) return CTK_E_NULL;
  *out_nodes = g->nodes;
  return CTK_OK;
}

extern "C" int ctk_window_graph_destroy(ctk_window_graph* g) {
  if (!g) return CTK_OK;
  (void)hipGraphExecDestroy(g->exec);
  (void)hipGraphDestroy(g->graph);
  delete g;
  return CTK_OK;
}
