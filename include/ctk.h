/*
 * ctk.h -- C-ABI of the MI355X (gfx950) CoTracker3 iterative-update hot path.
 *
 * The reference (facebookresearch/co-tracker @ 2025-03-04) is pure Python/PyTorch and
 * has no FFI; each entry point below replaces the reference interface cited beside
 * it (paths relative to the reference root), at the operator boundary fixed in
 * SURVEY.md section 8(b).  INTEGRATION.md shows the ctypes binding a maintainer
 * would add to cotracker/models/core/cotracker/cotracker3_online.py.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory (float32 unless
 *    stated) owned by the caller; the library never allocates, frees or retains
 *    device memory.  Its only process-wide state is (i) the option table of
 *    ctk_set_option (validated relaxed atomics: a launch uses what it reads when it is
 *    enqueued; no option changes what is computed), (ii) the opt-in bench recorder
 *    (ctk_profile_enable) and (iii) per-device caches of read-only queries (CU count,
 *    fork/join event rings); kernels write no device-side globals.  Entry points may be
 *    called concurrently from several host threads on different streams.
 *  - all work is enqueued on `stream` (a hipStream_t passed as void*); no host
 *    synchronisation, no host reads of device data -> safe under stream capture.
 *  - return value: 0 ok, <0 invalid argument (CTK_E_*), >0 a hipError_t.
 *  - batch size B = 1 per call (every reference config has B = 1; the Python host
 *    loops over B) -- except ctk_forward_window_batch, the opt-in joint call for B videos
 *    of equal shape.  C = 128 feature channels, hidden = 384, heads = 8 x 48,
 *    mlp = 1536, 64 virtual tracks, 4 pyramid levels, 7x7 taps -- the values fixed by
 *    cotracker/models/build_cotracker.py:31-38 and cotracker3_online.py:43-84.
 *
 * Data layout (ours, not the reference's)
 *  - feature pyramid level l: NHWC  [T, H_l, W_l, 128]   (reference: [B,T,128,H,W])
 *  - support patches   level l: [N, 49, 128]             (reference: [B,49,N,128])
 *  - window state: coords [S,N,2] (level-0 feature units), vis [S,N], conf [S,N] logits
 *  - transformer input x: [N*S, CTK_X_LD] row = n*S+t, columns
 *        [0,1024) corr embeddings (level-major), 1024 vis, 1025 conf,
 *        [1026,1110) posenc(84), [1110,1120) zero padding
 *    (reference order is [vis,conf,corr,posenc], cotracker3_online.py:212-245; the
 *    host permutes input_transform.weight columns once at load time)
 *  - tokens: [(N+64)*S, 384], row = n*S+t, virtual tracks are n = N..N+63
 */
#ifndef CTK_H_
#define CTK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history (what a binding written against an older header must know):
 *   v9, additive (number unchanged; no existing struct or symbol changed): + ctk_fit_align and ctk_fit_align_workspace_bytes on the new
 *       struct ctk_fit_align_args: per pair of 3-D point sets the similarity Y ~ s R X + t that maps one onto the other: every candidate
 *       is the transform of three sampled common points (the ratio of the triangles' sides, ctk_fit_p3p's polar(B A^-1)), scored by an
 *       integer count under a pixel and a depth tolerance and refitted by three fixed-point Gauss-Newton rounds on seven parameters
 *       (csrc/align_math.h); one launch, no atomics, no stream history.
 *   v9, additive (number unchanged; no existing struct or symbol changed): + ctk_fit_focal and ctk_fit_focal_workspace_bytes on the new
 *       struct ctk_fit_focal_args, which is ctk_fit_pose_args with a principal point in place of four intrinsics: K candidate focal
 *       lengths are swept through ctk_fit_pose's rules over ctk_fit_epipolar's matrices and labels, every (frame, candidate) gets an
 *       int64 cost in pixels, and per group the smallest total over the frames (and over earlier calls, curve_in) is chosen and
 *       refined, or refused where the curve is flat (csrc/focal_math.h); two launches, no atomics.
 *   v9, additive (number unchanged; no existing struct or symbol changed): + ctk_fit_p3p and ctk_fit_p3p_workspace_bytes on the new
 *       struct ctk_fit_p3p_args, which is ctk_fit_resection_args without seed_pose: per frame, the camera's pose against a fixed 3-D structure
 *       WITHOUT a seed: every candidate is the pose of three sampled points (six Newton rounds on their three scales from the
 *       structure's own distances, a cofactor solve, the polar steps), scored and refitted by ctk_fit_resection's rules
 *       (csrc/p3p_math.h); one launch, no atomics.
 *   v9, additive (number unchanged; no existing struct or symbol changed): + ctk_lens_frames on the new struct ctk_lens_frames_args and
 *       ctk_lens_points on the new struct ctk_lens_points_args, both around the new struct ctk_lens, a Brown-Conrady camera of sensor
 *       and ideal intrinsics and five coefficients: uint8 pictures resampled from sensor pixels to pinhole pixels or back, the map made
 *       once per pixel for all pictures of a launch, and positions carried either way by the closed form or eight Newton rounds in
 *       double (csrc/lens_math.h); CTK_LENS_TO_IDEAL, CTK_LENS_TO_SENSOR, CTK_LENS_ROUNDS; one launch each, no atomics.
 *   v9, additive (number unchanged; no existing struct or symbol changed): + ctk_fit_structure and ctk_fit_structure_workspace_bytes on the
 *       new struct ctk_fit_structure_args: per slot, the tracked positions on up to 256 localised frames become a 3-D point in the
 *       structure's unit (a linear midpoint start, three gated Gauss-Newton rounds on the reprojection error, a parallax test; plain
 *       double sums, one thread per slot in ascending view order; csrc/structure_math.h); the old structure is carried along and
 *       everything is restated in the camera of one of the frames, with the pose chain kept in `origin`; one launch, no atomics.
 *   v9, additive (number unchanged; no existing struct or symbol changed): + ctk_fit_resection and ctk_fit_resection_workspace_bytes on the
 *       new struct ctk_fit_resection_args: per frame, the camera's pose against a fixed 3-D structure in that structure's unit and
 *       coordinates (one-scalar candidates on a seed pose scored by integer counts of reprojection inliers, three order-independent
 *       fixed-point Gauss-Newton rounds on the reprojection error; csrc/resection_math.h); one launch, no atomics.
 *   v9, additive (number unchanged; no existing struct or symbol changed): + ctk_fit_pose and ctk_fit_pose_workspace_bytes on the new
 *       struct ctk_fit_pose_args: per frame, the fundamental matrix and the labels of ctk_fit_epipolar and four intrinsics become a
 *       rotation, a unit translation (closed-form decomposition, a cheirality vote, two order-independent fixed-point Gauss-Newton
 *       rounds on the Sampson error) and two depths per correspondence (csrc/pose_math.h); one launch, no atomics.
 *   v9, additive (number unchanged; no existing struct or symbol changed): + ctk_fit_epipolar and ctk_fit_epipolar_workspace_bytes on the
 *       new struct ctk_fit_epipolar_args: per frame, one robust fundamental matrix (eight-point hypotheses by a pivoted elimination, a
 *       division-free Sampson test, two order-independent fixed-point refits) fitted to the correspondences of two frames, with a
 *       label and a squared Sampson distance per point: what moves by itself against what only shows parallax
 *       (csrc/epipolar_math.h); one launch, no atomics.
 *   v9, additive (number unchanged; no existing struct or symbol changed): + ctk_fit_planes and ctk_fit_planes_workspace_bytes on the
 *       new struct ctk_fit_planes_args: per frame, up to 16 robust homography fits (four-point hypotheses, integer admissibility, an
 *       order-independent fixed-point refit) over the regions a caller labelled, in the frame of ctk_fit_objects' labels mode; and
 *       + ctk_warp_planes on the new struct ctk_warp_planes_args: uint8 pictures resampled under a 3 x 3 matrix each, with the new
 *       border CTK_WARP_KEEP that draws a picture into frames in place (csrc/plane_math.h); one launch each, no atomics.
 *   v9, additive (number unchanged; no existing struct or symbol changed): + ctk_fit_objects and ctk_fit_objects_workspace_bytes on the
 *       new struct ctk_fit_objects_args: per frame, up to 16 robust fits (ctk_fit_motion's rules) over sub-lists of one list of
 *       correspondences -- the regions a caller labelled, or what the earlier fits left --, against a fixed frame, f - lag or an
 *       anchor (ctk_track_field's three forms), with a label per point and a box per fit (csrc/objects_math.h); one launch, no atomics.
 *   v9, additive (number unchanged; no struct changed): a ctk_model_weights with corr_fc1_* set and BOTH corr_fc2_w and corr_fc2_p
 *       NULL -- CTK_E_NULL until now -- means "corr_mlp.fc2 is folded into the input projection": in_w / in_p are [384, CTK_XF_LD]
 *       and in_bias_t carries the folded bias (see the struct).  The window entry points take it; the stage entry points that
 *       need fc2 or the [384, CTK_X_LD] projection still answer CTK_E_NULL.  + ctk_window_tokens_batch (the tokens one
 *       iteration of a window hands to the update former, for tests).
 *   v9, additive (number unchanged; no existing struct or symbol changed): + ctk_track_field and ctk_track_field_workspace_bytes on the
 *       new struct ctk_track_field_args, and ctk_warp_field on the new struct ctk_warp_field_args: a dense displacement field
 *       interpolated from the tracked points on a grid of nodes (integer tent weights, int64 sums, a sum pyramid that fills the
 *       holes), and uint8 pictures or masks resampled through such a field (csrc/field_math.h); three launches and one, no atomics.
 *   v9, additive (number unchanged; no existing struct or symbol changed): + ctk_warp_frames on the new struct ctk_warp_args and
 *       ctk_smooth_path on the new struct ctk_smooth_path_args: uint8 pictures resampled under a 2 x 3 matrix each (Q24 fixed point,
 *       bilinear in 1/256 pixel), and the causal path rule that turns per-frame camera motions into such matrices
 *       (csrc/warp_math.h); one launch each, no atomics.
 *   v9, additive (number unchanged; no existing struct or symbol changed): + ctk_fit_motion and ctk_fit_motion_workspace_bytes on the
 *       new struct ctk_fit_motion_args: per frame, a robust fit (seeded hypotheses, integer scoring) of a translation or a similarity
 *       to the motion of the tracked points, and the points that do not follow it (csrc/motion_math.h); one launch, no atomics.
 *   v9, additive (number unchanged; no existing struct or symbol changed): + ctk_draw_tracks and ctk_draw_tracks_workspace_bytes on the
 *       new struct ctk_draw_args: marks and fading trails of the tracked points drawn onto uint8 frames on the device, by integer
 *       rules (csrc/draw_math.h); two launches, no atomics.
 *   v9, additive (number unchanged; no existing struct or symbol changed): + ctk_seed_points on the new struct ctk_seed_args: the
 *       best-textured pixel (integer corner score of the luminance) of every cell of a grid over one model-resolution frame -- where a
 *       stream should put a new point; one launch, integers only.
 *   v9, additive (number unchanged; struct ctk_stream_args unchanged): + ctk_stream_health on the new struct ctk_stream_health_args: per
 *       slot, how many of the newest frames the point has been lost for and which cell of a coverage grid it is in; per cell, how
 *       many points cover it -- one launch, integers only.
 *   v9, additive (number unchanged; struct ctk_stream_args unchanged): + ctk_stream_assign_resident / ctk_stream_assign_resident_ring: the
 *       slot assign for query frames of the window just tracked, sampled from the resident pyramid between two calls.
 *   v9, additive (number unchanged; struct ctk_stream_args unchanged): + ctk_stream_begin_ring / _support_ring / _commit_ring / _assign_ring
 *       (the same struct with T_cap read as a ring of R history rows, frame f in row f % R) and + ctk_stream_emit on the new struct
 *       ctk_stream_emit_args: history frames [f0, f1) -> contiguous tracks, logits and thresholded visibility in one launch.
 *   v9, additive (number unchanged; no existing struct or symbol changed): + ctk_ingest_frames on the new struct ctk_ingest_args: raw frames
 *       (uint8 / float32, channels-last / planar, strided) resized to the encoder's input in one launch.
 *   v9, additive (number unchanged; struct ctk_stream_args unchanged): + ctk_stream_assign: slots of the resident query table of a running
 *       stream are handed to new queries, or emptied, between two calls (CTK_STREAM_EMPTY_FRAME).
 *   v9, additive (number unchanged): + ctk_stream_begin / ctk_stream_support / ctk_stream_commit on the struct ctk_stream_args: the stream state
 *       of G query groups over one live video, stepped on the device.
 *   v9, additive (number unchanged): ctk_window_batch.reserved is now `flags` (same offset and size; 0 = as before) with the bit
 *       CTK_BATCH_SHARED_FMAPS (B query groups over ONE video: one pyramid copy, one grouped sampler launch per chunk piece);
 *       + ctk_corr_embed_batch and its workspace query (corr_embed of a joint window on its own, for tests).
 *   v9, additive (no existing struct or symbol changed, number unchanged): + ctk_forward_window_batch, its workspace query and
 *       ctk_window_batch_graph_create (joint windows of up to CTK_MAX_BATCH videos); + ctk_attention_ex (two-level batch).
 *   v9 (round 6): + ctk_set_option / ctk_get_option (every back-end choice of the library in one validated, atomic table; the
 *       environment variables are read ONCE when the library is loaded); - the two stream-K scratch entry points of v7 (the
 *       stream-K walk of the persistent GEMMs left the library); ctk_gemm_pp_mode(m) = ctk_set_option(CTK_OPT_GEMM_PP, m) and
 *       accepts bits 0 and 5 only; the release library has no debug switches and exports no ctk_debug_* symbol.
 *   v8 (round 4): + ctk_bilinear_sampler (Op D); ctk_window_args.flags must be 0 or CTK_WINDOW_NO_SPACE_ATTN -- unknown bits are
 *       CTK_E_SHAPE in every entry point taking the struct; ctk_probe_mfma kind 2; the *_workspace_bytes queries no longer include
 *       the stream-K scratch.
 *   v7: ctk_gemm_scratch_bytes and its setter (removed in v9).   v6: ctk_window_args.flags, the encoder entry points.   v5: CoTracker2 window. */
#define CTK_ABI_VERSION 9
#define CTK_LEVELS 4
#define CTK_C 128          /* latent_dim                       cotracker3_online.py:60  */
#define CTK_TAPS 49        /* (2*corr_radius+1)^2, radius 3    build_cotracker.py:33    */
#define CTK_CORR_K 2401    /* 49*49                            cotracker3_online.py:84  */
#define CTK_CORR_LD 2432   /* 2401 padded to a multiple of 32 (zero columns)            */
#define CTK_HID 384        /* hidden_size                      cotracker3_online.py:77  */
#define CTK_HEADS 8
#define CTK_HEAD_DIM 48
#define CTK_MLP 1536
#define CTK_VIRT 64        /* num_virtual_tracks               cotracker3_online.py:49  */
#define CTK_X_DIM 1110     /* input_dim                        cotracker3_online.py:71  */
#define CTK_X_LD 1120      /* 1110 padded to a multiple of 32                           */
#define CTK_X_CORR 0
#define CTK_X_VIS 1024
#define CTK_X_CONF 1025
#define CTK_X_POSENC 1026
/* folded transformer input xf (corr_mlp.fc2 folded into the input projection, see ctk_model_weights): [N*S, CTK_XF_LD],
 * columns [384 l, 384 l + 384) = GELU(corr_mlp.fc1) of level l, then the 96 small-feature columns of x (vis, conf, posenc, 0) */
#define CTK_XF_LD 1632     /* 4 * 384 + 96                                              */
#define CTK_XF_SMALL 1536  /* first small-feature column (x column CTK_X_VIS)           */
#define CTK_XF_DIM 1622    /* non-padding columns                                       */
#define CTK_DEPTH 3        /* time_depth = space_depth = 3     cotracker3_online.py:74-75 */

enum {
  CTK_OK = 0,
  CTK_E_NULL = -1,      /* required pointer is NULL            */
  CTK_E_SHAPE = -2,     /* size out of range / not supported   */
  CTK_E_ALIGN = -3,     /* pointer or leading dimension not aligned (16 bytes unless the entry point says otherwise) */
  CTK_E_WORKSPACE = -4, /* workspace too small                 */
  CTK_E_STATE = -5      /* call not allowed in the current state (e.g. graph capture while the profiler is on) */
};

enum { CTK_ACT_NONE = 0, CTK_ACT_GELU_ERF = 1, CTK_ACT_GELU_TANH = 2 };

/* Weights of one transformer block (AttnBlock blocks.py:401-438 or CrossAttnBlock
 * cotracker.py:534-577).  Linear weights are torch layout [out,in] row-major.        */
typedef struct ctk_block_weights {
  const float* wq;   const float* bq;    /* to_q      [384,384],[384]   blocks.py:375 */
  const float* wkv;  const float* bkv;   /* to_kv     [768,384],[768]   blocks.py:376 (k rows 0..383, v rows 384..767) */
  const float* wo;   const float* bo;    /* to_out    [384,384],[384]   blocks.py:377 */
  const float* w1;   const float* b1;    /* mlp.fc1   [1536,384],[1536] blocks.py:61  */
  const float* w2;   const float* b2;    /* mlp.fc2   [384,1536],[384]  blocks.py:67  */
  const float* ctx_gamma; const float* ctx_beta; /* norm_context [384] (cotracker.py:540) or NULL for AttnBlock */
  /* optional ctk_pack_weight blobs of wq/wkv/wo/w1/w2: when non-NULL that Linear runs on the
   * split-half MFMA back end, when NULL on the exact-f32 one (then the f32 pointer must be set) */
  const void* wq_p; const void* wkv_p; const void* wo_p; const void* w1_p; const void* w2_p;
} ctk_block_weights;

/* EfficientUpdateFormer (cotracker.py:387-531) + corr_mlp (cotracker3_online.py:84).
 *
 * Folded form (window entry points only: ctk_forward_window, ctk_forward_window_batch, their graphs, ctk_window_tokens_batch).
 * Nothing nonlinear lies between corr_mlp.fc2 and input_transform (cotracker3_online.py:205-247 concatenates and adds the
 * time embedding), so with Win_l = the 256 input_transform columns of level l
 *     tokens = sum_l h1_l (Win_l W2)^T + x_small Win_small^T + (in_bias_t + sum_l Win_l b2),     h1_l = GELU(fc1(volume_l)),
 * and the products are weights like any other.  A struct with corr_fc1_* set and corr_fc2_w == corr_fc2_p == NULL says so:
 *     in_w / in_p   [384, CTK_XF_LD]: columns [384 l, 384 l + 384) = Win_l W2, columns CTK_XF_SMALL.. = the x columns CTK_X_VIS..
 *     in_bias_t     [S,384] with sum_l Win_l b2 added;   corr_fc2_b is ignored.
 * One iteration then runs fc1 straight into the xf rows and ONE projection with K = CTK_XF_LD: fc2's launch and the write and
 * re-read of its 1024 output columns are gone.  Every other entry point taking this struct answers CTK_E_NULL to it. */
typedef struct ctk_model_weights {
  const float* corr_fc1_w;   /* [384, CTK_CORR_LD] zero-padded columns */
  const float* corr_fc1_b;   /* [384]  */
  const float* corr_fc2_w;   /* [256,384] */
  const float* corr_fc2_b;   /* [256]  */
  const float* in_w;         /* input_transform.weight, columns permuted to the x layout, [384, CTK_X_LD] */
  const float* in_bias_t;    /* [S,384] = input_transform.bias + W @ time_emb_S[t]  (time embedding
                                 folded into the projection: W(x+e_t)+b = Wx + (W e_t + b),
                                 cotracker3_online.py:247 + cotracker.py:484) */
  /* virtual_tokens, head_w and every ctx_gamma / ctx_beta are read 16 bytes at a time by the row kernels: the window
   * entry points, their graphs and ctk_update_former (and ctk_update_former_ex for its ctk_former_weights) answer CTK_E_ALIGN
   * to one that is not 16-byte aligned, with the rest of their validation -- before any launch.  ctk_update_former asks the
   * same of delta.                                                                                                       */
  const float* virtual_tokens; /* virual_tracks [64,384]        cotracker.py:416 */
  const float* head_w;       /* [4,384] = cat(flow_head.weight, vis_conf_head.weight)  cotracker.py:526-529 */
  const float* head_b;       /* [4] */
  const void* corr_fc1_p;    /* optional ctk_pack_weight blobs of corr_fc1_w / corr_fc2_w / in_w (see ctk_block_weights) */
  const void* corr_fc2_p;
  const void* in_p;
  ctk_block_weights time_blocks[CTK_DEPTH];
  ctk_block_weights virtual2point[CTK_DEPTH];
  ctk_block_weights virtual_self[CTK_DEPTH];
  ctk_block_weights point2virtual[CTK_DEPTH];
} ctk_model_weights;

/* One sliding window / offline pass.  Replaces CoTrackerThreeOnline.forward_window
 * (cotracker3_online.py:171-264) and the inline loop of cotracker3_offline.py:139-216. */
typedef struct ctk_window_args {
  int32_t S;                  /* frames in the window (16 online/sliding, T offline)  */
  int32_t N;                  /* tracked points                                       */
  int32_t iters;              /* update iterations (predictor.py:158 uses 6)          */
  int32_t H[CTK_LEVELS];      /* level sizes                                          */
  int32_t W[CTK_LEVELS];
  const float* fmaps[CTK_LEVELS];   /* NHWC [S,H_l,W_l,128], first frame of the window */
  const float* support[CTK_LEVELS]; /* [N,49,128]                                      */
  const uint8_t* point_mask;  /* [N] 1 = track already queried (attention_mask, cotracker3_online.py:484,493-496); NULL = all 1 */
  float* coords;              /* [S,N,2] in/out, level-0 feature units                 */
  float* vis;                 /* [S,N]   in/out, logits                                */
  float* conf;                /* [S,N]   in/out, logits                                */
  float scale_x, scale_y;     /* model_resolution / stride = (W/4, H/4)  cotracker3_online.py:224-232 */
  int32_t points_per_chunk;   /* correlation stage processes this many points at a time (0 = all) */
  void* aux_stream;           /* optional second HIP stream (or NULL).  When given, ctk_forward_window forks work onto it
                                 and joins it back before returning control of `stream` to later launches: the sampler of
                                 one point piece beside corr_mlp of the previous one, and the points<-virtual query
                                 projection beside the virtual-track chain.  Same results, bit for bit (the launches and
                                 their inputs are unchanged; only their stream differs).  Must not be the capture-origin
                                 of another graph; safe inside ctk_window_graph_create (it joins that capture).  */
  int32_t flags;              /* CTK_WINDOW_NO_SPACE_ATTN: EfficientUpdateFormer.forward(add_space_attn=False) -- only the time
                                 blocks run, the virtual tracks are still appended and stripped (cotracker.py:496-502,521-523).
                                 MUST be 0 otherwise: every entry point taking this struct returns CTK_E_SHAPE when an
                                 unknown bit is set (a caller that built the pre-v6 struct hands over 4 bytes of garbage) */
} ctk_window_args;
#define CTK_WINDOW_NO_SPACE_ATTN 1

int ctk_abi_version(void);
const char* ctk_error_string(int code);

/* ---- whole-window driver (Op A + C + B + state update, `iters` times) ----------- */
int ctk_forward_window_workspace_bytes(const ctk_window_args* a, size_t* out_bytes);
int ctk_forward_window(const ctk_window_args* a, const ctk_model_weights* w,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- hipGraph of a whole window (BASELINE.json configs[3]: streaming update captured once, replayed per chunk)
 * ctk_window_graph_create captures ONE ctk_forward_window(a, w, workspace) -- every launch of all `iters`
 * iterations -- on a private capture stream and instantiates it.  The executable graph bakes in the POINTERS
 * of *a, *w and workspace: the caller keeps those buffers alive and at the same addresses and refreshes their
 * CONTENTS (pyramid, support, coords/vis/conf, point_mask) before every ctk_window_graph_launch, which
 * enqueues the whole window on `stream` as one graph launch.  The handle is a host object owned by the caller
 * (destroy with ctk_window_graph_destroy); it holds no device memory.  Capture is refused (CTK_E_STATE)
 * while ctk_profile_enable(1) is active: events cannot be recorded inside a capture.                      */
typedef struct ctk_window_graph ctk_window_graph;
int ctk_window_graph_create(const ctk_window_args* a, const ctk_model_weights* w, void* workspace,
                            size_t workspace_bytes, ctk_window_graph** out);
int ctk_window_graph_launch(ctk_window_graph* g, void* stream);
int ctk_window_graph_nodes(const ctk_window_graph* g, int64_t* out_nodes); /* kernel nodes captured */
int ctk_window_graph_destroy(ctk_window_graph* g);

/* ---- joint batch: ONE window call for B videos of equal shape (the reference carries B through every tensor of forward,
 * cotracker3_online.py:294-541) ---------------------------------------------------------------------------------------
 * videos[0..B) are B ordinary windows, each with its own pyramid, support, point_mask and coords / vis / conf state.  They
 * must agree in S, N, iters, H, W, scale_x / scale_y, flags and in whether point_mask is given; 1 <= B <= CTK_MAX_BATCH.
 * Anything else is CTK_E_SHAPE / CTK_E_NULL before any launch.  Inside the workspace the token rows are stacked as all
 * point rows of all videos, then all virtual-track rows of all videos (point row (b*N + j)*S + t, virtual row
 * B*N*S + (b*64 + i)*S + t), so every Linear, LayerNorm, time attention and MLP is ONE launch over B times the rows, the
 * space attentions run with a two-level (video, frame) batch (ctk_attention_ex), token assembly, heads and the virtual-token
 * broadcast are one launch for all videos, and the correlation sampler is launched per video into its rows of the chunk.
 * points_per_chunk and aux_stream are taken from videos[0]: the chunk counts points of the STACKED list (0 = all B*N; a
 * chunk may straddle two videos), and aux_stream is IGNORED when B > 1.
 * B == 1 enqueues exactly the launches of ctk_forward_window(&videos[0]) and needs exactly its workspace.
 * Joint and one-by-one results are fp32-class equal, NOT bit-identical: which GEMM kernel a row tile lands on depends on the
 * total row count (CTK_OPT_GEMM_PP bit 5), and those kernels differ in the residual Linears' last bit.  What is exact: a
 * video's result does not depend on the CONTENTS of the other videos of the batch, and the call is deterministic.
 * Same contract as ctk_forward_window otherwise (caller allocates, no host synchronisation, capture-safe, both Linear back
 * ends).  ctk_window_batch_graph_create captures one such call; the handle is a ctk_window_graph -- launch / nodes / destroy
 * as above -- and bakes in the pointers of every videos[b], of *w and of workspace.
 * A captured graph -- of either kind -- also bakes in the OPTION values (ctk_set_option) read while it was captured:
 * changing an option later does not change what an existing graph runs; re-create the graph.
 *
 * Query groups over ONE video: flags = CTK_BATCH_SHARED_FMAPS.  The B windows are B independent query groups (each with its
 * own 64 virtual tracks, exactly as B videos) that track over the SAME frames:
 *   - videos[b].fmaps[l] == videos[0].fmaps[l] for every b and level;
 *   - the groups' state and support are equally strided slices of ONE allocation each, group b right behind group b - 1:
 *       videos[b].coords     == videos[0].coords     + b * S*N*2        (floats)
 *       videos[b].vis / conf == videos[0].vis / conf + b * S*N
 *       videos[b].support[l] == videos[0].support[l] + b * N*49*128
 *       videos[b].point_mask == videos[0].point_mask + b * N            (bytes; or NULL in every group)
 *     i.e. coords [B,S,N,2], vis / conf [B,S,N], support[l] [B*N,49,128], point_mask [B*N];
 *   anything else is CTK_E_SHAPE (a NULL among those pointers: CTK_E_NULL) before any launch.
 * The workspace then holds ONE split-half copy of the pyramid instead of B (the size query returns less), converted once per
 * window, and the correlation sampler -- split-half versions 3 and 1 and the exact-f32 one -- is launched ONCE per chunk piece
 * over the stacked points g = b*N + n of every group in it (the grouped instantiation of the same kernel body: point g reads
 * the shared pyramid, support row g and the coordinates of its own group; each point's arithmetic is that of the per-video
 * launch, so its volume rows are the same bits).  Everything after the sampler is the joint window above, unchanged: the
 * results are those of the same B windows passed with flags = 0 and aliased fmaps.  B == 1 with the flag is B == 1 without.
 * Unknown flag bits: CTK_E_SHAPE.                                                                                        */
#define CTK_MAX_BATCH 16
#define CTK_BATCH_SHARED_FMAPS 1    /* ctk_window_batch.flags: B query groups of one video (see above) */
typedef struct ctk_window_batch {
  int32_t B;
  int32_t flags;                    /* 0 or CTK_BATCH_SHARED_FMAPS (was `reserved`, 0) */
  const ctk_window_args* videos;    /* [B] */
} ctk_window_batch;
int ctk_forward_window_batch_workspace_bytes(const ctk_window_batch* batch, size_t* out_bytes);
int ctk_forward_window_batch(const ctk_window_batch* batch, const ctk_model_weights* w, void* workspace,
                             size_t workspace_bytes, void* stream);
int ctk_window_batch_graph_create(const ctk_window_batch* batch, const ctk_model_weights* w, void* workspace,
                                  size_t workspace_bytes, ctk_window_graph** out);
/* Op A (corr_embed, below) of a joint window on its own: x f32 [B*N*S, CTK_X_LD], row (b*N + n)*S + t, columns [0,1024)
 * written.  Same validation, chunking and sampler launches as the correlation stage of ctk_forward_window_batch (with or
 * without CTK_BATCH_SHARED_FMAPS); B == 1 is ctk_corr_embed(&videos[0]).                                                  */
int ctk_corr_embed_batch_workspace_bytes(const ctk_window_batch* batch, size_t* out_bytes);
int ctk_corr_embed_batch(const ctk_window_batch* batch, const ctk_model_weights* w, float* x, void* workspace,
                         size_t workspace_bytes, void* stream);
/* The first half of ONE iteration of ctk_forward_window_batch on its own (for tests): correlation stage, token assembly and
 * input projection, by the launches the window call makes for these weights (folded or not), then tokens f32 [B*N*S, 384],
 * row (b*N + n)*S + t, copied out of the workspace.  The state is not changed.  Workspace: that of the window call.      */
int ctk_window_tokens_batch(const ctk_window_batch* batch, const ctk_model_weights* w, float* tokens, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---- stream state step: G query groups over ONE live video, state resident on the device ---------------------------------
 * The streaming glue of the reference (cotracker3_online.py:349-360 history growth, :411-440 support accumulation, :457-484
 * carry-over and attention mask, :498-510 write-back) as three launches per streaming call for ALL G*N points, on buffers the
 * caller owns and keeps between calls:
 *   queries      [G*N,3]       (frame, x, y) in model-resolution pixels, as the reference's `queries`
 *   history      hist_coords [G,T_cap,N,2] pixels, hist_vis / hist_conf [G,T_cap,N] logits; rows [0, ind + T_valid) are valid
 *                after a commit; a capacity buffer the caller grows (T_cap >= ind + S is checked by every entry point)
 *   window state coords [G,S,N,2] feature units, vis / conf [G,S,N], point_mask [G*N]: the layouts ctk_window_batch wants under
 *                CTK_BATCH_SHARED_FMAPS, so they may be the window's (and a captured graph's) own buffers
 *   support[l]   [G*N,49,128] persistent accumulators, zero when the stream starts
 * `ind` is the first frame of the window (a multiple of `step`), the same number for every group; overlap = S - step.
 *   begin:   point_mask = qframe < ind + S.  A point with ind > 0 and qframe < ind + overlap takes history rows ind .. ind+overlap-1
 *            (coords / stride), the last of them repeated `step` times; any other point takes its query (x, y) / stride and zero
 *            logits.  qframe = (integer) queries[.,0], truncated as torch's .long().  A frame that is NaN or outside
 *            [-2^31, 2^31) matches no window: it reads as a frame beyond every ind + S in begin, support, the resident assign and
 *            health (point_mask 0, begun from its query, never sampled, never carried; a plain assign; a pending slot).
 *   support: per level, ONLY the points with left <= qframe < right (left = 0 at ind == 0, else ind + step; right = ind + S) are
 *            sampled at frame qframe - ind of fmaps[l] (NHWC [S,H_l,W_l,128], the window's pyramid) at (x, y) / stride / 2^l
 *            with the arithmetic of ctk_sample_support, and ADDED into support[l]; every other row is neither read nor written.
 *            The sample ranges of successive calls are disjoint: each point is written once per stream.
 *   commit:  history rows ind .. ind+T_valid-1 = (coords * stride, vis, conf) of window rows 0 .. T_valid-1 (T_valid < S: a short
 *            last chunk).  nonfinite (optional): a device word that gets 1 OR-ed in when a committed value is not finite.
 * Every float step is the IEEE operation of the reference expression (division, multiplication, addition; no contraction), so a
 * stream stepped by these calls carries the same bits as one stepped by the torch expressions.  Each entry point validates what
 * it reads (NULL: CTK_E_NULL; G, N, S, step <= 0, step >= S, ind < 0, ind % step != 0, T_cap < ind + S, T_valid outside 1..S,
 * stride outside (0, 65536], level sizes <= 0: CTK_E_SHAPE) before any launch; no host synchronisation; capture-safe.       */
typedef struct ctk_stream_args {
  int32_t G, N;               /* query groups, points per group                                   */
  int32_t S, step;            /* window length and advance per call (window_len, window_len // 2) */
  int32_t ind;                /* first frame of this call's window                                */
  int32_t T_valid;            /* commit: frames of the chunk (1..S)                               */
  int32_t T_cap;              /* frames the history buffers hold                                  */
  float stride;               /* model stride: pixels per level-0 feature cell (4)                */
  const float* queries;
  float* hist_coords; float* hist_vis; float* hist_conf;
  float* coords; float* vis; float* conf;
  uint8_t* point_mask;
  int32_t H[CTK_LEVELS];      /* support: level sizes of fmaps                                    */
  int32_t W[CTK_LEVELS];
  const float* fmaps[CTK_LEVELS];
  float* support[CTK_LEVELS];
  int32_t* nonfinite;         /* commit: optional flag word, or NULL                              */
} ctk_stream_args;
int ctk_stream_begin(const ctk_stream_args* a, void* stream);
int ctk_stream_support(const ctk_stream_args* a, void* stream);
int ctk_stream_commit(const ctk_stream_args* a, void* stream);

/* ---- slots of a running stream: assign and release between two calls ------------------------------------------------------------
 * A row of `queries` whose frame is CTK_STREAM_EMPTY_FRAME and whose (x, y) is (0, 0) is an EMPTY SLOT: by the rules above its
 * frame is never inside a sample range and never below ind + S, so it is never sampled, keeps point_mask == 0 and is tracked as
 * the reference tracks a point whose query frame has not arrived (a blank token; it costs what a point costs).  The constant is
 * finite, exact in float32 and converts to a long; no stream reaches it.
 *   assign:  for each of the M listed slots (flat indices g*N + n into [0, G*N), pairwise different: two writers of one row are
 *            not defined; a listed index outside the range writes nothing) the query row becomes new_queries[m] = (frame, x, y),
 *            the slot's 49 x 128 accumulator rows on all four levels become zero, and so do its history rows [0, rows) (coords,
 *            vis and conf): nothing of a previous occupant can be read back.  (EMPTY_FRAME, 0, 0) releases the slot.  The caller
 *            assigns BETWEEN two calls and only frames that no support call has handed out yet: trunc(frame) >= ind + step, ind
 *            the first frame of the NEXT call's window; an earlier frame would never be sampled.  The frame rule is the caller's
 *            (the frames live on the device); rows = the history rows committed so far.
 * Reads of `a`: G, N, T_cap, queries (written, although the struct declares it const for the three step calls), hist_*, support[]
 * (16-byte aligned: cleared with vector stores), and what every entry point validates.  slots [M] and new_queries [M,3] are device
 * memory.  One launch on `stream`; no float arithmetic, no atomics, no host synchronisation; capture-safe.  NULL a, slots,
 * new_queries, queries, history or accumulator pointer: CTK_E_NULL; M <= 0, M > G*N, rows < 0, rows > T_cap, a misaligned
 * accumulator and what the step calls refuse in G, N, S, step, ind, T_cap, stride: CTK_E_SHAPE; all before any launch. */
#define CTK_STREAM_EMPTY_FRAME 1073741824.0f /* 2^30 */
int ctk_stream_assign(const ctk_stream_args* a, const int32_t* slots, const float* new_queries, int32_t M, int32_t rows,
                      void* stream);

/* ---- endless streams: ring history and one emit launch ------------------------------------------------------------------------
 * Ring forms of the four stream entry points.  They take the same struct with T_cap read as the ring size R: the history
 * buffers hold R rows and frame f lives in row f % R, so a stream of any length keeps its memory.  `ind` stays the absolute frame
 * number: the query-frame comparisons and the support tap qframe - ind are those of the linear forms, and for R >= ind + S a ring
 * form addresses the very rows the linear form addresses.  The capacity rule is R >= S (instead of T_cap >= ind + S); everything
 * else is validated as in the linear forms, plus G <= 65535, S <= 65535 and ind + S <= 2^30 (CTK_E_SHAPE), before any launch.
 *   begin_ring    carry-over from rows (ind + min(t, overlap - 1)) % R
 *   support_ring  touches no history: ctk_stream_support behind the ring's capacity rule
 *   commit_ring   window rows 0 .. T_valid-1 -> history rows (ind + t) % R
 *   assign_ring   as ctk_stream_assign with ALL R rows of each listed slot cleared (bounded, so there is no `rows` argument): after
 *                 the ring has wrapped, a slot's rows hold frames of any age
 * Frame numbers are float32 in the query table: a caller keeps ind + S <= 2^24 (the host model raises there).               */
int ctk_stream_begin_ring(const ctk_stream_args* a, void* stream);
int ctk_stream_support_ring(const ctk_stream_args* a, void* stream);
int ctk_stream_commit_ring(const ctk_stream_args* a, void* stream);
int ctk_stream_assign_ring(const ctk_stream_args* a, const int32_t* slots, const float* new_queries, int32_t M, void* stream);

/* ---- resident assign: a slot for a query on a frame of the window just tracked -----------------------------------------------------
 * Between two calls the pyramid of the call just made is still on the device.  Here `ind` is the first frame of the NEXT call's window
 * (ind >= step: a window has been tracked), and fmaps / H / W name that resident pyramid: S frames [ind - step, ind - step + S) =
 * [ind - step, ind + overlap), frame f in row f - (ind - step).  One launch for all M listed slots; per slot, by qframe =
 * trunc(new_queries[m][0]):
 *   ind - step <= qframe < ind + overlap   the query row is written; support[l] of the slot = 0 + the trilinear patch of frame row
 *            qframe - (ind - step) at (x, y) / stride / 2^l, the arithmetic of ctk_stream_support operation for operation (what it
 *            would have added to a cleared accumulator had the query been there when the window ran); the history rows [0, rows) --
 *            a ring: all R -- become zero, EXCEPT the rows of frames [ind, ind + overlap) (a ring: rows f % R), which get coords
 *            (x, y) and zero logits: the next begin carries them over into x / stride at every t, zero logits and point_mask 1, bit
 *            for bit the state of a point that begins from its query.  The next support call does not sample it again (its range
 *            starts at ind + step = ind + overlap, even S).
 *   qframe >= ind + overlap (CTK_STREAM_EMPTY_FRAME included)   exactly ctk_stream_assign.
 *   qframe < ind - step   the frame has left the pyramid: the CALLER refuses it (the frames live on the device); treated as the
 *            plain assign here.
 * Validation before any launch: everything ctk_stream_assign checks (with this `ind`, so the linear form wants T_cap >= ind + S: the
 * carry rows are inside the buffer), plus NULL fmaps[l]: CTK_E_NULL; H[l] or W[l] <= 0, ind < step: CTK_E_SHAPE.  The ring form
 * takes no `rows`.  No LDS, no atomics, no host synchronisation; capture-safe.                                                  */
int ctk_stream_assign_resident(const ctk_stream_args* a, const int32_t* slots, const float* new_queries, int32_t M, int32_t rows,
                               void* stream);
int ctk_stream_assign_resident_ring(const ctk_stream_args* a, const int32_t* slots, const float* new_queries, int32_t M, void* stream);

/* emit: history frames [f0, f1), f1 - f0 <= R, of the first N_out <= N points of every group -> contiguous, frame-ordered outputs.
 * The history row of frame f is f % R: a linear history (R = T_cap >= f1) and a ring are read by the same formula.
 *   tracks     [G, f1-f0, N_out, 2] = hist_coords * (sx, sy), one float32 multiplication per component (sx = sy = 1: a copy)
 *   vis_logit  [G, f1-f0, N_out] and conf_logit: hist_vis / hist_conf bit for bit; either may be NULL
 *   visible    [G, f1-f0, N_out] uint8, optional: sigmoid(vis) * sigmoid(conf) > thresh, sigmoid(x) = 1 / (1 + expf(-x)) in float32 (a
 *              NaN logit: not visible), ANDed with f >= first_row[g, n] when first_row (int32 [G,N], device; INT32_MAX: an empty
 *              slot) is given
 * One launch on `stream`, no host synchronisation, capture-safe.  Before the launch: NULL a, hist_coords or tracks, hist_vis /
 * hist_conf when any of vis_logit / conf_logit / visible is asked for, first_row without visible: CTK_E_NULL; G, N, N_out, R <= 0,
 * N_out > N, f0 < 0, f1 <= f0, f1 - f0 > R, f1 > 2^30, G or f1 - f0 > 65535, G * N > 2^26, a NaN thresh with visible, reserved != 0:
 * CTK_E_SHAPE.                                                                                                                 */
typedef struct ctk_stream_emit_args {
  int32_t G, N;               /* query groups, points per group of the history                     */
  int32_t N_out;              /* points per group that are written (the first N_out)               */
  int32_t R;                  /* history rows per group (ring size, or the capacity of a linear one) */
  int32_t f0, f1;             /* frames [f0, f1)                                                   */
  float sx, sy;               /* tracks = history coords * (sx, sy)                                */
  float thresh;               /* visible: sigmoid(vis) * sigmoid(conf) > thresh                    */
  int32_t reserved;           /* 0 */
  const float* hist_coords; const float* hist_vis; const float* hist_conf;
  const int32_t* first_row;   /* optional */
  float* tracks;
  float* vis_logit; float* conf_logit;   /* optional */
  uint8_t* visible;           /* optional */
} ctk_stream_emit_args;
int ctk_stream_emit(const ctk_stream_emit_args* a, void* stream);

/* health: which slots track nothing any more, and which parts of the picture no point covers -- judged over the last `look`
 * committed frames [f1 - look, f1) of the first N_out <= N slots of every group, read by emit's f % R formula (linear or ring).
 * For slot (g, n), with qframe = trunc(queries[g*N+n][0]) and start = max(first_row[g,n], qframe):
 *   empty    first_row == INT32_MAX or query frame == CTK_STREAM_EMPTY_FRAME:  lost = -1, cell = -1
 *   pending  first_row >= ind_next (assigned since the last commit: its rows are not the occupant's tracks, whatever they hold -- a
 *            resident assign leaves (x, y) and zero logits there) or start >= f1 (its query frame has not been tracked):  lost = 0,
 *            cell = the cell of its QUERY position, -1 if that lies outside the bounds
 *   tracked  alive(f) = sigmoid(vis) * sigmoid(conf) > thresh (emit's `visible` expression, bit for bit) and x_lo <= x <= x_hi and
 *            y_lo <= y <= y_hi on the history coordinates of frame f; a NaN logit or coordinate: not alive.
 *            lost = the number of consecutive frames f1-1, f1-2, ... >= max(f1 - look, start) that are not alive (0 <= lost <=
 *            min(look, f1 - start)); cell = the cell of the position at frame f1 - 1 if alive there, else -1
 *   cell     cy * gw + cx, cx = clamp((int)floorf((x - x_lo) * inv_cw), 0, gw - 1), cy likewise: two float32 operations each
 *   cover    [G, gh*gw]: cover[g, c] = the number of slots n < N_out of group g with cell == c.  Every element is written (no fill
 *            beforehand), integer counting: the result does not depend on scheduling.
 * Slots n >= N_out are neither read nor judged.  One launch on `stream`, no host synchronisation, capture-safe; writes lost, cell and
 * cover only.  Before the launch: NULL a or any NULL pointer: CTK_E_NULL; G, N, N_out, R, gh, gw <= 0, N_out > N, gh * gw > 4096,
 * f1 <= 0, f1 > 2^30, look < 1, look > R, look > f1, ind_next < 0, G > 65535, G * N > 2^26, a NaN thresh, bounds that are not finite
 * or empty (x_hi <= x_lo, y_hi <= y_lo), inv_cw or inv_ch not finite or <= 0, reserved != 0: CTK_E_SHAPE.                      */
typedef struct ctk_stream_health_args {
  int32_t G, N;               /* query groups, points per group of the history                     */
  int32_t N_out;              /* slots per group that are judged (the first N_out)                 */
  int32_t R;                  /* history rows per group (ring size, or the capacity of a linear one) */
  int32_t f1;                 /* exclusive end: the committed frame count                          */
  int32_t look;               /* frames looked back, 1 <= look <= min(R, f1)                       */
  int32_t ind_next;           /* first frame of the next call's window                             */
  float thresh;               /* alive: sigmoid(vis) * sigmoid(conf) > thresh                      */
  float x_lo, x_hi, y_lo, y_hi; /* inclusive bounds, model-resolution pixels                       */
  int32_t gh, gw;             /* coverage grid, gh * gw <= 4096 cells                              */
  float inv_cw, inv_ch;       /* float32(gw) / (x_hi - x_lo), float32(gh) / (y_hi - y_lo)          */
  int32_t reserved;           /* 0 */
  const float* queries;       /* [G*N,3] */
  const float* hist_coords; const float* hist_vis; const float* hist_conf;
  const int32_t* first_row;   /* [G,N]; INT32_MAX: an empty slot */
  int32_t* lost;              /* out [G,N_out] */
  int32_t* cell;              /* out [G,N_out] */
  int32_t* cover;             /* out [G,gh*gw] */
} ctk_stream_health_args;
int ctk_stream_health(const ctk_stream_health_args* a, void* stream);

/* ---- seed points: where to put a new point -------------------------------------------------------------------------------------
 * The best-textured pixel of every cell of a gh x gw grid over ONE planar float32 frame [3,h,w] (nominally 0..255: a frame of
 * ctk_ingest_frames' output, or of the resized chunk), by a corner score in integer arithmetic stated once in csrc/seed_math.h:
 *   luminance  q = (int)rintf(min(max(p, 0), 255)) per channel, a NaN gives 0;  L = (77 qR + 150 qG + 29 qB + 128) >> 8
 *   gradient   gx = L(y, min(x+1, w-1)) - L(y, max(x-1, 0)), gy likewise (central differences, replicated borders)
 *   tensor     a = sum gx^2, b = sum gx gy, c = sum gy^2 over the (2 radius + 1)^2 window; pixels outside the image contribute nothing
 *   score      a + c - ceil_sqrt((a - c)^2 + 4 b^2) = floor(2 lambda_min), >= 0
 *   cell       pixel (px, py) with x_lo <= px <= x_hi and y_lo <= py <= y_hi (as float32) belongs to cell cy * gw + cx, cx =
 *              clamp((int)floorf((px - x_lo) * inv_cw), 0, gw - 1), cy likewise: the cell ctk_stream_health counts a point at that
 *              position in when it is given the same bounds, grid and inv_cw / inv_ch.  A cell's pixels are a rectangle
 *              [X0,X1] x [Y0,Y1] (possibly empty).
 *   candidates the pixels of the cell with X0 + inset <= px <= X1 - inset, Y0 + inset <= py <= Y1 - inset, margin <= px <= w - 1 - margin
 *              and margin <= py <= h - 1 - margin (margin >= radius + 1 keeps the window and its gradients inside the image)
 *   seeds      [gh*gw,3] int32: row c = (px, py, score) of the candidate with the highest score -- ties: the lowest py, then the
 *              lowest px -- or (-1, -1, -1) when the cell has no candidate or its best score is below min_score.
 * Every element of seeds is written by a plain store (no fill beforehand, no atomics); the result does not depend on scheduling.
 * One launch on `stream`, no host synchronisation, capture-safe; writes seeds only.  Before the launch: NULL a, frame or seeds:
 * CTK_E_NULL; h or w outside 1..CTK_INGEST_MAX_SIDE, radius outside 1..7, margin, inset or min_score < 0, gh or gw <= 0, gh * gw >
 * 65536, bounds that are not finite or empty (x_hi <= x_lo, y_hi <= y_lo), inv_cw or inv_ch not finite or <= 0, reserved != 0:
 * CTK_E_SHAPE; frame or seeds not 4-byte aligned: CTK_E_ALIGN.                                                                */
typedef struct ctk_seed_args {
  const float* frame;         /* [3,h,w] planar float32, contiguous                                */
  int32_t h, w;
  int32_t radius;             /* window radius, 1..7                                               */
  int32_t margin;             /* candidates keep this distance from the image border, pixels       */
  int32_t inset;              /* ... and this distance from the edges of their cell, pixels        */
  int32_t min_score;          /* a cell whose best score is below it reports no seed               */
  float x_lo, x_hi, y_lo, y_hi; /* inclusive bounds, model-resolution pixels                       */
  int32_t gh, gw;             /* grid, gh * gw <= 65536 cells                                      */
  float inv_cw, inv_ch;       /* float32(gw) / (x_hi - x_lo), float32(gh) / (y_hi - y_lo)          */
  int32_t reserved;           /* 0 */
  int32_t* seeds;             /* out [gh*gw,3]: (px, py, score) or (-1, -1, -1)                    */
} ctk_seed_args;
int ctk_seed_points(const ctk_seed_args* a, void* stream);

/* ---- frame ingest: decoder output -> encoder input in one launch -------------------------------------------------------------
 * Replaces, for a stream that is fed frame by frame, the per-chunk
 *     video_chunk = F.interpolate(video_chunk.reshape(B * T, C, H, W), tuple(self.interp_shape), mode="bilinear",
 *                                 align_corners=True)                                    (predictor.py:288-290)
 * and the float conversion in front of it (online_demo.py:54-62 restacks uint8 [H,W,3] frames and converts the whole window to
 * float on every step).  Value for value that call on the source read as float32 NCHW: the arithmetic is stated once in
 * csrc/ingest_math.h, FMAs where torch's GPU kernel has them, and a uint8 source gives the bits of the same values as float32.
 * No antialiasing, as the reference.
 *   src      F frames of H x W pixels, 3 channels; dtype CTK_INGEST_U8 or CTK_INGEST_F32
 *   layout   CTK_INGEST_HWC: element (f, y, x, c) at src[f * frame_stride + y * row_stride + x * 3 + c]
 *            CTK_INGEST_CHW: element (f, c, y, x) at src[f * frame_stride + (c * H + y) * row_stride + x]
 *            strides in ELEMENTS: a cropped view or a pitch-aligned decoder surface needs no copy
 *   dst      float32 planar [F,3,h,w], contiguous, values in the range of the source (0..255 for uint8): what
 *            ctk_enc_stem_im2col reads; the 2 * (v / 255) - 1 stays there
 * One launch on `stream`, no host synchronisation, capture-safe.  Validated before the launch: NULL a, src or dst: CTK_E_NULL; an
 * unknown dtype or layout, F, H, W, h or w <= 0, F > 65535, a side above CTK_INGEST_MAX_SIDE, row_stride smaller than a row
 * (3 W or W elements), frame_stride smaller than a frame (H or 3 H rows): CTK_E_SHAPE; dst not 16-byte aligned when w % 4 == 0 (the
 * rows are stored as 16-byte vectors; 4-byte aligned otherwise), a float32 src not 4-byte aligned: CTK_E_ALIGN.             */
#define CTK_INGEST_U8 0
#define CTK_INGEST_F32 1
#define CTK_INGEST_HWC 0
#define CTK_INGEST_CHW 1
#define CTK_INGEST_MAX_SIDE 32768
typedef struct ctk_ingest_args {
  const void* src;
  int32_t dtype, layout;
  int32_t F, H, W;
  int32_t h, w;
  int32_t reserved;     /* 0 */
  int64_t frame_stride; /* elements between two frames of src   */
  int64_t row_stride;   /* elements between two pixel rows      */
  float* dst;
} ctk_ingest_args;
int ctk_ingest_frames(const ctk_ingest_args* a, void* stream);

/* ---- draw tracks: the picture of what is tracked, on the device ------------------------------------------------------------------
 * Replaces, for a caller whose frames and tracks are on the device, cotracker/utils/visualizer.py (draw_tracks_on_video: video and
 * tracks to the host, then a PIL loop over frames x points x trail segments).  The reference's rasterisation cannot be pinned bit for
 * bit; the rules here are integer arithmetic stated once in csrc/draw_math.h, and the result depends on them alone:
 *   history    hist_coords [G,R,N,2] (and hist_vis / hist_conf [G,R,N]), the row of frame f is f % R as in ctk_stream_emit: a linear
 *              history, a ring, or a plain result tensor [T,N,2] with R = T.  Picture j of F shows frame f0 + j.
 *   position   v = x * sx (y * sy), one float32 multiplication; valid iff both components lie in -65536 .. 65536 (a NaN or an infinity
 *              does not); pixel q = (int)rintf(v), round half to even
 *   shown      frame f of slot (g, n): f >= 0, f >= first_row[g, n] (optional int32 [G,N]; INT32_MAX: an empty slot, of which nothing is
 *              drawn) and a valid position
 *   visible    visible[g, f % R, n] != 0 (uint8 [G,R,N]) when `visible` is given; otherwise sigmoid(vis) * sigmoid(conf) > thresh,
 *              ctk_stream_emit's expression bit for bit (a NaN logit: not visible)
 *   mark       of slot (g, n) on picture frame f, iff the frame is shown; d2 = squared pixel distance to q.  Visible: the disc
 *              d2 <= r*r + r; not visible: the ring (r-1)*(r-1) + (r-1) < d2 <= r*r + r            (r = radius)
 *   segment    k = 1 .. trail of slot (g, n) on picture frame f joins A = frame f - k to B = frame f - k + 1, iff both frames are
 *              shown AND visible and |Bx - Ax| <= max_jump and |By - Ay| <= max_jump.  With d = B - A, p = P - A, dd = d.d, t = p.d,
 *              w2 = hw*hw + hw (hw = half_width): t <= 0: p.p <= w2; t >= dd: |p - d|^2 <= w2; otherwise cross(p, d)^2 <= w2 * dd
 *   blend      out = (v * (255 - a) + c * a + 127) / 255 per channel, c = colors[g, n], a = alpha[k] (alpha[0]: the marks)
 *   order      a pixel = the source pixel with, first, every segment that covers it blended in for k = trail down to 1, inside that g
 *              ascending, inside that n ascending; then the marks, g ascending, n ascending.  Nothing else: no scheduling, no atomics.
 *   frames     dst (and the optional src: NULL = in place) uint8, F pictures of H x W pixels, layout and strides (in elements)
 *              exactly as ctk_ingest_args: CTK_INGEST_HWC element (j, y, x, c) at j * frame_stride + y * row_stride + x * 3 + c,
 *              CTK_INGEST_CHW element (j, c, y, x) at j * frame_stride + (c * H + y) * row_stride + x; src and dst share the strides.
 *              A pitch-aligned surface or a crop needs no copy: bytes of a row beyond W pixels are neither read nor written.  In place,
 *              only changed pixels' 4-pixel groups are written; with src every pixel of dst is.
 * Only the first N_out <= N slots of a group are drawn.  Two launches on `stream` (a table of F * (trail + 1) * G * N_out primitive
 * records in draw order into `workspace`, then one workgroup per pixel tile), no host synchronisation, capture-safe; writes dst and
 * the workspace only.  Before any launch: NULL a, hist_coords, colors, dst or workspace, `visible` NULL with hist_vis or hist_conf NULL:
 * CTK_E_NULL; G, N, N_out, R or F <= 0, N_out > N, F + trail > R, f0 < 0, f0 + F > 2^30, F > 65535, H or W outside
 * 1..CTK_INGEST_MAX_SIDE, an unknown layout, row_stride smaller than a row (3 W or W), frame_stride smaller than a frame (H or 3 H
 * rows), G > 65535, G * N > 2^26, a NaN thresh without `visible`, trail outside 0..64, radius outside 1..32, half_width outside 0..16,
 * max_jump outside 1..4095, reserved != 0, workspace_bytes below what ctk_draw_tracks_workspace_bytes answers: CTK_E_SHAPE; workspace
 * not 16-byte aligned, hist_coords not 8-byte aligned: CTK_E_ALIGN.  The query checks the same shapes and no pointer of the struct. */
typedef struct ctk_draw_args {
  int32_t G, N;               /* query groups, points per group of the history                     */
  int32_t N_out;              /* points per group that are drawn (the first N_out)                 */
  int32_t R;                  /* history rows per group                                            */
  int32_t f0, F;              /* picture j shows frame f0 + j, 0 <= j < F                          */
  int32_t trail;              /* segments per point and picture, 0..64                             */
  int32_t radius;             /* marks, 1..32                                                      */
  int32_t half_width;         /* segments, 0..16                                                   */
  int32_t max_jump;           /* a segment longer than this along x or y is not drawn, 1..4095     */
  float sx, sy;               /* pixel = rint(history coords * (sx, sy))                           */
  float thresh;               /* visible from logits: sigmoid(vis) * sigmoid(conf) > thresh        */
  int32_t layout;             /* CTK_INGEST_HWC / CTK_INGEST_CHW                                   */
  int32_t H, W;
  int32_t reserved;           /* 0 */
  uint8_t alpha[65];          /* alpha[0]: marks; alpha[k]: segment k                              */
  int64_t frame_stride;       /* elements between two pictures                                     */
  int64_t row_stride;         /* elements between two pixel rows                                   */
  const float* hist_coords;
  const uint8_t* visible;     /* [G,R,N], or NULL: hist_vis / hist_conf and thresh                 */
  const float* hist_vis; const float* hist_conf;
  const int32_t* first_row;   /* optional */
  const uint8_t* colors;      /* [G,N,3] */
  const uint8_t* src;         /* optional: NULL = in place                                         */
  uint8_t* dst;
} ctk_draw_args;
int ctk_draw_tracks_workspace_bytes(const ctk_draw_args* a, size_t* out_bytes);
int ctk_draw_tracks(const ctk_draw_args* a, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fit motion: how the camera moved between two frames, and which points moved differently ----------------------------------------
 * For a caller whose tracks are on the device: the motion of frame f - lag to frame f of every group g, f in [f0, f0 + F), fitted
 * robustly to the tracked points, and the points that do not follow it.  (cotracker/utils/visualizer.py:248-256 compensates camera
 * motion by the mean displacement of points a user-supplied mask calls background, on the host.)  The rules are integer arithmetic
 * stated once in csrc/motion_math.h, and the result depends on them alone:
 *   history    hist_coords [G,R,N,2] (and hist_vis / hist_conf [G,R,N]), the row of frame f is f % R as in ctk_stream_emit: a linear
 *              history, a ring, or a plain result tensor [T,N,2] with R = T.
 *   position   v = x * sx (y * sy), one float32 multiplication; valid iff both components are finite and |v| <= 8192;
 *              P = (int)rintf(v * 16.0f), 1/16 pixel (the product by 16 is exact), |P| <= 2^17
 *   pair       slot n is a correspondence of frame f iff f - lag >= 0, f - lag >= first_row[g, n] (optional int32 [G,N]; INT32_MAX: an
 *              empty slot), both positions are valid and both frames are visible: visible[g, f % R, n] != 0 (uint8 [G,R,N]) when
 *              `visible` is given, otherwise sigmoid(vis) * sigmoid(conf) > thresh, ctk_stream_emit's expression bit for bit.  The M
 *              correspondences are numbered m = 0 .. M - 1 in ascending n; P_m is the source (frame f - lag), Q_m the destination.
 *   hypothesis k of K: mix(x) = x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (uint32);
 *              h0 = mix(seed ^ mix(f * 0x9e3779b9 + 2k)), h1 = mix(seed ^ mix(f * 0x9e3779b9 + 2k + 1)); i = h0 % M; j = h1 % (M - 1),
 *              j += (j >= i).  f is the absolute frame number: a frame's answer does not depend on how a range is cut into calls.
 *   similarity (model 1) d = P_j - P_i, e = Q_j - Q_i, D = d.d, A = d.e, B = d x e in int64 (D, |A|, |B| <= 2^37).  Admissible iff
 *              D >= base2 = ((int64)rintf(min_base * 16))^2 and D >= 1.  With u = P_m - P_i, w = Q_m - Q_i:
 *              rx = D w.x - (A u.x - B u.y), ry = D w.y - (B u.x + A u.y) (products <= 2^55); m is an inlier iff |rx| <= T D and
 *              |ry| <= T D, T = (int)rintf(tol * 16) in 1..4096 (T D <= 2^49): a max-norm test of tol pixels, inside int64.
 *   translation (model 0) only i; m is an inlier iff |w.x - u.x| <= T and |w.y - u.y| <= T; admissible whenever M >= 1.
 *   best       the maximum of (inlier count, K - 1 - k) over the admissible hypotheses: most inliers, then the lowest k.
 *   refit      over the inliers of the best, int64 sums n, Spx, Spy, Sqx, Sqy, Spp = sum |P|^2, Sdot = sum P.Q, Scr = sum P x Q;
 *              den = n Spp - (Spx^2 + Spy^2), na = n Sdot - (Spx Sqx + Spy Sqy), nb = n Scr - (Spx Sqy - Spy Sqx), all below 2^63 for
 *              n <= 8192; then in double, one IEEE operation per step: a = na / den, b = nb / den,
 *              tx = (Sqx - (a Spx - b Spy)) / (n * 16), ty = (Sqy - (b Spx + a Spy)) / (n * 16).  Translation: a = 1, b = 0,
 *              tx = (Sqx - Spx) / (n * 16), ty likewise.
 *   outputs    motion float32 [G,F,2,3] = (float)[[a, -b, tx], [b, a, ty]]: destination = matrix * (source, 1), in the pixels of
 *              the scaled positions;  inlier int8 [G,F,N_out]: -1 no correspondence, 0 outlier, 1 inlier of the best hypothesis;
 *              stats int32 [G,F,4] = (M, inlier count, best k, 0).  With no admissible hypothesis (M < 2 for a similarity, M < 1 for
 *              a translation, every sampled pair closer than min_base) the matrix is the identity -- not NaN: callers multiply
 *              these up --, the stats are (M, 0, -1, 0) and the correspondences get 0.  Every element is written by one plain store.
 * Only the first N_out <= N slots of a group are looked at.  One launch on `stream`, one workgroup per (group, frame) with the
 * correspondences in N_out * 16 bytes of LDS; no atomics, no host synchronisation, capture-safe; writes the three outputs only.  The
 * workspace query answers 0 (nothing is kept outside LDS) and `workspace` may then be NULL.  Before any launch: NULL a, hist_coords,
 * motion, inlier or stats, `visible` NULL with hist_vis or hist_conf NULL: CTK_E_NULL; G, N, N_out, R or F <= 0, N_out > N,
 * N_out > 8192, lag < 1, F + lag > R, f0 < 0, f0 + F > 2^30, F > 65535, G > 65535, G * N > 2^26, model not 0 or 1, K outside 1..4096,
 * tol NaN or with T outside 1..4096, min_base NaN, negative or above 8192, sx or sy not finite or <= 0, a NaN thresh without
 * `visible`, reserved != 0, workspace_bytes below what ctk_fit_motion_workspace_bytes answers: CTK_E_SHAPE; hist_coords not 8-byte
 * aligned: CTK_E_ALIGN.  Frames with f - lag < 0 are no error: they have no correspondences.  The query checks the same shapes and
 * no pointer of the struct. */
typedef struct ctk_fit_motion_args {
  int32_t G, N;               /* query groups, points per group of the history                     */
  int32_t N_out;              /* points per group that are looked at (the first N_out), <= 8192    */
  int32_t R;                  /* history rows per group                                            */
  int32_t f0, F;              /* row j of the outputs is frame f0 + j, 0 <= j < F                  */
  int32_t lag;                /* the motion is that of frame f - lag to frame f, >= 1              */
  int32_t model;              /* 0 translation, 1 similarity                                       */
  int32_t K;                  /* hypotheses per frame, 1..4096                                     */
  uint32_t seed;
  float tol;                  /* inlier bound, pixels (max norm); T = rint(tol * 16) in 1..4096    */
  float min_base;             /* a similarity's sample pair is at least this far apart, pixels     */
  float sx, sy;               /* position = history coords * (sx, sy)                              */
  float thresh;               /* visible from logits: sigmoid(vis) * sigmoid(conf) > thresh        */
  int32_t reserved;           /* 0 */
  const float* hist_coords;
  const uint8_t* visible;     /* [G,R,N], or NULL: hist_vis / hist_conf and thresh                 */
  const float* hist_vis; const float* hist_conf;
  const int32_t* first_row;   /* optional */
  float* motion;              /* [G,F,2,3] */
  int8_t* inlier;             /* [G,F,N_out] */
  int32_t* stats;             /* [G,F,4] */
} ctk_fit_motion_args;
int ctk_fit_motion_workspace_bytes(const ctk_fit_motion_args* a, size_t* out_bytes);
int ctk_fit_motion(const ctk_fit_motion_args* a, void* workspace, size_t workspace_bytes, void* stream);

/* ---- warp frames: pictures resampled under a matrix, and the path that steadies a camera ---------------------------------------------
 * For a caller whose frames and camera motions (ctk_fit_motion) are on the device: what a stabiliser does with them, instead of
 * accumulating matrices on the host and resampling through F.grid_sample (uint8 -> float32, affine_grid, a float result, back to
 * uint8).  The rules are integer or one-IEEE-operation-per-step double arithmetic stated once in csrc/warp_math.h, and the results
 * depend on them alone.
 *
 * ctk_warp_frames: picture j of dst = picture j of src resampled under matrices[j].
 *   matrix     float32 2 x 3, maps an OUTPUT pixel to a SOURCE position: (sx, sy) = m (x, y, 1); pixel centres are at integers.
 *              Valid iff all six entries are finite, |m00|, |m01|, |m10|, |m11| <= 8 and |m02|, |m12| <= 32768; an invalid matrix
 *              counts as the identity (the picture is copied), as ctk_fit_motion answers the identity where nothing can be fitted.
 *   fixed point c_k = (int64)rint((double)m_k * 16777216.0): Q24, the product is exact, round half to even
 *   coordinate X = c00 x + c01 y + c02 + 32768 and Y likewise, int64 (below 2^45); ix = X >> 24 (a floor), fx = (X >> 16) & 255
 *   taps       (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1).  border CTK_WARP_FILL: a tap outside [0, W) x [0, H) has the
 *              value fill[c]; CTK_WARP_EDGE: tap indices are clamped into range.  Nothing outside the picture is ever read.
 *   blend      out = ((256 - fx)(256 - fy) p00 + fx (256 - fy) p01 + (256 - fx) fy p10 + fx fy p11 + 32768) >> 16 per channel, int32.
 *              The identity copies the source bit for bit; an integer translation is a shifted copy.
 *   frames     src and dst uint8, F pictures of H x W pixels, 3 channels, layout and strides (in elements) with ctk_ingest_args'
 *              meaning: CTK_INGEST_HWC element (j, y, x, c) at j * frame_stride + y * row_stride + x * 3 + c, CTK_INGEST_CHW element
 *              (j, c, y, x) at j * frame_stride + (c * H + y) * row_stride + x; src and dst have strides of their own.  Bytes of a row
 *              beyond W pixels are neither read nor written.  src and dst must not overlap: a warp cannot run in place.
 * One launch on `stream` (a workgroup stages the source box of its 64 x 16 output tile in 16 KiB of LDS, or reads memory directly where
 * the box does not fit), no atomics, no host synchronisation, capture-safe; writes dst only (whole dwords when dst,
 * dst_row_stride and dst_frame_stride are multiples of 4 bytes, bytes otherwise).  Before the launch: NULL a, matrices, src or dst:
 * CTK_E_NULL; F outside 1..65535, H or W outside 1..CTK_INGEST_MAX_SIDE, an unknown layout or border, a row stride smaller than a row
 * (3 W or W), a frame stride smaller than a frame (H or 3 H rows), a stride above 2^40, overlapping byte ranges of src and dst,
 * reserved != 0: CTK_E_SHAPE; matrices not 4-byte aligned: CTK_E_ALIGN.
 *
 * ctk_smooth_path: a causal, leaky lock-on whose state stays bounded.  W (2 x 3, double) maps a stabilised pixel to a position in the
 * current frame; state [G,6] holds it row-major per group, the identity before the first frame.  For frame f of group g, in order:
 *   input      M = motion[g, f] (ctk_fit_motion with lag 1: frame f - 1 to frame f), float32 converted to double; a matrix with a
 *              non-finite entry counts as the identity: the state persists and must never become NaN
 *   compose    P[r][0] = M[r][0] W[0][0] + M[r][1] W[1][0];  P[r][1] = M[r][0] W[0][1] + M[r][1] W[1][1];
 *              P[r][2] = (M[r][0] W[0][2] + M[r][1] W[1][2]) + M[r][2];  one rounded operation per step, no contraction
 *   blend      W' = k P elementwise, then W'[0][0] += a, W'[1][1] += a, with a = (double)alpha, k = 1.0 - a.  (With C_f the cumulative
 *              camera pose and S_f = (1 - alpha) S_f-1 + alpha C_f its exponential smoothing, the correction inverse(C_f) S_f obeys
 *              this recurrence.)  alpha = 0 locks onto the first frame, alpha = 1 corrects nothing.
 *   output     warp[g, f] = (float)W', or (float)(W' o post) composed by the same three formulas when post (float32 2 x 3, e.g. a
 *              zoom that hides the border) is given; post does not enter the state.  warp[g, f] is a matrix for ctk_warp_frames.
 * One launch on `stream`, one thread per group, sequential over the F frames; no host synchronisation, capture-safe; every element of
 * warp and state is written by one plain store, and a group's state is read and then written by its own thread only.  Before the
 * launch: NULL a, motion, state or warp: CTK_E_NULL; G or F outside 1..65535, alpha NaN or outside [0, 1], reserved != 0:
 * CTK_E_SHAPE; state not 8-byte aligned, motion, warp or post not 4-byte aligned: CTK_E_ALIGN.                                  */
#define CTK_WARP_FILL 0
#define CTK_WARP_EDGE 1
typedef struct ctk_warp_args {
  int32_t F, H, W;            /* pictures, and their size in pixels                                */
  int32_t layout;             /* CTK_INGEST_HWC / CTK_INGEST_CHW                                   */
  int32_t border;             /* CTK_WARP_FILL / CTK_WARP_EDGE                                     */
  int32_t reserved;           /* 0 */
  uint8_t fill[4];            /* the value of a tap outside the picture, per channel; three used   */
  int64_t src_frame_stride;   /* elements between two pictures of src                              */
  int64_t src_row_stride;     /* elements between two pixel rows of src                            */
  int64_t dst_frame_stride;
  int64_t dst_row_stride;
  const float* matrices;      /* [F,2,3], on the device                                            */
  const uint8_t* src;
  uint8_t* dst;
} ctk_warp_args;
int ctk_warp_frames(const ctk_warp_args* a, void* stream);

typedef struct ctk_smooth_path_args {
  int32_t G, F;               /* groups, frames per group                                          */
  float alpha;                /* 0 locks onto the first frame .. 1 corrects nothing                */
  int32_t reserved;           /* 0 */
  const float* motion;        /* [G,F,2,3] */
  const float* post;          /* [2,3], or NULL                                                    */
  double* state;              /* [G,6], read and then written                                      */
  float* warp;                /* [G,F,2,3] */
} ctk_smooth_path_args;
int ctk_smooth_path(const ctk_smooth_path_args* a, void* stream);

/* ---- lens: the distortion of a real lens taken out of pictures and positions, in front of everything else ------------------------------
 * Every fit below ("fit epipolar" .. "fit structure") assumes one pinhole camera.  A wide lens moves the corners of a 1080p picture by
 * more than a hundred pixels, the fits' tolerances are 1 - 2.  ctk_lens_frames resamples raw sensor pictures into pinhole pictures
 * BEFORE they enter a stream (or back); ctk_lens_points carries positions between sensor pixels and ideal pixels in either direction
 * (tracks made on sensor pixels into the fits, results back onto the original frames).  No fit kernel changes.  The rules are stated
 * once in csrc/lens_math.h: decisions are integers or single comparisons, everything in double is one IEEE operation per step in the
 * order written there, and the results depend on them alone.
 *   camera     struct ctk_lens: Brown-Conrady with k = (k1, k2, p1, p2, k3), the order every calibration tool writes.  sensor =
 *              (fx, fy, cx, cy), the pinhole part of the real camera in raw-video pixels; ideal = (fx', fy', cx', cy'), the camera the
 *              corrected pictures and positions are stated in (equal to `sensor` unless the caller wants another field of view or
 *              size); pixel centres at integers.  Valid iff all 13 numbers are finite, the four focal lengths lie in [1, 1e6],
 *              |centre| <= 32768, |coefficient| <= 64 and reserved == 0.  An invalid lens is refused; it never counts as the identity.
 *   forward    ideal -> sensor, (x, y) normalised ideal coordinates:  r2 = x x + y y;  rad = 1 + r2 (k1 + r2 (k2 + r2 k3));
 *              xd = x rad + 2 p1 x y + p2 (r2 + 2 x x);  yd = y rad + p1 (r2 + 2 y y) + 2 p2 x y;
 *              sensor pixel = (fx xd + cx, fy yd + cy), ideal pixel = (fx' x + cx', fy' y + cy').
 *   jacobian   with dr = k1 + r2 (2 k2 + 3 k3 r2):  a = rad + 2 x x dr + 2 p1 y + 6 p2 x;  b = c = 2 x y dr + 2 p1 x + 2 p2 y;
 *              d = rad + 2 y y dr + 6 p1 y + 2 p2 x;  det = a d - b c.
 *   inverse    sensor -> ideal: Newton from (x, y) = (xd, yd), CTK_LENS_ROUNDS = 8 rounds, always all of them: (ex, ey) = (xd, yd) -
 *              forward of (x, y), idet = 1 / det (the one division of a round), x += (d ex - b ey) idet, y += (a ey - c ex) idet.
 *              Accepted iff, at the result, det > 0 and the squared residual in sensor pixels (fx ex)^2 + (fy ey)^2 <= tol2 =
 *              (double)tol (double)tol.  A NaN fails both comparisons.  No root, no library call.  Where the polynomial folds
 *              inside the field (det <= 0) there is no inverse, and the point is reported as such.
 *   points     ctk_lens_points, direction CTK_LENS_TO_IDEAL: the position is read as two float32 widened to double; not finite, or
 *              |p| > 32768 on an axis: (NaN, NaN) with the bits 0x7FC00000, label -1.  Otherwise it is normalised with 1 / fx, 1 / fy
 *              (one division per launch, on the host) and inverted: accepted, the (float) of the ideal pixel, label 1; not accepted,
 *              NaN, label 0.  Every fit kernel treats a NaN position as "not on this frame": a point without an inverse never
 *              enters a fit.  CTK_LENS_TO_SENSOR: the same reading and refusal, normalised with 1 / fx', 1 / fy', forward; label 1 iff
 *              det > 0 at that point, else label 0 and NaN.
 *   pictures   ctk_lens_frames: for output pixel (x, y) the source position (px, py) in double -- forward for CTK_LENS_TO_IDEAL (the
 *              output is the pinhole picture), the inverse for CTK_LENS_TO_SENSOR.  The pixel is OUTSIDE when the point rule gives a
 *              label <= 0, or (px, py) is not finite or |p| > 32768 on an axis; an outside pixel takes fill[c] under either border.
 *              Otherwise X = llrint(px * 256.0) (round half to even), ix = X >> 8, fx = X & 255, Y likewise, and the four taps, the
 *              CTK_WARP_FILL / CTK_WARP_EDGE borders and the blend are exactly ctk_warp_frames'.  With all coefficients 0 and
 *              ideal == sensor the source is copied bit for bit (the round trip through the normalised coordinate is off by 1e-10
 *              pixel, far less than 1/512); a centre shifted by whole pixels gives a shifted copy.
 *   frames     src uint8, F pictures of H x W; dst uint8, F pictures of Ho x Wo (another size goes with another ideal or sensor
 *              camera); 3 channels; layouts, strides (in elements) and the whole-dword-or-byte store rule as in ctk_warp_args.  src
 *              and dst must not overlap.  The source position of a pixel does not depend on the picture: a thread computes the
 *              double-precision map of its 4 consecutive pixels of a row once and loops over the pictures (a slice of them per grid
 *              z, and more than one slice only where a small picture would not fill the device); memory is read directly.
 * One launch each on `stream`, no atomics, no host synchronisation, capture-safe; every output element is written by one plain store
 * and the inputs are only read.  ctk_lens_points: one thread per point, a position is one 8-byte load and one 8-byte store; src and
 * dst float32 [G,F,N,2] with group and frame strides in elements each; dst == src with equal strides is allowed (an element is read
 * and then written by its own thread), any other overlap is not; label int8 [G,F,N] dense, or NULL.
 * Before the launch.  ctk_lens_frames: NULL a, src or dst: CTK_E_NULL; F outside 1..65535, H, W, Ho or Wo outside
 * 1..CTK_INGEST_MAX_SIDE, an unknown layout, border or direction, a stride smaller than its row or frame or above 2^40, an invalid
 * lens, tol not > 0 (or not finite), overlapping byte ranges, reserved != 0: CTK_E_SHAPE.  ctk_lens_points: NULL a, src or dst:
 * CTK_E_NULL; G or F outside 1..65535, N outside 1..2^20, an unknown direction, a frame stride below 2 N, a group stride below F frame
 * strides, a stride above 2^40, an invalid lens, tol not > 0, reserved != 0, an overlap other than dst == src with equal strides
 * (label included): CTK_E_SHAPE; src or dst not 8-byte aligned or an odd stride: CTK_E_ALIGN.
 *
 * Known limits.  Five coefficients: no thin-prism, tilt or rational (k4 .. k6) terms, no fisheye (equidistant) model.  One lens per
 * launch.  Bilinear resampling, no prefilter: a picture shrunk by much more than 2 aliases.  The Newton start is the distorted
 * position itself: a lens so strong that this start lies beyond the fold reports label 0 there although an inverse exists. */
#define CTK_LENS_TO_IDEAL 0
#define CTK_LENS_TO_SENSOR 1
#define CTK_LENS_ROUNDS 8
typedef struct ctk_lens {
  double sensor[4];           /* fx, fy, cx, cy of the real camera, raw-video pixels               */
  double ideal[4];            /* fx', fy', cx', cy' of the pinhole camera                          */
  double k[5];                /* k1, k2, p1, p2, k3                                                */
  double reserved;            /* 0 */
} ctk_lens;

typedef struct ctk_lens_frames_args {
  int32_t F;                  /* pictures                                                          */
  int32_t H, W;               /* size of a src picture in pixels                                   */
  int32_t Ho, Wo;             /* size of a dst picture                                             */
  int32_t layout;             /* CTK_INGEST_HWC / CTK_INGEST_CHW                                   */
  int32_t border;             /* CTK_WARP_FILL / CTK_WARP_EDGE                                     */
  int32_t direction;          /* CTK_LENS_TO_IDEAL: dst is the pinhole picture / CTK_LENS_TO_SENSOR */
  float tol;                  /* residual of an accepted inverse, sensor pixels, > 0               */
  int32_t reserved;           /* 0 */
  uint8_t fill[4];            /* the value outside the picture, per channel; three used            */
  int64_t src_frame_stride;   /* elements between two pictures of src                              */
  int64_t src_row_stride;     /* elements between two pixel rows of src                            */
  int64_t dst_frame_stride;
  int64_t dst_row_stride;
  ctk_lens lens;
  const uint8_t* src;
  uint8_t* dst;
} ctk_lens_frames_args;
int ctk_lens_frames(const ctk_lens_frames_args* a, void* stream);

typedef struct ctk_lens_points_args {
  int32_t G, F, N;            /* groups, frames per group, points per frame                        */
  int32_t direction;          /* CTK_LENS_TO_IDEAL / CTK_LENS_TO_SENSOR                            */
  float tol;                  /* residual of an accepted inverse, sensor pixels, > 0               */
  int32_t reserved;           /* 0 */
  int64_t src_group_stride;   /* elements (floats) between two groups of src                       */
  int64_t src_frame_stride;   /* elements between two frames of src, >= 2 N                        */
  int64_t dst_group_stride;
  int64_t dst_frame_stride;
  ctk_lens lens;
  const float* src;           /* [G,F,N,2] */
  float* dst;                 /* [G,F,N,2]; may be src itself                                      */
  int8_t* label;              /* [G,F,N]: 1 carried, 0 no inverse / folded, -1 not a position; or NULL */
} ctk_lens_points_args;
int ctk_lens_points(const ctk_lens_points_args* a, void* stream);

/* ---- track field: a dense displacement field from the tracked points, and pictures carried along it ---------------------------------
 * For a caller whose tracks are on the device and whose scene does not move as one plane: what ctk_fit_motion's single matrix cannot
 * say.  An object mask, a paint stroke or a texture known on one frame is carried onto other frames along the tracked points, or a
 * dense flow picture is made of them, instead of a scattered-data interpolation on the host or a torch chain of float atomics,
 * F.interpolate and grid_sample.  The rules are integer arithmetic and one IEEE double division per node component, stated once in
 * csrc/field_math.h, and the results depend on them alone.
 *
 * ctk_track_field: for group g and frame f in [f0, f0 + F) ("at") against a frame "to", the field on the picture grid of frame f whose
 * value at a position is the displacement that leads to the matching position of frame "to": a picture known on frame "to" is
 * warped BACKWARDS onto frame f by ctk_warp_field.
 *   history    hist_coords [G,R,N,2] (and hist_vis / hist_conf [G,R,N]), the row of frame f is f % R, as in ctk_fit_motion.
 *   position   ctk_fit_motion's: v = x * sx (y * sy), one float32 multiplication; valid iff finite and |v| <= 8192;
 *              P = (int)rintf(v * 16.0f), 1/16 pixel.  P is on frame f, Q on frame "to", d = Q - P, |d| <= 2^18.
 *   to         exactly one of three forms: a fixed frame to >= 0 (lag = 0, no anchor);  f - lag with lag != 0 (to = -1, no anchor; a
 *              negative lag gives forward flow);  an anchor (to = -1, lag = 0): anchor_coords [G,N,2] float32 (scaled by sx, sy like the
 *              history) and anchor_visible [G,N] uint8, taken by the caller on frame anchor_frame >= 0 -- how a picture is carried on
 *              after a ring has dropped its source frame.
 *   pair       slot n is a correspondence iff both frames are >= 0, both are >= first_row[g, n] (optional int32 [G,N]; INT32_MAX: an
 *              empty slot; in anchor form anchor_frame counts as the "to" frame, so a slot released and reassigned after the anchor
 *              was taken drops out), both positions are valid and both are visible: by ctk_fit_motion's rule bit for bit on the
 *              history (visible [G,R,N] uint8, or sigmoid(vis) * sigmoid(conf) > thresh), anchor_visible[g, n] != 0 on an anchor.
 *              Only the first N_out <= 8192 slots are looked at; M = the number of correspondences.
 *   grid       cell c = 1 << cs, cs in 2..6; gw = ((W - 1) >> cs) + 2 nodes across and gh = ((H - 1) >> cs) + 2 down; node (i, j) sits
 *              at pixel (i c, j c), Nx = i * c * 16 in 1/16 pixel.
 *   weight     a separable tent of `radius` cells (1..4), rad = radius * c * 16: wx = max(0, 1024 - (|Px - Nx| * 1024) / rad), an
 *              integer floor division of non-negatives, wy likewise, w = wx * wy <= 2^20.
 *   sums       per node Wn = sum w, Sx = sum w d.x, Sy = sum w d.y in int64 (Wn <= 2^33, |S| <= 2^51): integer sums, so the order of
 *              accumulation does not matter and nothing needs float atomics.
 *   pyramid    level l + 1 has ceil(h / 2) x ceil(w / 2) nodes, each the sum of its up-to-four children, up to 1 x 1.
 *   value      node (i, j) takes the lowest level l at which node (j >> l, i >> l) has Wn >= 1:
 *              F = (int32)llrint((double)(S * 16) / (double)Wn) per component: 1/256 pixel, one IEEE division, round half to even.
 *              Where even the 1 x 1 level is empty (M = 0, or every correspondence beyond the reach of every node) F = 0 and the level
 *              is 255.
 *   outputs    field int32 [G,F,gh,gw,2] (x, y);  level uint8 [G,F,gh,gw]: 0 own support, l > 0 filled from level l, 255 nothing;
 *              stats int32 [G,F,4] = (M, nodes at level 0, highest level used -- 255 where nothing --, 0).  Every element is written
 *              by one plain store.
 * Three launches on `stream`: a gather (one workgroup per (g, f, 16 x 16 node tile); the correspondences are quantised once per
 * workgroup and staged through LDS in chunks of 256, culled against the tile's box grown by rad; a thread owns one node and keeps its
 * three sums in registers), the pyramid (one workgroup per (g, f)) and the values.  No atomics, no host synchronisation, capture-safe;
 * writes the three outputs and the workspace only.  ctk_track_field_workspace_bytes answers G * F * 24 bytes * the nodes of all levels.
 * Before any launch: NULL a, hist_coords, field, level or stats, `visible` NULL with hist_vis or hist_conf NULL, one of anchor_coords /
 * anchor_visible without the other, a NULL workspace: CTK_E_NULL; G, N, N_out, R or F <= 0, N_out > N, N_out > 8192, f0 < 0,
 * f0 + F > 2^30, F > 65535, G > 65535, G * N > 2^26, H or W outside 1..CTK_INGEST_MAX_SIDE, cs outside 2..6, radius outside 1..4, not
 * exactly one "to" form (to < -1, to >= 0 with lag != 0 or an anchor, lag != 0 with an anchor, none of the three), to > 2^30,
 * |lag| > 2^30, anchor_frame outside 0..2^30 with an anchor, rows of a ring that would alias (F + |lag| > R; with a fixed frame the
 * span of [f0, f0 + F) and `to` > R; F > R with an anchor), sx or sy not finite or <= 0, a NaN thresh without `visible`,
 * reserved != 0, workspace_bytes below what the query answers: CTK_E_SHAPE; hist_coords, anchor_coords, field or the workspace not
 * 8-byte aligned, stats not 4-byte aligned: CTK_E_ALIGN.  Frames whose "to" frame is negative are no error: they have no
 * correspondences.  The query checks the same shapes and reads no pointer of the struct (it only looks whether an anchor is given).
 *
 * ctk_warp_field: picture j of dst = picture j of src resampled through field[j]; output pixel (x, y):
 *   cell       i = x >> cs, ax = x & (c - 1); j, ay likewise; i + 1 <= gw - 1 holds by the grid rule
 *   position   D = (c - ax)(c - ay) F[j][i] + ax (c - ay) F[j][i+1] + (c - ax) ay F[j+1][i] + ax ay F[j+1][i+1] in int64;
 *              X = x * 256 + ((D + (c * c >> 1)) >> 2 cs), an arithmetic shift; Y likewise; ix = X >> 8, fx = X & 255
 *   taps       the four taps, the CTK_WARP_FILL / CTK_WARP_EDGE borders and the blend are exactly ctk_warp_frames'.  Nothing outside
 *              the picture is read.  A zero field copies the source bit for bit; an integer-pixel constant field is a shifted copy.
 *   flow       (optional, float32 [F,H,W,2]) = (float)(X - x * 256) / 256.0f and the same for Y: exact for |F| <= 2^24
 *   pictures   F pictures of H x W, C = 3 or C = 1 channels (a mask); layouts, strides (a row holds C W or W elements, a frame H or
 *              C H rows), fill and border as in ctk_warp_args; src_frame_stride = 0 is allowed too: every picture is resampled
 *              from the one source.  src and dst must not overlap.  field int32 [F,gh,gw,2] with the grid
 *              of ctk_track_field for (H, W, cs).  dst and flow are each optional, at least one must be given; src may be NULL when
 *              dst is.
 * One launch on `stream` (a workgroup reads the nodes round its 64 x 16 output tile, whose values bound the tile's source box, stages
 * that box in 16 KiB of LDS or reads memory directly where it does not fit), no atomics, no host synchronisation, capture-safe; writes
 * dst and flow only.  Before the launch: NULL a or field, dst and flow both NULL, dst without src: CTK_E_NULL; F outside 1..65535, H
 * or W outside 1..CTK_INGEST_MAX_SIDE, C not 1 or 3, an unknown layout or border, cs outside 2..6, reserved != 0, and with dst a row
 * stride smaller than a row, a frame stride smaller than a frame (but src_frame_stride = 0), a stride above 2^40 or overlapping byte ranges of src and dst:
 * CTK_E_SHAPE; field or flow not 8-byte aligned: CTK_E_ALIGN.
 *
 * Known limits.  The weighting is zeroth order (a weighted mean of displacements, no local affine fit per node).  On a 480 x 270 picture
 * with a jittered 24 x 24 grid of points under a similarity of 1.7 degrees and 2 % (c = 16, radius 2) the field is exact to about
 * 0.05-0.14 pixel inside a covered region, biased by about 0.6 pixel in the outermost `radius` cells, where the support is one-sided,
 * and blocky across large holes: 3.2 pixels across a hole of 180 x 140 pixels.                                                    */
typedef struct ctk_track_field_args {
  int32_t G, N;               /* query groups, points per group of the history                     */
  int32_t N_out;              /* points per group that are looked at (the first N_out), <= 8192    */
  int32_t R;                  /* history rows per group                                            */
  int32_t f0, F;              /* row j of the outputs is frame f0 + j, 0 <= j < F                  */
  int32_t H, W;               /* the picture of a frame, in the pixels of the scaled positions     */
  int32_t cs;                 /* log2 of the cell, 2..6                                            */
  int32_t radius;             /* reach of a point, in cells, 1..4                                  */
  int32_t to;                 /* a fixed "to" frame, or -1                                         */
  int32_t lag;                /* "to" = f - lag, or 0                                              */
  int32_t anchor_frame;       /* the frame the anchor was taken on (with anchor_coords)            */
  float sx, sy;               /* position = coords * (sx, sy)                                      */
  float thresh;               /* visible from logits: sigmoid(vis) * sigmoid(conf) > thresh        */
  int32_t reserved;           /* 0 */
  const float* hist_coords;
  const uint8_t* visible;     /* [G,R,N], or NULL: hist_vis / hist_conf and thresh                 */
  const float* hist_vis; const float* hist_conf;
  const int32_t* first_row;   /* optional */
  const float* anchor_coords; /* [G,N,2], or NULL                                                  */
  const uint8_t* anchor_visible; /* [G,N], with anchor_coords                                      */
  int32_t* field;             /* [G,F,gh,gw,2] */
  uint8_t* level;             /* [G,F,gh,gw] */
  int32_t* stats;             /* [G,F,4] */
} ctk_track_field_args;
int ctk_track_field_workspace_bytes(const ctk_track_field_args* a, size_t* out_bytes);
int ctk_track_field(const ctk_track_field_args* a, void* workspace, size_t workspace_bytes, void* stream);

typedef struct ctk_warp_field_args {
  int32_t F, H, W;            /* pictures, and their size in pixels                                */
  int32_t C;                  /* channels: 3, or 1 (a mask)                                        */
  int32_t layout;             /* CTK_INGEST_HWC / CTK_INGEST_CHW (the same thing for C = 1)        */
  int32_t border;             /* CTK_WARP_FILL / CTK_WARP_EDGE                                     */
  int32_t cs;                 /* log2 of the field's cell, 2..6                                    */
  int32_t reserved;           /* 0 */
  uint8_t fill[4];            /* the value of a tap outside the picture, per channel               */
  int64_t src_frame_stride;   /* elements between two pictures of src; 0: one source for all       */
  int64_t src_row_stride;     /* elements between two pixel rows of src                            */
  int64_t dst_frame_stride;
  int64_t dst_row_stride;
  const int32_t* field;       /* [F,gh,gw,2], on the device                                        */
  const uint8_t* src;
  uint8_t* dst;               /* or NULL */
  float* flow;                /* [F,H,W,2], or NULL */
} ctk_warp_field_args;
int ctk_warp_field(const ctk_warp_field_args* a, void* stream);

/* ---- fit objects: which points move together, and where such a group is on other frames --------------------------------------------
 * For a caller whose tracks are on the device: ctk_fit_motion says how the camera moved and which points moved differently; this says
 * which of those points move together (split mode) and how a group of points a caller chose -- a car, a person, a boxed region --
 * has moved since the frame it was chosen on (labels mode).  Up to L robust fits per group g and frame f in [f0, f0 + F), each over a
 * sub-list of ONE list of correspondences.  The rules are stated once in csrc/objects_math.h; everything not named here is
 * ctk_fit_motion's bit for bit: positions, mix, the sample, the hypothesis, inlier, key, refit.
 *   pair       P is the source, Q the destination, which is frame f: the matrix maps the source frame onto frame f.  The source takes
 *              exactly one of ctk_track_field's three forms: a fixed frame to >= 0 (lag = 0, no anchor);  f - lag with lag >= 1
 *              (to = -1, no anchor), as in ctk_fit_motion;  an anchor (to = -1, lag = 0): anchor_coords [G,N,2] float32 (scaled by sx,
 *              sy like the history) and anchor_visible [G,N] uint8, taken by the caller on frame anchor_frame >= 0 -- how a region
 *              is followed after a ring has dropped the frame it was chosen on.  Slot n is a correspondence by ctk_track_field's
 *              pair rule: both frames are >= 0 and >= first_row[g, n] (anchor_frame counts as the source frame, so a slot released
 *              and reassigned after the anchor was taken drops out), both positions are valid and both are visible (visible [G,R,N]
 *              uint8, or sigmoid(vis) * sigmoid(conf) > thresh; anchor_visible[g, n] != 0 on an anchor).  The M correspondences are
 *              numbered in ascending n.
 *   rounds     r = 0 .. L - 1, L in 1..16.  Round r takes list_r, a sub-list of the correspondences in ascending n with M_r entries.
 *              Labels mode (`labels` int8 [G,N] given): list_r holds the correspondences whose label is r; a label outside 0..L-1
 *              (-1 by convention) belongs to no round.  Split mode (`labels` NULL): list_0 holds all correspondences, list_{r+1} is
 *              list_r without the inliers of round r's best hypothesis.  Round r samples with seed_r = seed ^ mix(r) (mix(0) = 0:
 *              round 0 uses `seed` itself) and is otherwise ctk_fit_motion's hypothesis, scoring, best and refit over list_r, with f
 *              the absolute frame number.
 *   acceptance a round whose best has fewer than min_points (1..8192) inliers fits nothing, and so does a round with no admissible
 *              hypothesis: the identity, stats (M_r, 0, -1, 0), box (0, 0, -1, -1), none of its points taken.  In split mode such a
 *              round ends the rounds: every later round reports the same M_r and nothing else.  In labels mode the rounds are
 *              independent.  Split mode's round order is by inlier count per frame (each round takes the largest group that is
 *              left), so the same object may be round 1 on one frame and round 2 on the next: split once, follow by labels.
 *   outputs    motion float32 [G,F,L,2,3]: the refit rows;  label int8 [G,F,N_out]: -1 no correspondence, r = inlier of round r's
 *              accepted best, 127 (CTK_OBJECT_NONE of csrc/objects_math.h) = a correspondence no round took;  stats int32 [G,F,L,4] = (M_r, inliers, best k,
 *              0);  box int32 [G,F,L,4] = (min Qx, min Qy, max Qx, max Qy) over the round's inliers, 1/16 pixel.  Every element is
 *              written by one plain store.
 * In split mode with the lag form and min_points = 1, round 0's matrix and stats and (label == 0) equal ctk_fit_motion's motion, stats
 * and (inlier == 1) bit for bit.
 * Only the first N_out <= N slots of a group are looked at.  One launch on `stream`, one workgroup of 256 threads per (group, frame)
 * with the correspondences and their slots in N_out * 18 bytes of LDS (split mode gathers the rows once and removes a round's inliers
 * by a stable in-place compaction; labels mode gathers them twice -- a counting and a placing pass -- and runs the rounds over disjoint
 * segments); no atomics, no host synchronisation, capture-safe; writes the four outputs only.  The cost is about the sum of the
 * scored lists times K: one ctk_fit_motion in labels mode, at most L of them in split mode.  The workspace query answers 0 and
 * `workspace` may then be NULL.  Before any launch: NULL a, hist_coords, motion, label, stats or box, `visible` NULL with hist_vis or
 * hist_conf NULL, one of anchor_coords / anchor_visible without the other: CTK_E_NULL; the shapes ctk_fit_motion refuses (G, N, N_out,
 * R or F <= 0, N_out > N, N_out > 8192, f0 < 0, f0 + F > 2^30, F > 65535, G > 65535, G * N > 2^26, model not 0 or 1, K outside 1..4096,
 * tol NaN or with T outside 1..4096, min_base NaN, negative or above 8192, sx or sy not finite or <= 0, a NaN thresh without
 * `visible`, reserved != 0), the forms ctk_track_field refuses (not exactly one source form, to < -1, to > 2^30, lag > 2^30,
 * anchor_frame outside 0..2^30 with an anchor, rows of a ring that would alias: F + lag > R; with a fixed frame the span of
 * [f0, f0 + F) and `to` > R; F > R with an anchor), a negative lag, L outside 1..16, min_points outside 1..8192, workspace_bytes
 * below what the query answers: CTK_E_SHAPE; hist_coords or anchor_coords not 8-byte aligned, motion, stats or box not 4-byte aligned:
 * CTK_E_ALIGN.  `labels` needs no alignment.  Frames whose source frame is negative are no error: they have no correspondences.  The
 * query checks the same shapes and reads no pointer of the struct (it only looks whether an anchor is given).                      */
typedef struct ctk_fit_objects_args {
  int32_t G, N;               /* query groups, points per group of the history                     */
  int32_t N_out;              /* points per group that are looked at (the first N_out), <= 8192    */
  int32_t R;                  /* history rows per group                                            */
  int32_t f0, F;              /* row j of the outputs is frame f0 + j, 0 <= j < F                  */
  int32_t to;                 /* a fixed source frame, or -1                                       */
  int32_t lag;                /* source = f - lag (>= 1), or 0                                     */
  int32_t anchor_frame;       /* the frame the anchor was taken on (with anchor_coords)            */
  int32_t L;                  /* rounds (objects), 1..16                                           */
  int32_t min_points;         /* a fit needs this many inliers, 1..8192                            */
  int32_t model;              /* 0 translation, 1 similarity                                       */
  int32_t K;                  /* hypotheses per round, 1..4096                                     */
  uint32_t seed;
  float tol;                  /* inlier bound, pixels (max norm); T = rint(tol * 16) in 1..4096    */
  float min_base;             /* a similarity's sample pair is at least this far apart, pixels     */
  float sx, sy;               /* position = coords * (sx, sy)                                      */
  float thresh;               /* visible from logits: sigmoid(vis) * sigmoid(conf) > thresh        */
  int32_t reserved;           /* 0 */
  const float* hist_coords;
  const uint8_t* visible;     /* [G,R,N], or NULL: hist_vis / hist_conf and thresh                 */
  const float* hist_vis; const float* hist_conf;
  const int32_t* first_row;   /* optional */
  const float* anchor_coords; /* [G,N,2], or NULL                                                  */
  const uint8_t* anchor_visible; /* [G,N], with anchor_coords                                      */
  const int8_t* labels;       /* [G,N]: labels mode; NULL: split mode                              */
  float* motion;              /* [G,F,L,2,3] */
  int8_t* label;              /* [G,F,N_out] */
  int32_t* stats;             /* [G,F,L,4] */
  int32_t* box;               /* [G,F,L,4] */
} ctk_fit_objects_args;
int ctk_fit_objects_workspace_bytes(const ctk_fit_objects_args* a, size_t* out_bytes);
int ctk_fit_objects(const ctk_fit_objects_args* a, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fit planes / warp planes: planar surfaces under perspective, and pictures resampled under 3 x 3 matrices ---------------------
 * For a caller whose tracks are on the device and whose object is a planar surface seen under perspective -- a screen, a wall, a sign,
 * a pitch --, which a similarity (ctk_fit_objects) slides and shears on: ctk_fit_planes fits up to L homographies per group g and frame
 * f in [f0, f0 + F), and ctk_warp_planes resamples pictures under such matrices: a picture pinned onto the surface, or the surface
 * shown upright.  The rules are stated once in csrc/plane_math.h.
 *
 * ctk_fit_planes.  The frame of the call is ctk_fit_objects' labels mode; everything not named here is ctk_fit_objects' and
 * ctk_fit_motion's bit for bit: positions (1/16 pixel), the pair rule with its three source forms, first_row, `visible` or the logits
 * with thresh, N_out <= 8192, mix, the seed of a round, the key ("most inliers, then the lowest k"), min_points, the labels.
 *   lists      `labels` int8 [G,N] given: list_r holds the correspondences labelled r, L in 1..16 (CTK_PLANES_MAX, csrc/plane_math.h);
 *              `labels` NULL: L must be 1 and list_0 holds every correspondence.  There is no split mode.  The rounds are independent.
 *   inverse    0 / 1.  With 1 the roles of P (source) and Q (frame f) are swapped after staging: the matrix maps frame f onto the
 *              source frame, which is what a backward warp needs.  No matrix is inverted anywhere.
 *   sample     hypothesis k of a list with M_r >= 4 entries: h_t = mix(seed_r ^ mix(f * 0x9e3779b9 + 4k + t)), t = 0..3;
 *              i_t = h_t % (M_r - t), then bumped past the earlier indices taken in ascending order: four distinct indices; f is the
 *              absolute frame number.
 *   admissible integers only.  p_t = P_{i_t} - P_{i_0}, q_t likewise; d_abc = (p_b - p_a) x (p_c - p_a) over abc = 123, 023, 013, 012
 *              (|d| <= 2^37), e_abc of the q likewise.  Admissible iff every |d| and every |e| is at least base2 (ctk_fit_motion's,
 *              from min_base) and at least 1, and every d has the sign of its e: no three sample points are near a line,
 *              and the quad keeps its orientation.
 *   matrix     in double, one rounded operation per step, no contraction, no pivoting: the projective basis B_P = [l1 p1 | l2 p2 |
 *              l3 p3] on homogeneous (x, y, 1) with (l1, l2, l3) = (d_023, -d_013, d_012), every entry (double)l * (double)coordinate;
 *              B_Q from the e and q likewise; H' = B_Q adj(B_P), each cofactor a b - c d, each product entry (a b + c d) + e f; all
 *              nine entries divided by H'[2][2].  An entry that is then not finite makes the hypothesis inadmissible.
 *   inlier     u = P_m - P_{i_0}, w = Q_m - Q_{i_0} (exact in double): X = (h00 ux + h01 uy) + h02, Y and Z likewise; inlier iff Z > 0
 *              and |X - wx Z| <= T Z and |Y - wy Z| <= T Z, T = ctk_fit_motion's T (from tol).
 *   refit      over the inliers of the best, independent of the order of accumulation, no float atomics: an integer max of |u|, |w|
 *              gives e, its bit length (>= 1); coordinates are scaled by 2^-e into (-1, 1); the 23 sums of the normal equations of
 *              x h00 + y h01 + h02 - xX h20 - yX h21 = X and its twin for Y (h22 = 1) are each a sum of llrint(term * 2^44) in int64
 *              (below 2^59); the 8 x 8 system is solved by the square-root-free Cholesky N = L D L^T in a stated loop order (a
 *              division is one IEEE operation on every machine; that is why it is not the square-root form), and the normalisation
 *              and the centring are undone by stated products whose factors are powers of two and P_{i_0} / 16, all exact.  The output
 *              is (float) of that 3 x 3 matrix in pixels; it is not re-normalised: it is the matrix whose centred form has h22 = 1.
 *              A pivot <= 0 or not finite, or a solution that is not finite, falls back to the best hypothesis' own four-point
 *              matrix, moved to pixels the same way (stats[3] = 1).
 *   outputs    homography float32 [G,F,L,3,3]: (X, Y, Z) = H (x, y, 1) in pixels, the identity where nothing is fitted;  label int8
 *              [G,F,N_out]: -1 / r / 127 as ctk_fit_objects;  stats int32 [G,F,L,4] = (M_r, inliers, best k or -1, 1 if the refit
 *              fell back else 0);  box int32 [G,F,L,4] = (min x, min y, max x, max y) of the round's inliers ON FRAME f (with either
 *              value of inverse), 1/16 pixel, (0, 0, -1, -1) where nothing is fitted.  Every element is written by one plain store.
 * One launch on `stream`, one workgroup of 256 threads per (group, frame) with the correspondences and their slots in N_out * 18 bytes
 * of LDS; no atomics, no host synchronisation, capture-safe; writes the four outputs only.  The workspace query answers 0 and
 * `workspace` may be NULL.  Before any launch: NULL a, hist_coords, homography, label, stats or box, `visible` NULL with hist_vis or
 * hist_conf NULL, one of anchor_coords / anchor_visible without the other: CTK_E_NULL; every shape ctk_fit_objects refuses but `model`
 * (this struct has none), `inverse` outside 0..1, `labels` NULL with L != 1: CTK_E_SHAPE; hist_coords or anchor_coords not 8-byte
 * aligned, homography, stats or box not 4-byte aligned: CTK_E_ALIGN.  The query checks the same shapes and reads no pointer of the
 * struct (it only looks whether an anchor and labels are given).
 *
 * ctk_warp_planes.  Picture j of dst (H x W) is picture j of src (Hs x Ws, which may differ) under matrices[j], float32 3 x 3, which
 * maps an OUTPUT pixel to a SOURCE position; pixel centres are at integers.  src_frame_stride = 0: one source for all pictures.
 *   coordinate per pixel in double, one rounded operation per step: Xh = (m00 x + m01 y) + m02, Yh and Zh likewise.  The pixel is
 *              OUTSIDE iff the matrix has a non-finite entry, or !(Zh > 0), or r = 1.0 / Zh, sx = Xh r, sy = Yh r has
 *              !(|sx| <= 1048576 && |sy| <= 1048576).  Otherwise X = llrint(sx * 256.0), ix = X >> 8, fx = X & 255; the taps and the
 *              blend are ctk_warp_frames' exactly.  The identity on equal sizes copies bit for bit.
 *   borders    CTK_WARP_FILL and CTK_WARP_EDGE as before; an outside pixel takes `fill` under both.  CTK_WARP_KEEP = 2 (csrc/
 *              plane_math.h): a pixel that is outside, or that has a tap outside the source, is NOT WRITTEN -- how a picture is drawn
 *              into frames in place: dst may be the frames themselves; src, the picture, never overlaps them.  Bytes the rule does
 *              not write keep their value, pitch padding included.
 *   pictures   C = 3 or 1, layouts and strides as in struct ctk_warp_field_args: a row holds C W or W elements, a frame H or C H rows.
 * One launch on `stream` (warp.hip's shape: a 64 x 16 tile per workgroup, the tile's source box staged in 16 KiB of LDS where the four
 * tile corners bound it and it fits, memory read directly otherwise; under CTK_WARP_KEEP a tile whose box misses the source ends
 * early, no other tile is culled), no atomics, no host synchronisation, capture-safe; writes dst only..  Before the launch: NULL a,
 * matrices, src or dst: CTK_E_NULL; F outside 1..65535, H, W, Hs or Ws outside 1..CTK_INGEST_MAX_SIDE, C not 1 or 3, an unknown layout
 * or border, reserved != 0, a row stride smaller than a row, a frame stride smaller than a frame (but src_frame_stride = 0), a stride
 * above 2^40 or overlapping byte ranges of src and dst: CTK_E_SHAPE; matrices not 4-byte aligned: CTK_E_ALIGN.
 *
 * Known limits.  No split mode for planes, no affine model, no homography path in ctk_smooth_path; no alpha blending and no
 * anti-aliased edges where a picture is drawn, bilinear taps only (no bicubic); the refit is one algebraic least-squares step (no
 * Sampson or iterated refit); no lens distortion. ctk_lens_frames / ctk_lens_points correct a lens in front of
 * the fit ("lens" above). */
typedef struct ctk_fit_planes_args {
  int32_t G, N;               /* query groups, points per group of the history                     */
  int32_t N_out;              /* points per group that are looked at (the first N_out), <= 8192    */
  int32_t R;                  /* history rows per group                                            */
  int32_t f0, F;              /* row j of the outputs is frame f0 + j, 0 <= j < F                  */
  int32_t to;                 /* a fixed source frame, or -1                                       */
  int32_t lag;                /* source = f - lag (>= 1), or 0                                     */
  int32_t anchor_frame;       /* the frame the anchor was taken on (with anchor_coords)            */
  int32_t L;                  /* rounds (planes), 1..16; 1 without labels                          */
  int32_t min_points;         /* a fit needs this many inliers, 1..8192                            */
  int32_t inverse;            /* 0: source -> frame f; 1: frame f -> source                        */
  int32_t K;                  /* hypotheses per round, 1..4096                                     */
  uint32_t seed;
  float tol;                  /* inlier bound, pixels (max norm); T = rint(tol * 16) in 1..4096    */
  float min_base;             /* twice a sample triangle's area is at least min_base^2, pixels     */
  float sx, sy;               /* position = coords * (sx, sy)                                      */
  float thresh;               /* visible from logits: sigmoid(vis) * sigmoid(conf) > thresh        */
  int32_t reserved;           /* 0 */
  const float* hist_coords;
  const uint8_t* visible;     /* [G,R,N], or NULL: hist_vis / hist_conf and thresh                 */
  const float* hist_vis; const float* hist_conf;
  const int32_t* first_row;   /* optional */
  const float* anchor_coords; /* [G,N,2], or NULL                                                  */
  const uint8_t* anchor_visible; /* [G,N], with anchor_coords                                      */
  const int8_t* labels;       /* [G,N], or NULL: one list of every correspondence (L = 1)          */
  float* homography;          /* [G,F,L,3,3] */
  int8_t* label;              /* [G,F,N_out] */
  int32_t* stats;             /* [G,F,L,4] */
  int32_t* box;               /* [G,F,L,4] */
} ctk_fit_planes_args;
int ctk_fit_planes_workspace_bytes(const ctk_fit_planes_args* a, size_t* out_bytes);
int ctk_fit_planes(const ctk_fit_planes_args* a, void* workspace, size_t workspace_bytes, void* stream);

typedef struct ctk_warp_planes_args {
  int32_t F, H, W;            /* pictures, and the size of a picture of dst in pixels              */
  int32_t Hs, Ws;             /* the size of a picture of src                                      */
  int32_t C;                  /* channels: 3, or 1 (a mask)                                        */
  int32_t layout;             /* CTK_INGEST_HWC / CTK_INGEST_CHW (the same thing for C = 1)        */
  int32_t border;             /* CTK_WARP_FILL / CTK_WARP_EDGE / CTK_WARP_KEEP                     */
  int32_t reserved;           /* 0 */
  uint8_t fill[4];            /* the value of a tap or a pixel outside, per channel                */
  int64_t src_frame_stride;   /* elements between two pictures of src; 0: one source for all       */
  int64_t src_row_stride;     /* elements between two pixel rows of src                            */
  int64_t dst_frame_stride;
  int64_t dst_row_stride;
  const float* matrices;      /* [F,3,3], on the device                                            */
  const uint8_t* src;
  uint8_t* dst;
} ctk_warp_planes_args;
int ctk_warp_planes(const ctk_warp_planes_args* a, void* stream);

/* ---- fit epipolar: one fundamental matrix per frame, and the points that do not obey it -------------------------------------------------
 * For a caller whose tracks are on the device and whose camera TRANSLATES through a scene with depth: near and far points then move
 * differently in the picture, a similarity (ctk_fit_motion, ctk_fit_objects) or a homography (ctk_fit_planes) calls the nearer half of
 * the static scene outliers, and nothing tells a point that moves by itself from one that only shows parallax.  ctk_fit_epipolar fits
 * ONE fundamental matrix F per group g and frame f in [f0, f0 + F) robustly to the correspondences between a source frame and frame f:
 * every static point satisfies (Q, 1)^T F (P, 1) = 0 at any depth (P on the source frame, Q on frame f), a point that moves on its own
 * generally does not.  The rules are stated once in csrc/epipolar_math.h.
 *
 * The frame of the call is ctk_fit_planes' without labels; everything not named here is ctk_fit_motion's and ctk_fit_planes' bit for
 * bit: positions (1/16 pixel), the pair rule with its three source forms, first_row, `visible` or the logits with thresh, N_out <=
 * 8192, mix, T from tol, the key ("most inliers, then the lowest k"), ctk_plane_solve.  There are no lists and no rounds by label.
 *   fit list   `mask` int8 [G,N] given: a correspondence whose byte is nonzero may be sampled and refitted on; NULL: every
 *              correspondence may.  M = how many.  Every correspondence, masked or not, is classified and gets an error.
 *   sample     hypothesis k over M >= 8: h_t = mix(seed ^ mix(f * 0x9e3779b9 + 8k + t)), t = 0..7; i_t = h_t % (M - t), then bumped past
 *              the earlier indices taken in ascending order: eight distinct indices; f is the absolute frame number.
 *   admissible integers only.  Both frames are centred on the anchor pair (P_{i_0}, Q_{i_0}); each of the other seven offsets must have a
 *              squared length >= max(base2', 1) on both frames, base2' = b * b with b = rint(min_base * 16): every sample point lies at
 *              least min_base pixels from the anchor (ctk_fit_motion's base2; a squared length in 1/16 pixel).
 *   matrix     in double, one rounded operation per step, no contraction, no square root.  The anchor pair is a correspondence at both
 *              origins, so F[2][2] = 0 exactly.  e = the bit length of the largest |component| of the seven offset pairs (>= 1);
 *              offsets are scaled by 2^-e into (-1, 1), exactly.  A sample point gives the row (X x, X y, X, Y x, Y y, Y, x, y) for the
 *              entries (F00 .. F21); the null vector of the 7 x 8 system comes from Gaussian elimination with complete pivoting (the
 *              largest |entry| of the remaining block; ties: the lowest row, then the lowest column), back substitution with the free
 *              unknown 1 in one stated loop order, the permutation undone.  A pivot that is 0 or not finite, or a result that is
 *              not finite, makes the hypothesis inadmissible.  The entries are divided by the one of largest magnitude, j* (the
 *              lowest index on ties), which so becomes exactly 1.
 *   inlier     the Sampson test without a division or a root, on the scaled offsets u, w: a = F (u, 1), b = F^T (w, 1), r = (w, 1) . a,
 *              g = ((a0 a0 + a1 a1) + b0 b0) + b1 b1, Ts = T 2^-e: inlier iff g > 0 and r r <= (Ts Ts) g.
 *   refit      over the inliers among the fit list, independent of the order of accumulation, no float atomics: e' = the bit length of
 *              the inliers' integer reach; a = (X x, X y, X, Y x, Y y, Y, x, y, 1) in the scale e'; the 45 distinct sums of a a^T are
 *              each a sum of llrint(term * 2^44) in int64 (below 2^58); row and column j* are deleted and the 8 x 8 system N h =
 *              -column j* is solved by ctk_fit_planes' square-root-free L D L^T; F_{j*} = 1.  If it fails the hypothesis' own matrix
 *              stays, moved to the scale e' by exact powers of two (stats[3] bit 0).
 *   second     every entry of the fit list is classified again under the refitted matrix, and the refit is run once more over those
 *   round      inliers with j* = its entry of largest magnitude; if that fails the first refit's matrix stays (stats[3] bit 1).  This
 *              round is what keeps a noisy minimal sample from dropping static points.
 *   outputs    fundamental float32 [G,F,3,3] in pixels: (X, Y, 1) F (x, y, 1)^T = 0 for a static point at (x, y) on the source frame
 *              and (X, Y) on frame f: S_Q^T F S_P by stated products with powers of two and the anchor / 16, all exact but the two
 *              sums per entry of the last column and row; (float) of that, not renormalised.  label int8 [G,F,N_out]: -1 not on
 *              both frames, 0 violates the matrix, 1 consistent with it (the same test under the final matrix, for masked and unmasked
 *              correspondences alike).  error float32 [G,F,N_out]: the squared Sampson distance in pixels^2, (float)(((r r) / g)
 *              2^(2e'-8)), one division and one exact scaling; +inf (and label 0) where !(g > 0); -1 where there is no
 *              correspondence.  stats int32 [G,F,4] = (M, inliers among the fit list under the final matrix, best k or -1, the
 *              fall-back bits).  Every element is written by one plain store.
 *   no fit     M < 8, no admissible hypothesis, or fewer than min_points inliers of the best hypothesis: fundamental is all zero,
 *              every correspondence has label 0 and error -1, stats = (M, 0, -1, 0).
 * One launch on `stream`, one workgroup of 256 threads per (group, frame) with the correspondences and their slots in N_out * 18 bytes
 * of LDS (a lane per hypothesis walks the list by LDS broadcast; K above 256 takes further passes; thread 0 solves); no atomics, no
 * host synchronisation, capture-safe; writes the four outputs only.  The workspace query answers 0 and `workspace` may be NULL.  Before
 * any launch: NULL a, hist_coords, fundamental, label, error or stats, `visible` NULL with hist_vis or hist_conf NULL, one of
 * anchor_coords / anchor_visible without the other: CTK_E_NULL; every shape ctk_fit_planes refuses but L and inverse (this struct has
 * neither), min_points outside 8..8192: CTK_E_SHAPE; hist_coords or anchor_coords not 8-byte aligned, fundamental, error or stats not
 * 4-byte aligned: CTK_E_ALIGN.  The query checks the same shapes and reads no pointer of the struct (it only looks whether an anchor
 * is given).
 *
 * Known limits.  F is not unique without parallax -- a planar scene, a camera that only rotates, a static camera: the labels then
 * still mean "consistent with SOME camera motion", and a caller tells by comparing with ctk_fit_planes' inliers.  A point that moves
 * along its own epipolar line is not seen by any F.  No rank-2 enforcement; one algebraic refit per round (no iterated or Sampson-
 * weighted refit); no lens distortion; no essential matrix and no pose decomposition. ctk_lens_frames / ctk_lens_points correct a lens in front of
 * the fit ("lens" above). */
typedef struct ctk_fit_epipolar_args {
  int32_t G, N;               /* query groups, points per group of the history                     */
  int32_t N_out;              /* points per group that are looked at (the first N_out), <= 8192    */
  int32_t R;                  /* history rows per group                                            */
  int32_t f0, F;              /* row j of the outputs is frame f0 + j, 0 <= j < F                  */
  int32_t to;                 /* a fixed source frame, or -1                                       */
  int32_t lag;                /* source = f - lag (>= 1), or 0                                     */
  int32_t anchor_frame;       /* the frame the anchor was taken on (with anchor_coords)            */
  int32_t min_points;         /* a fit needs this many inliers of its best hypothesis, 8..8192     */
  int32_t K;                  /* hypotheses, 1..4096                                               */
  uint32_t seed;
  float tol;                  /* Sampson bound, pixels; T = rint(tol * 16) in 1..4096              */
  float min_base;             /* a sample point lies at least this far from the anchor, pixels     */
  float sx, sy;               /* position = coords * (sx, sy)                                      */
  float thresh;               /* visible from logits: sigmoid(vis) * sigmoid(conf) > thresh        */
  int32_t reserved;           /* 0 */
  const float* hist_coords;
  const uint8_t* visible;     /* [G,R,N], or NULL: hist_vis / hist_conf and thresh                 */
  const float* hist_vis; const float* hist_conf;
  const int32_t* first_row;   /* optional */
  const float* anchor_coords; /* [G,N,2], or NULL                                                  */
  const uint8_t* anchor_visible; /* [G,N], with anchor_coords                                      */
  const int8_t* mask;         /* [G,N], or NULL: every correspondence may be fitted on             */
  float* fundamental;         /* [G,F,3,3] */
  int8_t* label;              /* [G,F,N_out] */
  float* error;               /* [G,F,N_out] */
  int32_t* stats;             /* [G,F,4] */
} ctk_fit_epipolar_args;
int ctk_fit_epipolar_workspace_bytes(const ctk_fit_epipolar_args* a, size_t* out_bytes);
int ctk_fit_epipolar(const ctk_fit_epipolar_args* a, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fit pose: how the camera turned, where it went, and how deep every point is ---------------------------------------------------------
 * For a caller who knows the camera's intrinsics: ctk_fit_epipolar leaves a fundamental matrix F and a label per point in picture
 * coordinates; ctk_fit_pose turns them, per group g and frame f in [f0, f0 + F), into the 3-D product: the rotation R and the unit
 * translation t that map source-camera coordinates to frame-f coordinates, X_f = R X_s + t, and the depth of every correspondence on
 * both frames.  fx, fy, cx, cy describe ONE pinhole camera in raw-video pixels (the pixels of coords * (sx, sy)), the same on both
 * frames.  The rules are stated once in csrc/pose_math.h.
 *
 * The frame of the call is ctk_fit_epipolar's; everything not named here is its own bit for bit: positions (1/16 pixel), the pair rule
 * with its three source forms, first_row, `visible` or the logits with thresh, N_out <= 8192, the convention (Q, 1)^T F (P, 1) = 0 with
 * P on the source frame and Q on frame f, ctk_plane_solve.  The gather decides what a correspondence is -- call it with the source
 * form, first_row, visibility and scale the fundamental matrices were fitted with --; `label` only decides the fit list.
 *   fit list   the M correspondences whose byte of `label` int8 [G,F,N_out] is 1 and, with `mask` int8 [G,N] given, whose mask byte is
 *              nonzero.  Every correspondence, on the fit list or not, gets its depths.
 *   rays       x = ((Px / 16 - cx) / fx, (Py / 16 - cy) / fy, 1) on the source frame, y likewise on frame f, in double: one division
 *              per component.
 *   E          from `fundamental` float32 [G,F,3,3]: E = K^T F K expanded into stated products and sums, then divided by its entry of
 *              largest magnitude (the lowest index on ties).  F counts as no fit when it is all zero (ctk_fit_epipolar's no-fit
 *              row) or has an entry that is not finite.
 *   decompose  closed form, no SVD (Horn 1990): h = tr(E E^T) / 2, TT = h I - E E^T = t t^T up to scale; from its largest diagonal
 *              entry i (> 0 and finite) t0 = TT[i] * rsqrt(TT[i][i]); with the cofactor matrix C of E and W = [t0]x E:
 *              Ra = (C - W) / (t0 . t0), Rb = (C + W) / (t0 . t0); tn = t0 * rsqrt(t0 . t0).  Four candidates k = 0..3: (Ra, tn),
 *              (Ra, -tn), (Rb, tn), (Rb, -tn).  rsqrt is eight Newton steps of products and differences on a mantissa scaled by an
 *              exact even power of two: no library root is taken anywhere.  Every R is orthogonalised by four steps of
 *              R = 0.5 R (3 I - R^T R); a candidate whose determinant is then not > 0, or with an entry that is not finite as
 *              float32, is skipped.
 *   depths     of a correspondence under (R, t), a = R x: den = (a.a)(y.y) - (a.y)^2, z_s = ((a.y)(y.t) - (a.t)(y.y)) / den,
 *              z_f = ((a.a)(y.t) - (a.y)(a.t)) / den: the least-squares solution of z_s a + t = z_f y; +inf both where !(den > 0).
 *   cheirality each candidate counts the fit-list entries with z_s > 0 and z_f > 0; the largest count wins, the lowest k on ties.
 *   refine     two Gauss-Newton rounds on the Sampson error over the fit list, independent of the order of accumulation, no float
 *              atomics: per entry the residual r = y . (E x), ctk_fit_epipolar's four-term gradient sum g under E = [t]x R, and the
 *              derivatives Jw = (R x) x (y x t), Jt = (R x) x y; v = (Jw, Jt, r).  An entry takes part iff g > 0 and every
 *              v_i v_i <= 16 g, which bounds every term by 16: the 28 sums of llrint(((v_i v_j) / g) 2^44) in int64 stay below 2^61.
 *              With n t t^T on the translation block as the gauge (n entries take part) and an identity block that pads the system
 *              to 8 x 8, ctk_fit_planes' square-root-free L D L^T gives (dw, dt); R = polar((I + [dw]x) R),
 *              t = (t + dt) * rsqrt(|t + dt|^2).  A round whose solve or update fails keeps its pose (stats[3] bit 0 / 1); an entry
 *              that was left out sets stats[3] bit 2.
 *   outputs    pose float32 [G,F,3,4] = (R | t), the (float) of the doubles.  depth float32 [G,F,N_out,2] = (z_s, z_f) in units of
 *              the baseline, for EVERY correspondence: a point that moves by itself gets a depth that means nothing, and `label`
 *              says so; negative depths are written as they come; a NaN is the quiet NaN 0x7FC00000.  stats int32 [G,F,4] = (M,
 *              entries of the fit list with both depths > 0 under the final pose, the chosen k or -1, the bits).  Every element is
 *              written by one plain store.
 *   no fit     F is no fit, M < min_points, the decomposition fails, or no candidate is left: pose = (I | 0), every correspondence's
 *              depth is the quiet NaN 0x7FC00000, stats = (M, 0, -1, 0).  A slot without a correspondence has NaN depths in either
 *              case.
 * One launch on `stream`, one workgroup of 256 threads per (group, frame) with the correspondences and their slots in N_out * 18 bytes
 * of LDS (thread 0 decomposes and solves; the votes and the sums are reduced by wave shuffles and through LDS); no atomics, no host
 * synchronisation, capture-safe; `fundamental` and `label` are only read, the three outputs are all that is written.  The workspace
 * query answers 0 and `workspace` may be NULL.  Before any launch: NULL a, hist_coords, fundamental, label, pose, depth or stats,
 * `visible` NULL with hist_vis or hist_conf NULL, one of anchor_coords / anchor_visible without the other: CTK_E_NULL; every shape
 * ctk_fit_epipolar refuses for the fields both structs have, min_points outside 8..8192, fx or fy not finite or not > 0, cx or cy not
 * finite: CTK_E_SHAPE; hist_coords or anchor_coords not 8-byte aligned, fundamental, pose, depth or stats not 4-byte aligned:
 * CTK_E_ALIGN.  The query checks the same shapes and reads no pointer of the struct (it only looks whether an anchor is given).
 *
 * Known limits.  The scale is unknown: |t| = 1, depths are in baselines, and the unit changes from frame to frame.  One pinhole
 * camera, no lens distortion.  No parallax means no pose -- a camera that only turns, a planar scene, a static camera: the caller
 * tells by stats[1] / stats[0] and by comparing with ctk_fit_planes' inliers.  Two frames at a time: no bundle adjustment over more,
 * no chaining of poses.  ctk_lens_frames / ctk_lens_points correct a lens in front of the fit ("lens" above). */
typedef struct ctk_fit_pose_args {
  int32_t G, N;               /* query groups, points per group of the history                     */
  int32_t N_out;              /* points per group that are looked at (the first N_out), <= 8192    */
  int32_t R;                  /* history rows per group                                            */
  int32_t f0, F;              /* row j of the inputs and outputs is frame f0 + j, 0 <= j < F       */
  int32_t to;                 /* a fixed source frame, or -1                                       */
  int32_t lag;                /* source = f - lag (>= 1), or 0                                     */
  int32_t anchor_frame;       /* the frame the anchor was taken on (with anchor_coords)            */
  int32_t min_points;         /* a pose needs this many entries on its fit list, 8..8192           */
  float fx, fy, cx, cy;       /* the pinhole camera, raw-video pixels                              */
  float sx, sy;               /* position = coords * (sx, sy)                                      */
  float thresh;               /* visible from logits: sigmoid(vis) * sigmoid(conf) > thresh        */
  int32_t reserved;           /* 0 */
  const float* hist_coords;
  const uint8_t* visible;     /* [G,R,N], or NULL: hist_vis / hist_conf and thresh                 */
  const float* hist_vis; const float* hist_conf;
  const int32_t* first_row;   /* optional */
  const float* anchor_coords; /* [G,N,2], or NULL                                                  */
  const uint8_t* anchor_visible; /* [G,N], with anchor_coords                                      */
  const int8_t* mask;         /* [G,N], or NULL: every correspondence labelled 1 is fitted on      */
  const float* fundamental;   /* [G,F,3,3], as ctk_fit_epipolar wrote it; read only                */
  const int8_t* label;        /* [G,F,N_out], as ctk_fit_epipolar wrote it; read only              */
  float* pose;                /* [G,F,3,4] */
  float* depth;               /* [G,F,N_out,2] */
  int32_t* stats;             /* [G,F,4] */
} ctk_fit_pose_args;
int ctk_fit_pose_workspace_bytes(const ctk_fit_pose_args* a, size_t* out_bytes);
int ctk_fit_pose(const ctk_fit_pose_args* a, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fit resection: the camera's pose against a fixed 3-D structure, every frame in ONE unit ----------------------------------------------
 * ctk_fit_pose gives every frame a pose in a unit of its own (|t| = 1).  ctk_fit_resection fits the camera of group g and frame f in
 * [f0, f0 + F) against points whose 3-D positions are KNOWN -- `structure`, in the coordinates of the source camera and in one unit,
 * for instance the depths ctk_fit_pose gave for one pinned pair of frames, times their rays -- so that every pose of every call is in
 * that one unit and coordinate system: X_f = R X_source + t.  The rules are stated once in csrc/resection_math.h.
 *
 * The frame of the call is ctk_fit_pose's; everything not named here is its own bit for bit: positions (1/16 pixel), the pair rule
 * with its three source forms, first_row, `visible` or the logits with thresh, N_out <= 8192, the four intrinsics, rays,
 * ctk_plane_solve, the polar steps.  The gather decides what a correspondence is; only the position Q on frame f is then used.
 *   fit list   the correspondences whose byte of `valid` int8 [G,N] is nonzero and whose three floats of `structure` float32 [G,N,3]
 *              are finite, in ascending n.  The first 4096 take part (M of them; an LDS limit), more set stats[3] bit 3.
 *   project    X' = R X + t; behind the camera (!(Z' > 0)) the error is +inf; else p = (fx X'/Z' + cx, fy Y'/Z' + cy) (one division,
 *              iz = 1 / Z', per projection) and the error
 *              e = (px - Qx/16)^2 + (py - Qy/16)^2 in px^2 (a NaN counts as +inf); within tol iff e <= tol^2: no root is taken.
 *   seed       `seed_pose` float32 [G,F,3,4] = (R0 | t0), only read.  A seed with an entry that is not finite, or whose R0 has no
 *              determinant > 0 after the four polar steps (an all-zero seed), counts as (I | 0).
 *   candidates every candidate shares R0 or I and differs in one scalar, so a = R0 X is formed once per entry and a candidate is
 *              X' = a + s t0.  k < hypotheses (1..1024): the seeded generator of ctk_fit_motion picks an entry of the fit list, and
 *              s is the least-squares scale of lambda y = a + s t0 for its ray y, a 2 x 2 closed form; an s that is not finite or
 *              not > 0 is skipped.  Then the fixed candidates k = hypotheses: (R0, t0), k + 1: (R0, 0), k + 2: (I, 0).
 *   score      an integer count of fit-list entries within tol; the largest wins, the lowest k on ties; fewer than min_points
 *              (6..8192): no fit.
 *   still      every structure point with a correspondence (beyond the list cap too; at least one) sits where it sat on the source
 *              frame, Q = P in 1/16 pixel: as far as the tracks tell the frame IS the source frame.  Then only (I, 0) is scored and no
 *              round is run: with min_points entries within tol the pose is exactly (I | 0) and stats[2] = hypotheses + 2; stats[3]
 *              bit 5 is set either way.  (A refit there could only follow the float32 rounding of the structure.)
 *   refit      three Gauss-Newton rounds on the reprojection error over the entries within tol under the round's pose, independent of
 *              the order of accumulation, no float atomics: per entry and residual component v = (J (6), r); with
 *              c2 = 256 (fx^2 + fy^2) an entry takes part iff every v_i^2 <= 16 c2 (else stats[3] bit 2), which bounds every term by
 *              16: the 28 sums of llrint(((v_i v_j) (1 / c2)) 2^44) in int64 over at most 4096 entries x 2 stay below 2^61.  An identity
 *              block pads the 6 x 6 system to the 8 x 8 of ctk_fit_planes' square-root-free L D L^T; R = polar((I + [dw]x) R),
 *              t = t + dt; no gauge, the structure fixes the scale.  A round with fewer than 6 entries, or whose solve or update
 *              fails, keeps its pose (stats[3] bits 0 / 1 / 4 for rounds 1 / 2 / 3).
 *   outputs    pose float32 [G,F,3,4] = (R | t).  label int8 [G,F,N_out]: -1 no correspondence or the point is not in the structure,
 *              0 outside tol, behind the camera, or there is no fit, 1 within tol; entries beyond the list cap are classified too.
 *              error float32 [G,F,N_out]: e, -1 where the label is -1 or there is no fit.  stats int32 [G,F,4] = (M, slots labelled
 *              1 under the final pose, the winning k or -1, the bits: 0 / 1 / 4 a round fell back, 2 an entry was left out, 3 the list
 *              cap dropped entries, 5 the frame is still).  Every element is written by one plain store.
 *   no fit     pose = (I | 0), stats = (M, 0, -1, bits).
 * One launch on `stream`, one workgroup of 256 threads per (group, frame) with the fit list in min(N_out, 4096) * 34 bytes of LDS
 * (thread 0 orthogonalises and solves; counts by ballots, sums by wave shuffles and through LDS); no atomics, no host
 * synchronisation, capture-safe; `structure`, `valid` and `seed_pose` are only read.  The workspace query answers 0 and `workspace`
 * may be NULL.  Before any launch: NULL a, hist_coords, structure, valid, seed_pose, pose, label, error or stats, `visible` NULL
 * with hist_vis or hist_conf NULL, one of anchor_coords / anchor_visible without the other: CTK_E_NULL; every shape ctk_fit_pose
 * refuses for the fields both structs have (min_points from 6 on), hypotheses outside 1..1024, tol not finite or not > 0:
 * CTK_E_SHAPE; hist_coords or anchor_coords not 8-byte aligned, structure, seed_pose, pose, error or stats not 4-byte aligned:
 * CTK_E_ALIGN.  The query checks the same shapes and reads no pointer of the struct (it only looks whether an anchor is given).
 *
 * Known limits.  The unit is the structure's (the baseline of the pair it was reconstructed from).  A structure lives as long as
 * enough of its points stay tracked; ctk_fit_structure (below) adds points to it.  The candidates come from the seed: a seed whose rotation is far off
 * finds no fit (no minimal P3P solver).  One pinhole camera, no lens distortion.  No bundle adjustment: the structure is not refined. ctk_lens_frames / ctk_lens_points correct a lens in front of
 * the fit ("lens" above).  ctk_fit_p3p (below) is the entry point without a seed: its candidates come from three points each. */
typedef struct ctk_fit_resection_args {
  int32_t G, N;               /* query groups, points per group of the history                     */
  int32_t N_out;              /* points per group that are looked at (the first N_out), <= 8192    */
  int32_t R;                  /* history rows per group                                            */
  int32_t f0, F;              /* row j of the inputs and outputs is frame f0 + j, 0 <= j < F       */
  int32_t to;                 /* a fixed source frame, or -1                                       */
  int32_t lag;                /* source = f - lag (>= 1), or 0                                     */
  int32_t anchor_frame;       /* the frame the anchor was taken on (with anchor_coords)            */
  int32_t min_points;         /* a fit needs this many entries within tol, 6..8192                 */
  int32_t hypotheses;         /* sampled candidates, 1..1024                                       */
  uint32_t seed;              /* of the generator                                                  */
  float fx, fy, cx, cy;       /* the pinhole camera, raw-video pixels                              */
  float sx, sy;               /* position = coords * (sx, sy)                                      */
  float thresh;               /* visible from logits: sigmoid(vis) * sigmoid(conf) > thresh        */
  float tol;                  /* reprojection tolerance in raw-video pixels, finite and > 0        */
  const float* hist_coords;
  const uint8_t* visible;     /* [G,R,N], or NULL: hist_vis / hist_conf and thresh                 */
  const float* hist_vis; const float* hist_conf;
  const int32_t* first_row;   /* optional */
  const float* anchor_coords; /* [G,N,2], or NULL                                                  */
  const uint8_t* anchor_visible; /* [G,N], with anchor_coords                                      */
  const float* structure;     /* [G,N,3], source-camera coordinates; read only                     */
  const int8_t* valid;        /* [G,N], nonzero: the point is in the structure; read only          */
  const float* seed_pose;     /* [G,F,3,4]; read only                                              */
  float* pose;                /* [G,F,3,4] */
  int8_t* label;              /* [G,F,N_out] */
  float* error;               /* [G,F,N_out] */
  int32_t* stats;             /* [G,F,4] */
} ctk_fit_resection_args;
int ctk_fit_resection_workspace_bytes(const ctk_fit_resection_args* a, size_t* out_bytes);
int ctk_fit_resection(const ctk_fit_resection_args* a, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fit p3p: the camera's pose against a fixed 3-D structure from three points a candidate, no seed ------------------------------------
 * ctk_fit_resection scores candidates that all share the rotation of a seed pose, which a two-view fit has to find first: eight clean
 * points a sample, and no unique matrix on a planar structure.  ctk_fit_p3p needs no seed: candidate k is the pose that THREE sampled
 * entries of the fit list fix, and the rest of the call is ctk_fit_resection's bit for bit.  The rules are stated once in
 * csrc/p3p_math.h, on top of csrc/resection_math.h.
 *
 * Unchanged from ctk_fit_resection: the frame of the call and the gather (positions in 1/16 pixel, the pair rule with its three source
 * forms, first_row, `visible` or the logits with thresh, N_out <= 8192, the four intrinsics), the fit list (`valid` nonzero and three
 * finite floats of `structure`, ascending n, the first 4096 take part, M of them, more set stats[3] bit 3), project and within, the
 * `still` rule (bit 5), the score (an integer count of fit-list entries within tol; the largest wins, the lowest k on ties; fewer than
 * min_points, 6..8192: no fit), the three fixed-point Gauss-Newton rounds (the 28 int64 sums stay below 2^61, the 8 x 8 L D L^T; bits 0 /
 * 1 / 4 a round fell back, bit 2 an entry was left out), the outputs and no fit: pose float32 [G,F,3,4] = (R | t), (I | 0) where there
 * is no fit; label int8 [G,F,N_out] -1 / 0 / 1; error float32 [G,F,N_out]; stats int32 [G,F,4] = (M, slots labelled 1, the winning k or
 * -1, bits).  Every element is written by one plain store.
 *   candidates k < hypotheses (1..1024): the first three of the four distinct indices of ctk_fit_planes' seeded sample give the entries
 *              (X_i, Q_i) with rays y_i.  The unknowns are the scales l_i of the camera points Y_i = l_i y_i under
 *              l_i^2 |y_i|^2 + l_j^2 |y_j|^2 - 2 l_i l_j (y_i . y_j) = |X_i - X_j|^2 for the three pairs.  Start: the point's own distance
 *              from the structure's camera, l_i = |X_i|^2 rsqrt(|X_i|^2 |y_i|^2) (a point with |X_i|^2 not > 0 or not finite skips the
 *              candidate).  Six Newton rounds on the 3 x 3 system by a cofactor solve; a determinant that is zero or not finite, or an
 *              l_i that ends not finite or not > 0, skips the candidate.  A = [X_1 - X_0, X_2 - X_0, their cross product] as columns, B
 *              likewise from the Y_i; det A not > 0 (a collinear or repeated triple) skips the candidate; R = polar(B A^-1) by
 *              cofactors and the four polar steps, checked as ctk_fit_pose checks a rotation; t = Y_0 - R X_0.
 *              k = hypotheses: (I, 0), the only candidate on a still frame; stats[2] is in 0 .. hypotheses.
 * One launch on `stream`, one workgroup of 256 threads per (group, frame) with the fit list (X, Q and the slot) in min(N_out, 4096) * 34
 * bytes of LDS; a candidate is made by ONE lane, 64 a wave at a time, kept in that lane's registers and handed to the wave lane by lane
 * for the count by ballots; no atomics, no host synchronisation, capture-safe; `structure` and `valid` are only read.  The workspace
 * query answers 0 and `workspace` may be NULL.  Errors before any launch: ctk_fit_resection's for the fields both structs have (NULL a,
 * hist_coords, structure, valid, pose, label, error or stats, `visible` NULL with hist_vis or hist_conf NULL, half an anchor:
 * CTK_E_NULL; the shapes, min_points outside 6..8192, hypotheses outside 1..1024, tol not finite or not > 0, the camera: CTK_E_SHAPE;
 * hist_coords or anchor_coords not 8-byte aligned, structure, pose, error or stats not 4-byte aligned: CTK_E_ALIGN).
 *
 * Known limits.  Newton finds the P3P root nearest the structure's own distances: ONE root per triple, not the up to four of a closed
 * form.  Measured on the CPU (noise-free, 300 points 3..12 deep, 400 clean triples a row) the share of clean triples that return the
 * planted pose is 0.99 / 0.98 / 0.97 / 0.95 for a camera displaced by 0.3 / 1 / 2 / 3 units; a camera further from the structure's
 * camera than the nearest point is deep was not tried.  The rest are ctk_fit_resection's: the unit is the structure's, a structure
 * lives as long as enough of its points stay tracked, one pinhole camera without lens distortion, no bundle adjustment. */
typedef struct ctk_fit_p3p_args {
  int32_t G, N;               /* query groups, points per group of the history                     */
  int32_t N_out;              /* points per group that are looked at (the first N_out), <= 8192    */
  int32_t R;                  /* history rows per group                                            */
  int32_t f0, F;              /* row j of the outputs is frame f0 + j, 0 <= j < F                  */
  int32_t to;                 /* a fixed source frame, or -1                                       */
  int32_t lag;                /* source = f - lag (>= 1), or 0                                     */
  int32_t anchor_frame;       /* the frame the anchor was taken on (with anchor_coords)            */
  int32_t min_points;         /* a fit needs this many entries within tol, 6..8192                 */
  int32_t hypotheses;         /* sampled candidates, 1..1024                                       */
  uint32_t seed;              /* of the generator                                                  */
  float fx, fy, cx, cy;       /* the pinhole camera, raw-video pixels                              */
  float sx, sy;               /* position = coords * (sx, sy)                                      */
  float thresh;               /* visible from logits: sigmoid(vis) * sigmoid(conf) > thresh        */
  float tol;                  /* reprojection tolerance in raw-video pixels, finite and > 0        */
  const float* hist_coords;
  const uint8_t* visible;     /* [G,R,N], or NULL: hist_vis / hist_conf and thresh                 */
  const float* hist_vis; const float* hist_conf;
  const int32_t* first_row;   /* optional */
  const float* anchor_coords; /* [G,N,2], or NULL                                                  */
  const uint8_t* anchor_visible; /* [G,N], with anchor_coords                                      */
  const float* structure;     /* [G,N,3], source-camera coordinates; read only                     */
  const int8_t* valid;        /* [G,N], nonzero: the point is in the structure; read only          */
  float* pose;                /* [G,F,3,4] */
  int8_t* label;              /* [G,F,N_out] */
  float* error;               /* [G,F,N_out] */
  int32_t* stats;             /* [G,F,4] */
} ctk_fit_p3p_args;
int ctk_fit_p3p_workspace_bytes(const ctk_fit_p3p_args* a, size_t* out_bytes);
int ctk_fit_p3p(const ctk_fit_p3p_args* a, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fit focal: the focal length the camera had, read off the tracks -----------------------------------------------------------------------
 * ctk_fit_pose and everything behind it want four intrinsics.  The one a caller cannot guess is the focal length; the principal point
 * is the picture centre to within what these fits can see.  Over a fit list there is one focal length at which a rigid pose explains
 * the correspondences as well as the unconstrained fundamental matrix does: ctk_fit_focal sweeps K candidate focal lengths through
 * ctk_fit_pose's rules, scores each in pixels, sums the scores over the frames of the call (and of earlier calls) in integers, and
 * takes the minimum, per group g.  The rules are stated once in csrc/focal_math.h, on top of csrc/pose_math.h.
 *
 * The frame of the call is ctk_fit_pose's; everything not named here is its own bit for bit: the gather, the fit list (label 1 and
 * mask nonzero), `fundamental` and `label` as ctk_fit_epipolar wrote them, the rays, E, the decomposition, the vote, the two rounds.
 *   camera     of candidate k: fx = fy = focals[k] (device float32 [K]; ascending is the caller's duty), cx and cy the call's.
 *              Square pixels only.  A candidate stands iff it is finite and > 0; one that does not sets stats[3] bit 2.
 *   takes part a frame takes part iff its fit list has M >= min_points entries and ctk_fit_pose's E is accepted (F not all zero,
 *              finite, E finite) under at least one standing candidate.  A frame that does not costs 0 everywhere and is not counted.
 *   score      per (frame that takes part, candidate): the pose of ctk_fit_pose's rules under that camera; per fit-list entry under
 *              the final pose, with r and g of the refinement: c = min(((r r) / g) (f f) / (tol tol), 1), 1 where !(g > 0) or the
 *              quotient is a NaN -- the squared Sampson distance in pixels, truncated at tol^2, in units of tol^2;
 *              term = llrint(c 2^32).  cost int64 [G,F,K] = the sum of the terms; M 2^32 where the candidate does not stand or no
 *              pose comes out.  F <= 65535 keeps a call's sums below 2^61.
 *   totals     curve int64 [G,K+2]: curve[k] = curve_in[k] + the sum of cost[.][k] over the frames; curve[K] and curve[K+1] carry the
 *              counted frames and entries the same way.  curve_in (NULL: zeros) is the curve of an earlier call with the same focals:
 *              evidence accumulates over calls without a wait; two calls accumulated equal one call over both frame sets.
 *   choice     no fit when the counted frames < min_frames.  i = the smallest total (the lowest index on ties), mx = the largest.  No
 *              fit and bit 1 when !((double)mx >= contrast * (double)total[i]): the curve is flat -- the camera did not turn
 *              between the frames, and F does not depend on the focal length then -- or when candidate i does not stand.
 *   refine     0 < i < K-1: a = total[i-1] - total[i], d = total[i+1] - total[i] (in integers), delta = 0.5 (a - d) / (a + d) where
 *              a + d > 0; f = f_i + delta (f_{i+1} - f_i) for delta >= 0, f_i + delta (f_i - f_{i-1}) below; f_i where a + d is not
 *              > 0 or that neighbour does not stand.  At either end of the range f = f_i and bit 0: the range was too narrow.
 *   outputs    focal float32 [G], 0.0f where there is no fit; stats int32 [G,4] = (frames counted, i or -1, entries counted, bits),
 *              the counts clamped to int32.  Every element of the four outputs is written by one plain store.
 * Two launches on `stream`.  The sweep: grid (frame, group, four candidates), 256 threads, the fit list staged once in N_out * 18
 * bytes of LDS, a wave per candidate (wave shuffles for the votes and sums, lane 0 solves in the wave's own LDS).  The choice: one
 * workgroup per group adds the costs, counts the frames that took part by the sweep's own rule, chooses and refines.  No atomics, no
 * host synchronisation, capture-safe.  The workspace query answers 0 and `workspace` may be NULL.  Before any launch: NULL a,
 * hist_coords, fundamental, label, focals, focal, curve, cost or stats, `visible` NULL with hist_vis or hist_conf NULL, one of
 * anchor_coords / anchor_visible without the other: CTK_E_NULL; every shape ctk_fit_pose refuses for the fields both structs have,
 * K outside 1..256, min_frames < 1, tol not finite or not > 0, contrast not finite or < 1, cx or cy not finite: CTK_E_SHAPE;
 * hist_coords or anchor_coords not 8-byte aligned, fundamental, focals, focal or stats not 4-byte aligned, curve_in, curve or cost not
 * 8-byte aligned: CTK_E_ALIGN.  The query checks the same shapes and reads no pointer of the struct.
 *
 * Known limits.  Square pixels.  The principal point is assumed, not estimated.  The camera must TURN between the two frames of a
 * pair: under a pure translation every focal length explains F equally well, and the contrast rule refuses the fit.  One fixed focal
 * length per accumulation (no zoom).  No distortion estimate.  No second, finer sweep around the minimum. */
typedef struct ctk_fit_focal_args {
  int32_t G, N;               /* query groups, points per group of the history                     */
  int32_t N_out;              /* points per group that are looked at (the first N_out), <= 8192    */
  int32_t R;                  /* history rows per group                                            */
  int32_t f0, F;              /* row j of the inputs and of cost is frame f0 + j, 0 <= j < F       */
  int32_t to;                 /* a fixed source frame, or -1                                       */
  int32_t lag;                /* source = f - lag (>= 1), or 0                                     */
  int32_t anchor_frame;       /* the frame the anchor was taken on (with anchor_coords)            */
  int32_t min_points;         /* a frame takes part with this many entries on its fit list, 8..8192 */
  int32_t K;                  /* candidates, 1..256                                                */
  int32_t min_frames;         /* a fit needs this many frames that took part, >= 1                 */
  float cx, cy;               /* the principal point, raw-video pixels                             */
  float sx, sy;               /* position = coords * (sx, sy)                                      */
  float thresh;               /* visible from logits: sigmoid(vis) * sigmoid(conf) > thresh        */
  float tol;                  /* the score is truncated at tol^2; raw-video pixels, finite and > 0 */
  float contrast;             /* largest total / smallest total that a fit needs, finite and >= 1  */
  int32_t reserved;           /* 0 */
  const float* hist_coords;
  const uint8_t* visible;     /* [G,R,N], or NULL: hist_vis / hist_conf and thresh                 */
  const float* hist_vis; const float* hist_conf;
  const int32_t* first_row;   /* optional */
  const float* anchor_coords; /* [G,N,2], or NULL                                                  */
  const uint8_t* anchor_visible; /* [G,N], with anchor_coords                                      */
  const int8_t* mask;         /* [G,N], or NULL: every correspondence labelled 1 is fitted on      */
  const float* fundamental;   /* [G,F,3,3], as ctk_fit_epipolar wrote it; read only                */
  const int8_t* label;        /* [G,F,N_out], as ctk_fit_epipolar wrote it; read only              */
  const float* focals;        /* [K], the candidates in raw-video pixels; read only                */
  const int64_t* curve_in;    /* [G,K+2], or NULL: the curve of an earlier call; read only         */
  float* focal;               /* [G] */
  int64_t* curve;             /* [G,K+2] */
  int64_t* cost;              /* [G,F,K] */
  int32_t* stats;             /* [G,4] */
} ctk_fit_focal_args;
int ctk_fit_focal_workspace_bytes(const ctk_fit_focal_args* a, size_t* out_bytes);
int ctk_fit_focal(const ctk_fit_focal_args* a, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fit align: the similarity that maps one 3-D point set onto another ---------------------------------------------------------------------
 * Every structure of the 3-D chain lives in a unit and a camera frame of its own.  ctk_fit_align finds, per pair g, Y ~ s R X + t with
 * s > 0 between the points a[g] (X) and b[g] (Y) that share slots, robustly: points that moved between the two sets are labelled out.
 * The rules are stated once in csrc/align_math.h, on top of csrc/p3p_math.h; the kernel, a g++ build and numpy agree on every bit.
 *   correspondence  slot n with valid_a and valid_b nonzero, six finite floats of magnitude <= 2^20 and Y_z > 0.
 *   fit list   the correspondences whose mask byte is nonzero (mask NULL: all), ascending n, the first 4096 (M of them; more: stats[3]
 *              bit 3).  Every correspondence is classified, listed or not.
 *   candidates k < hypotheses (1..1024): the first three indices of ctk_fit_planes' seeded sample (frame 0); with M = 3 the entries
 *              (0, 1, 2).  s^2 = the sum of the three squared sides in b over that in a, s by ctk_fit_pose's reciprocal root;
 *              R = polar(B A^-1) of the two triangle frames as in ctk_fit_p3p, a's sides scaled by s first; a collinear or repeated
 *              triple in either set skips the candidate; t = Y_0 - s R X_0.  k = hypotheses: (1, I, 0).  Where every correspondence
 *              has the same floats in both sets only that one is scored (bit 5) and the result is exactly (1, I, 0).
 *   score      Z = s R X + t is within iff Z_z > 0, the squared pixel distance of the projections of Z and Y by (fx, fy, cx, cy) is
 *              <= tol^2 (compared without a division) and |Z_z - Y_z| <= depth_tol Y_z.  The integer count decides; the lowest k on
 *              ties; fewer than min_points (3..8192), M < 3 or no candidate: no fit.
 *   refit      three Gauss-Newton rounds over the entries within 4, 2, 1 x (tol, depth_tol) under the round's transform, seven
 *              parameters about b's camera centre: Z' = (1 + d)(I + [w]x) Z + T, so s' = s (1 + d), R' = polar(R + [w]x R),
 *              t' = ((t + w x t) + d t) + T.  The residual is what the score judges: the two pixel differences u - ub and v - vb with
 *              (u, v) = (Z_x, Z_y) / Z_z, (ub, vb) = (Y_x, Y_y) / Y_z, and the relative depth difference (Z_z - Y_z) / Y_z, weighted
 *              1 : fy / fx : tol / (fx depth_tol) (each in units of its tolerance, up to tol / fx).  T is solved in units of 2^e, e the
 *              largest frexp exponent of Y_z over the round's entries.  An entry's three rows of eight numbers (the gradient by
 *              (w, T 2^-e, d) and the residual) are scaled by 1/16 and by their weight; an entry with one of its 24 numbers above 4
 *              in magnitude is left out (bit 2), so the 36 int64 sums of llrint(x_i x_j 2^44) stay below 2^62; ctk_fit_planes' 8 x 8
 *              L D L^T with one padded row.  A round that fails -- fewer than 3 entries, the solve, a rotation or translation that
 *              ctk_fit_pose would not accept, an s that is not finite or not > 0 -- keeps its transform (bit 1).
 *   outputs    sim float32 [G,3,4]: row r = (s R[r][0..2], t[r]), to be applied to homogeneous points; scale float32 [G];
 *              label int8 [G,N]: 1 within tolerance, 0 not, -1 no correspondence; error float32 [G,N]: the squared pixel distance, +inf
 *              where Z_z <= 0, -1 without a correspondence or a fit; stats int32 [G,4] = (M, slots labelled 1, the winning k or -1,
 *              bits).  No fit: sim all zero, scale 0, every correspondence label 0 and error -1.
 * One launch on `stream`, one workgroup of 256 threads per pair with the fit list (six floats an entry) in min(N, 4096) * 24 bytes of
 * LDS; a candidate is made by ONE lane, 64 a wave at a time; no atomics, no host synchronisation, capture-safe; every output element
 * is one plain store and the inputs are only read.  The workspace query answers 0 and `workspace` may be NULL.  Errors before any
 * launch: NULL a, a, valid_a, b, valid_b, sim, scale, label, error or stats: CTK_E_NULL; G outside 1..65535, N outside 1..8192,
 * hypotheses outside 1..1024, min_points outside 3..8192, fx or fy not finite or not > 0, cx or cy not finite, tol or depth_tol not
 * finite or not > 0, reserved != 0: CTK_E_SHAPE; a, b, sim, scale, error or stats not 4-byte aligned: CTK_E_ALIGN.
 *
 * Known limits.  One similarity per pair; at least three non-collinear common points; no covariance; a degenerate inlier set keeps
 * the candidate's transform (bit 1); the refit turns about b's camera centre, so b is expected in a camera's frame. */
typedef struct ctk_fit_align_args {
  int32_t G, N;               /* pairs, slots per set                                              */
  int32_t min_points;         /* a fit needs this many entries within tolerance, 3..8192           */
  int32_t hypotheses;         /* sampled candidates, 1..1024                                       */
  uint32_t seed;              /* of the generator                                                  */
  int32_t reserved;           /* 0                                                                 */
  float fx, fy, cx, cy;       /* the pinhole camera of b's frame                                   */
  float tol;                  /* pixel tolerance in that camera, finite and > 0                    */
  float depth_tol;            /* relative depth tolerance, finite and > 0                          */
  const float* a;             /* [G,N,3]; read only                                                */
  const int8_t* valid_a;      /* [G,N], nonzero: the point exists; read only                       */
  const float* b;             /* [G,N,3]; read only                                                */
  const int8_t* valid_b;      /* [G,N]; read only                                                  */
  const uint8_t* mask;        /* [G,N], nonzero: the correspondence may be on the fit list; or NULL */
  float* sim;                 /* [G,3,4] */
  float* scale;               /* [G] */
  int8_t* label;              /* [G,N] */
  float* error;               /* [G,N] */
  int32_t* stats;             /* [G,4] */
} ctk_fit_align_args;
int ctk_fit_align_workspace_bytes(const ctk_fit_align_args* a, size_t* out_bytes);
int ctk_fit_align(const ctk_fit_align_args* a, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fit structure: points added to a 3-D structure, and the structure restated on a newer frame ---------------------------------------
 * ctk_fit_resection places cameras against a structure that only shrinks.  ctk_fit_structure turns "tracked on several localised
 * frames" into "a 3-D point in the structure's unit": per group g and slot n < N_out, the positions on the frames f0 + j, 0 <= j < F
 * (the VIEWS), under the poses ctk_fit_resection gave for them, are triangulated.  The rules are stated once in csrc/structure_math.h.
 *   views      pose float32 [G,F,3,4] (X_f = R X_source + t), optionally pose_stats int32 [G,F,4] (ctk_fit_resection's).  View j counts
 *              iff its twelve floats are finite, R passes the four polar steps and ctk_fit_pose's validity check, and pose_stats is
 *              NULL or pose_stats[g,j,2] >= 0.  A view that fails is dropped (it does not become the identity).  c = -R^T t.
 *   observation  slot n on view j: the view counts, f0 + j >= first_row[g,n] (when given), both coordinates quantise (1/16 pixel),
 *              the slot is visible there (`visible` or the logits with thresh).  One frame: no source frame, no pair rule.  m = their
 *              number; y = the ray of the position, d = R^T y.
 *   start      the linear midpoint solution: A = sum (I - d d^T / (d.d)), b = sum (I - d d^T / (d.d)) c, X = adj(A) b / det(A) by the
 *              symmetric 3 x 3 cofactor form with one division.  No start (stats[3] bit 3) when m < 2, det is not > 0 or not finite,
 *              or X is not finite.
 *   rounds     three Gauss-Newton rounds on the reprojection error; round r uses the observations with e <= (g_r tol)^2, g = 4, 2, 1,
 *              so that one bad view of a track drops out.  A round with fewer than min_views observations, a failed solve or an X
 *              that stops being finite keeps its X (stats[3] bits 0 / 1 / 2 for rounds 1 / 2 / 3).
 *   accept     the counted views are those within tol under the final X (behind a camera the error is +inf).  With a the first of
 *              them and w_j = X - c_j: parallax holds iff |w_a x w_j|^2 >= |w_a|^2 |w_j|^2 min_sin2 for some counted j (one
 *              comparison, no root, no division; stats[3] bit 4 where it does not).  Accepted iff counted >= min_views (2..256),
 *              at least half of the slot's observations are counted (2 counted >= m; stats[3] bit 6 where not: a point that moves by
 *              itself finds min_views neighbouring views that agree), parallax holds and the written point is finite.
 *   into       -1, or a view k in [0, F): every written point is R_k X + t_k, so the new structure is stated in the camera of frame
 *              f0 + k.  Where view k does not count there is no structure: every point zero, label 0 for every slot with an
 *              observation or in the old structure and -1 for every other, stats[3] bit 5 in every slot.
 *   carry      structure_in float32 [G,N,3] and valid_in int8 [G,N], both or neither: a slot is carried when its byte is nonzero, its
 *              floats are finite, first_row[g,n] <= source_frame (when first_row is given: a released and reassigned slot is not
 *              carried) and its point through the into pose is finite: label 2.  refine = 0: carried slots are not triangulated
 *              (stats (0, 0, -1, 0)).  refine = 1: they are; accepted, the new point wins (label 1), rejected, the old one stays (2).
 *   origin     origin_in float32 [G,3,4] or NULL (the identity); origin_out float32 [G,3,4] or NULL = (R_k R_o | R_k t_o + t_k): the
 *              pose of the new structure's camera against the first one's, so that compose(pose, origin) of every later pose is in
 *              one world.  A copy of origin_in where into < 0 or view k does not count.
 *   outputs    points float32 [G,N_out,3], zero where label < 1; label int8 [G,N_out]: -1 fewer than 2 observations and not carried,
 *              0 triangulated and rejected, 1 triangulated and accepted, 2 carried; error float32 [G,N_out]: the mean squared
 *              reprojection error over the counted views in px^2 (one division), -1 where the label is not 1; stats int32 [G,N_out,4]
 *              = (m, counted views, the first counted view or -1, bits).  Every element is written by one plain store.
 * One launch on `stream`: one thread per slot, workgroups of 64 threads (one wave), grid (ceil(N_out / 64), G); the views are
 * validated once per workgroup into 30.25 KiB of LDS; every thread walks the views in ascending order five times (the start, three
 * rounds, the classification), reading the positions again each time; plain double sums, deterministic because one thread owns a
 * slot.  No atomics, no host synchronisation, capture-safe; every input is only read.  The workspace query answers 0 and `workspace`
 * may be NULL.  Before any launch: NULL a, hist_coords, pose, points, label, error or stats, `visible` NULL with hist_vis or hist_conf
 * NULL, one of structure_in / valid_in without the other: CTK_E_NULL; G, N, N_out (<= 8192, <= N), R < 1, f0 < 0, F outside 1..256 or
 * > R, into outside -1..F-1, source_frame < 0, min_views outside 2..256, refine outside 0..1, tol not finite or not > 0, min_sin2 not
 * in (0, 1], the camera and the scale as ctk_fit_resection: CTK_E_SHAPE; hist_coords not 8-byte aligned, a float or int32 tensor not
 * 4-byte aligned: CTK_E_ALIGN.  The query checks the same shapes.
 *
 * Known limits.  A point stays in a structure's fits only while it is visible on the frame the structure is stated in.  Poses
 * chain once per restatement, not per frame.  No bundle adjustment: neither the poses nor the carried points are refined.  The
 * parallax test looks at the first counted view against the others only.  The start is not robust: the gates drop one wrong view of a
 * few tol, a grossly wrong one (tens of tol) rejects the slot.  One pinhole camera, no lens distortion. ctk_lens_frames / ctk_lens_points correct a lens in front of
 * the fit ("lens" above). */
typedef struct ctk_fit_structure_args {
  int32_t G, N;               /* query groups, points per group of the history                     */
  int32_t N_out;              /* points per group that are looked at (the first N_out), <= 8192    */
  int32_t R;                  /* history rows per group                                            */
  int32_t f0, F;              /* view j is frame f0 + j, 0 <= j < F <= 256                         */
  int32_t into;               /* the view whose camera the outputs are stated in, or -1            */
  int32_t source_frame;       /* the frame structure_in is stated in (against first_row)           */
  int32_t min_views;          /* an accepted point needs this many views within tol, 2..256        */
  int32_t refine;             /* 1: carried slots are triangulated too                             */
  float fx, fy, cx, cy;       /* the pinhole camera, raw-video pixels                              */
  float sx, sy;               /* position = coords * (sx, sy)                                      */
  float thresh;               /* visible from logits: sigmoid(vis) * sigmoid(conf) > thresh        */
  float tol;                  /* reprojection tolerance in raw-video pixels, finite and > 0        */
  float min_sin2;             /* the squared sine of the smallest parallax angle, in (0, 1]        */
  int32_t reserved;           /* 0 */
  const float* hist_coords;
  const uint8_t* visible;     /* [G,R,N], or NULL: hist_vis / hist_conf and thresh                 */
  const float* hist_vis; const float* hist_conf;
  const int32_t* first_row;   /* optional */
  const float* pose;          /* [G,F,3,4]; read only                                              */
  const int32_t* pose_stats;  /* [G,F,4], or NULL; read only                                       */
  const float* structure_in;  /* [G,N,3], or NULL; read only                                       */
  const int8_t* valid_in;     /* [G,N], with structure_in; read only                               */
  const float* origin_in;     /* [G,3,4], or NULL: the identity; read only                         */
  float* points;              /* [G,N_out,3] */
  int8_t* label;              /* [G,N_out] */
  float* error;               /* [G,N_out] */
  int32_t* stats;             /* [G,N_out,4] */
  float* origin_out;          /* [G,3,4], or NULL */
} ctk_fit_structure_args;
int ctk_fit_structure_workspace_bytes(const ctk_fit_structure_args* a, size_t* out_bytes);
int ctk_fit_structure(const ctk_fit_structure_args* a, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Op A: corr_embed  (cotracker3_online.py:190-210; get_correlation_feat :130-143,
 *      einsum :202-204, corr_mlp :205) -> x[:, 0:1024]                                */
int ctk_corr_embed_workspace_bytes(const ctk_window_args* a, size_t* out_bytes);
int ctk_corr_embed(const ctk_window_args* a, const ctk_model_weights* w, float* x /*[N*S,CTK_X_LD]*/,
                   void* workspace, size_t workspace_bytes, void* stream);
/* 49x49 correlation volume only (before corr_mlp), for parity tests:
 * out [4][N*S][CTK_CORR_LD], row = n*S+t.                                             */
int ctk_corr_volume(const ctk_window_args* a, float* out, void* stream);
/* The same volumes from the split-half pipeline's sampler (footprint x support on f16 MFMA x3, blend after
 * the correlation), in SH format: out halves [4][N*S][2*CTK_CORR_LD].  workspace holds the SH copy of the
 * window's pyramid (ctk_corr_volume_sh_workspace_bytes).                                                  */
int ctk_corr_volume_sh_workspace_bytes(const ctk_window_args* a, size_t* out_bytes);
int ctk_corr_volume_sh(const ctk_window_args* a, void* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Op C: assemble_tokens (cotracker3_online.py:212-245, posenc :19-39) -> x[:,1024:1120]
 * Row n*S + t, columns CTK_X_VIS + [vis, conf, 4 relative coordinates (c[t] - c[t+1], c[t] - c[t-1]) / scale, sin and cos
 * (sin of the argument + f32(pi/2)) of these times 2^0 .. 2^9, ten zeros]; a missing neighbour frame gives 0.  Every step of
 * the argument is the reference's own float32 operation; the sine is within 2.5e-7 of the exact sine of that float32
 * argument, at any magnitude (checked up to arguments of 1e7: tracks far outside the frame).  Only these 96 columns are
 * written.  x: 16-byte aligned (CTK_E_ALIGN).                                                                        */
int ctk_assemble_tokens(const ctk_window_args* a, void* x /* f32 [N*S,CTK_X_LD], or SH when x_split */,
                        int32_t x_split, void* stream);

/* ---- the row kernels of a window on their own (for tests): each entry point validates and makes ONE launch, the launch
 * ctk_forward_window / ctk_forward_window_batch / ctk_update_former make at that place.  A ctk_window_batch is read for
 * the STATE only: coords [S,N,2] / vis / conf [S,N], S, N (and, where said, scale_x / scale_y) of videos[0 .. B), which must
 * agree in S, N and the scales; 1 <= B <= CTK_MAX_BATCH; fmaps, support, iters and flags are not looked at.  Validation comes
 * before any HIP call, in this order: a missing pointer CTK_E_NULL, a bad size CTK_E_SHAPE, a pointer the kernel moves 16 bytes
 * at a time that is not 16-byte aligned CTK_E_ALIGN (named per entry point; the state is read and written 4 bytes at a time).
 *
 * Token assembly (Op C) into columns [base, base + 96) of rows `ld` columns apart: ld % 32 == 0, base % 32 == 0,
 * 0 <= base <= ld - 96 -- (CTK_X_LD, CTK_X_VIS) is ctk_assemble_tokens, (CTK_XF_LD, CTK_XF_SMALL) the folded input.  x f32
 * [B*N*S, ld], or SH [B*N*S][ld/32][2][32] halves when x_split; row (b*N + n)*S + t.  B == 1 is the single-video kernel,
 * B > 1 the joint one (per-video state pointers by value).  Reads the scales.  Aligned: x.                              */
int ctk_assemble_tokens_batch(const ctk_window_batch* batch, void* x, int32_t x_split, int32_t ld, int32_t base, void* stream);
/* dst[(b*64 + v)*S + t][0..384) = virtual_tokens[v][0..384)  (cotracker.py:487-488), b < B <= CTK_MAX_BATCH.
 * Aligned: virtual_tokens, dst.                                                                                          */
int ctk_virtual_init(const float* virtual_tokens /*[64,384]*/, int32_t S, int32_t B, float* dst /*[B*64*S,384]*/, void* stream);
/* d = tokens[row] @ head_w^T + head_b for every row (b*N + n)*S + t of tokens [B*N*S, 384] (head_w [4,384]: flow x, flow y,
 * vis, conf; head_b [4]), then   delta[row] = d   when delta is given, and   coords[t][n] += d[0..1], vis[t][n] += d[2],
 * conf[t][n] += d[3]   on video b's state when it is given (cotracker3_online.py:252-259).  B == 1: delta [N*S,4] and / or
 * the state -- coords, vis and conf all three or all NULL; neither is CTK_E_NULL.  B > 1 (the joint kernel): the state of
 * every video, delta must be NULL (CTK_E_SHAPE).  Aligned: tokens, head_w, delta.                                     */
int ctk_heads_update(const ctk_window_batch* batch, const float* tokens, const float* head_w, const float* head_b,
                     float* delta, void* stream);

/* ---- Op B: EfficientUpdateFormer.forward (cotracker.py:483-531): x -> delta [N*S,4] */
int ctk_update_former_workspace_bytes(int32_t S, int32_t N, size_t* out_bytes);
int ctk_update_former(int32_t S, int32_t N, const float* x, const ctk_model_weights* w,
                      float* delta /*[N*S,4] row=n*S+t*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---- general update former: CoTracker2 (cotracker.py:46-56: time_depth = space_depth = 6, input_dim 456,
 * output_dim 130, attention mask) on the same block kernels.  x [N*S, in_ld] (f32, or SH when x_split), row = n*S+t,
 * columns >= in_dim zero; delta [N*S, out_ld] f32 (columns >= out_dim are the zero-padded head rows).  point_mask [N]
 * (1 = track already queried) masks the point KEYS of virtual<-points and the point QUERIES of points<-virtual exactly
 * as CrossAttnBlock.forward does (cotracker.py:560-572); NULL = no mask.  Workspace: ctk_update_former_workspace_bytes. */
typedef struct ctk_former_weights {
  int32_t depth;               /* layers (6)                                                     */
  int32_t in_dim, in_ld;       /* 456, padded to a multiple of 32 (480)                          */
  int32_t out_dim, out_ld;     /* 130, padded to a multiple of 64 (192)                          */
  const float* in_w;           /* input_transform.weight [384, in_ld] (zero padded) or NULL when in_p */
  const void* in_p;            /* ctk_pack_weight blob: selects the split-half back end for EVERY Linear */
  const float* in_b;           /* input_transform.bias [384] (used when in_bias_t == NULL)       */
  const float* in_bias_t;      /* optional [S,384] = bias + W @ time_emb[t] (time embedding folded in) */
  const float* virtual_tokens; /* virual_tracks [64,384]                                         */
  const float* head_w;         /* flow_head.weight [out_ld,384] zero padded rows, or NULL when head_p */
  const void* head_p;
  const float* head_b;         /* [out_ld]                                                       */
  const ctk_block_weights* time_blocks;    /* [depth] */
  const ctk_block_weights* virtual2point;  /* [depth] */
  const ctk_block_weights* virtual_self;   /* [depth] */
  const ctk_block_weights* point2virtual;  /* [depth] */
} ctk_former_weights;
int ctk_update_former_ex(int32_t S, int32_t N, const void* x, int32_t x_split, const ctk_former_weights* w,
                         const uint8_t* point_mask, float* delta, void* workspace, size_t workspace_bytes, void* stream);

/* CoTracker2 iteration around CorrBlock and the former (cotracker.py:128-172).  Layouts: coords / track_mask / vis
 * [S,N,*], track_feat [S,N,128] (= CorrBlock targets), fcorrs [N,S,196] (ctk_corrblock_sample), pos [N,456].
 * ctk_v2_assemble: x[n*S+t][0..in_ld) = cat(get_2d_embedding(coords - coords[0]) (130), fcorrs (196), track_feat (128),
 *   track_mask, vis) + pos[n], zero padded to in_ld; the time embedding (:150) is folded into in_bias_t.
 * ctk_v2_apply_delta: coords[t,n] += delta[n*S+t][0:2]; normed[t*N+n][0:128] = GroupNorm(1,128)(delta[n*S+t][2:130])
 *   (:157-167; the Linear + GELU + residual of track_feat_updater is then one ctk_gemm with resid = C = track_feat).
 * ctk_v2_vis_head: vis_predictor (:172).  ctk_sample_features4d: sample_features4d (model_utils.py:258-290) of a
 *   channels-last map [H,W,C] at (x, y) -> [N,C] (4-D grid_sample semantics; used for pos_emb, :126-130).
 * Argument rules (checked before any launch): S, N, R > 0; in_ld >= 456 and in_ld % 32 == 0; out_ld >= 130 (any value: the
 *   delta rows are read with scalar loads); normed (ctk_v2_apply_delta), track_feat and w (ctk_v2_vis_head) 8-byte aligned,
 *   CTK_E_ALIGN otherwise (ctk_forward_window_v2 and its workspace / graph entry points check track_feat and vis_w up front).
 *   ctk_v2_vis_head accumulates its dot product in f64.  ctk_v2_apply_delta is two float32 passes over the row: next to the
 *   usual 2e-6 max|normed| its result carries the rounding of the float32 row sum, <= 2^-21 |row mean| rstd |gamma| -- a deliberate
 *   limit, negligible for rows whose offset is of the order of their spread (what the update former produces), 5e-5 of the
 *   output for an offset of 1e3 times the spread.                                                                           */
int ctk_v2_assemble(int32_t S, int32_t N, const float* coords, const float* fcorrs, const float* track_feat,
                    const float* track_mask, const float* vis, const float* pos, int32_t in_ld, void* x, int32_t x_split,
                    void* stream);
int ctk_v2_apply_delta(int32_t S, int32_t N, const float* delta, int32_t out_ld, float* coords, const float* gamma,
                       const float* beta, float eps, float* normed, void* stream);
int ctk_v2_vis_head(const float* track_feat, int64_t R, const float* w, const float* b, float* out, void* stream);
int ctk_sample_features4d(const float* map, int32_t H, int32_t W, int32_t C, const float* coords, int32_t N, float* out,
                          void* stream);

/* ---- Op D: the stand-alone bilinear_sampler with the reference's FULL signature (model_utils.py:191-255) ----
 * input  [B,C,H,W] (D = 0) with coords [B,P,2] = (x, y), or [B,C,D,H,W] (D > 0) with coords [B,P,3] = (t, x, y), both in
 *        the reference's own NCHW layout; P = product of the coords' inner dims (Ho*Wo, or Do*Ho*Wo);
 * align_corners 0 / 1, padding_mode CTK_PAD_ZEROS / CTK_PAD_BORDER ("reflection": CTK_E_SHAPE);  out [B,C,P].
 * Bit-identical to torch.nn.functional.grid_sample on the CPU for finite coordinates (4-D: ATen's vectorised kernel with its
 * FMA contractions; 5-D: the scalar grid_sampler_3d -- csrc/sampler_math.h), NaN coordinates are not specified.
 * Also what sample_features4d / sample_features5d (model_utils.py:258-323) reduce to (cotracker_amd/model_utils.py).     */
#define CTK_PAD_ZEROS 0
#define CTK_PAD_BORDER 1
int ctk_bilinear_sampler(const float* input, int32_t B, int32_t C, int32_t D, int32_t H, int32_t W, const float* coords,
                         int64_t P, int32_t align_corners, int32_t padding_mode, float* out, void* stream);

/* ---- CoTracker2 window driver: CoTracker2.forward_window (cotracker.py:86-173) as ONE capture-safe call per window
 * (the CoTracker2 counterpart of ctk_forward_window): sampled positional embedding once, then `iters` x { CorrBlock
 * sample -> token assembly -> update former (attention mask) -> coords += delta, GroupNorm(feature delta) ->
 * track_feat += GELU(Linear(.)) }, then the visibility head.  coords and track_feat are updated IN PLACE.
 * ctk_v2_window_graph_create captures one such call into a hipGraph (same ownership rules as ctk_window_graph_create;
 * launch / nodes / destroy through the ctk_window_graph_* functions).                                               */
typedef struct ctk_v2_window_args {
  int32_t S, N, iters;
  int32_t H[CTK_LEVELS], W[CTK_LEVELS];
  const float* fmaps[CTK_LEVELS]; /* NHWC [S,H_l,W_l,128] CorrBlock pyramid, NOT normalised (blocks.py:300-307)  */
  float* coords;                  /* [S,N,2] in/out, level-0 feature units                                       */
  float* track_feat;              /* [S,N,128] in/out, already multiplied by the attention mask (cotracker.py:346) */
  const float* vis;               /* [S,N] visibility logits fed to the former (constant over the iterations)    */
  const float* track_mask;        /* [S,N] 0/1 as float (cotracker.py:338-344)                                   */
  const uint8_t* point_mask;      /* [N] attention mask (cotracker.py:331-333) or NULL                           */
  float* vis_out;                 /* [S,N] vis_predictor(track_feat) after the last iteration (cotracker.py:172) */
} ctk_v2_window_args;
typedef struct ctk_v2_weights {
  ctk_former_weights former;      /* 6 + 6 layers, 456 -> 130 (in_ld / out_ld padded)                            */
  const float* pos_hwc; int32_t pos_h, pos_w;  /* pos_emb as channels-last [pos_h,pos_w,456] (cotracker.py:60-66) */
  const float* norm_w; const float* norm_b;    /* GroupNorm(1,128) (cotracker.py:79)                             */
  const float* upd_w; const void* upd_p; const float* upd_b; /* track_feat_updater Linear 128->128 (f32 and/or packed) */
  const float* vis_w; const float* vis_b;      /* vis_predictor Linear 128->1: [128], [1]                        */
} ctk_v2_weights;
int ctk_forward_window_v2_workspace_bytes(const ctk_v2_window_args* a, const ctk_v2_weights* w, size_t* out_bytes);
int ctk_forward_window_v2(const ctk_v2_window_args* a, const ctk_v2_weights* w, void* workspace, size_t workspace_bytes,
                          void* stream);
int ctk_v2_window_graph_create(const ctk_v2_window_args* a, const ctk_v2_weights* w, void* workspace,
                               size_t workspace_bytes, ctk_window_graph** out);

/* ---- Op D: standalone samplers --------------------------------------------------- */
/* Integer floor indices (x0,y0) of the 7 x-taps and 7 y-taps of every (t,n,level), exactly as
 * bilinear_sampler + ATen grid_sampler_3d compute them (model_utils.py:238-255).
 * out int32 [S,N,4,2,7].  The bit-exactness contract of BASELINE.md section 2.          */
int ctk_tap_indices(const ctk_window_args* a, int32_t* out, void* stream);
/* get_correlation_feat (cotracker3_online.py:130-143) for one level: out [S,N,49,128].  */
int ctk_sample_patches(const float* fmap /*NHWC [S,H,W,128]*/, int32_t S, int32_t H, int32_t W,
                       const float* coords /*[S,N,2] level-0 units*/, int32_t N, int32_t level,
                       float* out, void* stream);
/* get_track_feat (cotracker3_online.py:113-128, sample_features5d model_utils.py:293-323):
 * trilinear support patches for one level.  fmap NHWC [T,H,W,128]; frames [N] float (frame
 * index relative to fmap[0]); coords [N,2] in this level's units; out [N,49,128].        */
int ctk_sample_support(const float* fmap, int32_t T, int32_t H, int32_t W, const float* frames,
                       const float* coords, int32_t N, float* out, void* stream);
/* CorrBlock.corr + CorrBlock.sample fused (cotracker/models/core/cotracker/blocks.py:284-362, CoTracker2's 4D
 * correlation-volume sampler; num_levels=4, radius=3, padding_mode="border" as built at cotracker.py:119-124):
 * out[n*S+s][l*49 + a*7 + b] = bilinear sample (grid_sampler_2d, align_corners) of the level-l volume
 * <targets[s,n,:], fmaps_l[s,:,y,x]> / sqrt(128) at (x, y) = coords[s,n]/2^l + (a-3, b-3).  The volume is never
 * materialised: only the <=9x9 footprint dots are formed.  fmaps[l]: NHWC [S,H[l],W[l],128] (level l>0 =
 * ctk_avg_pool2_nhwc of level l-1, NOT normalised -- blocks.py:300-307); targets [S,N,128] (= track_feat,
 * blocks.py:342); coords [S,N,2] level-0 units; out [N,S,196] (the reference's [B*N,S,LRR], blocks.py:338-339). */
int ctk_corrblock_sample(const float* const* fmaps, const int32_t* H, const int32_t* W, int32_t S, int32_t N,
                         const float* targets, const float* coords, float* out, void* stream);
/* Channel L2-normalise + NCHW->NHWC (cotracker3_online.py:384-394) and 2x2 average pooling
 * (:401-409).  in [F,128,H,W] -> out NHWC [F,H,W,128]; pool: in NHWC [F,H,W,128] -> [F,H/2,W/2,128]. */
int ctk_normalize_to_nhwc(const float* in, int32_t F, int32_t H, int32_t W, float* out, void* stream);
int ctk_avg_pool2_nhwc(const float* in, int32_t F, int32_t H, int32_t W, float* out, void* stream);

/* ---- CNN feature encoder on the split-half MFMA path (round 3) ---------------------------------------------
 * BasicEncoder (cotracker/models/core/cotracker/blocks.py:141-219, ResidualBlock :79-138), called once per forward at
 * cotracker3_online.py:373-384 / cotracker3_offline.py:60-75.  Activations are NHWC; a convolution reads SH-format input
 * ([pixel][C/32] lines of 128 bytes: 32 hi | 32 lo halves, see the SH notes below) and writes f32 [pixel][n_out].  The host
 * side (co-tracker_amd/encoder_hip.py) strings these calls together in the reference's order.
 *
 * ctk_conv2d_sh: nn.Conv2d(Cin, n_out, (KH,KW), stride, padding=pad, zeros) as an implicit GEMM (no im2col buffer).
 *   in_sh  [F][Hin][Win][Cin/32] lines; Cin % 32 == 0
 *   wp     ctk_pack_weight blob of the matrix W'[n_pad][KH*KW*Cin], W'[n][(ky*KW+kx)*Cin + c] = weight[n][c][ky][kx], rows
 *          n >= n_out zero, n_pad % 128 == 0; bias: n_pad floats (zeros beyond n_out)
 *   out    f32 [F*Hout*Wout][n_out], Hout = (Hin + 2 pad - KH)/stride + 1; zeros: >= 128 zero bytes on the device
 *   Limits (CTK_E_SHAPE otherwise): n_out % 32 == 0, n_out <= n_pad <= 1024; F, KH, KW, stride > 0; 0 < Hin, Win <= 16000;
 *   Hout, Wout > 0; F*Hout*Wout and F*Hin*Win <= 2^31 - 1; KH*KW*Cin < 2^30; and the range of a row's first tap, which the
 *   kernel keeps in 15 + 16 bits biased by 16384:  0 <= pad <= 16384,  (Hout-1)*stride - pad <= 16383,
 *   (Wout-1)*stride - pad <= 49151 (implied by the limits on Win and pad).  E.g. Hin = 16000, 3x3, stride 1 takes pad <= 386.
 *   All five pointers non-NULL (CTK_E_NULL) and 16-byte aligned (CTK_E_ALIGN).                                              */
int ctk_conv2d_sh(const void* in_sh, int32_t F, int32_t Hin, int32_t Win, int32_t Cin, const void* wp, const float* bias,
                  int32_t n_out, int32_t n_pad, int32_t KH, int32_t KW, int32_t stride, int32_t pad, float* out,
                  const void* zeros, void* stream);
/* Stem: x = 2*(frame/255) - 1 (cotracker3_online.py:320) and the 7x7 stride-2 pad-3 patches of the 3-channel frames
 * [F,3,H,W] as SH rows of 160 columns ((ky,kx,c) order, 147 used, rest 0): conv1 (blocks.py:150-157) = ctk_conv2d_sh on
 * a [F][Ho][Wo] grid with Cin = 160, 1x1, stride 1.  out_sh: F*Ho*Wo*160*4 bytes, 16-byte aligned, Ho = (H-1)/2+1.
 * F > 0, H >= 7, W >= 7.                                                                                                  */
int ctk_enc_stem_im2col(const float* frames, int32_t F, int32_t H, int32_t W, void* out_sh, void* stream);
/* nn.InstanceNorm2d (no affine, eps, biased variance; blocks.py:110-113,147-148) statistics of x f32 [F][HW][C]:
 * stats [F][C][2] = (mean, 1/sqrt(var + eps)), sums in f64 in a fixed order.  workspace: ctk_enc_inorm_workspace_bytes
 * (= F * ceil(HW / 512) * C * 16).  0 < F <= 65535, HW > 0, C % 8 == 0, C <= 1024 (both entry points); x and workspace
 * 16-byte aligned.                                                                                                         */
int ctk_enc_inorm_workspace_bytes(int32_t F, int64_t HW, int32_t C, size_t* out_bytes);
int ctk_enc_inorm_stats(const float* x, int32_t F, int64_t HW, int32_t C, float eps, float* stats, void* workspace, void* stream);
/* y = relu((x - mean) * rstd)  (blocks.py:130-131, 188-190, 216-217); with skip: out = relu(skip' + y) (blocks.py:138) where
 * skip' = skip, or (skip - mean_s) * rstd_s when skip_stats is given (the 1x1 downsample branch, blocks.py:123-126,133-136).
 * Writes SH (out_sh, the next convolution's input) and / or f32 (out_f32), at least one of them; C % 32 == 0; F, HW > 0;
 * skip_stats needs skip; x, skip, out_sh and out_f32 16-byte aligned.                                                       */
int ctk_enc_inorm_apply(const float* x, const float* stats, const float* skip, const float* skip_stats, int32_t F, int64_t HW,
                        int32_t C, void* out_sh, float* out_f32, void* stream);
/* F.interpolate(., (Ho, Wo), bilinear, align_corners=True) of the four stage outputs (f32 NHWC [F][H_k][W_k][C_k]) and
 * torch.cat over channels (blocks.py:198-215) -> SH [F][Ho][Wo][sum C_k / 32] lines, the input of conv2.  Four sources, none
 * NULL; H_k, W_k, F, Ho, Wo > 0; C_k % 8 == 0 and sum C_k % 32 == 0; every source and out_sh 16-byte aligned.                */
int ctk_enc_fuse(const float* const* src, const int32_t* H, const int32_t* W, const int32_t* C, int32_t F, int32_t Ho, int32_t Wo,
                 void* out_sh, void* stream);
/* fmaps / sqrt(max(sum_c fmaps^2, 1e-12)) on NHWC [P][128] (cotracker3_online.py:384-394).  P > 0; out may be x.                */
int ctk_enc_l2norm(const float* x, int64_t P, float* out, void* stream);

/* ---- primitives (exported for unit tests and reuse) ------------------------------ */
/* C[M,N] = act(A[M,K] @ W[N,K]^T + bias[N] + bias_rows[(m % period),N]) + resid[M,N]
 * N % 64 == 0, K % 32 == 0, lda/ldw % 4 == 0, A and W 16-byte aligned.  batch > 1 repeats with
 * element strides a_bs / c_bs (shared W).  resid advances by c_bs per batch as well (rows by ldr): batch b adds
 * resid + b * c_bs.  Two back ends for the same nn.Linear contract:
 *   Wp == NULL : exact-f32 MFMA (v_mfma_f32_32x32x2_f32), W = torch layout [N,K] f32
 *   Wp != NULL : split-half MFMA (3 x v_mfma_f32_32x32x16_f16 per product, f32 accumulate, ~2^-21
 *                relative per product); Wp = blob written by ctk_pack_weight, W is ignored.      */
typedef struct ctk_gemm_args {
  const float* A; int64_t lda; int32_t M;
  const float* W; int64_t ldw; int32_t N; int32_t K;
  const void* Wp;
  float* C; int64_t ldc;
  const float* bias;
  const float* bias_rows; int32_t bias_period;
  const float* resid; int64_t ldr;
  int32_t act;
  int32_t batch; int64_t a_bs; int64_t c_bs;
  int32_t k_valid;         /* non-padding columns of K (0 = K); only used for flop accounting */
  int32_t a_split;         /* A is in SH format (see below): lda / a_bs count halves, lda % 64 == 0; needs Wp */
  int32_t c_split;         /* write C in SH format: ldc / c_bs count halves, ldc % 64 == 0, no resid; needs Wp */
} ctk_gemm_args;
int ctk_gemm(const ctk_gemm_args* g, void* stream);
/* Split a torch-layout weight [N,K] (K % 32 == 0, row stride ldw) into the packed two-half form
 * the split-half back end reads: 64-byte header {s, 1/s} (s = power of two, chosen on the device
 * from max|W|) + [N][K/32][2][32] IEEE halves (hi, lo of s*W).  Done once per weight at load.   */
/* SH ("split-half") format of an activation matrix X[M][K], K % 32 == 0: IEEE halves
 * [M][K/32][2][32] -- per row and 32-column tile one 128-byte line: 32 hi halves, 32 lo halves,
 * x = hi + lo (hi = rn16(x), lo = rn16(x - hi), |x| < 65504).  Same size as f32.  The split-half
 * GEMM streams it straight into LDS; LayerNorm / attention / GEMM epilogues / token assembly can
 * emit it.  ctk_split_rows converts f32 [M][K] (row stride ld floats) to SH.                      */
/* Numeric range of the split-half format (what "fp32-class" means here; pinned by tests/test_gpu_range.py):
 *   2^-3 <~ |x| < 65504   both halves are normal f16 numbers: x is carried with >= 21 significant bits, a product of two SH
 *                          operands (3 MFMAs, f32 accumulate) has ~2^-21 relative error;
 *   |x| <~ 2^-3            `lo` falls into the f16 subnormals (step 2^-24): the error becomes ABSOLUTE, <= 2^-25 per element;
 *                          below 6.1e-5 `hi` is subnormal too -- same absolute bound.  Harmless where the consumer is on an
 *                          absolute scale (softmax logits, residual adds on an O(1) stream), which is every consumer on this
 *                          path: LayerNorm re-normalises the residual stream before every GEMM, and packed weights are
 *                          pre-scaled by a power of two into [2^13, 2^14) so their own `lo` never underflows;
 *   |x| >= 65504           `hi` overflows to inf, `lo` becomes -inf/NaN, and the non-finite value reaches the window state
 *                          (coords / vis / conf) -- nothing on the path clamps or masks it.  The library itself does not test
 *                          for it; the CoTracker3 host models check the finished window state once per forward and re-run that
 *                          forward on the exact-f32 back end (Wp == NULL everywhere) when it is non-finite (cotracker_amd/model.py,
 *                          `range_guard`; with the streaming hipGraph the check is deferred by one call and a hit RAISES instead --
 *                          INTEGRATION.md).  The CoTracker2 host model (model_v2.py, ctk_forward_window_v2) does NOT check: it is
 *                          unguarded.  A caller that drives ctk_forward_window directly should do the check itself.  Measured
 *                          margin on synthetic weights at BASELINE configs[1] scale: the MLP hidden layer has to be scaled by
 *                          3e4 before the first fallback (profiles/r03_range_sweep_c2.json).
 * The exact-f32 back end (v_mfma_f32_32x32x2_f32, f32 operands in HBM) has the reference's range and ~1/3 of the speed.    */
int ctk_split_rows(const float* x, int64_t ld, int64_t M, int32_t K, void* out, void* stream);
int ctk_pack_weight_bytes(int32_t N, int32_t K, size_t* out_bytes);
int ctk_pack_weight(const float* W, int64_t ldw, int32_t N, int32_t K, void* packed, void* stream);

/* LayerNorm over 384 channels, rows [0,R): y = (x-mean)/sqrt(var+eps) [*gamma+beta].
 * y is f32 [R,384], or SH [R][12][2][32] halves when out_split != 0: the split of the f32
 * result, bit for bit.  gamma and beta: both or neither.  A row's result depends on that row
 * alone.  x, y, gamma, beta: 16-byte aligned (CTK_E_ALIGN), checked after NULL and R <= 0.   */
int ctk_layernorm(const float* x, void* y, int64_t R, const float* gamma, const float* beta,
                  float eps, int32_t out_split, void* stream);
/* Two normalisations from one read of x (for tests: the window's launch for the point tokens
 * of a depth): y as ctk_layernorm with (gamma, beta, eps), y2 as ctk_layernorm with (NULL, NULL,
 * eps2) -- the same bits as those two calls.  Same rules; y2 is required and aligned like y. */
int ctk_layernorm_dual(const float* x, void* y, void* y2, int64_t R, const float* gamma, const float* beta,
                       float eps, float eps2, int32_t out_split, void* stream);

/* softmax(q k^T * 48^-0.5) v  (Attention.forward, blocks.py:379-398), 8 heads x 48.
 * row(b,i) = b*bs + i*is (rows of a matrix with leading dimension ld floats).           */
typedef struct ctk_attn_args {
  const float* q; int64_t q_ld; int64_t q_bs; int64_t q_is;
  const float* k; const float* v; int64_t kv_ld; int64_t kv_bs; int64_t kv_is;
  void* out; int64_t o_ld; int64_t o_bs; int64_t o_is;   /* f32, or SH halves (o_ld = 768) when o_split */
  int32_t nbatch; int32_t n1; int32_t n2;
  int32_t splits;          /* key-range splits (>1 needs workspace) */
  float* partial;          /* [splits, nbatch, 8, n1, 50] or NULL    */
  int32_t o_split;         /* write out in SH format                 */
  /* CoTracker2's attention_mask (CrossAttnBlock.forward, cotracker.py:560-572), one flag per point, shared by all
   * batches (frames) and heads; NULL = no mask.  key_mask[j] == 0: key j gets logit -FLT_MAX (probability 0 unless
   * every key is masked, then uniform -- exactly the reference's additive bias).  query_mask[i] == 0: every logit of
   * query i is -FLT_MAX, i.e. that query attends uniformly (the reference's quirk for not-yet-queried tracks).   */
  const uint8_t* key_mask;   /* [n2] */
  const uint8_t* query_mask; /* [n1] */
} ctk_attn_args;
int ctk_attention(const ctk_attn_args* a, void* stream);
/* The same operator with a TWO-LEVEL batch: batch b = bo * inner + bi (nbatch % inner == 0) and
 *   row(b, i) = bo * os + bi * bs + i * is,
 * with separate outer strides (in rows) for the queries, the keys / values and the output; the masks of outer batch bo start
 * at key_mask + bo * key_mask_os / query_mask + bo * query_mask_os (bytes).  This is the space attention of a joint window
 * (ctk_forward_window_batch): bo = video, bi = frame, and the point rows and the virtual-track rows of a video lie
 * N*S and 64*S rows apart.  b2 == NULL or inner <= 0 is ctk_attention(a): every address is then the one the single-level
 * formula gives, and the results are the same bits.  `partial` is [splits, nbatch, 8, n1, 50] over the linear b, as before.
 * 64-key, 64-query and VALU shapes run on their usual kernels; a two-level SQUARE shape other than 64 x 64 runs on the
 * VALU kernel (the time-attention kernels take single-level batches only: stacked token rows keep the tracks of all videos
 * one linear batch).                                                                                                     */
typedef struct ctk_attn_batch2 {
  int32_t inner; int32_t reserved;         /* inner batch count (frames); reserved = 0 */
  int64_t q_os; int64_t kv_os; int64_t o_os;
  int64_t key_mask_os; int64_t query_mask_os;
} ctk_attn_batch2;
int ctk_attention_ex(const ctk_attn_args* a, const ctk_attn_batch2* b2, void* stream);

/* ---- opt-in kernel timing (bench.py) ------------------------------------------------
 * When enabled, every kernel launch of this library is bracketed by two HIP events recorded on
 * the launch stream; ctk_profile_read synchronises them and returns one row per kernel with the
 * launch count, summed duration and the summed ALGORITHMIC flops/bytes of those launches.
 * Bench-only: the recorder is process-global and not thread safe (the one exception to the
 * "no mutable global state" rule above; it is off by default).                              */
typedef struct ctk_profile_row {
  char name[32];
  int64_t launches;
  double total_ms;
  double flops;
  double bytes;
} ctk_profile_row;
int ctk_profile_enable(int on);
/* ---- back-end options ------------------------------------------------------------------
 * Where the library holds two kernels for one operator, the choice is an OPTION: a process-wide table of validated integers
 * (relaxed atomics: ctk_set_option may be called from any thread at any time; a launch uses the value it reads when it is
 * enqueued).  The initial value of every option comes from its environment variable, read ONCE when the library is loaded --
 * nothing in the library calls getenv() later.  No option changes what is computed: two back ends of one operator agree to the
 * last-bit differences stated below.  Unknown keys / out-of-range values: CTK_E_SHAPE, nothing changes.
 *   key                                env var            default  values
 *   CTK_OPT_GEMM_PP                    CTK_GEMM_PP        33       bit 0: the big split-half Linears (N % 256 == 0 or N % 192 == 0, >= one
 *                                                                  256-row tile per CU) run on the persistent ping-pong kernels of
 *                                                                  csrc/gemm_pp.hip (0 = always gemm_f16x3.hip's kernels: same products, same
 *                                                                  K order, bit-identical but for the residual Linears' last bit);
 *                                                                  bit 5 (32): tail split -- a last round of tiles that would be <= TAIL_PCT %
 *                                                                  full goes to the 64 x 64-tile kernel
 *   CTK_OPT_GEMM_TAIL_PCT              CTK_GEMM_TAIL_PCT  25       0..100
 *   CTK_OPT_CORR_VERSION               CTK_CORR           3        split-half correlation sampler: 3 = wave-owned footprint rows straight into
 *                                                                  MFMA registers, 1 = the round-3 kernel (footprint through LDS, two barriers per
 *                                                                  frame); same arithmetic, volumes agree to 3e-6
 *   CTK_OPT_CORR_MAP                   CTK_CORR_MAP       3        workgroup -> (point, level) dealing of version 3: 3 = level-major (neighbouring
 *                                                                  points of a grid query run together), 0 = point-major, 1 / 2 / 4 = pairs / blocks
 *   CTK_OPT_ATTENTION_VALU             CTK_ATTN           0        1 = every attention shape on the VALU kernel (the fallback of the MFMA kernels)
 *   CTK_OPT_ATTENTION_TIME_PERSISTENT  CTK_ATTN_TIME      1        time attention over <= 16 frames without masks: 1 = persistent; where q | k | v of
 *                                                                  16-frame tracks are one row-contiguous block of leading dimension 1152 (the
 *                                                                  update transformer's layout) and there are at least 8 track pairs per CU, one
 *                                                                  workgroup per track pair reads whole blocks, else one wave per (pair, head);
 *                                                                  2 = one wave per (pair, head) everywhere; 3 = as 1 at any number of pairs;
 *                                                                  0 = the non-persistent kernel (all four bit-identical)
 *   CTK_OPT_OVERLAP                    CTK_OVERLAP        0        use of ctk_window_args.aux_stream: bit 0 = sampler of one point piece beside
 *                                                                  corr_mlp of the previous one, bit 1 = the points<-virtual query projection
 *                                                                  beside the virtual-track chain (bit-identical; measured <= 0.2 % either way) */
enum {
  CTK_OPT_GEMM_PP = 0,
  CTK_OPT_GEMM_TAIL_PCT = 1,
  CTK_OPT_CORR_VERSION = 2,
  CTK_OPT_CORR_MAP = 3,
  CTK_OPT_ATTENTION_VALU = 4,
  CTK_OPT_ATTENTION_TIME_PERSISTENT = 5,
  CTK_OPT_OVERLAP = 6,
  CTK_OPT_COUNT = 7
};
int ctk_set_option(int key, int value);
int ctk_get_option(int key, int* value);
/* = ctk_set_option(CTK_OPT_GEMM_PP, mode), ignoring an invalid mode (the pre-v9 name) */
void ctk_gemm_pp_mode(int mode);
int ctk_profile_read(ctk_profile_row* rows, int max_rows, int* nrows);
/* Register-only MFMA loop (2 workgroups x 4 waves per CU) to calibrate the sustained peak of this
 * chip under its power budget: kind 0 = v_mfma_f32_32x32x2_f32, 1 = v_mfma_f32_32x32x16_bf16 (constant operands),
 * 2 = v_mfma_f32_32x32x16_f16 on pseudo-random operands (the instruction and the toggle activity of the split-half
 * kernels: bench.py's `sustained_mfma` figure).  Any other kind: CTK_E_SHAPE.                                   */
int ctk_probe_mfma(int kind, int iters, float* scratch, double* flops, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CTK_H_ */
