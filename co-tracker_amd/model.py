"""CoTracker3 tracker models on the MI355X hot path.

Host-side mirror of the reference's model interface:
  CoTrackerThreeOnline   <- cotracker/models/core/cotracker/cotracker3_online.py:159-541
  CoTrackerThreeOffline  <- cotracker/models/core/cotracker/cotracker3_offline.py:15-233
Same constructor kwargs, attributes (model_resolution, window_len, stride), ``forward``
signature / return tuple, online-state methods and -- crucially -- the same ``state_dict`` key
set, so reference checkpoints load unchanged and a reference ``CoTrackerPredictor`` can have its
``.model`` swapped for one of these.

Everything numeric runs in the HIP library through ``cotracker_amd.ops`` / ``encoder_hip``: the CNN
encoder (split-half implicit-GEMM convolutions, round 3; the PyTorch-ROCm / MIOpen encoder stays selectable
with ``encoder_backend = "torch"`` for A/B), feature normalisation + pyramid, support sampling, and the 6x
iterative update (correlation sampling, corr MLP, token assembly, EfficientUpdateFormer, state update).
Window scheduling and online state are Python glue, as in the reference.
Inference only (``is_train`` must be False).
"""
import contextlib
import copy
import operator
import warnings
from dataclasses import dataclass, replace
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import ops
from .encoder import BasicEncoder


# ------------------------------------------------------------------------------------------
# parameter containers: same names / shapes as the reference modules, no forward of their own
# ------------------------------------------------------------------------------------------
class _Lin(nn.Module):
    def __init__(self, fin, fout):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(fout, fin))
        self.bias = nn.Parameter(torch.zeros(fout))
        nn.init.xavier_uniform_(self.weight)  # cotracker.py:465-469


class _Mlp(nn.Module):  # blocks.py:40-76
    def __init__(self, fin, hidden, fout):
        super().__init__()
        self.fc1 = _Lin(fin, hidden)
        self.fc2 = _Lin(hidden, fout)


class _Attn(nn.Module):  # blocks.py:365-377
    def __init__(self, dim=384):
        super().__init__()
        self.to_q = _Lin(dim, dim)
        self.to_kv = _Lin(dim, 2 * dim)
        self.to_out = _Lin(dim, dim)


class _AttnBlock(nn.Module):  # blocks.py:401-424 (both LayerNorms are parameter-free)
    def __init__(self, dim=384, ratio=4):
        super().__init__()
        self.attn = _Attn(dim)
        self.mlp = _Mlp(dim, dim * ratio, dim)


class _Affine(nn.Module):  # nn.LayerNorm(384) parameters (cotracker.py:540)
    def __init__(self, dim=384):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))


class _CrossBlock(nn.Module):  # cotracker.py:534-557
    def __init__(self, dim=384, ratio=4):
        super().__init__()
        self.norm_context = _Affine(dim)
        self.cross_attn = _Attn(dim)
        self.mlp = _Mlp(dim, dim * ratio, dim)


class _UpdateFormerParams(nn.Module):  # cotracker.py:387-462
    def __init__(self, input_dim=1110, hidden=384, depth=3, num_virtual_tracks=64, flow_out=2, vis_conf_head=True, space_attn=True):
        """CoTracker3: flow_head(2) + vis_conf_head(2) (linear_layer_for_vis_conf=True) or one flow_head(4) (False);
        CoTracker2: one flow_head of output_dim = 130 and no vis_conf_head (cotracker.py:410-414).  space_attn=False
        (constructor add_space_attn=False): the three space block lists do not exist, as in cotracker.py:432-460."""
        super().__init__()
        self.input_transform = _Lin(input_dim, hidden)
        self.flow_head = _Lin(hidden, flow_out)
        nn.init.trunc_normal_(self.flow_head.weight, std=0.001)
        if vis_conf_head:
            self.vis_conf_head = _Lin(hidden, 2)
            nn.init.trunc_normal_(self.vis_conf_head.weight, std=0.001)
        self.virual_tracks = nn.Parameter(torch.randn(1, num_virtual_tracks, 1, hidden))  # (sic) reference key
        self.time_blocks = nn.ModuleList([_AttnBlock(hidden) for _ in range(depth)])
        if not space_attn:
            return
        self.space_virtual_blocks = nn.ModuleList([_AttnBlock(hidden) for _ in range(depth)])
        self.space_point2virtual_blocks = nn.ModuleList([_CrossBlock(hidden) for _ in range(depth)])
        self.space_virtual2point_blocks = nn.ModuleList([_CrossBlock(hidden) for _ in range(depth)])


DEFAULT_PRECISION = "f16x3"  # Linear back end of newly built models ("f16x3" | "f32"), see TrackerBase.precision


def sincos_time_embed(dim: int, window_len: int) -> torch.Tensor:
    """get_1d_sincos_pos_embed_from_grid on linspace(0, W-1, W) (embeddings.py:59-84) -> [1,W,dim]."""
    omega = torch.arange(dim // 2, dtype=torch.double) / (dim / 2.0)
    omega = 1.0 / 10000 ** omega
    pos = torch.linspace(0, window_len - 1, window_len).double()
    out = torch.einsum("m,d->md", pos, omega)
    return torch.cat([torch.sin(out), torch.cos(out)], dim=1)[None].float()


def interpolate_time_embed(te: torch.Tensor, S: int) -> torch.Tensor:
    """interpolate_time_embed (cotracker3_online.py:145-156): te [1,W,D] -> [S,D]."""
    if S != te.shape[1]:
        te = F.interpolate(te.permute(0, 2, 1), size=S, mode="linear").permute(0, 2, 1)
    return te[0]


def fold_input_weights(in_w: torch.Tensor, fc2_w: torch.Tensor, fc2_b: torch.Tensor):
    """corr_mlp.fc2 folded into input_transform (include/ctk.h, ctk_model_weights "folded form").  Nothing nonlinear lies between
    the two (cotracker3_online.py:205-247), so with Win_l = the 256 columns of input_transform.weight that read level l's embedding
        W x + b = sum_l (Win_l W2) h1_l + W_small x_small + (b + sum_l Win_l b2),       h1_l = GELU(fc1(volume_l)).
    in_w [384,1110] in the reference's column order [vis, conf, corr(4 x 256), posenc(84)], fc2_w [256,384], fc2_b [256] ->
    (weight [384, XF_LD] in the xf column order: 4 x 384 hidden, vis, conf, posenc, zero padding;  sum_l Win_l b2 [384]), float64."""
    w, w2, b2 = in_w.double(), fc2_w.double(), fc2_b.double()
    out = torch.zeros(w.shape[0], L.XF_LD, dtype=torch.float64, device=w.device)
    extra = torch.zeros(w.shape[0], dtype=torch.float64, device=w.device)
    for l in range(L.LEVELS):
        w_l = w[:, 2 + 256 * l:2 + 256 * (l + 1)]
        out[:, L.HID * l:L.HID * (l + 1)] = w_l @ w2
        extra += w_l @ b2
    out[:, L.XF_SMALL:L.XF_SMALL + 2] = w[:, 0:2]
    out[:, L.XF_SMALL + 2:L.XF_SMALL + 86] = w[:, 1026:1110]
    return out, extra


def input_bias_rows(te: torch.Tensor, in_w: torch.Tensor, in_b: torch.Tensor, extra: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The per-frame bias of the input projection, float64 [S,384]: input_transform(x + e_t) = W x + (W e_t + b)
    (cotracker3_online.py:247 + cotracker.py:484), plus `extra` (fold_input_weights) on the folded path."""
    rows = te.double() @ in_w.double().t() + in_b.double()
    return rows if extra is None else rows + extra.double()


# ------------------------------------------------------------------------------------------
# device-side packed weights (the ctk_model_weights struct of include/ctk.h)
# ------------------------------------------------------------------------------------------
class PackedWeights:
    """Contiguous fp32 device copies in the layouts the C-ABI wants, plus the ctypes struct."""

    def __init__(self, model: "CoTrackerThreeBase", device, precision: str = "f16x3"):
        if precision not in ("f16x3", "f32"):
            raise ValueError("precision must be 'f16x3' (split-half MFMA, default) or 'f32' (exact-f32 MFMA)")
        self.precision = precision
        split = precision == "f16x3"
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in model.state_dict().items()}
        self.device = device
        self.keep: List[torch.Tensor] = []
        self.time_emb = sd["time_emb"]  # [1,W,1110], reference column order
        st = L.ModelWeights()

        def hold(t: torch.Tensor) -> int:
            t = t.contiguous()
            self.keep.append(t)
            return t.data_ptr()

        def pack(t: torch.Tensor):
            """ctk_pack_weight blob of a Linear weight (None in exact-f32 mode)."""
            if not split:
                return None
            blob = ops.pack_weight(t.contiguous())
            self.keep.append(blob)
            return blob.data_ptr()

        fc1 = torch.zeros(384, L.CORR_LD, device=device)
        fc1[:, : L.CORR_K] = sd["corr_mlp.fc1.weight"]
        st.corr_fc1_w = hold(fc1)
        st.corr_fc1_p = pack(fc1)
        st.corr_fc2_p = pack(sd["corr_mlp.fc2.weight"])
        st.corr_fc1_b = hold(sd["corr_mlp.fc1.bias"])
        st.corr_fc2_w = hold(sd["corr_mlp.fc2.weight"])
        st.corr_fc2_b = hold(sd["corr_mlp.fc2.bias"])

        u = "updateformer."
        w_ref = sd[u + "input_transform.weight"]  # columns: [vis, conf, corr(1024), posenc(84)]
        self.in_w_ref = w_ref
        self.in_b = sd[u + "input_transform.bias"]
        in_w = torch.zeros(384, L.X_LD, device=device)
        in_w[:, 0:1024] = w_ref[:, 2:1026]
        in_w[:, 1024:1026] = w_ref[:, 0:2]
        in_w[:, 1026:1110] = w_ref[:, 1026:1110]
        st.in_w = hold(in_w)
        st.in_p = pack(in_w)
        st.virtual_tokens = hold(sd[u + "virual_tracks"].reshape(64, 384))
        if u + "vis_conf_head.weight" in sd:  # linear_layer_for_vis_conf=True: two heads, concatenated (cotracker.py:526-529)
            st.head_w = hold(torch.cat([sd[u + "flow_head.weight"], sd[u + "vis_conf_head.weight"]], dim=0))
            st.head_b = hold(torch.cat([sd[u + "flow_head.bias"], sd[u + "vis_conf_head.bias"]], dim=0))
        else:                                  # linear_layer_for_vis_conf=False: ONE Linear(384, 4) = the same [4,384] matrix
            assert sd[u + "flow_head.weight"].shape == (4, 384)
            st.head_w, st.head_b = hold(sd[u + "flow_head.weight"]), hold(sd[u + "flow_head.bias"])

        def block(prefix: str, attn_name: str, cross: bool) -> L.BlockWeights:
            b = L.BlockWeights()
            a = f"{prefix}{attn_name}."
            b.wq, b.bq = hold(sd[a + "to_q.weight"]), hold(sd[a + "to_q.bias"])
            b.wkv, b.bkv = hold(sd[a + "to_kv.weight"]), hold(sd[a + "to_kv.bias"])
            b.wo, b.bo = hold(sd[a + "to_out.weight"]), hold(sd[a + "to_out.bias"])
            b.w1, b.b1 = hold(sd[prefix + "mlp.fc1.weight"]), hold(sd[prefix + "mlp.fc1.bias"])
            b.w2, b.b2 = hold(sd[prefix + "mlp.fc2.weight"]), hold(sd[prefix + "mlp.fc2.bias"])
            b.wq_p, b.wkv_p, b.wo_p = pack(sd[a + "to_q.weight"]), pack(sd[a + "to_kv.weight"]), pack(sd[a + "to_out.weight"])
            b.w1_p, b.w2_p = pack(sd[prefix + "mlp.fc1.weight"]), pack(sd[prefix + "mlp.fc2.weight"])
            if cross:
                b.ctx_gamma = hold(sd[prefix + "norm_context.weight"])
                b.ctx_beta = hold(sd[prefix + "norm_context.bias"])
            return b

        has_space = f"{u}space_virtual_blocks.0.attn.to_q.weight" in sd
        for i in range(L.DEPTH):
            st.time_blocks[i] = block(f"{u}time_blocks.{i}.", "attn", False)
            if not has_space:
                # constructor add_space_attn=False: the model has no space blocks and every window runs with
                # CTK_WINDOW_NO_SPACE_ATTN, which never dereferences these slots; ctk_forward_window still validates them, so
                # they alias the time block (norm_context of the cross slots: any 384 floats)
                st.virtual_self[i] = st.virtual2point[i] = st.point2virtual[i] = st.time_blocks[i]
                st.virtual2point[i].ctx_gamma = st.point2virtual[i].ctx_gamma = st.time_blocks[i].bq
                st.virtual2point[i].ctx_beta = st.point2virtual[i].ctx_beta = st.time_blocks[i].bq
                continue
            st.virtual_self[i] = block(f"{u}space_virtual_blocks.{i}.", "attn", False)
            st.virtual2point[i] = block(f"{u}space_virtual2point_blocks.{i}.", "cross_attn", True)
            st.point2virtual[i] = block(f"{u}space_point2virtual_blocks.{i}.", "cross_attn", True)
        self.struct = st
        # The window path's struct: corr_mlp.fc2 folded into the input projection (one big GEMM less per iteration).  The
        # products are formed once here, in float64, and rounded once; the struct above stays for the stage operators.
        in_wf, self._bias_fold = fold_input_weights(w_ref, sd["corr_mlp.fc2.weight"], sd["corr_mlp.fc2.bias"])
        in_wf = in_wf.float()
        sf = L.ModelWeights.from_buffer_copy(st)
        sf.corr_fc2_w = sf.corr_fc2_p = sf.corr_fc2_b = None
        sf.in_w, sf.in_p = hold(in_wf), pack(in_wf)
        self.struct_folded = sf
        self._bias_t = {}

    def time_embed(self, S: int) -> torch.Tensor:
        """interpolate_time_embed (cotracker3_online.py:145-156) -> [S,1110] reference column order."""
        return interpolate_time_embed(self.time_emb, S)

    def struct_for(self, S: int, folded: bool = False) -> L.ModelWeights:
        """Struct whose in_bias_t folds the S-frame time embedding into the input projection:
        input_transform(x + e_t) = W x + (W e_t + b)   (cotracker3_online.py:247 + cotracker.py:484).
        folded: the struct of the window calls (fc2 inside the projection; its bias rows carry fc2's bias too)."""
        if (S, folded) not in self._bias_t:
            rows = input_bias_rows(self.time_embed(S), self.in_w_ref, self.in_b, self._bias_fold if folded else None)
            self._bias_t[S, folded] = rows.float().contiguous()
        st = self.struct_folded if folded else self.struct
        st.in_bias_t = self._bias_t[S, folded].data_ptr()
        return st


# ------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------
def tail_aliases(prev, cur, dim, step):
    """True iff `cur` is the window of the SAME live allocation as `prev`, advanced by `step` entries along `dim` (so that
    cur[..., :n-step, ...] and prev[..., step:, ...] are the same bytes) and nothing wrote to that allocation through a
    tensor sharing its version counter in between.  Host-side metadata only: no kernel, no synchronisation.  The caller
    must have kept `prev` alive since it was recorded (a freed allocation could be handed out again at the same address)."""
    if prev is None or cur is None or prev.shape != cur.shape or prev.dtype != cur.dtype or prev.device != cur.device:
        return False
    if prev.stride() != cur.stride() or cur.shape[dim] <= step:
        return False
    try:
        same = prev.untyped_storage().data_ptr() == cur.untyped_storage().data_ptr()
    except Exception:  # storage-less tensors
        return False
    if not (same and cur.storage_offset() == prev.storage_offset() + step * prev.stride(dim)):
        return False
    # Tensors created under torch.inference_mode() do not track a version counter (reading `_version` raises): writes to them
    # cannot be seen from the host, so the overlap cannot be PROVEN -> not an alias, the caller re-encodes (advisor, round 4).
    try:
        recorded = prev._ctk_version if hasattr(prev, "_ctk_version") else prev._version
        return bool(recorded == cur._version)
    except Exception:
        return False


@dataclass
class OnlineState:
    """The online state of ONE video (the reference batches it inside its state tensors, cotracker3_online.py:163-169 /
    cotracker.py:187-191; here every batch element owns one).  The tensors in it are never written in place -- every update
    rebinds the field -- so a shallow copy (dataclasses.replace) is a snapshot."""
    ind: int = 0
    track_support: Optional[list] = None   # CoTracker3: the accumulated support features, one [N,49,128] per level
    track_feat: Optional[torch.Tensor] = None  # CoTracker2: the accumulated track features [S,N,128]
    coords_predicted: Optional[torch.Tensor] = None
    vis_predicted: Optional[torch.Tensor] = None
    conf_predicted: Optional[torch.Tensor] = None
    f0_tail: Optional[torch.Tensor] = None      # level-0 features of the frames the NEXT chunk starts with (feature cache)
    prev_frames: Optional[torch.Tensor] = None  # the previous chunk itself (a reference), to prove the overlap on the host

    def __getstate__(self):  # pickles / deep copies: the feature cache is tied to a live allocation and rebuilt on demand
        return {**self.__dict__, "f0_tail": None, "prev_frames": None}


def _online_attr(field):
    """A reference-visible ``online_*`` attribute: that field of the online state (B > 1: of the last batch element)."""
    return property(lambda self: getattr(self._online[-1], field))


class TrackerBase(nn.Module):
    """What CoTrackerThreeBase and CoTracker2 (model_v2.py) share and the reference does not have: the attributes that are not
    reference kwargs, the packed-weight and graph caches, pickling, the f16 range guard, and the forward path over B videos."""

    PACKED_WEIGHTS = None  # the packed-weights class of the model family
    stream_window_start = None  # (a model pickled before the attribute existed)
    BATCH_MODES = ("loop", "joint")

    def __init__(self):
        super().__init__()
        self._packed = {}  # precision -> PACKED_WEIGHTS
        self._hip_encoder = None  # encoder_hip.HipEncoder for the current device (repacked convolution weights)
        # arithmetic of the Linear layers: "f16x3" = split-half MFMA (3 f16 MFMAs per product, f32 accumulate,
        # fp32-class accuracy at 5.3x the f32-MFMA ceiling), "f32" = exact-f32 MFMA.  Not a reference kwarg.
        self.precision = DEFAULT_PRECISION
        # hipGraph replay of the streaming window (BASELINE.json configs[3]): with is_online=True the whole
        # window (iters x ~190 launches) is captured once per (S, N, iters) and replayed with one graph launch
        # per chunk.  Not a reference kwarg; CoTrackerOnlinePredictor switches it on.
        self.hip_graph = False
        self._graphs = {}
        # f16 range guard of the split-half back end (include/ctk.h "numeric range"): an activation beyond +-65504
        # becomes inf/NaN in its hi/lo halves and reaches the window state as a non-finite value (nothing on the path
        # clamps or masks it), so every forward checks its outputs once and, on a hit, re-runs that forward on the
        # exact-f32 MFMA back end of the same library (fp32 range, as the reference).  range_fallbacks counts hits.
        self.range_guard = True
        self.range_fallbacks = 0
        # graph streaming only: "deferred" (default) examines a chunk's finiteness flag at the start of the NEXT call, so the
        # stream of chunk calls never waits for the GPU -- a hit then raises (the chunk was already returned); "immediate" waits
        # for the flag inside the call (one device-to-host sync per chunk) and, on a hit, restores the online state and re-runs
        # that chunk on the exact-f32 back end before returning it -- the behaviour of every non-streaming path.
        self.stream_range_check = "deferred"
        self._pending_range = None
        # "hip" (default): the CNN runs on the library's split-half implicit-GEMM convolutions (encoder_hip.py, csrc/conv_pp.hip,
        # csrc/encoder.hip) -- fp32-class accuracy at 2.2x the speed of MIOpen's fp32 convolutions; "torch": nn.Conv2d on
        # PyTorch-ROCm / MIOpen (the round-1/2 path, kept for A/B and for `encoder_dtype` experiments).  Not a reference kwarg.
        self.encoder_backend = "hip"
        self.encoder_chunk = 16  # frames per CNN call (see _encode); not a reference kwarg
        # pre-sigmoid outputs of the last forward, [B,T,N] each -- (visibility, confidence), CoTracker2: (visibility,); parity
        # tests compare logits
        self.last_logits = None
        # B > 1: "loop" (default) runs the B videos one after the other, each through its own window calls; "joint" runs every
        # window / iteration chain ONCE for all B videos (ctk_forward_window_batch: one launch per Linear over B times the
        # rows) and the encoder on the B*T frames as one frame batch.  Results are fp32-class equal to "loop", not
        # bit-identical (include/ctk.h).  Not a reference kwarg: set it after construction, like hip_graph and precision.
        # A query-group call -- video [1,T,3,H,W] with queries [G,N,3], G > 1 -- tracks G independent query sets over the ONE
        # video: the encoder, the pyramid and the support sampling run once for the call, and the groups' windows run one after
        # the other ("loop": bit-identical to G separate calls) or as joint windows of up to CTK_MAX_BATCH groups that share the
        # pyramid ("joint": ctk_window_batch.flags = CTK_BATCH_SHARED_FMAPS).  Returns [G,T,N,.] tensors.  Offline / sliding; streaming: stream_groups below.
        self.batch_mode = "loop"
        # Streaming query groups (CoTracker3 online model only; opt-in like batch_mode / online_feature_cache): with it on,
        # forward(video [1,T,3,H,W], queries [G,N,3], is_online=True), G > 1, streams G independent query sets over the ONE live
        # video -- one encoder run and one pyramid per chunk, the stream state of all groups resident on the device and stepped by
        # three launches per call (ops.StreamGroups, csrc/stream.hip), the groups' windows one after the other ("loop":
        # bit-identical to G single-group streams) or as shared-pyramid joint windows ("joint").  Off: that call raises, as before.
        self.stream_groups = False
        # Slots on a running stream (CoTracker3 online model only; opt-in): with it on, EVERY forward(video [1,T,3,H,W], queries
        # [G,N,3], is_online=True) -- G == 1 included, which otherwise takes the torch glue of _video_gen -- runs on the
        # device-resident stream state and returns [G,T_so_far,N,.].  A row of the query table whose frame is ops.EMPTY_FRAME (and
        # whose position is (0, 0)) is an EMPTY SLOT: tracked as the reference tracks a query that has not arrived (a blank token of
        # the space attention: the number of spare slots is part of the result, as the support grid is).  Between two calls
        # stream_assign() hands slots to new queries and stream_release() empties them: writes into resident buffers, so no shape,
        # no address and no captured graph changes.  More than one video with the switch on: NotImplementedError.
        self.stream_slots = False
        # Endless streams (CoTracker3 online model only; opt-in): None (default), or K >= window_len frames of history.  Read at
        # the FIRST call of a stream.  With it set, every streaming call -- forward(..., is_online=True) chunks and stream_push,
        # G == 1 included, both batch_modes, with and without hip_graph -- runs on the device stream state with a RING history of
        # K rows (ops.StreamGroups(ring_rows=K): frame f in row f % K, allocated once) and returns THIS WINDOW's rows only:
        # (coords [G,T,N,2], sigmoid(vis), sigmoid(conf), None) for frames stream_window_start .. stream_window_start + T - 1,
        # copied out of the ring by one launch (ctk_stream_emit; the bits the default mode returns for those rows).  Memory and
        # the cost of a call no longer depend on the age of the stream; nothing is re-allocated or re-captured after the first
        # window.  The first window_len - window_len // 2 rows of a call supersede what the previous call returned for those
        # frames; older rows are final.  last_logits are the emitted logits, and the reference-visible online_coords_predicted /
        # online_vis_predicted / online_conf_predicted are the RING buffers [G,K,N,.] (row f % K holds frame f), not [.,T_so_far,.].
        # stream_assign / stream_release clear all K rows of a slot.  Frame numbers are float32 in the query table, so a stream
        # ends before frame 2^24 (about 6 days at 30 fps): the call whose window would reach it raises RuntimeError before any
        # launch.  More than one video with it set: NotImplementedError.
        self.stream_history_frames = None
        self.stream_window_start = None  # the frame number of row 0 of the last return under stream_history_frames

    @property
    def stream_history_frames(self) -> Optional[int]:
        return getattr(self, "_stream_history_frames", None)  # (a model pickled before the attribute existed)

    @stream_history_frames.setter
    def stream_history_frames(self, K):
        if K is not None:
            try:
                K = None if isinstance(K, bool) else operator.index(K)
            except TypeError:
                K = None
            if K is None:
                raise ValueError("stream_history_frames must be None or an int >= window_len")
            S = getattr(self, "window_len", None)
            if K < (S if S is not None else 1):
                raise ValueError(f"stream_history_frames must be None or an int >= window_len ({S}), got {K}")
        self._stream_history_frames = K

    @property
    def stream_slots(self) -> bool:
        return getattr(self, "_stream_slots", False)  # (a model pickled before the attribute existed)

    @stream_slots.setter
    def stream_slots(self, on):
        self._stream_slots = bool(on)

    @property
    def stream_groups(self) -> bool:
        return getattr(self, "_stream_groups", False)  # (a model pickled before the attribute existed)

    @stream_groups.setter
    def stream_groups(self, on):
        self._stream_groups = bool(on)

    @property
    def batch_mode(self) -> str:
        return getattr(self, "_batch_mode", "loop")  # (a model pickled before the attribute existed)

    @batch_mode.setter
    def batch_mode(self, mode):
        if mode not in self.BATCH_MODES:
            raise ValueError(f"batch_mode must be one of {self.BATCH_MODES}, got {mode!r}")
        self._batch_mode = mode

    # -- weights ------------------------------------------------------------------------
    def load_state_dict(self, *args, **kwargs):
        self.invalidate_packed_weights()
        return super().load_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self.invalidate_packed_weights()
        return super()._apply(fn, *args, **kwargs)

    def packed(self, device, precision: Optional[str] = None):
        precision = precision or self.precision
        pw = self._packed.get(precision)
        if pw is None or pw.device != device:
            pw = self._packed[precision] = self.PACKED_WEIGHTS(self, device, precision)
        return pw

    def invalidate_packed_weights(self):
        """Call after mutating parameters in place (e.g. weights.fill_synthetic_)."""
        self._packed = {}
        self._hip_encoder = None
        self._drop_graphs()  # captured graphs hold pointers into the old packed weights

    def _drop_graphs(self):
        if getattr(self, "_graphs", None):
            # a replay may still be in flight on the current stream: destroying the exec / freeing its private
            # workspace under it is undefined, so drain first
            if torch.cuda.is_available():
                torch.cuda.current_stream().synchronize()
            self._graphs = {}

    def _graph_cache(self, generation, pw):
        """The one cache of captured window graphs, self._graphs.  A graph bakes in its buffers, the weights `pw` and the option
        table as read at capture, so those join `generation` -- what the caller's graphs have in common (shapes, iters, model
        settings) -- in every key.  ONE eviction rule: graphs of any other generation are dropped (their workspaces freed) before
        a new one is captured.  The host paths have one graph per generation, so one live graph per model; the sub-batches of a
        streaming query-group call (G = 18 in joint mode: 16 + 2) are the members of one.  Returns get(member, build) -> the
        member's graph, captured by build() on a miss."""
        gen = (generation, id(pw), pw.device.index, L.option_values())
        if any(k[0] != gen for k in self._graphs):
            self._drop_graphs()

        def get(member, build):
            if (gen, member) not in self._graphs:
                self._graphs[gen, member] = build()
            return self._graphs[gen, member]
        return get

    def _graphed_windows(self, reqs, iters, pw, ident=(), **window_kw):
        """Streaming with hip_graph: one window per request (see _run_windows) through ONE captured hipGraph per (shapes, iters,
        model settings `ident`, number of requests).  It is captured on private clones of the first call's windows (the static
        buffers), which later calls refresh in place before the replay.  Returns every window's result(): views of the static
        buffers, overwritten by the next replay (CoTracker3 consumes them at once; CoTracker2 hands out clones, as ever)."""
        captured = []

        def capture():
            captured.extend(self._window(r, iters, **window_kw).clone() for r in reqs)
            return self._window_graph(captured, pw, len(reqs) > 1)
        shapes = tuple(t_.shape for t_ in ops.window_tensors(reqs[0]))
        g = self._graph_cache((shapes, len(reqs), int(iters), ident), pw)(None, capture)
        if not captured:
            for win, r in zip(g.wins, reqs):
                win.refresh(r)
        g.launch()
        return [w_.result() for w_ in g.wins]

    # device-side caches (ctypes structs with raw pointers) are rebuilt on demand: keep them out of pickles / deep copies
    # (the online state is ordinary tensors and is copied, less its feature cache: OnlineState.__getstate__)
    _TRANSIENT = {"_packed": dict, "_graphs": dict, "_hip_encoder": type(None), "_pending_range": type(None)}

    def __getstate__(self):
        # a pending (pinned flag, cuda Event) pair cannot be pickled, and must not be lost: pickling (like deepcopy) a model in
        # the middle of a graph stream waits for the last chunk and may raise FloatingPointError
        self._resolve_deferred_range_check()
        st = self.__dict__.copy()
        for k, mk in self._TRANSIENT.items():
            if k in st:
                st[k] = mk()
        return st

    def __setstate__(self, state):
        super().__setstate__(state)
        for k, mk in self._TRANSIENT.items():  # (a pickle of an earlier tree may hold None where this one holds {})
            if k in self.__dict__:
                self.__dict__[k] = mk()

    def __deepcopy__(self, memo):
        cls = self.__class__
        # may synchronise and raise FloatingPointError (a pending deferred range check of graph streaming): do it BEFORE the
        # half-built copy is registered in memo, so a raise leaves no partial object behind
        self._resolve_deferred_range_check()
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = self._TRANSIENT[k]() if k in self._TRANSIENT else copy.deepcopy(v, memo)
        return new

    # -- f16 range guard ----------------------------------------------------------------
    def _guarded(self, run, snapshot, restore, deferred=False, nonfinite=None, what="forward"):
        """run(precision, check) -> outputs (coords, vis_logit[, conf_logit]) under the f16 range guard described in __init__;
        check: whether the guard examines this run.  The verdict is read from the outputs (all finite?) or, `nonfinite` given,
        from that device flag word, which the run raises itself (non-zero: something was not finite).  On a hit the state is put
        back -- restore(what snapshot() returned before the run) -- and `what` re-runs on the exact-f32 back end.
        deferred=True (streaming): the flag of this call is copied to the host asynchronously and examined at the START of the
        next call, so the stream of chunk calls never waits for the GPU; a hit then raises (the chunk that overflowed has
        already been returned, and the online state is poisoned: the stream must be re-run with ``precision="f32"``)."""
        self._resolve_deferred_range_check()
        guard = self.precision == "f16x3" and self.range_guard
        saved = snapshot() if guard and not deferred else None
        out = run(self.precision, guard)
        if not guard:
            return out
        # (flag, the value of it that means "fine"): interpreted on the host, whichever way round the device computed it
        flag, fine = (torch.stack([torch.isfinite(o).all() for o in out]).all(), True) if nonfinite is None else (nonfinite, 0)
        if deferred:
            pinned = torch.empty(flag.shape, dtype=flag.dtype, pin_memory=True)
            pinned.copy_(flag, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._pending_range = (pinned, fine, ev)
        elif flag.item() != fine:
            self.range_fallbacks += 1
            warnings.warn("cotracker_amd: non-finite tracks from the split-half (f16x3) back end -- an activation left "
                          f"the f16 range (|x| < 65504) or the input is non-finite; re-running this {what} on the "
                          "exact-f32 MFMA back end", RuntimeWarning, stacklevel=3)
            restore(saved)
            out = run("f32", False)
        return out

    def _resolve_deferred_range_check(self):
        pending, self._pending_range = getattr(self, "_pending_range", None), None
        if pending is not None:
            pinned, fine, ev = pending
            ev.synchronize()
            if pinned.item() != fine:
                self.range_fallbacks += 1
                raise FloatingPointError("cotracker_amd: the previous streaming chunk produced non-finite tracks on the "
                                         "split-half (f16x3) back end (an activation left the f16 range |x| < 65504, or the "
                                         "input was non-finite); restart the stream with model.precision = 'f32'")

    # -- the forward path: B videos, loop or joint, offline / sliding / streaming --------
    def _check_call(self, video, is_train):
        if is_train:
            raise NotImplementedError("inference-only implementation (training is out of scope)")
        if not video.is_cuda:
            raise RuntimeError("cotracker_amd runs on an MI355X GPU only: move the model and inputs to 'cuda'. "
                               "There is no CPU path.")

    def _online_states(self, B, T):
        """The per-video states of a streaming call (is_online=True): one OnlineState per batch element."""
        assert T <= self.window_len, "Online mode: video chunk must be <= window size."
        assert getattr(self, "_online", None), "Call model.init_video_online_processing() first."
        if len(self._online) == 1 and B > 1:  # every element starts from the state init_video_online_processing left
            self._online = [replace(self._online[0]) for _ in range(B)]
        assert len(self._online) == B, "batch size changed between online calls"
        return self._online

    def _track(self, video, iters, make_gens, states=None, units=None, **window_kw):
        """The one forward path.  make_gens(group) -> one generator per video of `group` (a list of batch indices): one
        video's host code, which yields one window request per window, receives that window's result and returns that video's
        logits (coords, vis[, conf]).  The videos are grouped -- groups of one in "loop" mode, ONE group of B in "joint" mode --
        and each group advances in lock step, all its requests going through one _run_windows call.  The range guard wraps one
        group: "loop" checks every video and re-runs a hit on the exact-f32 back end on its own; "joint" checks the stacked
        outputs once and re-runs the whole batch.  states: the OnlineStates of a streaming call (None: offline / sliding), put
        back as they were before the re-run.  units: the G query groups of a query-group call (one video; see __init__) -- they
        take the place of the B videos, and "joint" runs them in sub-batches of at most CTK_MAX_BATCH, each under its own
        range guard.  Returns forward's tuple: (coords, sigmoid of every logit ..., None)."""
        joint, groups = self._index_groups(video.shape[0] if units is None else units, units is not None)
        graphed = bool(states is not None and self.hip_graph)
        # streaming with the window graph (CoTrackerOnlinePredictor): deferred range check, the chunk stream stays asynchronous
        deferred = graphed and len(groups) == 1 and self.stream_range_check == "deferred"
        parts = []
        for group in groups:
            def run(precision, _check):
                pw = self.packed(video.device, precision)
                outs = self._drive(make_gens(group), lambda reqs: self._run_windows(reqs, iters, pw, graphed, **window_kw))
                return tuple(torch.stack(o) for o in zip(*outs)) if joint else outs[0]

            def restore(saved):  # (offline / sliding: no online state to put back before the exact-f32 re-run)
                for b, st in zip(group, saved or ()):
                    states[b] = st
            parts.append(self._guarded(run, lambda: states and [replace(states[b]) for b in group], restore, deferred))
        if joint:
            out = parts[0] if len(parts) == 1 else tuple(torch.cat(o) for o in zip(*parts))
        else:
            out = tuple(torch.stack(o) for o in zip(*parts))
        self.last_logits = out[1:]
        return (out[0], *[torch.sigmoid(o) for o in out[1:]], None)

    def _index_groups(self, n, units=False):
        """How a call over n videos -- or over the n query groups of one video (units) -- splits into window calls: -> (joint,
        index groups).  "loop": one index per group; "joint": ONE group of all n videos, or sub-batches of at most CTK_MAX_BATCH
        query groups."""
        joint = n > 1 and self.batch_mode == "joint"
        size = (L.MAX_BATCH if units else n) if joint else 1
        return joint, [list(range(i, min(i + size, n))) for i in range(0, n, size)]

    @staticmethod
    def _drive(gens, run_windows):
        """Advance the per-video generators in lock step: collect one window request from each, run them with
        run_windows(requests) -> results, hand every generator its result, until they return."""
        B = len(gens)
        reqs, outs = [None] * B, [None] * B

        def step(b, value):
            try:
                reqs[b] = gens[b].send(value)
            except StopIteration as stop:
                reqs[b], outs[b] = None, stop.value

        for b in range(B):
            step(b, None)
        while any(r is not None for r in reqs):
            assert all(r is not None for r in reqs), "joint batch: the videos must have the same number of windows"
            res = run_windows(reqs)
            for b in range(B):
                step(b, res[b])
        return outs

    # -- what the sliding / streaming host code of both model families shares -------------
    @staticmethod
    def _pad_history(T, step, *hist):
        """Streaming: the prediction histories of the chunks so far, grown by the rows this chunk adds (cotracker3_online.py:349-360,
        cotracker.py:247-259)."""
        p = min(step, T - step)
        return [F.pad(h_, (0, 0) * (h_.dim() - 1) + (0, p)) for h_ in hist]

    def _carry_over(self, qframes, ind, S, step, preds, inits):
        """The window at frame ind > 0 starts from its predecessor (cotracker3_online.py:457-482, cotracker.py:306-327): for the
        tracks queried before the end of the overlap, the overlapping rows of the prediction histories `preds` (coordinates first,
        in pixels), the last one repeated over the `step` new frames, replace `inits`.  Returns the new inits."""
        overlap = S - step
        copy_over = (qframes < ind + overlap)[None, :]
        prevs = [p_[ind:ind + overlap] / self.stride if i == 0 else p_[ind:ind + overlap] for i, p_ in enumerate(preds)]
        prevs = [torch.cat([p_, p_[-1:].expand(step, *p_.shape[1:])], dim=0) for p_ in prevs]
        return [torch.where(copy_over[..., None] if x0.dim() == 3 else copy_over, p_, x0).contiguous() for p_, x0 in zip(prevs, inits)]

    def _hip_encode(self, frames, step, normalize):
        """frames [T,3,H,W] in 0..255 -> NHWC level-0 features [T,H/4,W/4,128] from this device's HipEncoder (built on first use),
        `step` frames per call, every chunk written straight into its frame range of the preallocated output."""
        enc = getattr(self, "_hip_encoder", None)
        if enc is None or enc.device != frames.device:
            from .encoder_hip import HipEncoder
            enc = self._hip_encoder = HipEncoder(self.fnet, frames.device, normalize=normalize)
        T, _, H, W = frames.shape
        out = torch.empty(T, H // self.stride, W // self.stride, self.latent_dim, device=frames.device, dtype=torch.float32)
        for t0 in range(0, T, step):
            enc(frames[t0:t0 + step].float().contiguous(), out=out[t0:t0 + step])
        return out


class CoTrackerThreeBase(TrackerBase):
    """Constructor mirrors cotracker3_online.py:43-92."""

    PACKED_WEIGHTS = PackedWeights

    def __init__(self, window_len=8, stride=4, corr_radius=3, corr_levels=4, num_virtual_tracks=64,
                 model_resolution=(384, 512), add_space_attn=True, linear_layer_for_vis_conf=True):
        super().__init__()
        if (corr_radius, corr_levels, num_virtual_tracks) != (3, 4, 64):
            raise NotImplementedError("the HIP kernels are specialised to corr_radius=3 (7x7 taps), corr_levels=4 and 64 virtual "
                                      "tracks -- the shapes every released model has (build_cotracker.py:31-38); see INTEGRATION.md")
        # constructor add_space_attn=False (cotracker.py:432: no space blocks at all) and linear_layer_for_vis_conf=False
        # (cotracker.py:413-414: one flow_head of width 4) are supported since round 4: same kernels, different parameter set
        self.add_space_attn = bool(add_space_attn)
        self.window_len = window_len
        self.stride = stride
        self.corr_radius = corr_radius
        self.corr_levels = corr_levels
        self.hidden_dim = 256
        self.latent_dim = 128
        self.num_virtual_tracks = num_virtual_tracks
        self.model_resolution = model_resolution
        self.input_dim = 1110
        self.linear_layer_for_vis_conf = linear_layer_for_vis_conf
        self.fnet = BasicEncoder(input_dim=3, output_dim=self.latent_dim, stride=stride)
        self.updateformer = _UpdateFormerParams(self.input_dim, 384, 3, num_virtual_tracks, flow_out=2 if linear_layer_for_vis_conf else 4,
                                                vis_conf_head=bool(linear_layer_for_vis_conf), space_attn=bool(add_space_attn))
        self.corr_mlp = _Mlp(49 * 49, 384, 256)
        self.register_buffer("time_emb", sincos_time_embed(self.input_dim, window_len))
        self.max_corr_rows = 262144  # (point,frame) rows of correlation volume resident at once (~10 GB)
        self.encoder_dtype = torch.float32  # fp32 as the reference; see tools/probe_encoder_precision.py for why not lower
        # streaming: reuse the previous chunk's features for the overlapping frames (see _encode_online).  Not a reference
        # kwarg and OFF by default (the reference re-encodes whatever chunk it is given, predictor.py:288-290); opt in for
        # streams whose chunks are overlapping VIEWS of one resident video (see _encode_online: the overlap is proven on the host
        # by storage aliasing; bench.py --workload c4_online --feature-cache)
        self.online_feature_cache = False

    def _window(self, r, iters, space_attn=True):
        return ops.Window(r.fmaps, r.support, r.coords, r.vis, r.conf, self._scale_xy(), iters=iters, point_mask=r.mask,
                          max_corr_rows=self.max_corr_rows, space_attn=space_attn)

    def _window_graph(self, wins, pw, joint, shared=False):
        """One window: the single-window graph (ctk_window_graph_create); joint: ONE graph of the joint window of all of them
        (ctk_window_batch_graph_create)."""
        return ops.WindowBatchGraph(wins, pw, self.max_corr_rows, shared=shared) if joint else ops.WindowGraph(wins[0], pw)

    def _run_windows(self, reqs, iters, pw, graphed, space_attn=True, shared=False):
        """One window per request (ops.WindowRequest), one request per video -- all of them in ONE call when there are several
        (joint batch mode).  The window overwrites its coords / vis / conf: a request that is not `owned` hands over state it
        still needs (the sliding carry-over), so the window gets clones.  shared: the requests are query groups of one video (the
        same fmaps): several of them run as one shared-pyramid joint window.  Returns every video's (coords, vis, conf)."""
        if graphed:
            ident = (int(self.max_corr_rows), tuple(self.model_resolution), int(self.stride), space_attn)
            return self._graphed_windows(reqs, iters, pw, ident, space_attn=space_attn)
        if shared and len(reqs) > 1:
            wins = self._group_windows(reqs, iters, space_attn)
        else:
            wins = [self._window(r if r.owned else r._replace(coords=r.coords.clone(), vis=r.vis.clone(), conf=r.conf.clone()),
                                 iters, space_attn) for r in reqs]
        if len(wins) == 1:
            ops.forward_window(wins[0], pw)
        else:
            ops.forward_windows(wins, pw, self.max_corr_rows, shared=shared)
        return [w_.result() for w_ in wins]

    def _group_windows(self, reqs, iters, space_attn):
        """The requests of G query groups over one video as the windows of a shared joint window: the groups' state is stacked
        into one [G,S,N,.] tensor each (a copy, so nobody's carry-over is overwritten); the support patches are used where they
        are when they already lie one group behind the other (slices of the one sample_support result of _group_context) and
        stacked otherwise."""
        N = reqs[0].coords.shape[1]
        cols = ops.WindowRequest(*zip(*reqs))  # field by field: cols.coords = every group's coords, ...

        def consecutive(parts):
            step = parts[0].numel() * parts[0].element_size()
            return all(p_.is_contiguous() and p_.data_ptr() == parts[0].data_ptr() + i * step for i, p_ in enumerate(parts))
        support = []
        for l in range(self.corr_levels):
            parts = [sup[l] for sup in cols.support]
            support.append(torch.cat(parts) if not consecutive(parts) else
                           parts[0].as_strided((len(parts) * N, *parts[0].shape[1:]), parts[0].stride()))
        mask = None if cols.mask[0] is None else torch.stack(cols.mask)
        return ops.group_windows(reqs[0].fmaps, support, torch.stack(cols.coords), torch.stack(cols.vis), torch.stack(cols.conf), self._scale_xy(), point_mask=mask, iters=iters,
                                 max_corr_rows=self.max_corr_rows, space_attn=space_attn)

    def _group_context(self, video, queries, chunk, pad_to=None):
        """What the G groups of a query-group call share: the ONE video's level-0 features (padded with the last feature map to a
        multiple of `pad_to` frames -- the sliding model), the pyramid, and the support patches of all groups from one
        sample_support per level over the concatenated query list [G*N] (sliced per group by the caller: consecutive slices of
        one allocation, which is what the shared joint window wants).  The encoder and the support sampler are per frame / per
        point: every group gets the bits its own call would have computed."""
        G, N = queries.shape[:2]
        f0 = self._encode(video.float(), chunk)
        T = f0.shape[0]
        if pad_to and T % pad_to:
            f0 = torch.cat([f0, f0[-1:].expand(pad_to - T % pad_to, -1, -1, -1)], dim=0).contiguous()
        pyr = ops.build_pyramid(f0, self.corr_levels)
        qframes, qcoords = self._split_queries(queries.reshape(G * N, 3))
        support = self._support(pyr, qframes.float().contiguous(), qcoords)
        return pyr, [[s_[g * N:(g + 1) * N] for s_ in support] for g in range(G)]

    # -- shared pieces ------------------------------------------------------------------
    def _scale_xy(self):
        return (self.model_resolution[1] / self.stride, self.model_resolution[0] / self.stride)

    def _encode(self, frames: torch.Tensor, chunk: int) -> torch.Tensor:
        """frames [T,3,H,W] in 0..255 -> L2-normalised NHWC level-0 features [T,H/4,W/4,128].
        The CNN is per-frame, so the frames go through it `encoder_chunk` at a time whatever `fmaps_chunk_size` the caller
        asked for: 16 frames keep the layer activations (150 MB at 384x512) inside the 256 MB Infinity Cache -- the same
        speed as one 120-frame batch in situ (C3 step 1 521 vs 1 517-1 533 ms; 100 vs 102-130 ms in
        tools/bench_encoder_chunk.py) at a tenth of the activation memory; every chunk is normalised straight into its
        frame range of the output (no torch.cat of the 755 MB feature tensor)."""
        step = max(1, min(int(chunk), int(self.encoder_chunk)))
        if self.encoder_backend == "hip" and self.encoder_dtype == torch.float32:
            return self._hip_encode(frames, step, normalize=True)
        T, _, H, W = frames.shape
        out = torch.empty(T, H // self.stride, W // self.stride, self.latent_dim, device=frames.device, dtype=torch.float32)
        for t0 in range(0, T, step):
            x = 2 * (frames[t0:t0 + step] / 255.0) - 1.0  # cotracker3_online.py:320
            if self.encoder_dtype == torch.float32:
                f = self.fnet(x)
            else:  # experiment knob (tools/probe_encoder_precision.py): MIOpen convolutions in half precision
                with torch.autocast("cuda", dtype=self.encoder_dtype):
                    f = self.fnet(x)
            ops.normalize_to_nhwc(f.float().contiguous(), out=out[t0:t0 + step])
        return out

    def _encode_batch(self, video: torch.Tensor, chunk: int) -> torch.Tensor:
        """Joint batch mode: the frames of all B videos as ONE frame batch [B*T,3,H,W] -> features [B,T,H/4,W/4,128].  The CNN is
        per-frame and its result does not depend on which frames share a call (tests/test_gpu_parity.py)."""
        B, T = video.shape[:2]
        f0 = self._encode(video.reshape(B * T, *video.shape[2:]).float(), chunk)
        return f0.view(B, T, *f0.shape[1:])

    def _split_queries(self, queries):
        """queries [N,3] = (frame, x, y) in pixels -> query frames [N] (long), coordinates [N,2] in feature units."""
        queries = queries.float()
        return queries[:, 0].long(), (queries[:, 1:3] / self.stride).contiguous()  # cotracker3_online.py:333-336

    def _support(self, pyr, frames_f: torch.Tensor, qcoords: torch.Tensor):
        return [ops.sample_support(pyr[l], frames_f, (qcoords / 2 ** l).contiguous()) for l in range(self.corr_levels)]

    def _check_inputs(self, video, queries, is_train, add_space_attn):
        """-> (B, T, whether this call runs the space attention, whether it is a query-group call).  The third is the forward-time
        flag of the reference (cotracker.py:496-502: `add_space_attn and hasattr(self, "space_virtual_blocks")`).  A query-group
        call is ONE video with G > 1 query sets (queries [G,N,3]): B is then G, the number of result rows."""
        self._check_call(video, is_train)
        B, T, C, H, W = video.shape
        assert H % self.stride == 0 and W % self.stride == 0
        G = queries.shape[0]
        assert (G == B or (B == 1 and G > 1)) and queries.shape[2] == 3
        return G, T, bool(add_space_attn) and self.add_space_attn, G != B


class CoTrackerThreeOnline(CoTrackerThreeBase):
    """Sliding-window / streaming tracker (cotracker3_online.py:159-541)."""

    _TRANSIENT = {**CoTrackerThreeBase._TRANSIENT, "_overlap_hint": type(None)}
    _gstream = None  # ops.StreamGroups of a streaming query-group call (stream_groups), of any stream with stream_slots, of a push stream
    _window_return = True  # stream_history_frames: False while the predictor's own call runs (it emits its result itself: quiet_return)

    @contextlib.contextmanager
    def quiet_return(self):
        """For the predictor: inside the block a call on a ring stream steps the state and returns (None, None, None, None) -- the
        caller emits what it hands back with stream_emit.  The switch is put back when the block is left, whatever the call raised;
        a stream without a ring returns as ever."""
        self._window_return = False
        try:
            yield
        finally:
            self._window_return = True
    _feed = None     # how the running stream gets its frames: "forward" (chunks) or "push" (stream_push: new frames only); None: no tracked call yet
    online_ind = _online_attr("ind")
    online_track_support = _online_attr("track_support")
    online_coords_predicted = _online_attr("coords_predicted")
    online_vis_predicted = _online_attr("vis_predicted")
    online_conf_predicted = _online_attr("conf_predicted")
    online_f0_tail = _online_attr("f0_tail")

    def init_video_online_processing(self):  # cotracker3_online.py:163-169
        self._resolve_deferred_range_check()  # the last chunk of the previous stream (graph streaming defers its check by one call)
        self._online = [OnlineState(track_support=[None] * self.corr_levels)]  # (B > 1: replicated by the first call)
        self.online_track_feat = [None] * self.corr_levels  # unused by v3, kept for API parity
        self._overlap_hint = None  # the predictor's verdict for the NEXT call (it resizes chunks into fresh tensors)
        if self._gstream is not None:  # its buffers (and the graphs captured on them) serve the next stream of the same shape
            self._gstream.live = False
        self._feed = None

    def _fed(self, how, mark=True):
        """One stream is fed one way: overlapping chunks through forward, or new frames only through stream_push.  The chunk path may
        run on the torch glue, which leaves no resident pyramid to continue from, and a pushed stream has no chunk to be handed."""
        if self._feed not in (None, how):
            raise RuntimeError(f"this stream is fed through {'stream_push' if self._feed == 'push' else 'forward'}: call "
                               "init_video_online_processing() before feeding the model the other way")
        if mark:
            self._feed = how

    @torch.no_grad()
    def forward(self, video, queries, iters=4, is_train=False, add_space_attn=True, fmaps_chunk_size=200,
                is_online=False):
        B, T, space_attn, grouped = self._check_inputs(video, queries, is_train, add_space_attn)
        assert self.window_len >= 2
        if is_online and self.stream_slots and video.shape[0] != 1:
            raise NotImplementedError("stream_slots streams the query sets of ONE video: a batch of videos with the switch on is not "
                                      "implemented")
        ring = is_online and self._ring_rows() is not None
        if ring and video.shape[0] != 1:
            raise NotImplementedError("stream_history_frames streams the query sets of ONE video: a batch of videos with it set is not "
                                      "implemented")
        if is_online:
            self._fed("forward")
        if is_online and (ring or self.stream_slots or (grouped and self.stream_groups)):
            return self._forward_stream_groups(video, queries, iters, fmaps_chunk_size, space_attn)
        if grouped and is_online:
            raise NotImplementedError("streaming (is_online=True) takes one query set per video: a query-group call (video [1,...], "
                                      f"queries [{B},...]) is available offline and sliding only")
        states = self._online_states(B, T) if is_online else None
        hint, self._overlap_hint = getattr(self, "_overlap_hint", None), None  # the verdict for THIS call, all batch elements
        ctx = []  # query-group call: what the groups share, computed once for the call (a range-guard re-run included)

        def make_gens(group):
            if grouped:
                if not ctx:
                    ctx.extend(self._group_context(video[0], queries, fmaps_chunk_size, pad_to=self.window_len))
                return [self._video_gen(video[0], queries[g], fmaps_chunk_size, None, pyr=ctx[0], support=ctx[1][g]) for g in group]
            # joint batch mode: the frames of the whole batch through the encoder as ONE frame batch -- unless every element
            # encodes through its own feature cache (per-video encoder calls)
            f0 = self._encode_batch(video, fmaps_chunk_size) if len(group) > 1 and not (is_online and self.online_feature_cache) else None
            return [self._video_gen(video[b], queries[b], fmaps_chunk_size, states[b] if is_online else None, hint,
                                    None if f0 is None else f0[b]) for b in group]
        return self._track(video, iters, make_gens, states, units=B if grouped else None, space_attn=space_attn, shared=grouped)

    # -- slots of a running stream (stream_slots): assign and release between two calls ---------------------------------------
    def _slot_stream(self):
        """The stream state that stream_assign / stream_release write, or RuntimeError: the switch is off, no call of a stream
        has been made yet (its queries go through forward), or a short chunk has closed the stream."""
        # (a push stream and a stream with a ring history always run on the device stream state)
        if not self.stream_slots and self._feed != "push" and self._ring_rows() is None:
            raise RuntimeError("model.stream_slots is off: this stream has no slots to assign")
        gs, st = self._gstream, getattr(self, "_online", None)
        if gs is None or not gs.live or not st or st[0].ind == 0:
            raise RuntimeError("no stream is running: the queries of the first call go through forward(); slots are assigned between "
                               "two calls of a stream")
        if gs.closed:
            raise RuntimeError("a chunk shorter than the window has ended the stream")
        return gs, st[0].ind

    def stream_assign(self, slots, queries, resident=False):
        """Between two streaming calls: slot slots[m] (flat index g*N + n of the [G,N] query table) tracks queries[m] = (frame, x,
        y), model-resolution pixels, from now on; an occupied slot gets a new occupant.  The frame must not lie below
        online_ind + window_len // 2, the first frame that the stream has not handed to the support sampling yet (ValueError: "its
        features have left the stream"); frames beyond the next window are fine, the slot stays blank until its frame arrives.
        The slot's support features and all its history rows committed so far are cleared; stream_first_row tells from which row
        on the returned tracks belong to the new occupant.  Nothing of the next call changes shape or address: no graph is
        captured again.  The frame column is checked on the host (queries on the device: one small copy, the only wait);
        every refusal is raised before anything is written.  The `queries` argument of later forward calls is checked for shape
        and device only: the resident table (stream_queries) is the truth.

        resident=True admits the frames of the window just tracked as well, stream_resident_frames = [online_ind - window_len // 2,
        online_ind + window_len - window_len // 2): the pyramid of that window is still on the device, so the point's support
        features are sampled from it now (ops.StreamGroups.assign), and the next window starts the point at its query position on
        every frame, as the first window of any point does.  The finished window is not run again for it: its rows below
        online_ind stay empty (stream_first_row)."""
        gs, ind = self._slot_stream()
        step = self.window_len // 2
        if not resident:
            return gs.assign(slots, queries, min_frame=ind + step)
        gs.assign(slots, queries, resident=True)  # (its own frame rule: the refusal names the admissible range)

    @property
    def stream_resident_frames(self):
        """(first, last + 1) of the frames whose features the running stream still holds between two calls -- the window just
        tracked: what stream_assign(resident=True) admits besides later frames."""
        gs, ind = self._slot_stream()
        return (ind - self.window_len // 2, ind - self.window_len // 2 + self.window_len)

    def stream_release(self, slots):
        """Between two streaming calls: empty the listed slots (frame ops.EMPTY_FRAME, position (0, 0), state cleared)."""
        gs, _ = self._slot_stream()
        gs.release(slots)

    @property
    def stream_occupied(self):
        """[G,N] bool on the host: the slots that hold a query (host bookkeeping; a copy)."""
        return self._slot_stream()[0].occupied.clone()

    @property
    def stream_first_row(self):
        """[G,N] long on the host: the history row from which a slot's rows belong to its present occupant (0 for the queries of
        the first call, online_ind at the time of an assign); the rows below it carry no information (a copy)."""
        return self._slot_stream()[0].first_row.clone()

    @property
    def stream_queries(self):
        """[G,N,3] on the device: the resident query table as it stands (a copy)."""
        gs = self._slot_stream()[0]
        return gs.queries.reshape(gs.G, gs.N, 3).clone()

    # -- endless streams (stream_history_frames): ring history, this window's rows per call ----------------------------------------
    FRAME_LIMIT = 2 ** 24  # frame numbers are float32 in the query table: every integer below is exact

    def _ring_rows(self):
        """The ring size of the stream the next call belongs to: stream_history_frames as it stands when that call is the first of
        a stream; after that the running stream's own -- None for one that runs without a ring, on the device state or on the torch
        glue: the attribute is read at the first call, and a change in mid-stream waits for the next stream."""
        st, gs = getattr(self, "_online", None), self._gstream
        if st and st[0].ind > 0:
            return gs.ring_rows if gs is not None and gs.live else None
        return self.stream_history_frames

    def _check_frame_limit(self, ind):
        """Before any launch of a call on a ring: its window [ind, ind + window_len) must stay below FRAME_LIMIT."""
        if ind + self.window_len > self.FRAME_LIMIT:
            raise RuntimeError(f"the stream has reached frame {ind}: the next window would pass frame 2^24, beyond which float32 query "
                               "frames are not exact; start a new stream (init_video_online_processing)")

    def _running_stream(self):
        """The device stream state of the running (or just closed) stream, for the readers of its history below; RuntimeError when there
        is none, or nothing has been committed to it yet."""
        gs = self._gstream
        if gs is None or not gs.live or gs.committed == 0:
            raise RuntimeError("no stream is running on the device stream state")
        return gs

    def stream_emit(self, f0, f1, N_out=None, scale=(1.0, 1.0), logits=True, thresh=None, first_row=None):
        """Frames [f0, f1) of the running (or just closed) stream's history, in frame order, by one launch: ops.StreamGroups.emit.
        Serves a ring history and the default one alike."""
        return self._running_stream().emit(f0, f1, N_out, scale, logits, thresh, first_row)

    def stream_health(self, look, grid, thresh, N_out, first_row, bounds):
        """The slots of the running (or just closed) stream judged over its last `look` frames, by one launch and without a wait:
        ops.StreamGroups.health -> (lost, cell, cover) on the device.  Serves a ring history and the default one alike."""
        return self._running_stream().health(look, grid, thresh, N_out, first_row, bounds)

    def stream_draw(self, frames, f0, colors, **kw):
        """Points of the running (or just closed) stream drawn onto uint8 frames from its own history, by two launches and without a
        wait: ops.StreamGroups.draw.  Serves a ring history and the default one alike."""
        return self._running_stream().draw(frames, f0, colors, **kw)

    def stream_motion(self, f0, F, **kw):
        """The camera motion of frames [f0, f0 + F) of the running (or just closed) stream fitted to its own history, by one launch and
        without a wait: ops.StreamGroups.motion.  Serves a ring history and the default one alike."""
        return self._running_stream().motion(f0, F, **kw)

    def stream_stabilize(self, frames, f0, **kw):
        """uint8 frames [f0, f0 + F) of the running (or just closed) stream steadied by the camera motion fitted to its own history, by
        three launches and without a wait: ops.StreamGroups.stabilize.  Serves a ring history and the default one alike."""
        return self._running_stream().stabilize(frames, f0, **kw)

    def stream_field(self, f0, F, **kw):
        """The displacement fields of frames [f0, f0 + F) of the running (or just closed) stream towards another frame or an anchor,
        interpolated from its own history by three launches and without a wait: ops.StreamGroups.field.  Serves a ring history and the
        default one alike."""
        return self._running_stream().field(f0, F, **kw)

    def stream_objects(self, f0, F, **kw):
        """Up to `objects` motion fits per frame [f0, f0 + F) of the running (or just closed) stream over sub-lists of its points --
        labelled regions, or what the earlier fits left -- against f - lag, a fixed frame or an anchor, from its own history by one
        launch and without a wait: ops.StreamGroups.objects.  Serves a ring history and the default one alike."""
        return self._running_stream().objects(f0, F, **kw)

    def stream_planes(self, f0, F, **kw):
        """Up to `planes` homography fits per frame [f0, f0 + F) of the running (or just closed) stream over the labelled regions of its
        points -- or over all of them -- against f - lag, a fixed frame or an anchor, from its own history by one launch and without a
        wait: ops.StreamGroups.planes.  Serves a ring history and the default one alike."""
        return self._running_stream().planes(f0, F, **kw)

    def stream_epipolar(self, f0, F, **kw):
        """One fundamental matrix per frame [f0, f0 + F) of the running (or just closed) stream, fitted to the correspondences with a
        source frame, and the points that violate it -- straight from the history and logits on the device, by one launch and without
        a wait: ops.StreamGroups.epipolar.  Serves a ring history and the default one alike."""
        return self._running_stream().epipolar(f0, F, **kw)

    def stream_pose(self, f0, F, intrinsics, fundamental, label, **kw):
        """One camera pose per frame [f0, f0 + F) of the running (or just closed) stream and two depths per point, from what
        stream_epipolar returned for the same frames and the camera's intrinsics -- straight from the history and logits on the device,
        by one launch and without a wait: ops.StreamGroups.pose.  Serves a ring history and the default one alike."""
        return self._running_stream().pose(f0, F, intrinsics, fundamental, label, **kw)

    def stream_focal(self, f0, F, fundamental, label, **kw):
        """The focal length of the camera from the frames [f0, f0 + F) of the running (or just closed) stream, from what stream_epipolar
        returned for the same frames: a sweep of candidate focal lengths through stream_pose's rules, summed over the frames (and over
        earlier calls, curve=) -- straight from the history and logits on the device, by two launches and without a wait:
        ops.StreamGroups.focal.  Serves a ring history and the default one alike."""
        return self._running_stream().focal(f0, F, fundamental, label, **kw)

    def stream_resection(self, f0, F, intrinsics, structure, valid, seed_pose, **kw):
        """One camera pose per frame [f0, f0 + F) of the running (or just closed) stream against a 3-D structure, in that structure's
        unit and coordinates, started from what stream_pose returned for the same frames -- straight from the history and logits on
        the device, by one launch and without a wait: ops.StreamGroups.resection.  Serves a ring history and the default one alike."""
        return self._running_stream().resection(f0, F, intrinsics, structure, valid, seed_pose, **kw)

    def stream_p3p(self, f0, F, intrinsics, structure, valid, **kw):
        """One camera pose per frame [f0, f0 + F) of the running (or just closed) stream against a 3-D structure, in that structure's
        unit and coordinates, WITHOUT a seed pose (every candidate comes from three points of the structure) -- straight from the
        history and logits on the device, by one launch and without a wait: ops.StreamGroups.p3p.  Serves a ring history and the
        default one alike."""
        return self._running_stream().p3p(f0, F, intrinsics, structure, valid, **kw)

    def stream_align(self, a, valid_a, b, valid_b, intrinsics, **kw):
        """The similarity between two point sets over the slots of the running (or just closed) stream, by one launch and without a
        wait: ops.StreamGroups.align.  It reads no history and touches nothing of the stream."""
        return self._running_stream().align(a, valid_a, b, valid_b, intrinsics, **kw)

    def stream_structure(self, f0, F, intrinsics, pose, **kw):
        """One 3-D point per slot from the frames [f0, f0 + F) of the running (or just closed) stream under the poses stream_resection
        returned for them, the old structure carried along and everything restated in the camera of one of the frames -- straight
        from the history and logits on the device, by one launch and without a wait: ops.StreamGroups.structure.  Serves a ring
        history and the default one alike."""
        return self._running_stream().structure(f0, F, intrinsics, pose, **kw)

    # -- streaming query groups (stream_groups): the state of all groups on the device ---------------------------------------
    def _forward_stream_groups(self, video, queries, iters, chunk, space_attn):
        """One streaming call for G query groups over the one live video (see TrackerBase.__init__, stream_groups).  The chunk is
        encoded once (through the stream's ONE feature cache), the pyramid is built once into the resident buffers of
        ops.StreamGroups, and _stream_step runs the window on them."""
        T, S = video.shape[1], self.window_len
        step = S // 2
        st = self._online_states(1, T)[0]
        hint, self._overlap_hint = getattr(self, "_overlap_hint", None), None
        if self._ring_rows() is not None:
            self._check_frame_limit(st.ind)
        self._resolve_deferred_range_check()
        gs = self._stream_state(queries, st, video.shape[3], video.shape[4])
        gs.closed = T < S
        f0 = self._encode_online(video[0], chunk, S, step, st, hint)
        gs.set_pyramid(f0)
        return self._stream_step(gs, st, video.device, T, iters, space_attn)

    def _stream_state(self, queries, st, H, W):
        """The resident stream state for this call: the running one, the buffers of the previous stream of the same shape handed to
        a new stream (no new graph), or a new ops.StreamGroups."""
        S = self.window_len
        step = S // 2
        sizes = [((H // self.stride) >> l, (W // self.stride) >> l) for l in range(self.corr_levels)]
        gs = self._gstream
        ring = self._ring_rows()  # (read at the first call of a stream; the running stream's own afterwards)
        if gs is None or not gs.fits(queries, S, step, self.stride, sizes, ring):
            assert st.ind == 0, "the query groups of a stream are fixed by its first call"
            self._drop_graphs()  # (they hold pointers into the old stream's buffers)
            gs = self._gstream = ops.StreamGroups(queries, S, step, self.stride, sizes, ring_rows=ring)
        elif not gs.live:
            assert st.ind == 0, "the query groups of a stream are fixed by its first call"
            gs.restart(queries)
        assert not gs.closed, "a chunk shorter than the window ends the stream"
        return gs

    def _stream_step(self, gs, st, device, T, iters, space_attn):
        """What every call on the device stream state does once the resident pyramid holds this window's S frames (T of them real):
        three launches step the state of all G*N points -- support (the points whose query frame entered this window), begin
        (carry-over and masks), then the groups' windows, then commit (history rows, non-finite flag).  Returns views of the first
        ind + T history rows, [G,T_so_far,N,.]: the next call refines the overlapping rows in place.  On a ring
        (stream_history_frames): this window's T rows, copied out by one emit launch."""
        S = self.window_len
        step = S // 2
        ind = st.ind
        gs.sample_support(ind)  # independent of the Linear back end: not repeated by a range-guard re-run
        graphed = bool(self.hip_graph)
        joint, groups = self._index_groups(gs.G, units=True)
        kw = dict(iters=int(iters), max_corr_rows=int(self.max_corr_rows), space_attn=bool(space_attn))
        # what a window step overwrites and a re-run must find again: the history rows the carry-over reads (commit rewrites them)
        rows = gs.frame_rows(ind, ind + S - step)  # (one slice; two where a ring wraps)

        def run(precision, check):
            """begin, the groups' windows -- one group after the other ("loop") or shared-pyramid joint windows of at most
            CTK_MAX_BATCH groups ("joint"); graphed: each replays its own graph, a member of this stream state's generation --, commit."""
            pw = self.packed(device, precision)
            gs.begin(ind)
            graphs = graphed and self._graph_cache(("stream_groups", gs.serial, tuple(self.model_resolution), int(self.stride), joint,
                                                    *kw.values()), pw)
            for group in groups:
                wins = gs.windows(group[0], group[-1] + 1, self._scale_xy(), **kw)
                if graphed:
                    graphs(group[0], lambda: self._window_graph(wins, pw, joint, shared=True)).launch()
                elif joint:
                    ops.forward_windows(wins, pw, self.max_corr_rows, shared=True)
                else:
                    ops.forward_window(wins[0], pw)
            gs.commit(ind, T, check)

        def restore(saved):
            for h_, s_ in zip(gs.hist, saved or ()):
                for r_, p_ in zip(rows, s_):
                    h_[:, r_].copy_(p_)
            gs.nonfinite.zero_()
        self._guarded(run, lambda: ind > 0 and [[h_[:, r_].clone() for r_ in rows] for h_ in gs.hist], restore,
                      graphed and self.stream_range_check == "deferred", gs.nonfinite, "streaming call of all query groups")
        st.ind = ind + step
        if gs.ring_rows is not None:
            # reference-visible online_* attributes: the RING buffers [G,K,N,.] (frame f in row f % K)
            st.track_support, (st.coords_predicted, st.vis_predicted, st.conf_predicted) = gs.support, gs.hist
            self.stream_window_start = ind
            if not self._window_return:  # the predictor emits what it hands back itself (stream_emit): one launch instead of this one and its own
                self.last_logits = None
                return (None, None, None, None)
            coords, vis, conf = gs.emit(ind, ind + T)
            self.last_logits = (vis, conf)
            return (coords, torch.sigmoid(vis), torch.sigmoid(conf), None)
        out = gs.history(ind + T)
        # reference-visible online_* attributes (API parity): the state of ALL groups, views of the resident buffers
        st.track_support, (st.coords_predicted, st.vis_predicted, st.conf_predicted) = gs.support, out
        self.last_logits = out[1:]
        return (out[0], torch.sigmoid(out[1]), torch.sigmoid(out[2]), None)

    # -- push stream: new frames only, the overlap stays in the resident pyramid ------------------------------------------------
    @torch.no_grad()
    def stream_push(self, frames, queries, iters=4, add_space_attn=True, final=False):
        """One streaming call that is handed the NEW frames only: frames [n,3,H,W] float32 in 0..255 at model resolution, queries
        [G,N,3] as forward takes them (G == 1 included).  The first tracked call of a stream brings the whole first window,
        n == window_len; every later one the n == window_len // 2 frames the window advances by.  final=True admits fewer (at least
        one): a video shorter than a window, or the short closing chunk, which ends the stream exactly as forward's chunk of
        T = window_len // 2 + n < window_len frames does.  Returns what forward(chunk, queries, is_online=True) returns for the chunk
        of the last window_len (or T) frames on the device stream state -- the same bits: the encoder and the pooling are per frame,
        so the features the resident pyramid keeps from the previous call (ops.StreamGroups.advance_pyramid) are the ones a
        re-computation would give -- while every frame is encoded and pooled once.  Always on the device stream state, whatever
        stream_groups / stream_slots say, in both batch_modes, with and without hip_graph; stream_assign / stream_release work on
        it; online_feature_cache plays no part.  A stream is fed one way: after a tracked forward call this raises RuntimeError until
        init_video_online_processing(), and forward does after a push."""
        if not (isinstance(frames, torch.Tensor) and frames.dim() == 4 and frames.shape[1] == 3 and frames.dtype == torch.float32):
            raise ValueError("stream_push: frames must be a float32 tensor [n,3,H,W] (the new frames, model resolution, 0..255)")
        self._fed("push", mark=False)
        self._check_call(frames, False)
        n, _, H, W = frames.shape
        assert H % self.stride == 0 and W % self.stride == 0
        assert queries.dim() == 3 and queries.shape[2] == 3
        S = self.window_len
        step = S // 2
        assert S >= 2 and 2 * step == S, "stream_push: window_len must be even (the kept half and the new half of a window)"
        st = self._online_states(1, min(n, S))[0]
        first = st.ind == 0
        full = S if first else step
        if not (n == full or (final and 1 <= n < full)):
            raise ValueError(f"stream_push: this call takes {full} new frames ({'the first window' if first else 'one step'}), or "
                             f"1..{full - 1} with final=True; got {n}" + ("" if final or n >= full else " without final=True"))
        T = n if first else S - step + n
        if self._ring_rows() is not None:
            self._check_frame_limit(st.ind)
        self._fed("push")
        self._resolve_deferred_range_check()
        gs = self._stream_state(queries, st, H, W)
        gs.closed = T < S
        f_new = self._encode(frames.contiguous(), S)  # (the CNN is per frame: these are the bits a full chunk's call computes)
        if first:
            gs.set_pyramid(f_new)
        else:
            gs.advance_pyramid(f_new, T)
        return self._stream_step(gs, st, frames.device, T, iters, bool(add_space_attn) and self.add_space_attn)

    def _encode_online(self, video, chunk, S, step, st, hint):
        """Streaming: consecutive chunks overlap by S - step frames (predictor.py:225,288-290 feeds the last 2*step frames
        every step), and the encoder is per-frame, so the overlapping frames' level-0 features are the ones computed one
        call ago.  With ``online_feature_cache`` (opt-in) only the `step` NEW frames go through the CNN (half the encoder
        time of a streaming call) -- when the overlap is PROVEN ON THE HOST, with no device work and no synchronisation: the
        new chunk's first S - step frames must be the very memory of the previous chunk's last S - step frames (same live
        storage, offset advanced by `step` frames, same strides / dtype, tensor version unchanged: `tail_aliases`), which is
        what slicing a resident video gives (``video[:, i:i + S]``, then ``video[:, i + step:i + step + S]``).
        CoTrackerOnlinePredictor applies the same test to the chunk it is handed and passes the verdict down
        (``_overlap_hint`` -> `hint`), because it resizes every chunk into a fresh tensor.  A chunk whose overlap cannot be
        proven that way is simply encoded in full, exactly what the reference does with it (round 3 compared the frames on the
        device with torch.equal: a blocking device-to-host wait in every streaming call -- ADVICE r3)."""
        T = video.shape[0]
        ov = S - step
        tail = st.f0_tail
        proven = hint if hint is not None else tail_aliases(st.prev_frames, video, 0, step)
        if self.online_feature_cache and T == S and tail is not None and tail.shape[0] == ov and proven:
            f0 = torch.cat([tail, self._encode(video[ov:].float(), chunk)], dim=0)
        else:
            f0 = self._encode(video.float(), chunk)
        if self.online_feature_cache and T == S:
            st.f0_tail = f0[step:]
            st.prev_frames = video  # a reference, not a copy: keeps the storage alive, so "same address" means "same allocation"
            try:
                video._ctk_version = video._version  # the version the cached features were computed from
            except Exception:
                pass
        else:
            st.f0_tail = st.prev_frames = None
        return f0

    def _video_gen(self, video, queries, chunk, st, hint=None, f0=None, pyr=None, support=None):
        """One video's host code as a generator (see _track): yields one request per window, receives that window's (coords,
        vis, conf), returns (coords_pred, vis_pred, conf_pred).  st: this video's OnlineState (streaming: ONE window, at
        st.ind) or None (sliding over all T frames).  f0: this video's level-0 features when the caller has encoded them
        already (joint batch mode).  pyr, support: the (padded) pyramid and this query set's support patches when the caller
        has them already (one group of a query-group call, sliding only: _group_context)."""
        is_online = st is not None
        T = video.shape[0]
        N = queries.shape[0]
        S = self.window_len
        step = S // 2
        dev = video.device
        qframes, qcoords = self._split_queries(queries)

        # encoder + pyramid.  The reference pads the *video* by repeating its last frame
        # (:321-328); the encoder is per-frame, so repeating the last feature map is identical.
        pad = (S - T) if is_online else (S - T % S) % S
        if pyr is None:
            if f0 is not None:
                if is_online:  # encoded by the caller: this element's feature cache is not fed
                    st.f0_tail = st.prev_frames = None
            else:
                f0 = self._encode_online(video, chunk, S, step, st, hint) if is_online else self._encode(video.float(), chunk)
            if pad > 0:
                f0 = torch.cat([f0, f0[-1:].expand(pad, -1, -1, -1)], dim=0).contiguous()
            pyr = ops.build_pyramid(f0, self.corr_levels)

        coords_pred = torch.zeros(T, N, 2, device=dev)
        vis_pred = torch.zeros(T, N, device=dev)
        conf_pred = torch.zeros(T, N, device=dev)
        if is_online:
            if st.coords_predicted is not None:
                coords_pred, vis_pred, conf_pred = self._pad_history(T, step, st.coords_predicted, st.vis_predicted, st.conf_predicted)
            left = 0 if st.ind == 0 else st.ind + step
            right = st.ind + S
            sample_mask = ((qframes >= left) & (qframes < right)).float()[:, None, None]  # :411-414
            frames_rel = (qframes - st.ind).float().contiguous()
        else:
            frames_rel = qframes.float().contiguous()

        if support is None:
            support = self._support(pyr, frames_rel, qcoords)
        if is_online:  # :424-440 -- accumulate only the tracks whose query frame is in this chunk (a NEW list: see OnlineState)
            st.track_support = support = [(torch.zeros_like(s_) if acc is None else acc) + s_ * sample_mask
                                          for acc, s_ in zip(st.track_support, support)]

        coords_init = qcoords[None].expand(S, N, 2).contiguous()
        vis_init = torch.zeros(S, N, device=dev)
        conf_init = torch.zeros(S, N, device=dev)

        num_windows = (T - S + step - 1) // step + 1
        indices = [st.ind] if is_online else range(0, step * num_windows, step)
        for ind in indices:
            if ind > 0:
                coords_init, vis_init, conf_init = self._carry_over(qframes, ind, S, step, (coords_pred, vis_pred, conf_pred),
                                                                    (coords_init, vis_init, conf_init))
            mask = (qframes < ind + S).to(torch.uint8).contiguous()  # attention_mask :484, used as :493-496
            fm = pyr if is_online else [p_[ind:ind + S] for p_ in pyr]
            coords, vis, conf = yield ops.WindowRequest(fm, support, coords_init, vis_init, conf_init, mask, False)
            S_trim = T if is_online else min(T - ind, S)
            coords_pred[ind:ind + S] = (coords * float(self.stride))[:S_trim]
            vis_pred[ind:ind + S] = vis[:S_trim]
            conf_pred[ind:ind + S] = conf[:S_trim]
        if is_online:
            st.ind += step
            st.coords_predicted, st.vis_predicted, st.conf_predicted = coords_pred, vis_pred, conf_pred
        return coords_pred, vis_pred, conf_pred


class CoTrackerThreeOffline(CoTrackerThreeBase):
    """Single-window tracker over all T frames (cotracker3_offline.py:15-233)."""

    @torch.no_grad()
    def forward(self, video, queries, iters=4, is_train=False, add_space_attn=True, fmaps_chunk_size=200):
        B, T, space_attn, grouped = self._check_inputs(video, queries, is_train, add_space_attn)
        assert T >= 1
        ctx = []  # query-group call: what the groups share, computed once for the call (a range-guard re-run included)

        def make_gens(group):  # joint batch mode: the B*T frames through the encoder as one frame batch
            if grouped:
                if not ctx:
                    ctx.extend(self._group_context(video[0], queries, fmaps_chunk_size))
                return [self._video_gen(None, queries[g], fmaps_chunk_size, pyr=ctx[0], support=ctx[1][g]) for g in group]
            f0 = self._encode_batch(video, fmaps_chunk_size) if len(group) > 1 else None
            return [self._video_gen(video[b], queries[b], fmaps_chunk_size, None if f0 is None else f0[b]) for b in group]
        return self._track(video, iters, make_gens, units=B if grouped else None, space_attn=space_attn, shared=grouped)

    def _video_gen(self, video, queries, chunk, f0=None, pyr=None, support=None):
        """One video's host code (see _track): the single window over all T frames.  f0: its level-0 features [T,H/4,W/4,128]
        when the caller has encoded them already; pyr, support: the pyramid and this query set's support patches when the caller
        has them already (one group of a query-group call: _group_context).  The window carries no point mask and may overwrite
        the tensors it is given."""
        qframes, qcoords = self._split_queries(queries)
        if pyr is None:
            if f0 is None:
                f0 = self._encode(video.float(), chunk)
            pyr = ops.build_pyramid(f0, self.corr_levels)
        T = pyr[0].shape[0]
        N = queries.shape[0]
        dev = pyr[0].device
        if support is None:
            support = self._support(pyr, qframes.float().contiguous(), qcoords)
        coords = qcoords[None].expand(T, N, 2).contiguous()
        vis = torch.zeros(T, N, device=dev)
        conf = torch.zeros(T, N, device=dev)
        coords, vis, conf = yield ops.WindowRequest(pyr, support, coords, vis, conf, None, True)
        return coords * float(self.stride), vis, conf
