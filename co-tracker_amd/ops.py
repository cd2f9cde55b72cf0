"""Torch-tensor front end of the C-ABI ops (device memory + stream plumbing only).

Every function enqueues HIP kernels from libctk_hip.so on the current torch stream; nothing here
computes on the CPU and nothing falls back to PyTorch ops.
"""
import ctypes as C
import math
import struct
from collections import namedtuple
from typing import List, Optional, Sequence

import torch

from . import _lib as L


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    return t.data_ptr()


def _ptr_at(t: torch.Tensor, g0: int) -> int:
    """The address of t[g0:], without making the view."""
    return t.data_ptr() + g0 * t.stride(0) * t.element_size() if g0 else t.data_ptr()


def _chk_f32(*ts):
    for t in ts:
        if t is None:
            continue
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("expected contiguous float32 CUDA(HIP) tensors")


def _query_bytes(name: str, *args) -> int:
    """A `*_bytes` query of the C-ABI (the size comes back through the trailing size_t*)."""
    nbytes = C.c_size_t(0)
    L.check(getattr(L.load(), name)(*args, C.byref(nbytes)), name)
    return nbytes.value


# ------------------------------------------------------------------------------------------
# primitives
# ------------------------------------------------------------------------------------------
def pack_weight(w: torch.Tensor) -> torch.Tensor:
    """Split a torch-layout Linear weight [N,K] (K % 32 == 0) into the two-half blob of the split-half
    GEMM back end (ctk_pack_weight).  Returns a uint8 device tensor that must outlive its users."""
    _chk_f32(w)
    N, K = w.shape
    blob = torch.empty(_query_bytes("ctk_pack_weight_bytes", N, K), device=w.device, dtype=torch.uint8)
    L.check(L.load().ctk_pack_weight(_ptr(w), K, N, K, _ptr(blob), _stream()), "ctk_pack_weight")
    return blob


def gemm(a: torch.Tensor, w: torch.Tensor, bias=None, act: int = L.ACT_NONE, resid=None, bias_rows=None,
         out: Optional[torch.Tensor] = None, packed: Optional[torch.Tensor] = None, out_split: bool = False) -> torch.Tensor:
    """out[M,N] = act(a[M,K] @ w[N,K]^T + bias + bias_rows[m % period]) + resid.
    packed = pack_weight(w) selects the split-half (3 x f16 MFMA) back end; None the exact-f32 one.
    With the split-half back end, a may be an SH tensor [M,K/32,2,32] float16 (split_rows) and out_split
    returns the result in SH form."""
    a_split = a.dtype == torch.float16
    if a_split:
        assert packed is not None and a.is_cuda and a.is_contiguous() and a.dim() == 4
        _chk_f32(w, bias, bias_rows)
        M, K = a.shape[0], a.shape[1] * 32
    else:
        _chk_f32(a, w, bias, bias_rows)
        M, K = a.shape
    for t_ in (resid, out):  # row-strided views are fine (leading dimension is passed explicitly)
        if t_ is not None and not (t_.is_cuda and t_.dtype == torch.float32 and t_.stride(1) == 1):
            raise ValueError("out/resid must be float32 device tensors with unit column stride")
    N = w.shape[0]
    if out_split:
        assert packed is not None and resid is None and out is None
        out = torch.empty(M, N // 32, 2, 32, device=a.device, dtype=torch.float16)
    elif out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    g = L.GemmArgs()
    g.A, g.lda, g.M = _ptr(a), (2 * K if a_split else K), M
    g.a_split, g.c_split = int(a_split), int(out_split)
    g.W, g.ldw, g.N, g.K = _ptr(w), w.shape[1], N, K
    g.Wp = _ptr(packed)
    g.C, g.ldc = _ptr(out), (2 * N if out_split else out.stride(0))
    g.bias = _ptr(bias)
    g.bias_rows = _ptr(bias_rows)
    g.bias_period = bias_rows.shape[0] if bias_rows is not None else 0
    g.resid, g.ldr = _ptr(resid), (resid.stride(0) if resid is not None else 0)
    g.act = act
    g.batch, g.a_bs, g.c_bs, g.k_valid = 1, 0, 0, 0
    L.check(L.load().ctk_gemm(C.byref(g), _stream()), "ctk_gemm")
    return out


def split_rows(x: torch.Tensor) -> torch.Tensor:
    """f32 [M,K] (K % 32 == 0) -> SH format: float16 tensor [M, K/32, 2, 32] (hi plane, lo plane), x = hi + lo."""
    _chk_f32(x)
    M, K = x.shape
    out = torch.empty(M, K // 32, 2, 32, device=x.device, dtype=torch.float16)
    L.check(L.load().ctk_split_rows(_ptr(x), K, M, K, _ptr(out), _stream()), "ctk_split_rows")
    return out


def unsplit(sh: torch.Tensor) -> torch.Tensor:
    """SH tensor [M, K/32, 2, 32] float16 -> f32 [M,K] (test helper: hi + lo)."""
    M, KT = sh.shape[0], sh.shape[1]
    return (sh[:, :, 0].float() + sh[:, :, 1].float()).reshape(M, KT * 32)


def layernorm(x: torch.Tensor, gamma=None, beta=None, eps: float = 1e-6, out_split: bool = False) -> torch.Tensor:
    _chk_f32(x, gamma, beta)
    assert x.shape[-1] == L.HID
    R = x.numel() // L.HID
    y = torch.empty(R, L.HID // 32, 2, 32, device=x.device, dtype=torch.float16) if out_split else torch.empty_like(x)
    L.check(L.load().ctk_layernorm(_ptr(x), _ptr(y), R, _ptr(gamma), _ptr(beta), float(eps), int(out_split), _stream()),
            "ctk_layernorm")
    return y


def layernorm_dual(x: torch.Tensor, gamma=None, beta=None, eps: float = 1e-5, eps2: float = 1e-6, out_split: bool = False):
    """(LayerNorm(x; gamma, beta, eps), LayerNorm(x; eps2)) from one read of x (ctk_layernorm_dual: the window's launch for the
    point tokens of a depth)."""
    _chk_f32(x, gamma, beta)
    assert x.shape[-1] == L.HID
    R = x.numel() // L.HID
    y, y2 = (torch.empty(R, L.HID // 32, 2, 32, device=x.device, dtype=torch.float16) if out_split else torch.empty_like(x)
             for _ in range(2))
    L.check(L.load().ctk_layernorm_dual(_ptr(x), _ptr(y), _ptr(y2), R, _ptr(gamma), _ptr(beta), float(eps), float(eps2),
                                        int(out_split), _stream()), "ctk_layernorm_dual")
    return y, y2


def virtual_init(virtual_tokens: torch.Tensor, S: int, B: int = 1) -> torch.Tensor:
    """The virtual-token rows a window starts from (ctk_virtual_init): [B*64*S, 384], row (b*64 + v)*S + t = virtual_tokens[v]."""
    _chk_f32(virtual_tokens)
    assert virtual_tokens.shape == (L.VIRT, L.HID)
    dst = torch.empty(B * L.VIRT * S, L.HID, device=virtual_tokens.device, dtype=torch.float32)
    L.check(L.load().ctk_virtual_init(_ptr(virtual_tokens), S, B, _ptr(dst), _stream()), "ctk_virtual_init")
    return dst


def state_batch(states, S: int, N: int, scale_xy=(1.0, 1.0)):
    """ctk_window_batch of B videos' state alone, for ctk_assemble_tokens_batch / ctk_heads_update: states = [(coords [S,N,2], vis
    [S,N], conf [S,N])] per video, as tensors, addresses or None.  -> (the struct, what it points to: keep it alive)."""
    arr = (L.WindowArgs * len(states))()
    for a, (c, v, f) in zip(arr, states):
        a.S, a.N = S, N
        a.coords, a.vis, a.conf = (_ptr(p) if torch.is_tensor(p) else p for p in (c, v, f))
        a.scale_x, a.scale_y = float(scale_xy[0]), float(scale_xy[1])
    return L.WindowBatch(len(states), 0, C.cast(arr, C.POINTER(L.WindowArgs))), (arr, states)


def assemble_tokens_batch(states, scale_xy, x: torch.Tensor, folded: bool = False) -> torch.Tensor:
    """The 96 small-feature columns of B videos (ctk_assemble_tokens_batch) into x: f32 [B*N*S, ld] or SH [B*N*S, ld/32, 2, 32], ld
    and the first column those of the plain (CTK_X_LD, CTK_X_VIS) or the folded (CTK_XF_LD, CTK_XF_SMALL) input."""
    S, N = states[0][1].shape
    ld, base = (L.XF_LD, L.XF_SMALL) if folded else (L.X_LD, L.X_VIS)
    assert x.is_cuda and x.is_contiguous() and x.numel() == len(states) * N * S * ld * (2 if x.dtype == torch.float16 else 1)
    batch, keep = state_batch(states, S, N, scale_xy)
    L.check(L.load().ctk_assemble_tokens_batch(C.byref(batch), _ptr(x), int(x.dtype == torch.float16), ld, base, _stream()),
            "ctk_assemble_tokens_batch")
    return x


def heads_update(tokens: torch.Tensor, head_w: torch.Tensor, head_b: torch.Tensor, S: int, N: int, states=None,
                 want_delta: bool = False) -> Optional[torch.Tensor]:
    """delta = tokens @ head_w^T + head_b per row (ctk_heads_update), added in place to the (coords, vis, conf) of `states` (one
    triple per video; None: delta only) and / or returned [N*S, 4] (want_delta: one video only)."""
    _chk_f32(tokens, head_w, head_b)
    states = states or [(None, None, None)]
    assert tokens.shape == (len(states) * N * S, L.HID) and head_w.shape == (4, L.HID) and head_b.shape == (4,)
    delta = torch.empty(N * S, 4, device=tokens.device, dtype=torch.float32) if want_delta or states[0][0] is None else None
    batch, keep = state_batch(states, S, N)
    L.check(L.load().ctk_heads_update(C.byref(batch), _ptr(tokens), _ptr(head_w), _ptr(head_b), _ptr(delta), _stream()),
            "ctk_heads_update")
    return delta


def _attn_args(q, k, v, nbatch: int, N1: int, N2: int, q_bs: int, kv_bs: int, inner: int, splits: int, out_split: bool,
               key_mask, query_mask):
    """ctk_attn_args of `nbatch` problems q [N1 rows] over k / v [N2 rows]: batch strides q_bs (q, out) / kv_bs (k, v) and inner
    stride `inner`, in rows.  Returns (args, out, split-K partials): the caller keeps the third alive across its launch."""
    _chk_f32(q, k, v)
    out = torch.empty(nbatch * N1, L.HID // 32, 2, 32, device=q.device, dtype=torch.float16) if out_split else torch.empty_like(q)
    a = L.AttnArgs()
    a.q, a.q_ld, a.q_bs, a.q_is = _ptr(q), L.HID, q_bs, inner
    a.k, a.v, a.kv_ld, a.kv_bs, a.kv_is = _ptr(k), _ptr(v), L.HID, kv_bs, inner
    a.out, a.o_ld, a.o_bs, a.o_is = _ptr(out), (2 * L.HID if out_split else L.HID), q_bs, inner
    a.o_split = int(out_split)
    a.nbatch, a.n1, a.n2 = nbatch, N1, N2
    a.splits = splits
    part = torch.empty(splits * nbatch * 8 * N1 * 50, device=q.device, dtype=torch.float32) if splits > 1 else None
    a.partial = _ptr(part)
    a.key_mask, a.query_mask = _ptr(key_mask), _ptr(query_mask)  # uint8, per key / per query (CoTracker2 attention mask)
    return a, out, part


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, splits: int = 1, out_split: bool = False,
              key_mask: Optional[torch.Tensor] = None, query_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q [B,N1,384], k/v [B,N2,384] (8 heads x 48, heads contiguous in the last dim) -> [B,N1,384]
    (or its SH form [B*N1, 12, 2, 32] float16 when out_split).  key_mask [N2] / query_mask [N1] uint8."""
    (B, N1, _), N2 = q.shape, k.shape[1]
    a, out, _part = _attn_args(q, k, v, B, N1, N2, N1, N2, 1, splits, out_split, key_mask, query_mask)
    L.check(L.load().ctk_attention(C.byref(a), _stream()), "ctk_attention")
    return out


def attention_batch2(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, splits: int = 1, out_split: bool = False,
                     key_mask: Optional[torch.Tensor] = None, query_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ctk_attention_ex on the operand layout of a joint window: q [Bo, N1, Bi, 384], k / v [Bo, N2, Bi, 384] (outer batch =
    video, then the track, then the inner batch = frame) -> out [Bo, N1, Bi, 384] (or its SH form [Bo*N1*Bi, 12, 2, 32]).
    Batch (bo, bi) attends q[bo, :, bi] over k / v[bo, :, bi]: ONE launch with inner = Bi, row strides bs = 1, is = Bi and the
    outer strides N1*Bi (q, out) and N2*Bi (k, v) -- different for the two sides.  key_mask [Bo, N2] / query_mask [Bo, N1] uint8."""
    (Bo, N1, Bi, _), N2 = q.shape, k.shape[1]
    assert k.shape == (Bo, N2, Bi, L.HID) and v.shape == k.shape
    a, out, _part = _attn_args(q, k, v, Bo * Bi, N1, N2, 1, 1, Bi, splits, out_split, key_mask, query_mask)
    b2 = L.AttnBatch2()
    b2.inner, b2.reserved = Bi, 0
    b2.q_os, b2.kv_os, b2.o_os = N1 * Bi, N2 * Bi, N1 * Bi
    b2.key_mask_os, b2.query_mask_os = N2, N1
    L.check(L.load().ctk_attention_ex(C.byref(a), C.byref(b2), _stream()), "ctk_attention_ex")
    return out


# ------------------------------------------------------------------------------------------
# pyramid / samplers
# ------------------------------------------------------------------------------------------
def ingest_frames(src: torch.Tensor, out: torch.Tensor, layout: Optional[str] = None) -> torch.Tensor:
    """Raw frames -> the encoder's input (ctk_ingest_frames): src uint8 or float32, channels-last [F,H,W,3] (layout "hwc") or
    planar [F,3,H,W] ("chw"), on the device; out float32 [F,3,h,w], contiguous -- e.g. a frame range of a resident buffer.  Value
    for value F.interpolate(src as float NCHW, (h, w), mode="bilinear", align_corners=True).  layout None: read off the shape
    (ValueError when both readings fit: H == 3 or W == 3).  The strides are taken from the tensor: a view is read where it lies
    when its innermost dimensions are dense -- the pixels of a row ("hwc": channel stride 1, pixel stride 3) or the rows of a
    frame's planes ("chw": element stride 1, channel stride H rows) -- and refused otherwise (ValueError; no silent copy)."""
    if src.dim() != 4 or src.dtype not in (torch.uint8, torch.float32) or not src.is_cuda:
        raise ValueError("ingest_frames: src must be a uint8 or float32 device tensor [F,H,W,3] or [F,3,H,W]")
    if layout is None:
        hwc, chw = src.shape[3] == 3, src.shape[1] == 3
        if hwc == chw:
            raise ValueError(f"ingest_frames: cannot tell the layout of a {tuple(src.shape)} source: pass layout='hwc' or 'chw'")
        layout = "hwc" if hwc else "chw"
    if layout not in ("hwc", "chw") or src.shape[3 if layout == "hwc" else 1] != 3:
        raise ValueError(f"ingest_frames: a {tuple(src.shape)} source is not layout {layout!r} with 3 channels")
    a = L.IngestArgs()
    if layout == "hwc":
        a.F, a.H, a.W = src.shape[:3]
        dense = src.stride(3) == 1 and src.stride(2) == 3
        a.row_stride, a.layout = src.stride(1), L.INGEST_HWC
        frame = a.H * a.row_stride
    else:
        a.F, a.H, a.W = src.shape[0], src.shape[2], src.shape[3]
        a.row_stride, a.layout = src.stride(2), L.INGEST_CHW
        dense = src.stride(3) == 1 and src.stride(1) == a.H * a.row_stride
        frame = 3 * a.H * a.row_stride
    if a.H == 1:  # (the stride of a dimension of size 1 is arbitrary)
        a.row_stride = a.W * (3 if layout == "hwc" else 1)
        frame = a.row_stride * (1 if layout == "hwc" else 3)
        dense = src.stride(3) == 1 and (src.stride(2) == 3 if layout == "hwc" else (a.W == 1 or src.stride(1) == a.W))
    if not dense:
        raise ValueError(f"ingest_frames: the innermost dimensions of the {layout} source are not dense (strides {src.stride()})")
    a.frame_stride = src.stride(0) if a.F > 1 else frame
    if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 4 and
            tuple(out.shape[:2]) == (a.F, 3) and out.device == src.device):
        raise ValueError(f"ingest_frames: out must be a contiguous float32 [{a.F},3,h,w] tensor on the source's device")
    a.h, a.w = out.shape[2:]
    a.dtype = L.INGEST_U8 if src.dtype == torch.uint8 else L.INGEST_F32
    a.src, a.dst = _ptr(src), _ptr(out)
    L.check(L.load().ctk_ingest_frames(C.byref(a), _stream()), "ctk_ingest_frames")
    return out


SEED_CELLS_MAX = 65536  # (csrc/seed.hip: one workgroup per cell)


def cell_scale(n: int, lo: float, hi: float) -> float:
    """inv_cw / inv_ch of ctk_stream_health_args and ctk_seed_args: float32 operands, float32 quotient, rounded once."""
    return float(torch.tensor(float(n), dtype=torch.float32) / (torch.tensor(hi, dtype=torch.float32) - torch.tensor(lo, dtype=torch.float32)))


def seed_points(frame: torch.Tensor, grid, bounds=None, radius: int = 3, margin: Optional[int] = None, inset: int = 0,
                min_score: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The best-textured pixel of every cell of grid = (gh, gw) over ONE frame, by ONE launch (ctk_seed_points; include/ctk.h and
    csrc/seed_math.h have the rules): frame float32 [3,h,w] (nominally 0..255), contiguous, on the device -- a frame of a resized
    chunk or of the push buffer -> int32 [gh*gw,3] on the device, row cy * gw + cx = (px, py, score) or (-1, -1, -1) for a cell
    without a candidate or whose best score is below min_score.  bounds = (x_lo, x_hi, y_lo, y_hi), inclusive, model-resolution
    pixels (default: the picture, (0, w - 1, 0, h - 1)): with the bounds and grid of StreamGroups.health a seed lies in the cell health
    counts it in.  margin (default radius + 1: the window and its gradients stay inside the image) and inset keep candidates away
    from the image border and from the edges of their cell.  out: a contiguous int32 [gh*gw,3] device tensor to write instead of a new
    one.  No wait."""
    if not (isinstance(frame, torch.Tensor) and frame.is_cuda and frame.dtype == torch.float32 and frame.dim() == 3 and
            frame.shape[0] == 3 and frame.is_contiguous()):
        raise ValueError("seed_points: frame must be a contiguous float32 device tensor [3,h,w]")
    gh, gw = (int(v) for v in grid)
    if gh < 1 or gw < 1 or gh * gw > SEED_CELLS_MAX:
        raise ValueError(f"seed_points: the grid must have between 1 and {SEED_CELLS_MAX} cells, got {gh} x {gw}")
    radius = int(radius)
    margin = radius + 1 if margin is None else int(margin)
    if not 1 <= radius <= 7 or margin < 0 or int(inset) < 0 or int(min_score) < 0:
        raise ValueError("seed_points: radius must lie in 1..7; margin, inset and min_score must be >= 0")
    a = L.Seed.Args()
    a.h, a.w = frame.shape[1:]
    a.radius, a.margin, a.inset, a.min_score, a.reserved, a.gh, a.gw = radius, margin, int(inset), int(min_score), 0, gh, gw
    a.x_lo, a.x_hi, a.y_lo, a.y_hi = (float(v) for v in (bounds if bounds is not None else (0.0, a.w - 1.0, 0.0, a.h - 1.0)))
    if not (a.x_hi > a.x_lo and a.y_hi > a.y_lo):
        raise ValueError(f"seed_points: empty bounds {(a.x_lo, a.x_hi, a.y_lo, a.y_hi)}")
    a.inv_cw, a.inv_ch = cell_scale(gw, a.x_lo, a.x_hi), cell_scale(gh, a.y_lo, a.y_hi)
    seeds = torch.empty(gh * gw, 3, device=frame.device, dtype=torch.int32) if out is None else out
    if not (seeds.dtype == torch.int32 and tuple(seeds.shape) == (gh * gw, 3) and seeds.device == frame.device and seeds.is_contiguous()):
        raise ValueError(f"seed_points: out must be a contiguous int32 [{gh * gw},3] tensor on the frame's device")
    a.frame, a.seeds = _ptr(frame), _ptr(seeds)
    L.check(L.load().ctk_seed_points(C.byref(a), _stream()), "ctk_seed_points")
    return seeds


# ------------------------------------------------------------------------------------------
# readers of tracks: the tensor source (a finished result), stated once.  draw_tracks and the fit readers differ in the history rows
# they need (`rows`) and in their own struct fields; StreamGroups has the other source, a stream's history.
# ------------------------------------------------------------------------------------------
_scratch_cache = {}


def _scratch(kind: str, nbytes: int, device) -> torch.Tensor:
    """The workspace of one kind of reader ("draw", "motion" -- fit_objects, fit_planes and fit_epipolar share it --, "field"), cached per kind and device like
    _workspace -- but never in that cache: captured window graphs bake the address of that one in, and a reader must never be the
    reason it moves.  Nor does one kind ever move the buffer of another."""
    key = (kind, device.index if device.index is not None else torch.cuda.current_device())
    buf = _scratch_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _scratch_cache[key] = None  # (the old buffer goes before the larger one comes)
        buf = _scratch_cache[key] = torch.empty(max(nbytes, 16), device=device, dtype=torch.uint8)
    return buf


def _track_tensors(tracks, visible, who: str, points_max: Optional[int] = None):
    """tracks [T,N,2] / [G,T,N,2], visible [T,N] / [G,T,N] checked -> (tracks [G,T,N,2], visible [G,T,N], G, T, N, device)."""
    if not (isinstance(tracks, torch.Tensor) and tracks.is_cuda and tracks.dtype == torch.float32 and tracks.dim() in (3, 4) and
            tracks.shape[-1] == 2):
        raise ValueError(f"{who}: tracks must be a float32 device tensor [T,N,2] or [G,T,N,2]")
    tracks = (tracks[None] if tracks.dim() == 3 else tracks)
    G, T, N, _ = tracks.shape
    dev = tracks.device
    if not (isinstance(visible, torch.Tensor) and visible.dtype in (torch.bool, torch.uint8) and visible.device == dev and
            visible.numel() == G * T * N and tuple(visible.shape[-2:]) == (T, N)):
        raise ValueError(f"{who}: visible must be a bool or uint8 tensor [{T},{N}] or [{G},{T},{N}] on {dev}")
    if points_max is not None and not 1 <= N <= points_max:
        raise ValueError(f"{who}: between 1 and {points_max} points per group, got {N}")
    return tracks, visible.reshape(G, T, N), G, T, N, dev


def _frames_of(first_frame, frames, T: int, who: str):
    """(first_frame, frames) -> (f0, F), frames None: to the end; the rows must lie in [0, T)."""
    f0 = int(first_frame)
    F_ = T - f0 if frames is None else int(frames)
    if f0 < 0 or F_ < 1 or f0 + F_ > T:
        raise ValueError(f"{who}: frames [{f0}, {f0 + F_}) of {T} tracked frames")
    return f0, F_


def _first_row_i32(first_row, G: int, N: int, dev):
    """first_row int [N] / [G,N] (or None) as the C-ABI wants it: contiguous int32 [G,N] on the device."""
    if first_row is None:
        return None
    big = torch.iinfo(torch.int32).max  # (an int64 table marks an empty slot with its own maximum: clamped, not wrapped)
    return torch.as_tensor(first_row, device=dev).clamp(min=-big, max=big).to(torch.int32).expand(G, N).contiguous()


def _bind_tensors(a, tracks, visible, first_row, *, rows: int, f0: int, scale, F: Optional[int] = None, N_out: Optional[int] = None):
    """The source fields of a reader's args from result tensors (_track_tensors, _first_row_i32).  The C-ABI keeps the rows one call
    reads apart (rows of a ring must not alias), so `rows` > T appends rows that hold no visible point.  `a` keeps the tensors it now
    points into (padded or made contiguous here, they have no other owner) alive until its launch is issued."""
    G, T, N, _ = tracks.shape
    if rows > T:
        tracks = torch.cat([tracks, tracks.new_zeros(G, rows - T, N, 2)], dim=1)
        visible = torch.cat([visible, visible.new_zeros(G, rows - T, N)], dim=1)
    tracks, visible = tracks.contiguous(), visible.contiguous()
    visible = visible.view(torch.uint8) if visible.dtype == torch.bool else visible
    a.G, a.N, a.N_out, a.R, a.f0 = G, N, (N if N_out is None else N_out), tracks.shape[1], f0
    if F is not None:
        a.F = F
    a.sx, a.sy, a.thresh = float(scale[0]), float(scale[1]), 0.0
    a.hist_coords, a.visible, a.first_row = _ptr(tracks), _ptr(visible), _ptr(first_row)
    a._held = (tracks, visible, first_row)


def _out_tuple(out, specs, device, who: str):
    """The outputs of a reader, specs = [(name, dtype, shape)]: allocated, or `out` checked against them."""
    if out is None:
        return tuple([torch.empty(sh, device=device, dtype=dt) for _, dt, sh in specs])
    out = tuple(out)
    if len(out) != len(specs) or any(not isinstance(t_, torch.Tensor) or t_.device != device or t_.dtype != dt or tuple(t_.shape) != sh or
                                     not t_.is_contiguous() for t_, (_, dt, sh) in zip(out, specs)):
        want = ", ".join(f"{name} {str(dt)[6:]} {list(sh)}" for name, dt, sh in specs)
        raise ValueError(f"{who}: out must be contiguous ({want}) on {device}")
    return out


def _anchor_ptrs(anchor, G: int, N: int, device, who: str):
    """A FieldAnchor checked against the G groups and N points it must match -> (frame, coords pointer, visible pointer)."""
    c, v = anchor.coords, anchor.visible
    if not (isinstance(c, torch.Tensor) and c.dtype == torch.float32 and tuple(c.shape) == (G, N, 2) and c.device == device and
            c.is_contiguous() and isinstance(v, torch.Tensor) and v.dtype in (torch.uint8, torch.bool) and tuple(v.shape) == (G, N) and
            v.device == device and v.is_contiguous()) or anchor.frame < 0:
        raise ValueError(f"{who}: anchor must hold contiguous coords float32 [{G},{N},2] and visible uint8 [{G},{N}] on {device} and a "
                         f"frame >= 0")
    return anchor.frame, _ptr(c), _ptr(v.view(torch.uint8) if v.dtype == torch.bool else v)


# ------------------------------------------------------------------------------------------
# the fit readers (fit_motion, track_field, fit_objects, fit_planes, fit_epipolar, fit_pose, fit_resection, fit_p3p, fit_structure and the
# StreamGroups methods of the same names): the rules they share, each stated once; their two sources behind one interface; their one
# launch.  A reader's body (_motion_fit ... _structure_fit) makes its args, applies its rules, binds its source with its own back / fwd
# / to, and launches; the public functions build the source and call the body.
# ------------------------------------------------------------------------------------------
_F32, _I8, _I32, _BYTES = (torch.float32,), (torch.int8,), (torch.int32,), (torch.int8, torch.uint8, torch.bool)


def _kinds(dtypes) -> str:
    names = [str(d)[6:] for d in dtypes]
    return names[0] if len(names) == 1 else ", ".join(names[:-1]) + " or " + names[-1]


def _tensor_ptr(x, dtypes: tuple, shape: tuple, name: str, device, who: str, note: str = "") -> int:
    """The pointer of x, checked: a contiguous tensor of one of `dtypes` and of `shape` on `device`; note: a trailing word on whose it is."""
    if not (isinstance(x, torch.Tensor) and x.dtype in dtypes and x.device == device and tuple(x.shape) == shape and x.is_contiguous()):
        raise ValueError(f"{who}: {name} must be a contiguous {_kinds(dtypes)} tensor {list(shape)} on {device}{note}")
    return x.data_ptr()


def _source_form(a, lag, to, anchor, G: int, N: int, device, who: str, flow: bool = False) -> None:
    """Where the source frame of frame f is -- f - lag, a fixed frame `to`, or a FieldAnchor that matches G groups of N points --, as
    the fields to, lag, anchor_frame, anchor_coords, anchor_visible of a reader's args.  `to` or `anchor` replaces the lag, which is
    then not looked at; both at once are refused.  flow, track_field's form: exactly one of the three is given, and a negative lag
    leads to the frame ahead."""
    if flow and (to is not None) + (lag is not None) + (anchor is not None) != 1:
        raise ValueError(f"{who}: exactly one of to (a frame), lag (frame f against f - lag) and anchor (FieldAnchor) says where the field leads")
    if to is not None and anchor is not None:
        raise ValueError(f"{who}: one of to (a frame) and anchor (FieldAnchor) says where the motion starts, not both")
    a.to, a.lag, a.anchor_frame, a.anchor_coords, a.anchor_visible = -1, 0, 0, None, None
    if to is not None:
        a.to = int(to)
        if a.to < 0:
            raise ValueError(f"{who}: to must be a frame >= 0")
    elif anchor is not None:
        a.anchor_frame, a.anchor_coords, a.anchor_visible = _anchor_ptrs(anchor, G, N, device, who)
    else:
        a.lag = lag = int(lag)
        if lag == 0 or (lag < 0 and not flow):
            raise ValueError(f"{who}: lag must " + ("not be 0 (negative: forward flow)" if flow else "be >= 1"))


def _min_points_of(min_points, least: int, who: str) -> int:
    min_points = int(min_points)
    if not least <= min_points <= L.Motion.POINTS_MAX:
        raise ValueError(f"{who}: min_points must lie in {least}..{L.Motion.POINTS_MAX}")
    return min_points


def _positive_tol(tol, who: str) -> float:
    tol = float(tol)
    if not (math.isfinite(tol) and 0.0 < tol <= 3.0e38):
        raise ValueError(f"{who}: tol must be finite and > 0 (raw-video pixels)")
    return tol


def _sampling(a, hypotheses, seed, tol, min_base, who: str, resection: bool = False) -> None:
    """The seeded hypotheses of a robust fit and its bounds.  ctk_fit_resection has a ceiling of its own, calls the count
    `hypotheses`, takes any seed by its low 32 bits, wants a finite positive tol and has no min_base."""
    hypotheses, seed = int(hypotheses), int(seed)
    top = L.Resection.HYPOTHESES_MAX if resection else L.Motion.HYPOTHESES_MAX
    if not 1 <= hypotheses <= top:
        raise ValueError(f"{who}: hypotheses must lie in 1..{top}")
    if resection:
        a.hypotheses, a.seed, a.tol = hypotheses, seed & 0xffffffff, _positive_tol(tol, who)
        return
    if not 0 <= seed < 2 ** 32:
        raise ValueError(f"{who}: seed must lie in 0..2^32 - 1")
    a.K, a.seed, a.tol, a.min_base, a.reserved = hypotheses, seed, float(tol), float(min_base), 0


def _intrinsics(a, intrinsics, who: str) -> None:
    if isinstance(intrinsics, torch.Tensor) or len(intrinsics) != 4:
        raise ValueError(f"{who}: intrinsics must be four Python floats (fx, fy, cx, cy) in raw-video pixels")
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    if not (math.isfinite(fx) and math.isfinite(fy) and fx > 0.0 and fy > 0.0 and math.isfinite(cx) and math.isfinite(cy)):
        raise ValueError(f"{who}: intrinsics (fx, fy, cx, cy): fx and fy must be finite and > 0, cx and cy finite")
    a.fx, a.fy, a.cx, a.cy = fx, fy, cx, cy


def _frame_pair(frames):
    """frames = (first_frame, n), or None: every tracked frame -> what _frames_of takes."""
    return (0, None) if frames is None else (frames[0], int(frames[1]))


def _group_axis(x, dims: int):
    """A per-group input of the tensor form given without its group axis (`dims` axes) gets it."""
    return x[None] if isinstance(x, torch.Tensor) and x.dim() == dims else x


class _FitSource:
    """What the body of a fit reader asks of its source: who is called, the G groups of N points and the device that its own inputs
    must match, the N_out points and F frames of its outputs, bind() for the source fields of its args."""
    __slots__ = ("who", "G", "N", "N_out", "f0", "F", "device", "first_row", "scale")

    def per_point_ptr(self, x, dtypes, name: str) -> Optional[int]:
        """The pointer of a per-point list (labels, mask) [N] / [G,N] of the groups read, or None."""
        if x is None:
            return None
        if not (isinstance(x, torch.Tensor) and x.dtype in dtypes and x.device == self.device and x.numel() == self.G * self.N and
                x.shape[-1] == self.N and x.is_contiguous()):
            raise ValueError(f"{self.who}: {name} must be a contiguous {_kinds(dtypes)} tensor [{self.N}] or [{self.G},{self.N}] on {self.device}")
        return _ptr(x)


class _TensorSource(_FitSource):
    """A finished result as the source of a fit reader: tracks [T,N,2] / [G,T,N,2] and visible checked (_track_tensors), the frames
    [f0, f0 + F) of them (_frames_of), all N points unless the reader takes an N_out (at most out_max)."""
    __slots__ = ("tracks", "visible", "T", "kept")

    def __init__(self, who: str, tracks, visible, first_frame=0, frames=None, *, first_row=None, scale=(1, 1), N_out=None,
                 points_max: Optional[int] = L.Motion.POINTS_MAX, out_max: Optional[int] = None):
        self.who, self.first_row, self.scale = who, first_row, scale
        self.tracks, self.visible, self.G, self.T, self.N, self.device = _track_tensors(tracks, visible, who, points_max)
        self.N_out = self.N if N_out is None else int(N_out)
        if out_max is not None and not 1 <= self.N_out <= min(self.N, out_max):
            raise ValueError(f"{who}: N_out must lie in [1, {min(self.N, out_max)}]")
        self.f0, self.F = _frames_of(first_frame, frames, self.T, who)

    def per_point_ptr(self, x, dtypes, name: str) -> Optional[int]:
        """labels / mask [N] serve every group: the copy lives as long as the source, that is until the launch is issued."""
        if isinstance(x, torch.Tensor) and x.dim() == 1 and self.G > 1:
            x = self.kept = x.expand(self.G, -1).contiguous()
        return super().per_point_ptr(x, dtypes, name)

    def bind(self, a, back: int = 0, fwd: int = 0, to: int = -1, hint: str = "") -> None:
        """The source fields of `a` for a reader that reads, besides its frames, the `back` frames before each, the frame `fwd` after
        each and the frame `to`: the rows one call reads are kept apart (_bind_tensors), so there are at least F + back + fwd."""
        if to >= self.T:
            raise ValueError(f"{self.who}: to = {to} of {self.T} tracked frames")
        _bind_tensors(a, self.tracks, self.visible, _first_row_i32(self.first_row, self.G, self.N, self.device),
                      rows=max(self.T, self.F + back + fwd, self.f0 + self.F + fwd), f0=self.f0, F=self.F, N_out=self.N_out, scale=self.scale)


class _HistorySource(_FitSource):
    """A stream's history as the source of a fit reader: whom it reads (StreamGroups._reader), which frames it may (_held, with the
    reader's back / fwd / to) and the source fields (_bind_history).  N is the stream's: labels, masks and anchors match it; outputs
    and what an earlier reader wrote per point match N_out."""
    __slots__ = ("gs", "g0", "thresh")

    def __init__(self, gs, who: str, f0, F, N_out, group, first_row, scale, thresh, points_max: int = L.Motion.POINTS_MAX):
        self.N_out, self.g0, self.G = gs._reader(who, N_out, group, first_row, points_max)
        self.gs, self.who, self.first_row, self.scale, self.thresh = gs, who, first_row, scale, thresh
        self.f0, self.F, self.N, self.device = int(f0), int(F), gs.N, gs.queries.device

    def bind(self, a, back: int = 0, fwd: int = 0, to: int = -1, hint: str = "") -> None:
        self.gs._held(self.who, self.f0, self.F, back=back, fwd=fwd, to=to, hint=hint)
        self.gs._bind_history(a, self.g0, self.G, self.N_out, self.f0, self.F, self.scale, self.thresh, self.first_row)


def _field_outs(G: int, F: int, H: int, W: int, cs: int):
    gh, gw = ((H - 1) >> cs) + 2, ((W - 1) >> cs) + 2  # (field_grid's nodes)
    return [("field", torch.int32, (G, F, gh, gw, 2)), ("level", torch.uint8, (G, F, gh, gw)), ("stats", torch.int32, (G, F, 4))]


_Fit = namedtuple("_Fit", "args entry scratch outs")  # outs: (G, F, N_out, args) -> [(the struct field of an output = its name, dtype, shape)]
_FITS = {
    "motion": _Fit(L.Motion.Args, "ctk_fit_motion", "motion", lambda G, F, n, a: [
        ("motion", torch.float32, (G, F, 2, 3)), ("inlier", torch.int8, (G, F, n)), ("stats", torch.int32, (G, F, 4))]),
    "field": _Fit(L.Field.Args, "ctk_track_field", "field", lambda G, F, n, a: _field_outs(G, F, a.H, a.W, a.cs)),
    "objects": _Fit(L.Objects.Args, "ctk_fit_objects", "motion", lambda G, F, n, a: [
        ("motion", torch.float32, (G, F, a.L, 2, 3)), ("label", torch.int8, (G, F, n)), ("stats", torch.int32, (G, F, a.L, 4)),
        ("box", torch.int32, (G, F, a.L, 4))]),
    "planes": _Fit(L.Planes.Args, "ctk_fit_planes", "motion", lambda G, F, n, a: [
        ("homography", torch.float32, (G, F, a.L, 3, 3)), ("label", torch.int8, (G, F, n)), ("stats", torch.int32, (G, F, a.L, 4)),
        ("box", torch.int32, (G, F, a.L, 4))]),
    "epipolar": _Fit(L.Epipolar.Args, "ctk_fit_epipolar", "motion", lambda G, F, n, a: [
        ("fundamental", torch.float32, (G, F, 3, 3)), ("label", torch.int8, (G, F, n)), ("error", torch.float32, (G, F, n)),
        ("stats", torch.int32, (G, F, 4))]),
    "pose": _Fit(L.Pose.Args, "ctk_fit_pose", "motion", lambda G, F, n, a: [
        ("pose", torch.float32, (G, F, 3, 4)), ("depth", torch.float32, (G, F, n, 2)), ("stats", torch.int32, (G, F, 4))]),
    "resection": _Fit(L.Resection.Args, "ctk_fit_resection", "motion", lambda G, F, n, a: [
        ("pose", torch.float32, (G, F, 3, 4)), ("label", torch.int8, (G, F, n)), ("error", torch.float32, (G, F, n)),
        ("stats", torch.int32, (G, F, 4))]),
    "p3p": _Fit(L.P3p.Args, "ctk_fit_p3p", "motion", lambda G, F, n, a: [
        ("pose", torch.float32, (G, F, 3, 4)), ("label", torch.int8, (G, F, n)), ("error", torch.float32, (G, F, n)),
        ("stats", torch.int32, (G, F, 4))]),
    "focal": _Fit(L.Focal.Args, "ctk_fit_focal", "motion", lambda G, F, n, a: [
        ("focal", torch.float32, (G,)), ("curve", torch.int64, (G, a.K + 2)), ("cost", torch.int64, (G, F, a.K)),
        ("stats", torch.int32, (G, 4))]),
    "structure": _Fit(L.Structure3D.Args, "ctk_fit_structure", "motion", lambda G, F, n, a: [
        ("points", torch.float32, (G, n, 3)), ("label", torch.int8, (G, n)), ("error", torch.float32, (G, n)), ("stats", torch.int32, (G, n, 4)),
        ("origin_out", torch.float32, (G, 3, 4))]),
}


def _fit_launch(kind: str, a, out, device, who: str):
    """The launch of a fit reader, by its row of _FITS: the outputs for the G, F and N_out of `a` allocated (or `out` checked) and
    their pointers written, the workspace asked for and taken from the scratch buffer of the row's kind, the entry point called."""
    _, entry, scratch, outs = _FITS[kind]
    specs = outs(a.G, a.F, a.N_out, a)
    out = _out_tuple(out, specs, device, who)
    for (name, _, _), t_ in zip(specs, out):
        setattr(a, name, t_.data_ptr())
    ref = C.byref(a)
    ws = _scratch(scratch, _query_bytes(entry + "_workspace_bytes", ref), device)
    L.check(getattr(L.load(), entry)(ref, ws.data_ptr(), ws.numel(), _stream()), entry)
    return out


# ------------------------------------------------------------------------------------------
# draw tracks (csrc/draw.hip; include/ctk.h, "draw tracks")
# ------------------------------------------------------------------------------------------
def rainbow_colors(y: torch.Tensor) -> torch.Tensor:
    """Default colours of draw_tracks: y [...,N] (the points' y on their first row) -> uint8 [...,N,3], an integer HSV ramp red ->
    yellow -> green -> cyan -> blue over min(y) .. max(y) of each row of points (the idea of the reference visualiser's
    mode="rainbow", without matplotlib): t = floor((y - lo) / (hi - lo) * 1020) in 0..1020, four ramps of 255 steps.  A y that is not
    finite takes t = 0.  Torch glue: it runs when the point set changes, not per drawn frame."""
    y = y.float()
    finite = torch.isfinite(y)
    big = torch.finfo(torch.float32).max
    lo = torch.where(finite, y, y.new_tensor(big)).amin(dim=-1, keepdim=True)
    hi = torch.where(finite, y, y.new_tensor(-big)).amax(dim=-1, keepdim=True)
    t = ((y - lo) / (hi - lo).clamp_min(1e-6) * 1020.0).nan_to_num(0.0, 0.0, 0.0).clamp(0.0, 1020.0).long()
    seg, x = t // 255, t % 255
    zero, full = torch.zeros_like(x), torch.full_like(x, 255)
    r = torch.where(seg == 0, full, torch.where(seg == 1, 255 - x, zero))
    g = torch.where(seg == 0, x, torch.where(seg <= 2, full, torch.where(seg == 3, 255 - x, zero)))
    b = torch.where(seg <= 1, zero, torch.where(seg == 2, x, full))
    return torch.stack([r, g, b], dim=-1).to(torch.uint8)


def default_alpha(trail: int) -> List[int]:
    """alpha[0] = 255 (marks), alpha[k] = 255 * (L + 1 - k)^2 // (L + 1)^2 for segment k of L = trail: the quadratic fade of the
    reference visualiser's trails, in integers."""
    return [255] + [255 * (trail + 1 - k) ** 2 // (trail + 1) ** 2 for k in range(1, trail + 1)]


def _draw_surface(frames: torch.Tensor, layout: Optional[str], who: str):
    """uint8 device frames [F,H,W,3] / [F,3,H,W] -> (layout, F, H, W, row_stride, frame_stride), strides in elements, read off the
    tensor by the rules of ingest_frames: a view is used where it lies when its innermost dimensions are dense."""
    if not (isinstance(frames, torch.Tensor) and frames.dim() == 4 and frames.dtype == torch.uint8 and frames.is_cuda):
        raise ValueError(f"{who}: frames must be a uint8 device tensor [F,H,W,3] or [F,3,H,W]")
    if layout is None:
        hwc, chw = frames.shape[3] == 3, frames.shape[1] == 3
        if hwc == chw:
            raise ValueError(f"{who}: cannot tell the layout of {tuple(frames.shape)} frames: pass layout='hwc' or 'chw'")
        layout = "hwc" if hwc else "chw"
    if layout not in ("hwc", "chw") or frames.shape[3 if layout == "hwc" else 1] != 3:
        raise ValueError(f"{who}: {tuple(frames.shape)} frames are not layout {layout!r} with 3 channels")
    if layout == "hwc":
        F_, H, W = frames.shape[:3]
        row = frames.stride(1)
        dense, frame = frames.stride(3) == 1 and frames.stride(2) == 3, H * row
    else:
        F_, H, W = frames.shape[0], frames.shape[2], frames.shape[3]
        row = frames.stride(2)
        dense, frame = frames.stride(3) == 1 and frames.stride(1) == H * row, 3 * H * row
    if H == 1:  # (the stride of a dimension of size 1 is arbitrary)
        row = W * (3 if layout == "hwc" else 1)
        frame = row * (1 if layout == "hwc" else 3)
        dense = frames.stride(3) == 1 and (frames.stride(2) == 3 if layout == "hwc" else (W == 1 or frames.stride(1) == W))
    if F_ < 1 or not dense:
        raise ValueError(f"{who}: the innermost dimensions of the {layout} frames are not dense (strides {frames.stride()})")
    return layout, F_, H, W, row, (frames.stride(0) if F_ > 1 else frame)


def _draw_style(a, trail, radius, half_width, alpha, max_jump, who: str) -> None:
    trail, radius, half_width, max_jump = int(trail), int(radius), int(half_width), int(max_jump)
    D = L.Draw
    if not (0 <= trail <= D.TRAIL_MAX and 1 <= radius <= D.RADIUS_MAX and 0 <= half_width <= D.HALF_WIDTH_MAX and 1 <= max_jump <= D.JUMP_MAX):
        raise ValueError(f"{who}: trail must lie in 0..{D.TRAIL_MAX}, radius in 1..{D.RADIUS_MAX}, half_width in 0..{D.HALF_WIDTH_MAX}, "
                         f"max_jump in 1..{D.JUMP_MAX}")
    alpha = default_alpha(trail) if alpha is None else [int(v) for v in alpha]
    if len(alpha) < trail + 1 or any(not 0 <= v <= 255 for v in alpha):
        raise ValueError(f"{who}: alpha must hold trail + 1 = {trail + 1} values in 0..255 (alpha[0]: the marks)")
    a.trail, a.radius, a.half_width, a.max_jump, a.reserved = trail, radius, half_width, max_jump, 0
    for k in range(trail + 1):
        a.alpha[k] = alpha[k]


def _draw_launch(a, frames: torch.Tensor, out: Optional[torch.Tensor], layout: Optional[str], who: str) -> torch.Tensor:
    """Fills the surface fields of ctk_draw_args from `frames` (and `out`), then the two launches of ctk_draw_tracks."""
    geo = _draw_surface(frames, layout, who)
    a.layout = L.INGEST_HWC if geo[0] == "hwc" else L.INGEST_CHW
    _, a.F, a.H, a.W, a.row_stride, a.frame_stride = geo
    if out is None or out is frames:
        a.src, a.dst, out = None, _ptr(frames), frames
    else:
        if out.device != frames.device or out.shape != frames.shape or _draw_surface(out, geo[0], who) != geo:
            raise ValueError(f"{who}: out must be uint8 frames of the shape, strides and device of `frames`")
        a.src, a.dst = _ptr(frames), _ptr(out)
    ws = _scratch("draw", _query_bytes("ctk_draw_tracks_workspace_bytes", C.byref(a)), frames.device)
    L.check(L.load().ctk_draw_tracks(C.byref(a), _ptr(ws), ws.numel(), _stream()), "ctk_draw_tracks")
    return out


def draw_tracks(frames: torch.Tensor, tracks: torch.Tensor, visible: torch.Tensor, colors: Optional[torch.Tensor] = None, *,
                trail: int = 0, radius: int = 4, half_width: int = 1, alpha=None, max_jump: int = 256, first_frame: int = 0,
                scale=(1.0, 1.0), first_row: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                layout: Optional[str] = None) -> torch.Tensor:
    """Marks and fading trails of tracked points drawn onto uint8 frames on the device by two launches and without a wait
    (ctk_draw_tracks; include/ctk.h and csrc/draw_math.h have the rules) -- what the reference does on the host in
    cotracker/utils/visualizer.py.  Works on any result of any predictor here, offline ones included.

    frames   uint8 [F,H,W,3] or [F,3,H,W] on the device, drawn IN PLACE unless `out` (same shape and strides) is given; the strides
             are taken from the tensor and the layout is inferred as ingest_frames does it.  Picture j shows frame first_frame + j.
    tracks   float32 [T,N,2] or [G,T,N,2], pixels = rint(tracks * scale); visible bool / uint8 [T,N] or [G,T,N].
    colors   uint8 [N,3] or [G,N,3]; default rainbow_colors of the points' y on their first row (first_row, else frame 0).
    A visible point is a disc of `radius`, an invisible one a ring; segment k = 1..trail joins frames f-k and f-k+1 where both are
    visible and no more than max_jump pixels apart, `half_width` pixels to each side, blended with alpha[k] (default: the
    quadratic fade default_alpha(trail); alpha[0]: the marks).  first_row int [N] / [G,N]: nothing of a point is drawn below that
    frame (INT32_MAX: never).  Returns the drawn frames (`frames` itself, or `out`)."""
    who = "draw_tracks"
    tracks, visible, G, T, N, dev = _track_tensors(tracks, visible, who)
    if not (isinstance(frames, torch.Tensor) and frames.dim() == 4):
        raise ValueError(f"{who}: frames must be a uint8 device tensor [F,H,W,3] or [F,3,H,W]")
    F_, first_frame = frames.shape[0], int(first_frame)
    if first_frame < 0 or first_frame + F_ > T:
        raise ValueError(f"{who}: pictures of frames [{first_frame}, {first_frame + F_}) of {T} tracked frames")
    a = L.Draw.Args()
    _draw_style(a, trail, radius, half_width, alpha, max_jump, who)
    first_row = _first_row_i32(first_row, G, N, dev)
    if colors is None:
        at = torch.zeros(G, 1, N, dtype=torch.long, device=dev) if first_row is None else first_row.long().clamp(0, T - 1)[:, None]
        colors = rainbow_colors(tracks[..., 1].gather(1, at)[:, 0])
    if not (isinstance(colors, torch.Tensor) and colors.dtype == torch.uint8 and colors.numel() == G * N * 3 and colors.shape[-1] == 3):
        raise ValueError(f"{who}: colors must be a uint8 tensor [{N},3] or [{G},{N},3]")
    colors = colors.to(dev).reshape(G, N, 3).contiguous()
    _bind_tensors(a, tracks, visible, first_row, rows=F_ + a.trail, f0=first_frame, scale=scale)
    a.colors = _ptr(colors)
    return _draw_launch(a, frames, out, layout, who)


# ------------------------------------------------------------------------------------------
# fit motion (csrc/motion.hip; include/ctk.h, "fit motion")
# ------------------------------------------------------------------------------------------
MOTION_MODELS = {"translation": L.Motion.TRANSLATION, "similarity": L.Motion.SIMILARITY}


def _model_of(model, who: str) -> int:
    if model not in MOTION_MODELS:
        raise ValueError(f"{who}: model must be one of {sorted(MOTION_MODELS)}, got {model!r}")
    return MOTION_MODELS[model]


def _motion_fit(src, lag, model, tol, hypotheses, min_base, seed, out):
    a, who = _FITS["motion"].args(), src.who
    lag = int(lag)
    if lag < 1:  # (ctk_fit_motion has the lag form alone: no `to`, no anchor, no _source_form)
        raise ValueError(f"{who}: lag must be >= 1")
    a.lag, a.model = lag, _model_of(model, who)
    _sampling(a, hypotheses, seed, tol, min_base, who)
    src.bind(a, back=lag, hint=": fit fewer frames per call")
    return _fit_launch("motion", a, out, src.device, who)


def fit_motion(tracks: torch.Tensor, visible: torch.Tensor, *, lag: int = 1, model: str = "similarity", tol: float = 2.0,
               hypotheses: int = 128, min_base: float = 16.0, seed: int = 0, scale=(1.0, 1.0), first_frame: int = 0,
               frames: Optional[int] = None, out=None):
    """How the camera moved from frame f - lag to frame f, and which points moved differently: a robust fit over the tracked points,
    per frame, by one launch and without a wait (ctk_fit_motion; include/ctk.h and csrc/motion_math.h have the rules).  Works on any
    result of any predictor here, offline ones included.

    tracks   float32 [T,N,2] or [G,T,N,2] (N <= 8192), positions = tracks * scale; visible bool / uint8 [T,N] or [G,T,N]: a point
             counts on a frame pair when it is visible on both.
    model    "similarity" (rotation, scale, shift) or "translation"; `hypotheses` seeded samples per frame are scored with the bound
             `tol` (pixels, max norm) and the best one is refitted over its inliers; a similarity's sample pair is at least
             `min_base` pixels apart.  The same seed gives the same answer for a frame however a range is cut into calls.
    Rows are the frames first_frame .. first_frame + frames - 1 (default: to the end).  Returns (motion float32 [G,F,2,3]:
    destination = motion @ (source, 1); inlier int8 [G,F,N]: -1 no correspondence, 0 outlier, 1 inlier; stats int32 [G,F,4] =
    (correspondences, inliers, best hypothesis or -1, 0)) -- `out` when given.  A frame without an admissible hypothesis (among
    them every f < lag) has the identity."""
    src = _TensorSource("fit_motion", tracks, visible, first_frame, frames, scale=scale)
    return _motion_fit(src, lag, model, tol, hypotheses, min_base, seed, out)


# ------------------------------------------------------------------------------------------
# warp frames (csrc/warp.hip; include/ctk.h, "warp frames")
# ------------------------------------------------------------------------------------------
WARP_BORDERS = {"fill": L.Warp.BORDER_FILL, "edge": L.Warp.BORDER_EDGE}


def _warp_border_fill(border: str, fill, who: str) -> List[int]:
    """The border's name checked and the three fill values as integers (warp_frames, lens_frames)."""
    if border not in WARP_BORDERS:
        raise ValueError(f"{who}: border must be one of {sorted(WARP_BORDERS)}, got {border!r}")
    fill = [int(v) for v in fill]
    if len(fill) != 3 or any(not 0 <= v <= 255 for v in fill):
        raise ValueError(f"{who}: fill must hold three values in 0..255")
    return fill


def _warp_args(frames: torch.Tensor, out: Optional[torch.Tensor], border: str, fill, layout: Optional[str], who: str):
    """Everything of ctk_warp_args but the matrices, from `frames` and `out` (allocated dense when None) -> (args, out)."""
    lay, F_, H, W, row, frame = _draw_surface(frames, layout, who)
    fill = _warp_border_fill(border, fill, who)
    if out is None:
        out = torch.empty(tuple(frames.shape), dtype=torch.uint8, device=frames.device)
    elif out is frames or not isinstance(out, torch.Tensor) or out.device != frames.device or out.shape != frames.shape:
        raise ValueError(f"{who}: out must be uint8 frames of the shape and device of `frames`, and not `frames` itself (a warp cannot "
                         f"run in place)")
    _, _, _, _, orow, oframe = _draw_surface(out, lay, who)
    rows, row_bytes = (H, 3 * W) if lay == "hwc" else (3 * H, W)
    ends = [t_.data_ptr() + (F_ - 1) * fs + (rows - 1) * rs + row_bytes for t_, fs, rs in ((frames, frame, row), (out, oframe, orow))]
    if frames.data_ptr() < ends[1] and out.data_ptr() < ends[0]:
        raise ValueError(f"{who}: out overlaps `frames` (a warp cannot run in place)")
    a = L.Warp.Args()
    a.F, a.H, a.W, a.layout, a.border, a.reserved = F_, H, W, (L.INGEST_HWC if lay == "hwc" else L.INGEST_CHW), WARP_BORDERS[border], 0
    for k in range(3):
        a.fill[k] = fill[k]
    a.src_frame_stride, a.src_row_stride, a.dst_frame_stride, a.dst_row_stride = frame, row, oframe, orow
    a.src, a.dst = _ptr(frames), _ptr(out)
    return a, out


def _warp_launch(a, matrices: torch.Tensor, device, who: str) -> None:
    if not (isinstance(matrices, torch.Tensor) and matrices.dtype == torch.float32 and matrices.device == device and
            matrices.numel() == a.F * 6 and tuple(matrices.shape[-2:]) == (2, 3) and matrices.is_contiguous()):
        raise ValueError(f"{who}: matrices must be a contiguous float32 tensor [{a.F},2,3] on {device}")
    a.matrices = _ptr(matrices)
    L.check(L.load().ctk_warp_frames(C.byref(a), _stream()), "ctk_warp_frames")


def warp_frames(frames: torch.Tensor, matrices: torch.Tensor, *, out: Optional[torch.Tensor] = None, border: str = "fill",
                fill=(0, 0, 0), layout: Optional[str] = None) -> torch.Tensor:
    """uint8 pictures resampled under one 2 x 3 matrix each, on the device, by one launch and without a wait (ctk_warp_frames;
    include/ctk.h and csrc/warp_math.h have the rules) -- what a caller otherwise writes as uint8 -> float, affine_grid,
    grid_sample, round, -> uint8.

    frames   uint8 [F,H,W,3] or [F,3,H,W] on the device; the strides are taken from the tensor and the layout is inferred as
             ingest_frames does it (a pitch-aligned surface or a crop needs no copy).
    matrices float32 [F,2,3] on the device: matrices[j] maps an OUTPUT pixel to a SOURCE position, (sx, sy) = m (x, y, 1), pixel
             centres at integers.  A matrix that is not finite or out of range (|linear| > 8, |shift| > 32768) copies its picture.
    border   "fill": a tap outside the picture has the value `fill` (three values 0..255); "edge": the edge pixels go on for ever.
    out      uint8 frames of the same shape with strides of their own; must not overlap `frames`.  Default: a new dense tensor.
    Bilinear in 1/256 pixel with Q24 coefficients: the identity copies bit for bit, an integer shift is a shifted copy.  Returns out."""
    who = "warp_frames"
    a, out = _warp_args(frames, out, border, fill, layout, who)
    _warp_launch(a, matrices, frames.device, who)
    return out


def zoom_matrix(H: int, W: int, zoom: float) -> torch.Tensor:
    """The float32 `post` [2,3] of smooth_path that scales by 1 / zoom about the centre of an H x W picture ((W - 1) / 2, (H - 1) / 2):
    zoom > 1 shows the middle of the stabilised picture enlarged, which hides the border a correction uncovers.  float32 arithmetic:
    s = 1 / zoom, t = c - s * c.  On the host."""
    zoom = float(zoom)
    if not (zoom > 0.0 and zoom < float("inf")):
        raise ValueError(f"zoom_matrix: zoom must be positive and finite, got {zoom!r}")
    s = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(zoom, dtype=torch.float32)
    cx, cy = torch.tensor((int(W) - 1) / 2, dtype=torch.float32), torch.tensor((int(H) - 1) / 2, dtype=torch.float32)
    zero = torch.tensor(0.0, dtype=torch.float32)
    return torch.stack([s, zero, cx - s * cx, zero, s, cy - s * cy]).reshape(2, 3)


def _path_state(G: int, device) -> torch.Tensor:
    """The state of smooth_path before the first frame: the identity per group, float64 [G,6] on the device (no copy from the host)."""
    state = torch.zeros(G, 6, dtype=torch.float64, device=device)
    state[:, 0::4] = 1.0
    return state


def smooth_path(motion: torch.Tensor, state: Optional[torch.Tensor] = None, *, alpha: float = 0.1, post: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None):
    """Per-frame camera motions (fit_motion with lag = 1) -> the matrices that steady the camera, for warp_frames, by one launch and
    without a wait (ctk_smooth_path; include/ctk.h and csrc/warp_math.h have the rule): a causal, leaky lock-on.  With C_f the
    cumulative camera pose and S_f = (1 - alpha) S_f-1 + alpha C_f its exponential smoothing, warp[f] = inverse(C_f) S_f.

    motion   float32 [G,F,2,3] or [F,2,3] on the device; a matrix that is not finite counts as the identity.
    state    float64 [G,6] on the device, updated IN PLACE: what the previous call for the frames just before these returned.  None:
             the identity (the first frame of `motion` is the one locked onto).
    alpha    0 locks onto the first frame for ever, 1 corrects nothing; a steady pan of v pixels a frame settles (1 - alpha) v / alpha
             pixels behind.
    post     float32 [2,3] (zoom_matrix): composed onto every output, not part of the state.
    Returns (warp float32 of the shape of `motion` -- `out` when given --, state): a range cut into calls gives the bits of one call."""
    who = "smooth_path"
    if not (isinstance(motion, torch.Tensor) and motion.is_cuda and motion.dtype == torch.float32 and motion.dim() in (3, 4) and
            tuple(motion.shape[-2:]) == (2, 3) and motion.numel() > 0):
        raise ValueError(f"{who}: motion must be a float32 device tensor [G,F,2,3] or [F,2,3]")
    dev, shape = motion.device, tuple(motion.shape)
    G, F_ = (1, shape[0]) if motion.dim() == 3 else shape[:2]
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"{who}: alpha must lie in [0, 1], got {alpha!r}")
    if state is None:
        state = _path_state(G, dev)
    elif not (isinstance(state, torch.Tensor) and state.dtype == torch.float64 and state.device == dev and tuple(state.shape) == (G, 6) and
              state.is_contiguous()):
        raise ValueError(f"{who}: state must be a contiguous float64 tensor [{G},6] on {dev}")
    if post is not None:
        post = torch.as_tensor(post)
        if post.dtype != torch.float32 or tuple(post.shape) != (2, 3):
            raise ValueError(f"{who}: post must be a float32 tensor [2,3]")
        post = post.to(dev).contiguous()
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.device == dev and tuple(out.shape) == shape and
              out.is_contiguous()):
        raise ValueError(f"{who}: out must be a contiguous float32 tensor {list(shape)} on {dev}")
    motion = motion.contiguous()
    a = L.Warp.PathArgs()
    a.G, a.F, a.alpha, a.reserved = G, F_, alpha, 0
    a.motion, a.post, a.state, a.warp = _ptr(motion), _ptr(post), _ptr(state), _ptr(out)
    L.check(L.load().ctk_smooth_path(C.byref(a), _stream()), "ctk_smooth_path")
    return out, state


def stabilize(frames: torch.Tensor, tracks: torch.Tensor, visible: torch.Tensor, *, alpha: float = 0.1, zoom: float = 1.0,
              border: str = "fill", fill=(0, 0, 0), out: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None,
              model: str = "similarity", tol: float = 2.0, hypotheses: int = 128, min_base: float = 16.0, seed: int = 0):
    """Frames steadied by the motion of their tracked points, on the device: fit_motion(lag = 1), smooth_path, warp_frames -- three
    launches, no wait.  Works on any result of any predictor here, offline ones included.

    frames   uint8 [F,H,W,3] or [F,3,H,W] on the device; tracks float32 [F,N,2] (or [1,F,N,2]) in the pixels of the frames, visible
             bool / uint8 [F,N]: picture j is frame j of the tracks.
    alpha, zoom   smooth_path's alpha; zoom > 1 enlarges the middle (zoom_matrix) to hide the border a correction uncovers.
    border, fill, out   as warp_frames;  model, tol, hypotheses, min_base, seed   as fit_motion.
    state    smooth_path's state [1,6] of the frames just before these (None: lock onto frame 0), updated in place.
    Returns (out, warp float32 [F,2,3]: a point at position x of frame j appears at inverse(warp[j]) x, state)."""
    who = "stabilize"
    if not (isinstance(tracks, torch.Tensor) and tracks.dim() in (3, 4) and (tracks.dim() == 3 or tracks.shape[0] == 1)):
        raise ValueError(f"{who}: tracks must be a float32 device tensor [F,N,2] or [1,F,N,2]")
    if not (isinstance(frames, torch.Tensor) and frames.dim() == 4 and frames.shape[0] == tracks.shape[-3]):
        raise ValueError(f"{who}: frames must be uint8 [F,H,W,3] or [F,3,H,W] with one picture per tracked frame")
    a, out = _warp_args(frames, out, border, fill, None, who)
    post = None if float(zoom) == 1.0 else zoom_matrix(a.H, a.W, zoom).to(frames.device)
    motion = fit_motion(tracks, visible, lag=1, model=model, tol=tol, hypotheses=hypotheses, min_base=min_base, seed=seed)[0]
    warp, state = smooth_path(motion, state, alpha=alpha, post=post)
    _warp_launch(a, warp, frames.device, who)
    return out, warp[0], state


# ------------------------------------------------------------------------------------------
# lens (csrc/lens.hip; include/ctk.h, "lens")
# ------------------------------------------------------------------------------------------
LENS_DIRECTIONS = {"ideal": L.LENS_TO_IDEAL, "sensor": L.LENS_TO_SENSOR}


class Lens:
    """A real camera: the pinhole part of the sensor, the five Brown-Conrady coefficients every calibration tool writes, and the ideal
    (pinhole) camera that corrected pictures and positions are stated in (include/ctk.h, "lens"; csrc/lens_math.h has the model).

    intrinsics    (fx, fy, cx, cy) of the sensor in raw-video pixels, plain Python floats
    coefficients  (k1, k2, p1, p2, k3), the usual order
    ideal         (fx', fy', cx', cy') of the pinhole camera; default: `intrinsics`
    Refused (ValueError) unless all 13 numbers are finite, the focal lengths lie in [1, 1e6], |centre| <= 32768 and |coefficient| <=
    64: an invalid lens never counts as "no lens".  .intrinsics, .coefficients and .ideal are tuples; .ideal is what a caller hands to
    pose() / reconstruct() / ops.fit_pose as `intrinsics` once pictures or tracks have been corrected."""

    def __init__(self, intrinsics, coefficients, ideal=None):
        def floats(v, n, name):
            if isinstance(v, torch.Tensor) or len(v) != n:
                raise ValueError(f"Lens: {name} must be {n} Python floats")
            return tuple(float(x) for x in v)
        self.intrinsics = floats(intrinsics, 4, "intrinsics (fx, fy, cx, cy)")
        self.coefficients = floats(coefficients, 5, "coefficients (k1, k2, p1, p2, k3)")
        self.ideal = self.intrinsics if ideal is None else floats(ideal, 4, "ideal (fx', fy', cx', cy')")
        B = L.Lens
        for cam in (self.intrinsics, self.ideal):
            if not (all(math.isfinite(v) for v in cam) and all(B.FOCAL_MIN <= v <= B.FOCAL_MAX for v in cam[:2]) and
                    all(abs(v) <= B.REACH for v in cam[2:])):
                raise ValueError(f"Lens: a camera (fx, fy, cx, cy) needs finite numbers, focal lengths in [{B.FOCAL_MIN:g}, {B.FOCAL_MAX:g}] "
                                 f"and |centre| <= {B.REACH:g}; got {cam}")
        if not all(math.isfinite(v) and abs(v) <= B.COEFF_MAX for v in self.coefficients):
            raise ValueError(f"Lens: the coefficients must be finite with |k| <= {B.COEFF_MAX:g}; got {self.coefficients}")

    def __repr__(self):
        return f"Lens(intrinsics={self.intrinsics}, coefficients={self.coefficients}, ideal={self.ideal})"

    def bind(self, cam) -> None:
        """Fills a ctk_lens."""
        for i in range(4):
            cam.sensor[i], cam.ideal[i] = self.intrinsics[i], self.ideal[i]
        for i in range(5):
            cam.k[i] = self.coefficients[i]
        cam.reserved = 0.0


def _lens_common(a, lens, to, tol, who: str) -> None:
    if not isinstance(lens, Lens):
        raise ValueError(f"{who}: lens must be an ops.Lens")
    if to not in LENS_DIRECTIONS:
        raise ValueError(f"{who}: to must be one of {sorted(LENS_DIRECTIONS)}, got {to!r}")
    lens.bind(a.lens)
    a.direction, a.tol, a.reserved = LENS_DIRECTIONS[to], _positive_tol(tol, who), 0


def lens_frames(frames: torch.Tensor, lens: Lens, *, to: str = "ideal", size=None, out: Optional[torch.Tensor] = None, border: str = "fill",
                fill=(0, 0, 0), tol: float = 0.01, layout: Optional[str] = None) -> torch.Tensor:
    """uint8 pictures resampled between the pixels of a real lens and those of a pinhole camera, on the device, by one launch and
    without a wait (ctk_lens_frames; include/ctk.h and csrc/lens_math.h have the rules) -- what a caller otherwise writes as an
    undistortion map on the host, uint8 -> float, grid_sample, round, -> uint8.  The map is made once per pixel for all pictures of the
    call, in double.

    frames   uint8 [F,H,W,3] or [F,3,H,W] on the device; strides and layout as warp_frames reads them.
    lens     an ops.Lens.
    to       "ideal": the pictures come from the sensor and the result is what lens.ideal sees -- straight lines are straight, and
             every reader of tracks made on such pictures (epipolar() .. extend()) is right as it stands, given lens.ideal as the
             intrinsics.  "sensor": pinhole pictures as the real lens would show them (eight Newton rounds per pixel).
    size     (H, W) of the result (default: the source's); another size goes with another lens.ideal (or, to="sensor", intrinsics).
    out      uint8 pictures of that size and the source's layout with strides of their own; must not overlap `frames`.
    border   "fill" / "edge" as warp_frames; a pixel that has no source at all (the lens folds there, or `tol`, the residual of an
             accepted inverse in sensor pixels, is not met) takes `fill` under both.
    Bilinear in 1/256 pixel; Lens(K, (0, 0, 0, 0, 0)) copies bit for bit.  Returns out."""
    who = "lens_frames"
    lay, F_, H, W, row, frame = _draw_surface(frames, layout, who)
    fill = _warp_border_fill(border, fill, who)
    Ho, Wo = (H, W) if size is None else (int(size[0]), int(size[1]))
    want = (F_, Ho, Wo, 3) if lay == "hwc" else (F_, 3, Ho, Wo)
    if out is None:
        if Ho < 1 or Wo < 1:
            raise ValueError(f"{who}: size = (H, W) must be positive")
        out = torch.empty(want, dtype=torch.uint8, device=frames.device)
    elif out is frames or not isinstance(out, torch.Tensor) or out.device != frames.device or tuple(out.shape) != want:
        raise ValueError(f"{who}: out must be uint8 frames {list(want)} on {frames.device}, and not `frames` itself")
    _, _, _, _, orow, oframe = _draw_surface(out, lay, who)
    a = L.Lens.FramesArgs()
    _lens_common(a, lens, to, tol, who)
    a.F, a.H, a.W, a.Ho, a.Wo, a.layout, a.border = F_, H, W, Ho, Wo, (L.INGEST_HWC if lay == "hwc" else L.INGEST_CHW), WARP_BORDERS[border]
    for k in range(3):
        a.fill[k] = fill[k]
    a.src_frame_stride, a.src_row_stride, a.dst_frame_stride, a.dst_row_stride = frame, row, oframe, orow
    a.src, a.dst = _ptr(frames), _ptr(out)
    L.check(L.load().ctk_lens_frames(C.byref(a), _stream()), "ctk_lens_frames")  # (overlapping frames and out: refused there)
    return out


def lens_points(tracks: torch.Tensor, lens: Lens, *, to: str = "ideal", out: Optional[torch.Tensor] = None, labels: bool = False,
                tol: float = 0.01):
    """Positions carried between the pixels of a real lens and those of a pinhole camera, on the device, by one launch and without a
    wait (ctk_lens_points; include/ctk.h and csrc/lens_math.h have the rules).

    tracks   float32 [...,N,2] on the device, contiguous, any leading shape ([N,2], [T,N,2], [B,T,N,2], ...).
    to       "ideal": sensor pixels -> the pixels of lens.ideal, by eight Newton rounds in double; a position without an inverse
             (the lens folds there, or the residual exceeds `tol` sensor pixels) becomes NaN, which every fit reads as "not on this
             frame".  "sensor": ideal pixels -> sensor pixels by the closed form, for drawing results onto the original frames
             (ops.draw_tracks); NaN where the lens folds.  A position that is not finite or beyond 32768 becomes NaN either way.
    out      float32 of the same shape; out=tracks works in place.  Default: a new tensor.
    labels   True: also int8 [...,N]: 1 carried, 0 no image under the lens, -1 not a position.
    This completes the offline path without further code: tracks, vis = predictor(video); ideal = ops.lens_points(tracks, lens); then
    ops.fit_epipolar(ideal, vis, ...) -> ops.fit_pose(..., lens.ideal, ...) -> ops.fit_resection -> ops.fit_structure as today.
    Returns out, or (out, label)."""
    who = "lens_points"
    if not (isinstance(tracks, torch.Tensor) and tracks.is_cuda and tracks.dtype == torch.float32 and tracks.dim() >= 2 and
            tracks.shape[-1] == 2 and tracks.is_contiguous() and tracks.numel() > 0):
        raise ValueError(f"{who}: tracks must be a contiguous float32 device tensor [...,N,2]")
    if out is None:
        out = torch.empty_like(tracks)
    elif not (isinstance(out, torch.Tensor) and out.device == tracks.device and out.dtype == torch.float32 and out.shape == tracks.shape and
              out.is_contiguous()):
        raise ValueError(f"{who}: out must be a contiguous float32 tensor of the shape and device of `tracks` (or `tracks` itself)")
    N = tracks.shape[-2]
    rows = tracks.numel() // (2 * N)  # the leading shape folded to [G,F]: F as long as the ABI allows, G the rest
    F_ = next((f for f in range(min(rows, 65535), 0, -1) if rows % f == 0), 1)
    G = rows // F_
    if N > L.Lens.POINTS_MAX or G > 65535:
        raise ValueError(f"{who}: {tuple(tracks.shape)} tracks do not fold to [G,F,N,2] with G, F <= 65535 and N <= {L.Lens.POINTS_MAX}")
    label = torch.empty(tracks.shape[:-1], dtype=torch.int8, device=tracks.device) if labels else None
    a = L.Lens.PointsArgs()
    _lens_common(a, lens, to, tol, who)
    a.G, a.F, a.N = G, F_, N
    a.src_group_stride = a.dst_group_stride = F_ * N * 2
    a.src_frame_stride = a.dst_frame_stride = N * 2
    a.src, a.dst, a.label = _ptr(tracks), _ptr(out), _ptr(label)
    L.check(L.load().ctk_lens_points(C.byref(a), _stream()), "ctk_lens_points")
    return (out, label) if labels else out


# ------------------------------------------------------------------------------------------
# track field (csrc/field.hip; include/ctk.h, "track field")
# ------------------------------------------------------------------------------------------
class FieldAnchor:
    """One frame's row of a group, kept on the device for track_field's anchor form: coords float32 [G,N,2] (unscaled history
    positions), visible uint8 [G,N], the frame number they were taken on and the group of a stream they belong to."""
    __slots__ = ("coords", "visible", "frame", "group")

    def __init__(self, coords: torch.Tensor, visible: torch.Tensor, frame: int, group: int = 0):
        self.coords, self.visible, self.frame, self.group = coords, visible, int(frame), int(group)


def _field_cs(cell, who: str) -> int:
    cell = int(cell)
    cs = cell.bit_length() - 1
    if cell < 1 or 1 << cs != cell or not L.Field.CS_MIN <= cs <= L.Field.CS_MAX:
        raise ValueError(f"{who}: cell must be a power of two in {1 << L.Field.CS_MIN}..{1 << L.Field.CS_MAX}, got {cell}")
    return cs


def field_grid(size, cell: int = 16):
    """(gh, gw): the nodes of track_field's grid over a picture of size = (H, W) with cells of `cell` pixels."""
    cs = _field_cs(cell, "field_grid")
    return ((int(size[0]) - 1) >> cs) + 2, ((int(size[1]) - 1) >> cs) + 2


def _field_fit(src, size, cell, radius, to, lag, anchor, out):
    a, who = _FITS["field"].args(), src.who
    H, W, radius = int(size[0]), int(size[1]), int(radius)
    if not (1 <= H <= 32768 and 1 <= W <= 32768 and 1 <= radius <= L.Field.RADIUS_MAX):
        raise ValueError(f"{who}: size = (H, W) must lie in 1..32768 and radius in 1..{L.Field.RADIUS_MAX}")
    a.H, a.W, a.cs, a.radius, a.reserved = H, W, _field_cs(cell, who), radius, 0
    _source_form(a, lag, to, anchor, src.G, src.N, src.device, who, flow=True)
    src.bind(a, back=max(a.lag, 0), fwd=max(-a.lag, 0), to=a.to)  # (a negative lag reads the frame ahead)
    return _fit_launch("field", a, out, src.device, who)


def track_field(tracks: torch.Tensor, visible: torch.Tensor, *, size, cell: int = 16, radius: int = 2, to: Optional[int] = None,
                lag: Optional[int] = None, anchor: Optional[FieldAnchor] = None, scale=(1.0, 1.0), N_out: Optional[int] = None,
                first_frame: int = 0, frames: Optional[int] = None, first_row: Optional[torch.Tensor] = None, out=None):
    """A dense displacement field interpolated from the tracked points, per frame, by three launches and without a wait
    (ctk_track_field; include/ctk.h and csrc/field_math.h have the rules).  Works on any result of any predictor here.  The field of
    frame f lives on f's picture grid and leads to the matching position of a frame "to": a picture known on frame "to" is warped
    backwards onto frame f by warp_field.

    tracks   float32 [T,N,2] or [G,T,N,2], positions = tracks * scale; visible bool / uint8 [T,N] or [G,T,N].
    size     (H, W) of the picture in the pixels of the scaled positions; cell: pixels per grid cell, a power of two 4..64; radius: the
             reach of a point in cells, 1..4.
    to / lag / anchor   exactly one: a fixed frame; frame f against f - lag (negative: forward flow); a FieldAnchor.
    N_out    only the first N_out <= 8192 points are looked at (default: all N).  first_row int [N] / [G,N]: a point counts from that
             frame on (INT32_MAX: never).
    Rows are the frames first_frame .. first_frame + frames - 1 (default: to the end).  Returns (field int32 [G,F,gh,gw,2] in 1/256
    pixel, node (i, j) at pixel (i cell, j cell); level uint8 [G,F,gh,gw]: 0 own support, l filled from pyramid level l, 255 nothing;
    stats int32 [G,F,4] = (correspondences, nodes at level 0, highest level used, 0)) -- `out` when given."""
    src = _TensorSource("track_field", tracks, visible, first_frame, frames, first_row=first_row, scale=scale, N_out=N_out, points_max=None,
                        out_max=L.Field.POINTS_MAX)
    return _field_fit(src, size, cell, radius, to, lag, anchor, out)


def _field_surface(pics: torch.Tensor, layout: Optional[str], who: str):
    """uint8 device pictures [F,H,W,3] / [F,3,H,W] (as _draw_surface) or masks [F,H,W] -> (C, layout, F, H, W, row_stride,
    frame_stride), strides in elements."""
    if isinstance(pics, torch.Tensor) and pics.dim() == 3 and pics.dtype == torch.uint8 and pics.is_cuda:
        F_, H, W = pics.shape
        row = pics.stride(1) if H > 1 else W
        if F_ < 1 or (W > 1 and pics.stride(2) != 1) or row < W:
            raise ValueError(f"{who}: the rows of the [F,H,W] pictures are not dense (strides {pics.stride()})")
        return 1, "hwc", F_, H, W, row, (pics.stride(0) if F_ > 1 else H * row)
    if not (isinstance(pics, torch.Tensor) and pics.dim() == 4):
        raise ValueError(f"{who}: pictures must be a uint8 device tensor [F,H,W,3], [F,3,H,W] or [F,H,W]")
    return (3,) + tuple(_draw_surface(pics, layout, who))


def _warp_field_args(src: Optional[torch.Tensor], size, cell, border: str, fill, out, flow, layout: Optional[str], F_: int, who: str,
                     device=None):
    """ctk_warp_field_args but the field, from `src` and `out` (allocated dense when None), or from size = (H, W) alone when only the
    flow is asked for -> (args, out, flow)."""
    a = L.Field.WarpArgs()
    a.cs, a.reserved = _field_cs(cell, who), 0
    if border not in WARP_BORDERS:
        raise ValueError(f"{who}: border must be one of {sorted(WARP_BORDERS)}, got {border!r}")
    a.border = WARP_BORDERS[border]
    if src is None:
        a.F, a.H, a.W, a.C, a.layout = F_, int(size[0]), int(size[1]), 1, L.INGEST_HWC
        a.src, a.dst, out = None, None, None
    else:
        C_, lay, F_, H, W, row, frame = _field_surface(src, layout, who)
        device = src.device
        fill = [int(v) for v in ((fill,) * 3 if isinstance(fill, int) else fill)]
        if len(fill) != 3 or any(not 0 <= v <= 255 for v in fill):
            raise ValueError(f"{who}: fill must hold three values in 0..255 (or one)")
        if out is None:
            out = torch.empty(tuple(src.shape), dtype=torch.uint8, device=device)
        elif out is src or not isinstance(out, torch.Tensor) or out.device != device or out.shape != src.shape:
            raise ValueError(f"{who}: out must be uint8 pictures of the shape and device of the source, and not the source itself (a warp "
                             f"cannot run in place)")
        _, _, _, _, _, orow, oframe = _field_surface(out, lay, who)
        rows, row_bytes = (H, C_ * W) if lay == "hwc" else (C_ * H, W)
        ends = [t_.data_ptr() + (F_ - 1) * fs + (rows - 1) * rs + row_bytes for t_, fs, rs in ((src, frame, row), (out, oframe, orow))]
        if src.data_ptr() < ends[1] and out.data_ptr() < ends[0]:
            raise ValueError(f"{who}: out overlaps the source (a warp cannot run in place)")
        a.F, a.H, a.W, a.C, a.layout = F_, H, W, C_, (L.INGEST_HWC if lay == "hwc" else L.INGEST_CHW)
        for k in range(3):
            a.fill[k] = fill[k]
        a.src_frame_stride, a.src_row_stride, a.dst_frame_stride, a.dst_row_stride = frame, row, oframe, orow
        a.src, a.dst = _ptr(src), _ptr(out)
    if flow is True:
        flow = torch.empty(a.F, a.H, a.W, 2, dtype=torch.float32, device=device)
    elif flow is False or flow is None:
        flow = None
    elif not (isinstance(flow, torch.Tensor) and flow.dtype == torch.float32 and tuple(flow.shape) == (a.F, a.H, a.W, 2) and
              flow.is_cuda and (device is None or flow.device == device) and flow.is_contiguous()):
        raise ValueError(f"{who}: flow must be True or a contiguous float32 tensor [{a.F},{a.H},{a.W},2] on the device")
    a.flow = _ptr(flow)
    return a, out, flow


def _warp_field_launch(a, field: torch.Tensor, who: str) -> None:
    gh, gw = ((a.H - 1) >> a.cs) + 2, ((a.W - 1) >> a.cs) + 2
    if not (isinstance(field, torch.Tensor) and field.dtype == torch.int32 and field.is_cuda and field.numel() == a.F * gh * gw * 2 and
            tuple(field.shape[-3:]) == (gh, gw, 2) and field.is_contiguous()):
        raise ValueError(f"{who}: field must be a contiguous int32 device tensor [{a.F},{gh},{gw},2] (track_field's, for this size and cell)")
    a.field = _ptr(field)
    L.check(L.load().ctk_warp_field(C.byref(a), _stream()), "ctk_warp_field")


def warp_field(src: torch.Tensor, field: torch.Tensor, *, cell: int, border: str = "fill", fill=(0, 0, 0), out: Optional[torch.Tensor] = None,
               flow=False, layout: Optional[str] = None):
    """uint8 pictures or masks resampled through one displacement field each, on the device, by one launch and without a wait
    (ctk_warp_field; include/ctk.h and csrc/field_math.h have the rules): out(x, y) = src((x, y) + field there), bilinear in 1/256
    pixel with ctk_warp_frames' borders.  A zero field copies bit for bit, a constant field of whole pixels is a shifted copy.

    src      uint8 [F,H,W,3], [F,3,H,W] or [F,H,W] (masks) on the device; strides and layout as warp_frames reads them.
    field    int32 [F,gh,gw,2], 1/256 pixel, on track_field's grid for (H, W) and `cell`.
    flow     True (or a float32 tensor [F,H,W,2] to fill): also the per-pixel displacement in pixels.
    Returns out, or (out, flow) when a flow is asked for."""
    who = "warp_field"
    a, out, flow = _warp_field_args(src, None, cell, border, fill, out, flow, layout, 0, who)
    _warp_field_launch(a, field, who)
    return out if flow is None else (out, flow)


def propagate(picture: torch.Tensor, tracks: torch.Tensor, visible: torch.Tensor, *, src_frame: int, frames=None, cell: int = 16,
              radius: int = 2, border: str = "fill", fill=(0, 0, 0), scale=(1.0, 1.0), N_out: Optional[int] = None,
              first_row: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """A picture (or mask, or paint layer) given on frame src_frame carried onto other frames along the tracked points, on the device:
    track_field(to = src_frame) and warp_field -- four launches, no wait.  Works on any result of any predictor here.

    picture  uint8 [H,W,3], [3,H,W] or [H,W] on the device, in the pixels of tracks * scale.
    tracks   float32 [T,N,2] (or [1,T,N,2]); visible bool / uint8 [T,N].
    frames   (first_frame, n), or None: every tracked frame.
    Returns the pictures [n, ...] in the layout and dtype of `picture` (`out` when given)."""
    who = "propagate"
    if not (isinstance(picture, torch.Tensor) and picture.dtype == torch.uint8 and picture.is_cuda and picture.dim() in (2, 3)):
        raise ValueError(f"{who}: picture must be a uint8 device tensor [H,W,3], [3,H,W] or [H,W]")
    if not (isinstance(tracks, torch.Tensor) and tracks.dim() in (3, 4) and (tracks.dim() == 3 or tracks.shape[0] == 1)):
        raise ValueError(f"{who}: tracks must be a float32 device tensor [T,N,2] or [1,T,N,2]")
    T = tracks.shape[-3]
    first_frame, n = (0, T) if frames is None else (int(frames[0]), int(frames[1]))
    if n < 1:
        raise ValueError(f"{who}: frames = (first_frame, n) with n >= 1")
    src = picture[None].expand(n, *picture.shape)  # (a frame stride of 0: every output picture reads the one source)
    a, out, _ = _warp_field_args(src, None, cell, border, fill, out, None, None, 0, who)
    field = track_field(tracks, visible, size=(a.H, a.W), cell=cell, radius=radius, to=int(src_frame), scale=scale, N_out=N_out,
                        first_frame=first_frame, frames=n, first_row=first_row)[0]
    _warp_field_launch(a, field[0], who)
    return out


def dense_flow(tracks: torch.Tensor, visible: torch.Tensor, *, size, lag: int = 1, frames=None, cell: int = 16, radius: int = 2,
               scale=(1.0, 1.0), N_out: Optional[int] = None, first_row: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """A dense flow picture per frame interpolated from the tracked points, on the device: track_field(lag) and warp_field's flow --
    four launches, no wait.  flow[j, y, x] = the displacement in pixels from pixel (x, y) of frame f to its position on frame f - lag
    (a negative lag: forward flow).  size = (H, W); frames = (first_frame, n) or None: every frame.  Returns float32 [n,H,W,2]."""
    who = "dense_flow"
    if not (isinstance(tracks, torch.Tensor) and tracks.dim() in (3, 4) and (tracks.dim() == 3 or tracks.shape[0] == 1)):
        raise ValueError(f"{who}: tracks must be a float32 device tensor [T,N,2] or [1,T,N,2]")
    T = tracks.shape[-3]
    first_frame, n = (0, T) if frames is None else (int(frames[0]), int(frames[1]))
    field = track_field(tracks, visible, size=size, cell=cell, radius=radius, lag=lag, scale=scale, N_out=N_out, first_frame=first_frame,
                        frames=n, first_row=first_row)[0]
    a, _, flow = _warp_field_args(None, size, cell, "fill", (0, 0, 0), None, True if out is None else out, None, n, who, device=field.device)
    _warp_field_launch(a, field[0], who)
    return flow


# ------------------------------------------------------------------------------------------
# fit objects (csrc/objects.hip; include/ctk.h, "fit objects")
# ------------------------------------------------------------------------------------------
OBJECT_NONE = L.Objects.NONE


class ObjectSet:
    """Which points of a query set belong to which object, and the frame that was decided on: labels int8 [N] on the device (-1: no
    object's), the anchor (FieldAnchor) pinned on that frame, and the number of objects.  What split_objects() and label_objects()
    of the online predictor return and follow() takes."""
    __slots__ = ("labels", "anchor", "objects")

    def __init__(self, labels: torch.Tensor, anchor: FieldAnchor, objects: int):
        self.labels, self.anchor, self.objects = labels, anchor, int(objects)


def _objects_fit(src, labels, objects, lag, to, anchor, model, tol, hypotheses, min_base, min_points, seed):
    a, who = _FITS["objects"].args(), src.who
    objects = int(objects)
    if not 1 <= objects <= L.Objects.OBJECTS_MAX:
        raise ValueError(f"{who}: objects must lie in 1..{L.Objects.OBJECTS_MAX}")
    a.L, a.min_points, a.model = objects, _min_points_of(min_points, 1, who), _model_of(model, who)
    _sampling(a, hypotheses, seed, tol, min_base, who)
    _source_form(a, lag, to, anchor, src.G, src.N, src.device, who)
    a.labels = src.per_point_ptr(labels, _I8, "labels")
    src.bind(a, back=a.lag, to=a.to)  # (_source_form: the lag is >= 1, or 0 beside `to` and an anchor; never ahead)
    return _fit_launch("objects", a, None, src.device, who)


def fit_objects(tracks: torch.Tensor, visible: torch.Tensor, *, labels: Optional[torch.Tensor] = None, objects: int = 4, lag: int = 1,
                to: Optional[int] = None, anchor: Optional[FieldAnchor] = None, model: str = "similarity", tol: float = 2.0,
                hypotheses: int = 128, min_base: float = 16.0, min_points: int = 8, seed: int = 0, scale=(1, 1), frames=None,
                first_row: Optional[torch.Tensor] = None):
    """Which points move together, and how each such group has moved: up to `objects` robust fits per frame over sub-lists of the
    tracked points, by one launch and without a wait (ctk_fit_objects; include/ctk.h and csrc/objects_math.h have the rules).  Works on
    any result of any predictor here, offline ones included.

    tracks   float32 [T,N,2] or [G,T,N,2] (N <= 8192), positions = tracks * scale; visible bool / uint8 [T,N] or [G,T,N].
    source   the matrix of frame f maps a source frame onto f: f - lag (the default), a fixed frame `to`, or a FieldAnchor (positions
             kept from a frame the tracks no longer hold); `to` or `anchor` replaces the lag.  A point counts when it is visible on
             both frames (and at or above first_row: int [N] / [G,N], INT32_MAX: never).
    labels   int8 [N] / [G,N], labels mode: round r fits the points labelled r (anything outside 0..objects-1, -1 by convention:
             no round's), the rounds are independent.  None, split mode: round 0 fits all points, round r + 1 what round r's
             inliers left; a round with fewer than min_points inliers ends the rounds.  Split mode's round order is by size -- most
             inliers first -- per pair of frames and NOT stable from pair to pair: split once, then follow by labels.
    Each round is fit_motion's fit (model, tol, hypotheses, min_base) seeded with seed ^ mix(r).  Rows are the frames of
    frames = (first_frame, n); None: every tracked frame.  Returns (motion float32 [G,F,objects,2,3]: position on frame f = motion @
    (position on the source frame, 1), the identity where nothing was fitted; label int8 [G,F,N]: -1 not on both frames, r = inlier of
    round r, 127 (OBJECT_NONE) = no round took it; stats int32 [G,F,objects,4] = (points of the round, inliers, best hypothesis or -1,
    0); box int32 [G,F,objects,4] = (min x, min y, max x, max y) of the round's inliers on frame f in 1/16 pixel, (0, 0, -1, -1) where
    nothing was fitted)."""
    src = _TensorSource("fit_objects", tracks, visible, *_frame_pair(frames), first_row=first_row, scale=scale)
    return _objects_fit(src, labels, objects, lag, to, anchor, model, tol, hypotheses, min_base, min_points, seed)


# ------------------------------------------------------------------------------------------
# fit planes / warp planes (csrc/planes.hip, csrc/warp_planes.hip; include/ctk.h, "fit planes / warp planes")
# ------------------------------------------------------------------------------------------
PLANE_BORDERS = {"fill": L.Warp.BORDER_FILL, "edge": L.Warp.BORDER_EDGE, "keep": L.Planes.BORDER_KEEP}


def _planes_fit(src, labels, planes, lag, to, anchor, inverse, tol, hypotheses, min_base, min_points, seed):
    a, who = _FITS["planes"].args(), src.who
    planes = int(planes)
    if not 1 <= planes <= L.Planes.PLANES_MAX:
        raise ValueError(f"{who}: planes must lie in 1..{L.Planes.PLANES_MAX}")
    if labels is None and planes != 1:
        raise ValueError(f"{who}: without labels there is one list of all points: planes must be 1, got {planes}")
    a.L, a.min_points, a.inverse = planes, _min_points_of(min_points, 1, who), 1 if inverse else 0
    _sampling(a, hypotheses, seed, tol, min_base, who)
    _source_form(a, lag, to, anchor, src.G, src.N, src.device, who)
    a.labels = src.per_point_ptr(labels, _I8, "labels")
    src.bind(a, back=a.lag, to=a.to)
    return _fit_launch("planes", a, None, src.device, who)


def fit_planes(tracks: torch.Tensor, visible: torch.Tensor, *, labels: Optional[torch.Tensor] = None, planes: int = 1, lag: int = 1,
               to: Optional[int] = None, anchor: Optional[FieldAnchor] = None, inverse: bool = False, tol: float = 2.0,
               hypotheses: int = 128, min_base: float = 16.0, min_points: int = 8, seed: int = 0, scale=(1, 1), frames=None,
               first_row: Optional[torch.Tensor] = None):
    """How planar surfaces seen under perspective -- a screen, a wall, a sign, a pitch -- have moved: up to `planes` robust homography
    fits per frame over labelled sub-lists of the tracked points, by one launch and without a wait (ctk_fit_planes; include/ctk.h and
    csrc/plane_math.h have the rules).  Works on any result of any predictor here, offline ones included.

    tracks   float32 [T,N,2] or [G,T,N,2] (N <= 8192), positions = tracks * scale; visible bool / uint8 [T,N] or [G,T,N].
    source   the matrix of frame f maps a source frame onto f: f - lag (the default), a fixed frame `to`, or a FieldAnchor; `to` or
             `anchor` replaces the lag.  inverse=True: the matrix maps frame f onto the source frame instead (what a backward warp
             needs; fitted that way round, nothing is inverted).
    labels   int8 [N] / [G,N]: plane r is fitted to the points labelled r (anything outside 0..planes-1: no plane's), the planes are
             independent.  None: planes must be 1 and every point belongs to it.
    Each fit scores `hypotheses` seeded four-point samples with the bound `tol` (pixels, max norm; a sample needs triangles of twice
    the area min_base^2) and refits the best over its inliers; one with fewer than min_points inliers is no fit.  Rows are the frames
    of frames = (first_frame, n); None: every tracked frame.  Returns (homography float32 [G,F,planes,3,3]: (X, Y, Z) = H @ (x, y, 1),
    position = (X / Z, Y / Z), the identity where nothing was fitted; label int8 [G,F,N]: -1 not on both frames, r = inlier of plane r,
    127 = no plane took it; stats int32 [G,F,planes,4] = (points of the plane, inliers, best hypothesis or -1, 1 if the refit fell back
    to the best sample's own matrix); box int32 [G,F,planes,4] = (min x, min y, max x, max y) of the inliers on frame f in 1/16 pixel,
    (0, 0, -1, -1) where nothing was fitted)."""
    src = _TensorSource("fit_planes", tracks, visible, *_frame_pair(frames), first_row=first_row, scale=scale)
    return _planes_fit(src, labels, planes, lag, to, anchor, inverse, tol, hypotheses, min_base, min_points, seed)


def warp_planes(src: torch.Tensor, matrices: torch.Tensor, *, size=None, out: Optional[torch.Tensor] = None, border: str = "fill",
                fill=(0, 0, 0), layout: Optional[str] = None) -> torch.Tensor:
    """uint8 pictures resampled under one 3 x 3 matrix each, on the device, by one launch and without a wait (ctk_warp_planes;
    include/ctk.h and csrc/plane_math.h have the rules) -- what a caller otherwise writes as a projective grid, grid_sample and a
    torch.where composite.

    src      uint8 [F,Hs,Ws,3], [F,3,Hs,Ws] or [F,Hs,Ws] (masks) on the device, strides and layout as warp_field reads them; one picture
             ([1, ...], or expanded with a frame stride of 0) serves every matrix.
    matrices float32 [F,3,3] on the device: matrices[j] maps an OUTPUT pixel to a SOURCE position, (X, Y, Z) = m (x, y, 1), position =
             (X / Z, Y / Z), pixel centres at integers.  A pixel with Z <= 0, with a position beyond 2^20, or under a matrix that is not
             finite is outside.
    size     (H, W) of the output pictures (default: the source's); out: uint8 pictures [F,H,W,...] of the source's layout with
             strides of their own, which must not overlap the source.
    border   "fill": a tap outside the source has the value `fill`; "edge": the edge pixels go on for ever; an outside pixel takes
             `fill` under both.  "keep": a pixel that is outside or has a tap outside the source is NOT written -- the picture is
             drawn into `out` (required then), which may be the frames of a video themselves.
    Bilinear in 1/256 pixel: the identity on equal sizes copies bit for bit, an integer shift is a shifted copy.  Returns out."""
    who = "warp_planes"
    if border not in PLANE_BORDERS:
        raise ValueError(f"{who}: border must be one of {sorted(PLANE_BORDERS)}, got {border!r}")
    if not (isinstance(matrices, torch.Tensor) and matrices.is_cuda and matrices.dtype == torch.float32 and matrices.dim() == 3 and
            tuple(matrices.shape[1:]) == (3, 3) and matrices.shape[0] >= 1 and matrices.is_contiguous()):
        raise ValueError(f"{who}: matrices must be a contiguous float32 device tensor [F,3,3]")
    F_ = matrices.shape[0]
    if isinstance(src, torch.Tensor) and src.dim() in (3, 4) and src.shape[0] == 1 and F_ > 1:
        src = src.expand(F_, *src.shape[1:])
    C_, lay, Fs, Hs, Ws, row, frame = _field_surface(src, layout, who)
    if Fs != F_ or src.device != matrices.device:
        raise ValueError(f"{who}: {Fs} pictures on {src.device} for {F_} matrices on {matrices.device}")
    fill = [int(v) for v in ((fill,) * 3 if isinstance(fill, int) else fill)]
    if len(fill) != 3 or any(not 0 <= v <= 255 for v in fill):
        raise ValueError(f"{who}: fill must hold three values in 0..255 (or one)")
    H, W = (Hs, Ws) if size is None else (int(size[0]), int(size[1]))
    want = (F_, H, W) if src.dim() == 3 else ((F_, H, W, 3) if lay == "hwc" else (F_, 3, H, W))
    if out is None:
        if border == "keep":
            raise ValueError(f"{who}: border 'keep' draws into `out`: pass the pictures to draw into")
        if H < 1 or W < 1:
            raise ValueError(f"{who}: size = (H, W) must be positive")
        out = torch.empty(want, dtype=torch.uint8, device=src.device)
    elif not isinstance(out, torch.Tensor) or out.device != src.device or (size is not None and tuple(out.shape) != want) or out.dim() != src.dim():
        raise ValueError(f"{who}: out must be uint8 pictures {list(want)} on {src.device}")
    Co, olay, Fo, H, W, orow, oframe = _field_surface(out, lay if src.dim() == 4 else None, who)
    if (Co, olay, Fo) != (C_, lay, F_):
        raise ValueError(f"{who}: out must hold {F_} pictures in the layout of the source")
    a = L.Planes.WarpArgs()
    a.F, a.H, a.W, a.Hs, a.Ws, a.C, a.layout = F_, H, W, Hs, Ws, C_, (L.INGEST_HWC if lay == "hwc" else L.INGEST_CHW)
    a.border, a.reserved = PLANE_BORDERS[border], 0
    for k in range(3):
        a.fill[k] = fill[k]
    a.src_frame_stride, a.src_row_stride, a.dst_frame_stride, a.dst_row_stride = frame, row, oframe, orow
    a.matrices, a.src, a.dst = _ptr(matrices), _ptr(src), _ptr(out)
    L.check(L.load().ctk_warp_planes(C.byref(a), _stream()), "ctk_warp_planes")  # (overlapping src and out: refused there)
    return out


def quad_matrix(corners, size) -> torch.Tensor:
    """The float64 3 x 3 matrix [h22 = 1] that maps the pixels of an h x w picture (size = (h, w)) onto a quad: the picture's corner
    pixels (0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1) land on corners [4,2] = ((x, y), ...) in that order.  On the host, from host
    values only (a list, an array or a host tensor): nothing waits for the device."""
    who = "quad_matrix"
    if isinstance(corners, torch.Tensor) and corners.is_cuda:
        raise ValueError(f"{who}: corners must be host values [4,2] (a device tensor would have to be waited for)")
    c = torch.as_tensor(corners, dtype=torch.float64).reshape(-1)
    h, w = int(size[0]), int(size[1])
    if c.numel() != 8 or not bool(torch.isfinite(c).all()) or h < 2 or w < 2:
        raise ValueError(f"{who}: corners must hold four finite points [4,2] and size = (h, w) at least (2, 2)")
    c = c.reshape(4, 2)
    src = torch.tensor([[0.0, 0.0], [w - 1.0, 0.0], [w - 1.0, h - 1.0], [0.0, h - 1.0]], dtype=torch.float64)
    A, b = torch.zeros(8, 8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)
    for k in range(4):
        (x, y), (X, Y) = src[k].tolist(), c[k].tolist()
        A[2 * k] = torch.tensor([x, y, 1.0, 0.0, 0.0, 0.0, -x * X, -y * X], dtype=torch.float64)
        A[2 * k + 1] = torch.tensor([0.0, 0.0, 0.0, x, y, 1.0, -x * Y, -y * Y], dtype=torch.float64)
        b[2 * k], b[2 * k + 1] = X, Y
    pts = c.tolist()
    flat = any((pts[j][0] - pts[i][0]) * (pts[k][1] - pts[i][1]) - (pts[j][1] - pts[i][1]) * (pts[k][0] - pts[i][0]) == 0.0
               for i, j, k in ((1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2)))
    try:
        sol = None if flat else torch.linalg.solve(A, b)
    except RuntimeError:
        sol = None
    if sol is None or not bool(torch.isfinite(sol).all()):
        raise ValueError(f"{who}: the corners do not span a quad (three of them lie on a line)")
    return torch.cat([sol, torch.ones(1, dtype=torch.float64)]).reshape(3, 3)


_quad_cache = {}
_QUAD_CACHE_MAX = 64


def quad_constant(corners, size, device, *, inverse: bool) -> torch.Tensor:
    """quad_matrix(corners, size) -- inverse=True: its inverse -- as a float64 [3,3] constant on `device`, for plane_matrices.  Kept per
    (corners, size, inverse, device), like the `post` matrix StreamGroups.stabilize keeps: a picture that stays pinned to the same quad
    costs the 8 x 8 host solve, the inverse and the upload once, not per call.  A new quad goes up through pinned memory with a
    non-blocking copy: the host never waits for what is queued on the stream.  The last 64 quads are kept."""
    if isinstance(corners, torch.Tensor) and corners.is_cuda:
        raise ValueError("quad_constant: corners must be host values [4,2] (a device tensor would have to be waited for)")
    flat = torch.as_tensor(corners, dtype=torch.float64).reshape(-1).tolist()
    device = torch.device(device)
    key = (tuple(flat), int(size[0]), int(size[1]), bool(inverse), device.type, device.index if device.index is not None else torch.cuda.current_device())
    q = _quad_cache.get(key)
    if q is None:
        host = quad_matrix(corners, size)
        host = torch.linalg.inv(host) if inverse else host
        q = host.contiguous().pin_memory().to(device, non_blocking=True)
        while len(_quad_cache) >= _QUAD_CACHE_MAX:
            _quad_cache.pop(next(iter(_quad_cache)))
        _quad_cache[key] = q
    return q


def plane_matrices(homography: torch.Tensor, stats: torch.Tensor, quad: torch.Tensor, *, inverse: bool) -> torch.Tensor:
    """The matrices warp_planes wants from one plane's fits: homography float32 [F,3,3] and stats int32 [F,4] of fit_planes, and the
    quad of the picture on the source frame: `quad` is quad_constant(..., inverse=inverse) on the device -- the cached constant, used as
    it is --, or the host float64 quad_matrix, which is inverted here when `inverse` and goes up through pinned memory with a
    non-blocking copy.  inverse=True (the fits were made with inverse=True): a frame's pixel -> the picture's pixel, inverse(quad) @ H,
    and the zero matrix -- every pixel outside -- on a frame without a fit.  inverse=False: an upright picture's pixel -> the frame's
    pixel, H @ quad.  One small float64 matmul and a where on the device; the host waits for nothing."""
    if not (isinstance(quad, torch.Tensor) and quad.dtype == torch.float64 and tuple(quad.shape) == (3, 3)):
        raise ValueError("plane_matrices: quad must be a float64 [3,3] tensor (quad_constant, or quad_matrix)")
    if quad.is_cuda:
        q = quad
    else:
        q = (torch.linalg.inv(quad) if inverse else quad).contiguous().pin_memory().to(homography.device, non_blocking=True)
    h = homography.to(torch.float64)
    m = torch.matmul(q, h) if inverse else torch.matmul(h, q)
    if inverse:
        m = torch.where((stats[:, 1] > 0)[:, None, None], m, torch.zeros_like(m))
    return m.to(torch.float32).contiguous()


def _plane_of(tracks, who: str):
    if not (isinstance(tracks, torch.Tensor) and tracks.dim() in (3, 4) and (tracks.dim() == 3 or tracks.shape[0] == 1)):
        raise ValueError(f"{who}: tracks must be a float32 device tensor [T,N,2] or [1,T,N,2]")


def overlay(frames: torch.Tensor, picture: torch.Tensor, corners, tracks: torch.Tensor, visible: torch.Tensor, *, src_frame: int,
            first_frame: int = 0, labels: Optional[torch.Tensor] = None, planes: int = 1, index: int = 0, layout: Optional[str] = None,
            **fit) -> torch.Tensor:
    """A picture pinned onto a planar surface so that it stays put, drawn IN PLACE onto uint8 frames on the device: fit_planes(to =
    src_frame, inverse=True), plane_matrices with the cached quad_constant, warp_planes(border="keep") -- two launches plus elementwise
    torch, no wait.  Works on any
    result of any predictor here.

    frames   uint8 [F,H,W,3] or [F,3,H,W] on the device: picture j shows frame first_frame + j of the tracks.
    picture  uint8 [h,w,3] (or [3,h,w] for planar frames) on the device; its corner pixels sit at corners [4,2] (host values, the
             order of quad_matrix) on frame src_frame, in the pixels of tracks * scale.
    labels, planes, index   the plane that carries the picture: the points labelled `index` (None: all points); **fit: fit_planes'
             scale, tol, hypotheses, min_base, min_points, seed, first_row.
    A frame without a fit gets nothing.  No alpha blending and no anti-aliased edge.  Returns frames."""
    who = "overlay"
    _plane_of(tracks, who)
    if not (isinstance(frames, torch.Tensor) and frames.dim() == 4 and isinstance(picture, torch.Tensor) and picture.dim() == 3):
        raise ValueError(f"{who}: frames must be uint8 [F,H,W,3] or [F,3,H,W] and picture [h,w,3] or [3,h,w] on the device")
    lay = _draw_surface(frames, layout, who)[0]
    size = tuple(picture.shape[:2]) if lay == "hwc" else tuple(picture.shape[1:])
    quad = quad_constant(corners, size, frames.device, inverse=True)
    hom, _, stats, _ = fit_planes(tracks, visible, labels=labels, planes=planes, to=int(src_frame), inverse=True,
                                  frames=(int(first_frame), frames.shape[0]), **fit)
    m = plane_matrices(hom[0, :, int(index)], stats[0, :, int(index)], quad, inverse=True)
    return warp_planes(picture[None], m, out=frames, border="keep", layout=lay)


def rectify(frames: torch.Tensor, corners, tracks: torch.Tensor, visible: torch.Tensor, *, src_frame: int, size, first_frame: int = 0,
            labels: Optional[torch.Tensor] = None, planes: int = 1, index: int = 0, border: str = "fill", fill=(0, 0, 0),
            out: Optional[torch.Tensor] = None, layout: Optional[str] = None, **fit) -> torch.Tensor:
    """A planar surface shown upright: the quad whose corners sit at corners [4,2] on frame src_frame, resampled from every frame into
    an h x w picture (size = (h, w)) through the forward matrices -- fit_planes(to = src_frame), plane_matrices, warp_planes: two
    launches plus elementwise torch, no wait.  The arguments are overlay()'s; border, fill and out are warp_planes'.  A frame without a
    fit shows the quad where it was on frame src_frame.  Returns the pictures [F,h,w,3] (or [F,3,h,w])."""
    who = "rectify"
    _plane_of(tracks, who)
    if not (isinstance(frames, torch.Tensor) and frames.dim() == 4):
        raise ValueError(f"{who}: frames must be a uint8 device tensor [F,H,W,3] or [F,3,H,W]")
    lay = _draw_surface(frames, layout, who)[0]
    quad = quad_constant(corners, size, frames.device, inverse=False)
    hom, _, stats, _ = fit_planes(tracks, visible, labels=labels, planes=planes, to=int(src_frame), inverse=False,
                                  frames=(int(first_frame), frames.shape[0]), **fit)
    m = plane_matrices(hom[0, :, int(index)], stats[0, :, int(index)], quad, inverse=False)
    return warp_planes(frames, m, size=size, out=out, border=border, fill=fill, layout=lay)


def normalize_to_nhwc(fmaps_nchw: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[F,128,H,W] -> channel-L2-normalised NHWC [F,H,W,128] (cotracker3_online.py:384-394); `out` = a contiguous
    [F,H,W,128] destination (e.g. a frame range of a preallocated feature tensor)."""
    _chk_f32(fmaps_nchw)
    F_, Cc, H, W = fmaps_nchw.shape
    assert Cc == 128
    if out is None:
        out = torch.empty(F_, H, W, Cc, device=fmaps_nchw.device, dtype=torch.float32)
    else:
        _chk_f32(out)
        assert out.shape == (F_, H, W, Cc)
    L.check(L.load().ctk_normalize_to_nhwc(_ptr(fmaps_nchw), F_, H, W, _ptr(out), _stream()), "ctk_normalize_to_nhwc")
    return out


def avg_pool2_nhwc(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk_f32(x, out)
    F_, H, W, Cc = x.shape
    if out is None:
        out = torch.empty(F_, H // 2, W // 2, Cc, device=x.device, dtype=torch.float32)
    assert out.shape == (F_, H // 2, W // 2, Cc)
    L.check(L.load().ctk_avg_pool2_nhwc(_ptr(x), F_, H, W, _ptr(out), _stream()), "ctk_avg_pool2_nhwc")
    return out


def build_pyramid(level0_nhwc: torch.Tensor, levels: int = L.LEVELS) -> List[torch.Tensor]:
    pyr = [level0_nhwc]
    for _ in range(levels - 1):
        pyr.append(avg_pool2_nhwc(pyr[-1]))
    return pyr


def sample_support(fmap_nhwc: torch.Tensor, frames: torch.Tensor, coords: torch.Tensor) -> torch.Tensor:
    """get_track_feat (cotracker3_online.py:113-128): fmap [T,H,W,128], frames [N] float, coords [N,2] -> [N,49,128]."""
    _chk_f32(fmap_nhwc, frames, coords)
    T, H, W, _ = fmap_nhwc.shape
    N = coords.shape[0]
    out = torch.empty(N, 49, 128, device=coords.device, dtype=torch.float32)
    L.check(L.load().ctk_sample_support(_ptr(fmap_nhwc), T, H, W, _ptr(frames), _ptr(coords), N, _ptr(out), _stream()),
            "ctk_sample_support")
    return out


def sample_patches(fmap_nhwc: torch.Tensor, coords: torch.Tensor, level: int) -> torch.Tensor:
    """get_correlation_feat (cotracker3_online.py:130-143): fmap [S,H,W,128], coords [S,N,2] level-0 -> [S,N,49,128]."""
    _chk_f32(fmap_nhwc, coords)
    S, H, W, _ = fmap_nhwc.shape
    N = coords.shape[1]
    out = torch.empty(S, N, 49, 128, device=coords.device, dtype=torch.float32)
    L.check(L.load().ctk_sample_patches(_ptr(fmap_nhwc), S, H, W, _ptr(coords), N, level, _ptr(out), _stream()),
            "ctk_sample_patches")
    return out


def corrblock_sample(pyr_nhwc: Sequence[torch.Tensor], targets: torch.Tensor, coords: torch.Tensor) -> torch.Tensor:
    """CorrBlock.corr + .sample fused (blocks.py:309-362): pyr_nhwc 4 x [S,H_l,W_l,128], targets [S,N,128],
    coords [S,N,2] (level-0 units) -> [N,S,196].  The correlation volume is never materialised."""
    _chk_f32(*pyr_nhwc, targets, coords)
    assert len(pyr_nhwc) == L.LEVELS
    S, N = coords.shape[0], coords.shape[1]
    assert targets.shape == (S, N, 128) and coords.shape == (S, N, 2)
    fm = (C.c_void_p * L.LEVELS)(*[_ptr(f) for f in pyr_nhwc])
    Hs = (C.c_int32 * L.LEVELS)(*[f.shape[1] for f in pyr_nhwc])
    Ws = (C.c_int32 * L.LEVELS)(*[f.shape[2] for f in pyr_nhwc])
    for f in pyr_nhwc:
        assert f.shape[0] == S and f.shape[3] == 128
    out = torch.empty(N, S, L.LEVELS * 49, device=coords.device, dtype=torch.float32)
    L.check(L.load().ctk_corrblock_sample(fm, Hs, Ws, S, N, _ptr(targets), _ptr(coords), _ptr(out), _stream()),
            "ctk_corrblock_sample")
    return out


# ------------------------------------------------------------------------------------------
# fit epipolar (csrc/epipolar.hip; include/ctk.h, "fit epipolar")
# ------------------------------------------------------------------------------------------
def _epipolar_fit(src, mask, lag, to, anchor, tol, hypotheses, min_base, min_points, seed, out):
    a, who = _FITS["epipolar"].args(), src.who
    a.min_points = _min_points_of(min_points, L.Epipolar.MIN_POINTS, who)
    _sampling(a, hypotheses, seed, tol, min_base, who)
    _source_form(a, lag, to, anchor, src.G, src.N, src.device, who)
    a.mask = src.per_point_ptr(mask, _BYTES, "mask")
    src.bind(a, back=a.lag, to=a.to)
    return _fit_launch("epipolar", a, out, src.device, who)


def fit_epipolar(tracks: torch.Tensor, visible: torch.Tensor, *, mask: Optional[torch.Tensor] = None, lag: int = 1, to: Optional[int] = None,
                 anchor: Optional[FieldAnchor] = None, tol: float = 1.0, hypotheses: int = 512, min_base: float = 16.0, min_points: int = 16,
                 seed: int = 0, first_row: Optional[torch.Tensor] = None, scale=(1, 1), out=None):
    """Which points are consistent with ONE camera moving through a scene with depth, and which move by themselves: per frame a robust
    fundamental matrix fitted to the correspondences between a source frame and the frame, by one launch and without a wait
    (ctk_fit_epipolar; include/ctk.h and csrc/epipolar_math.h have the rules).  Where fit_motion and fit_planes call the nearer half
    of a static scene outliers under a translating camera, a static point obeys (X, Y, 1) F (x, y, 1)^T = 0 at any depth.  Works on any
    result of any predictor here, offline ones included.

    tracks   float32 [T,N,2] or [G,T,N,2] (N <= 8192), positions = tracks * scale; visible bool / uint8 [T,N] or [G,T,N].
    source   (x, y) is on a source frame and (X, Y) on frame f: f - lag (the default), a fixed frame `to`, or a FieldAnchor; `to` or
             `anchor` replaces the lag.  A point counts when it is visible on both frames (and at or above first_row: int [N] / [G,N]).
    mask     int8 / uint8 / bool [N] / [G,N]: nonzero = the point may be sampled and refitted on (say, what is known to be background);
             None: every point may.  Every point, masked or not, is classified and gets an error.
    The fit scores `hypotheses` seeded eight-point samples with the Sampson bound `tol` (pixels; every sample point lies at least
    min_base pixels from the first), refits the best over its inliers and once more over the inliers of that; a best sample with fewer
    than min_points (>= 8) inliers is no fit.  Rows are all T frames.  Returns (fundamental float32 [G,T,3,3] in pixels, all zero where
    nothing was fitted; label int8 [G,T,N]: -1 not on both frames, 0 violates the matrix (or nothing was fitted), 1 consistent with it;
    error float32 [G,T,N]: the squared Sampson distance in pixels^2, -1 without a correspondence or a fit; stats int32 [G,T,4] = (points
    that may be fitted on, inliers among them, best hypothesis or -1, bit 0 / 1: the first / second refit fell back)); `out`: such a
    tuple to write into.  F is not unique without parallax (a plane, a camera that only turns or stands): the labels then still mean
    "consistent with some camera motion"; a point that moves along its own epipolar line is not seen."""
    src = _TensorSource("fit_epipolar", tracks, visible, first_row=first_row, scale=scale)
    return _epipolar_fit(src, mask, lag, to, anchor, tol, hypotheses, min_base, min_points, seed, out)


# ------------------------------------------------------------------------------------------
# fit pose (csrc/pose.hip; include/ctk.h, "fit pose")
# ------------------------------------------------------------------------------------------
def _pose_fit(src, intrinsics, fundamental, label, mask, lag, to, anchor, min_points, out):
    a, who, dev = _FITS["pose"].args(), src.who, src.device
    a.min_points, a.reserved = _min_points_of(min_points, L.Pose.MIN_POINTS, who), 0
    _intrinsics(a, intrinsics, who)
    _source_form(a, lag, to, anchor, src.G, src.N, dev, who)
    a.fundamental = _tensor_ptr(fundamental, _F32, (src.G, src.F, 3, 3), "fundamental", dev, who, " (fit_epipolar's)")
    a.label = _tensor_ptr(label, _I8, (src.G, src.F, src.N_out), "label", dev, who, " (fit_epipolar's)")
    a.mask = src.per_point_ptr(mask, _BYTES, "mask")
    src.bind(a, back=a.lag, to=a.to)
    return _fit_launch("pose", a, out, dev, who)


def fit_pose(tracks: torch.Tensor, visible: torch.Tensor, intrinsics, fundamental: torch.Tensor, label: torch.Tensor, *,
             mask: Optional[torch.Tensor] = None, lag: int = 1, to: Optional[int] = None, anchor: Optional[FieldAnchor] = None,
             min_points: int = 8, first_row: Optional[torch.Tensor] = None, scale=(1, 1), out=None):
    """How the camera turned, in which direction it moved, and how deep every tracked point is: per frame the fundamental matrix and
    the labels of fit_epipolar become a pose and two depths per point, by one launch and without a wait (ctk_fit_pose; include/ctk.h
    and csrc/pose_math.h have the rules).  Works on any result of any predictor here, offline ones included.

    tracks, visible, lag / to / anchor, first_row, scale   what fit_epipolar was called with: they decide what a correspondence is.
    intrinsics   (fx, fy, cx, cy), four Python floats: one pinhole camera in the pixels of tracks * scale, the same on both frames.
    fundamental, label   float32 [G,T,3,3] and int8 [G,T,N] as fit_epipolar returned them; they are only read.
    mask     int8 / uint8 / bool [N] / [G,N]: nonzero = the point may be fitted on if its label is 1; None: every point labelled 1.
    The pose maps source-camera coordinates to the frame's, X_f = R X_s + t with |t| = 1: a closed-form decomposition of E = K^T F K,
    the candidate that puts most of the fit list in front of both cameras, two Gauss-Newton rounds on the Sampson error.  Rows are all T
    frames.  Returns (pose float32 [G,T,3,4] = (R | t), (I | 0) where there is no fit; depth float32 [G,T,N,2] = (depth on the source
    frame, depth on the frame) in units of the baseline, NaN without a correspondence or a fit -- a point that moves by itself gets a
    depth that means nothing, and `label` says so; stats int32 [G,T,4] = (points fitted on, those of them in front of both cameras,
    the chosen candidate or -1, bit 0 / 1: the first / second round fell back, bit 2: an entry was left out of a round)); `out`: such a
    tuple to write into.  A fit needs min_points (>= 8) points labelled 1.  The scale is unknown and changes from frame to frame; no
    parallax (a camera that only turns or stands, a plane) means no pose: look at stats[..., 1] / stats[..., 0]."""
    src = _TensorSource("fit_pose", tracks, visible, first_row=first_row, scale=scale)
    return _pose_fit(src, intrinsics, fundamental, label, mask, lag, to, anchor, min_points, out)


# ------------------------------------------------------------------------------------------
# fit focal (csrc/focal.hip; include/ctk.h, "fit focal")
# ------------------------------------------------------------------------------------------
_focal_cache = {}
_FOCAL_CACHE_MAX = 64


def focal_candidates(size, device, *, candidates: int = 64, span=(0.25, 4.0)) -> torch.Tensor:
    """The default candidates of fit_focal as a float32 [candidates] constant on `device`: geometric over span * W of size = (H, W),
    lo * (hi / lo)^(k / (K - 1)) in Python floats (one candidate: the geometric mean).  Kept per (span, K, W, device) as quad_constant
    keeps its quads: computed and uploaded once, through pinned memory with a non-blocking copy."""
    K, W = int(candidates), float(size[1])
    lo, hi = float(span[0]) * W, float(span[1]) * W
    if not 1 <= K <= L.Focal.K_MAX:
        raise ValueError(f"fit_focal: candidates must lie in 1..{L.Focal.K_MAX}")
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= hi <= 3.0e38):
        raise ValueError("fit_focal: span = (lo, hi) in picture widths with 0 < lo <= hi, and size = (H, W) with W > 0")
    device = torch.device(device)
    key = (lo, hi, K, device.type, device.index if device.index is not None else torch.cuda.current_device())
    q = _focal_cache.get(key)
    if q is None:
        host = [(lo * hi) ** 0.5] if K == 1 else [lo * (hi / lo) ** (k / (K - 1)) for k in range(K)]
        q = torch.tensor(host, dtype=torch.float32).pin_memory().to(device, non_blocking=True)
        while len(_focal_cache) >= _FOCAL_CACHE_MAX:
            _focal_cache.pop(next(iter(_focal_cache)))
        _focal_cache[key] = q
    return q


def _focal_list(focals, size, candidates, span, device, who: str) -> torch.Tensor:
    """focals: None (the cached default of `size`), a device tensor (taken as it is) or host numbers (checked) -> float32 [K] on device."""
    if focals is None:
        if size is None:
            raise ValueError(f"{who}: give size = (H, W) of the picture for the default candidates, or focals")
        return focal_candidates(size, device, candidates=candidates, span=span)
    if isinstance(focals, torch.Tensor) and focals.is_cuda:
        if not (focals.dtype == torch.float32 and focals.dim() == 1 and 1 <= focals.numel() <= L.Focal.K_MAX and focals.is_contiguous() and
                focals.device == device):
            raise ValueError(f"{who}: focals on the device must be a contiguous float32 tensor [K], K in 1..{L.Focal.K_MAX}, on {device}")
        return focals
    host = [float(v) for v in (focals.tolist() if isinstance(focals, torch.Tensor) else focals)]
    if not 1 <= len(host) <= L.Focal.K_MAX or any(not (math.isfinite(v) and 0.0 < v <= 3.0e38) for v in host) or \
            any(b <= a for a, b in zip(host, host[1:])):
        raise ValueError(f"{who}: focals must be 1..{L.Focal.K_MAX} finite numbers > 0 in ascending order (raw-video pixels)")
    return torch.tensor(host, dtype=torch.float32).pin_memory().to(device, non_blocking=True)


def _focal_fit(src, fundamental, label, focals, size, candidates, span, principal, mask, lag, to, anchor, tol, min_points, min_frames,
               contrast, curve, out):
    a, who, dev = _FITS["focal"].args(), src.who, src.device
    a.min_points, a.reserved = _min_points_of(min_points, L.Pose.MIN_POINTS, who), 0
    focals = _focal_list(focals, size, candidates, span, dev, who)
    a.focals, a.K = focals.data_ptr(), focals.numel()
    if principal is None:
        if size is None:
            raise ValueError(f"{who}: give principal = (cx, cy), or size = (H, W) for the picture centre")
        principal = ((float(size[1]) - 1.0) * 0.5, (float(size[0]) - 1.0) * 0.5)
    cx, cy = (float(v) for v in principal)
    if not (math.isfinite(cx) and math.isfinite(cy)):
        raise ValueError(f"{who}: principal = (cx, cy) must be two finite numbers (raw-video pixels)")
    a.cx, a.cy, a.tol = cx, cy, _positive_tol(tol, who)
    a.min_frames, a.contrast = int(min_frames), float(contrast)
    if a.min_frames < 1 or not (math.isfinite(a.contrast) and a.contrast >= 1.0):
        raise ValueError(f"{who}: min_frames must be >= 1 and contrast finite and >= 1")
    _source_form(a, lag, to, anchor, src.G, src.N, dev, who)
    if src.F > L.Focal.FRAMES_MAX:
        raise ValueError(f"{who}: at most {L.Focal.FRAMES_MAX} frames a call (accumulate through curve=)")
    a.fundamental = _tensor_ptr(fundamental, _F32, (src.G, src.F, 3, 3), "fundamental", dev, who, " (fit_epipolar's)")
    a.label = _tensor_ptr(label, _I8, (src.G, src.F, src.N_out), "label", dev, who, " (fit_epipolar's)")
    a.mask = src.per_point_ptr(mask, _BYTES, "mask")
    a.curve_in = None if curve is None else _tensor_ptr(curve, (torch.int64,), (src.G, a.K + 2), "curve", dev, who,
                                                        " (an earlier call's, same focals)")
    src.bind(a, back=a.lag, to=a.to)
    return _fit_launch("focal", a, out, dev, who) + (focals,)


def fit_focal(tracks: torch.Tensor, visible: torch.Tensor, fundamental: torch.Tensor, label: torch.Tensor, *, focals=None, size=None,
              candidates: int = 64, span=(0.25, 4.0), principal=None, mask: Optional[torch.Tensor] = None, lag: int = 1,
              to: Optional[int] = None, anchor: Optional[FieldAnchor] = None, tol: float = 1.0, min_points: int = 16, min_frames: int = 1,
              contrast: float = 1.5, curve: Optional[torch.Tensor] = None, first_row: Optional[torch.Tensor] = None, scale=(1, 1), out=None):
    """The focal length the camera had, read off the tracks: the one of four intrinsics that fit_pose and everything behind it want and
    a caller with a phone clip does not know.  K candidate focal lengths are swept through fit_pose's rules over the matrices and
    labels of fit_epipolar; each (frame, candidate) gets an integer cost -- the squared Sampson distance in pixels under the
    candidate's best rigid pose, truncated at tol^2, summed over the points labelled 1 --; the costs are summed over the frames, and
    the candidate with the smallest total is refined by a parabola through its neighbours.  Two launches, no wait (ctk_fit_focal;
    include/ctk.h and csrc/focal_math.h have the rules).  Works on any result of any predictor here, offline ones included.

    tracks, visible, lag / to / anchor, first_row, scale, mask   what fit_epipolar and fit_pose take: they decide the fit list.
    fundamental, label   float32 [G,T,3,3] and int8 [G,T,N] as fit_epipolar returned them; they are only read.
    focals    None: `candidates` (1..256) focal lengths geometric over span * W of size = (H, W), cached on the device; a list of
              ascending finite numbers > 0 (raw-video pixels); or a float32 device tensor [K], taken as it is.
    principal (cx, cy) in raw-video pixels; None: the centre ((W - 1) / 2, (H - 1) / 2) of `size`.  It is assumed, not estimated.
    curve     the `curve` an earlier call returned for the same focals: the new curve is the running sum, so evidence accumulates over
              calls -- more frames, other videos of the same camera -- without a wait; two calls accumulated equal one over both.
    A frame takes part with min_points (>= 8) points labelled 1 and a usable matrix; a fit needs min_frames such frames (earlier
    calls' included) and a curve whose largest total is at least `contrast` times its smallest -- a camera that does not TURN between
    the two frames of a pair leaves the curve flat (F does not depend on the focal length then) and is refused.  Rows are all T
    frames.  Returns (focal float32 [G], 0 where there is no fit; curve int64 [G,K+2]: the totals, then the frames and entries
    counted; cost int64 [G,T,K], in units of 2^-32 tol^2; stats int32 [G,4] = (frames counted, the chosen candidate or -1, entries
    counted, bit 0: the minimum lies at an end of the range, bit 1: the curve is flat, bit 2: a candidate is not finite and > 0);
    focals float32 [K]); `out`: a tuple of the first four to write into.  Known limits: square pixels, an assumed principal point, a
    camera that must turn, one fixed focal length per accumulation (no zoom), no distortion estimate."""
    src = _TensorSource("fit_focal", tracks, visible, first_row=first_row, scale=scale)
    return _focal_fit(src, fundamental, label, focals, size, candidates, span, principal, mask, lag, to, anchor, tol, min_points,
                      min_frames, contrast, curve, out)


# ------------------------------------------------------------------------------------------
# fit resection (csrc/resection.hip; include/ctk.h, "fit resection")
# ------------------------------------------------------------------------------------------
class _StructureOrigin:
    """The fifth field of Structure, in a slot of its own so that Structure.__slots__ stays the four names its callers unpack."""
    __slots__ = ("origin",)


class Structure(_StructureOrigin):
    """The static points of a query set in 3-D, and the frame whose camera they are stated in: points float32 [N,3] on the device in
    that camera's coordinates and in the baseline of the pair they were reconstructed from as the unit, valid int8 [N] (nonzero: the
    point is in the structure), the anchor (FieldAnchor) pinned on that frame, and the intrinsics (fx, fy, cx, cy) they were made
    with.  What reconstruct() of the online predictor returns and localize() takes.  origin: float32 [3,4] on the device, the pose of
    this structure's camera against the camera of the first structure it was extended from (extend() of the online predictor), or
    None: the identity; compose_pose(pose, origin) states a pose against this structure in that first camera's coordinates."""
    __slots__ = ("points", "valid", "anchor", "intrinsics")

    def __init__(self, points: torch.Tensor, valid: torch.Tensor, anchor: FieldAnchor, intrinsics, origin: Optional[torch.Tensor] = None):
        self.points, self.valid, self.anchor, self.intrinsics = points, valid, anchor, tuple(float(v) for v in intrinsics)
        self.origin = origin


def compose_pose(pose: torch.Tensor, origin: Optional[torch.Tensor]) -> torch.Tensor:
    """A pose [...,3,4] = (R | t) against a structure whose camera stands at origin [...,3,4] = (R_o | t_o) against a first camera ->
    the pose against that first camera, (R R_o | R t_o + t) (elementwise torch, no wait).  origin None: the pose itself."""
    if origin is None:
        return pose
    R, t = pose[..., :3], pose[..., 3:]
    return torch.cat([R @ origin[..., :3], R @ origin[..., 3:] + t], dim=-1)


def structure_from_pose(tracks_row: torch.Tensor, intrinsics, depth: torch.Tensor, label: torch.Tensor, *, max_depth: float = 64.0,
                        scale=(1, 1)):
    """The 3-D points that one pair of frames gives, from what fit_pose and fit_epipolar returned for it (elementwise torch, no wait):
    tracks_row float32 [...,N,2] = the positions on the LATER frame of the pair, depth float32 [...,N,2] and label int8 [...,N] of that
    frame's row.  X = z * ray with the depth z on the later frame and ray = ((x * sx - cx) / fx, (y * sy - cy) / fy, 1): camera
    coordinates of the later frame, in baselines of the pair.  A point is valid when it is labelled 1, both its depths are finite and
    > 0, and z <= max_depth baselines (a parameter, not a measured optimum: far points carry no parallax, their depth is mostly noise).
    -> (points float32 [...,N,3], zero where not valid; valid int8 [...,N])."""
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    zs, zf = depth[..., 0], depth[..., 1]
    rx, ry = (tracks_row[..., 0] * float(scale[0]) - cx) / fx, (tracks_row[..., 1] * float(scale[1]) - cy) / fy
    ok = (label == 1) & torch.isfinite(zs) & torch.isfinite(zf) & (zs > 0) & (zf > 0) & (zf <= float(max_depth))
    pts = torch.stack([rx * zf, ry * zf, zf], dim=-1)
    return torch.where(ok[..., None], pts, torch.zeros_like(pts)), ok.to(torch.int8)


def _resection_fit(src, intrinsics, structure, valid, seed_pose, lag, to, anchor, tol, hypotheses, min_points, seed, out, kind="resection"):
    """The body of fit_resection and, as kind "p3p", of fit_p3p: the same args, rules and source; ctk_fit_p3p takes no seed_pose."""
    a, who, dev = _FITS[kind].args(), src.who, src.device
    a.min_points = _min_points_of(min_points, L.Resection.MIN_POINTS, who)
    _sampling(a, hypotheses, seed, tol, None, who, resection=True)
    _intrinsics(a, intrinsics, who)
    _source_form(a, lag, to, anchor, src.G, src.N, dev, who)
    a.structure = _tensor_ptr(structure, _F32, (src.G, src.N, 3), "structure", dev, who)
    a.valid = _tensor_ptr(valid, _BYTES, (src.G, src.N), "valid", dev, who)
    if kind == "resection":
        a.seed_pose = _tensor_ptr(seed_pose, _F32, (src.G, src.F, 3, 4), "seed_pose", dev, who, " (fit_pose's)")
    src.bind(a, back=a.lag, to=a.to)
    return _fit_launch(kind, a, out, dev, who)


def fit_resection(tracks: torch.Tensor, visible: torch.Tensor, intrinsics, structure: torch.Tensor, valid: torch.Tensor,
                  seed_pose: torch.Tensor, *, lag: int = 1, to: Optional[int] = None, anchor: Optional[FieldAnchor] = None,
                  tol: float = 2.0, hypotheses: int = 256, min_points: int = 16, seed: int = 0,
                  first_row: Optional[torch.Tensor] = None, scale=(1, 1), out=None):
    """Where the camera is on every frame, in ONE unit and ONE coordinate system: per frame the camera's pose against 3-D points that
    are known in the source camera's coordinates (a structure: structure_from_pose on one pair of frames), by one launch and without
    a wait (ctk_fit_resection; include/ctk.h and csrc/resection_math.h have the rules).  Works on any result of any predictor here,
    offline ones included.

    tracks, visible, lag / to / anchor, first_row, scale   as in fit_pose: they decide what a correspondence is; the source frame
             (usually a fixed `to` or an anchor) is the frame whose camera the structure is stated in.
    intrinsics   (fx, fy, cx, cy), four Python floats: one pinhole camera in the pixels of tracks * scale.
    structure, valid   float32 [G,N,3] / [N,3] and int8 / uint8 / bool [G,N] / [N]: the points and which of them count; only read.
    seed_pose    float32 [G,T,3,4] / [T,3,4]: a pose per frame to start from, fit_pose's for the same source (its |t| = 1 is rescaled
             against the structure) or the poses of an earlier call; a row that is not finite counts as (I | 0); only read.
    Every candidate keeps the seed's rotation (or the identity) and differs in one scale of its translation; the one with most points
    within tol pixels of their reprojection wins and is refined by three Gauss-Newton rounds on the reprojection error.  Rows are all
    T frames.  Returns (pose float32 [G,T,3,4] = (R | t) with X_f = R X_source + t in the structure's unit, (I | 0) where there is
    no fit; label int8 [G,T,N]: -1 no correspondence or not in the structure, 0 outside tol, behind the camera or no fit, 1 within
    tol; error float32 [G,T,N]: the squared reprojection error in px^2, -1 where the label is -1 or there is no fit; stats int32
    [G,T,4] = (points fitted on, points labelled 1, the winning candidate or -1, bits 0 / 1 / 4: round 1 / 2 / 3 fell back, bit 2: an
    entry was left out of a round, bit 3: more than 4096 points, the first 4096 were fitted on, bit 5: the frame is the source frame
    itself, the pose is exactly (I | 0))); `out`: such a tuple to write into.  A fit needs min_points (>= 6) points within tol.  The
    unit is the structure's; the seed's rotation must be close (no minimal solver); one pinhole camera without distortion; the
    structure is not refined (no bundle adjustment).  fit_p3p asks the same question without a seed."""
    src = _TensorSource("fit_resection", tracks, visible, first_row=first_row, scale=scale)
    return _resection_fit(src, intrinsics, _group_axis(structure, 2), _group_axis(valid, 1), _group_axis(seed_pose, 3), lag, to, anchor, tol,
                          hypotheses, min_points, seed, out)


# ------------------------------------------------------------------------------------------
# fit p3p (csrc/p3p.hip; include/ctk.h, "fit p3p")
# ------------------------------------------------------------------------------------------
def fit_p3p(tracks: torch.Tensor, visible: torch.Tensor, intrinsics, structure: torch.Tensor, valid: torch.Tensor, *, lag: int = 1,
            to: Optional[int] = None, anchor: Optional[FieldAnchor] = None, tol: float = 2.0, hypotheses: int = 256, min_points: int = 16,
            seed: int = 0, first_row: Optional[torch.Tensor] = None, scale=(1, 1), out=None):
    """Where the camera is on every frame against a 3-D structure, WITHOUT a seed pose: fit_resection's question answered from the
    structure alone, by one launch and without a wait (ctk_fit_p3p; include/ctk.h and csrc/p3p_math.h have the rules).  Each of the
    `hypotheses` candidates is the pose that three sampled structure points fix (the scales of their rays by six Newton rounds that
    start at the points' own distances from the structure's camera, then the rotation by the polar steps); the candidate with most
    points within tol pixels of their reprojection wins, the lowest on ties, and is refined by fit_resection's three Gauss-Newton
    rounds.  No two-view fit comes first, so a structure of which most points have begun to move, or a planar one, is no obstacle.

    tracks, visible, intrinsics, structure, valid, lag / to / anchor, first_row, scale   as in fit_resection.
    Returns fit_resection's tuple (pose float32 [G,T,3,4], label int8 [G,T,N], error float32 [G,T,N], stats int32 [G,T,4]) with the
    same meaning; the winning candidate stats[..., 2] lies in 0 .. hypotheses, the last being (I | 0) -- the only one on the source
    frame itself, whose pose is exactly (I | 0).  `out`: such a tuple to write into.  A fit needs min_points (>= 6) points within tol.
    Limits: Newton finds the P3P root nearest the structure's own distances, one root per triple -- measured on camera displacements
    up to the depth of the nearest point; the rest are fit_resection's (the unit is the structure's; one pinhole camera without
    distortion; no bundle adjustment)."""
    src = _TensorSource("fit_p3p", tracks, visible, first_row=first_row, scale=scale)
    return _resection_fit(src, intrinsics, _group_axis(structure, 2), _group_axis(valid, 1), None, lag, to, anchor, tol, hypotheses, min_points,
                          seed, out, kind="p3p")


# ------------------------------------------------------------------------------------------
# fit align (csrc/align.hip; include/ctk.h, "fit align")
# ------------------------------------------------------------------------------------------
def _align_fit(a, valid_a, b, valid_b, intrinsics, mask, tol, depth_tol, hypotheses, min_points, seed, out, who: str):
    """The body of fit_align and StreamGroups.align: the args, the rules and the one launch of ctk_fit_align.  There is no history in
    this call, so no source is bound."""
    if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32 and a.dim() in (2, 3) and a.shape[-1] == 3):
        raise ValueError(f"{who}: a must be a float32 device tensor [N,3] or [G,N,3]")
    a, valid_a, b, valid_b, mask = _group_axis(a, 2), _group_axis(valid_a, 1), _group_axis(b, 2), _group_axis(valid_b, 1), _group_axis(mask, 1)
    G, N, dev = a.shape[0], a.shape[1], a.device
    if not (1 <= N <= L.Motion.POINTS_MAX and 1 <= G <= 65535):
        raise ValueError(f"{who}: between 1 and {L.Motion.POINTS_MAX} slots per set and at most 65535 pairs, got {N} and {G}")
    g = L.Align.Args()
    g.G, g.N, g.reserved = G, N, 0
    g.min_points = _min_points_of(min_points, L.Align.MIN_POINTS, who)
    _sampling(g, hypotheses, seed, tol, None, who, resection=True)
    _intrinsics(g, intrinsics, who)
    g.depth_tol = float(depth_tol)
    if not (math.isfinite(g.depth_tol) and 0.0 < g.depth_tol <= 3.0e38):
        raise ValueError(f"{who}: depth_tol must be finite and > 0 (a share of the depth)")
    g.a = _tensor_ptr(a, _F32, (G, N, 3), "a", dev, who)
    g.valid_a = _tensor_ptr(valid_a, _BYTES, (G, N), "valid_a", dev, who)
    g.b = _tensor_ptr(b, _F32, (G, N, 3), "b", dev, who)
    g.valid_b = _tensor_ptr(valid_b, _BYTES, (G, N), "valid_b", dev, who)
    g.mask = None if mask is None else _tensor_ptr(mask, _BYTES, (G, N), "mask", dev, who)
    specs = [("sim", torch.float32, (G, 3, 4)), ("scale", torch.float32, (G,)), ("label", torch.int8, (G, N)),
             ("error", torch.float32, (G, N)), ("stats", torch.int32, (G, 4))]
    out = _out_tuple(out, specs, dev, who)
    for (name, _, _), t_ in zip(specs, out):
        setattr(g, name, t_.data_ptr())
    L.check(L.load().ctk_fit_align(C.byref(g), None, 0, _stream()), "ctk_fit_align")  # (the workspace query answers 0)
    return out


def fit_align(a: torch.Tensor, valid_a: torch.Tensor, b: torch.Tensor, valid_b: torch.Tensor, intrinsics, mask: Optional[torch.Tensor] = None,
              tol: float = 2.0, depth_tol: float = 0.1, hypotheses: int = 256, min_points: int = 8, seed: int = 0, out=None):
    """The similarity that best maps one set of 3-D points onto another, b ~ s R a + t with s > 0, robustly: by one launch and without
    a wait (ctk_fit_align; include/ctk.h and csrc/align_math.h have the rules).  Works on any tensors -- two structures of a stream,
    offline results, surveyed points -- as long as slot n of both sets is the same point.

    a, b         float32 [G,N,3] / [N,3]: the two sets; b in the coordinates of a camera (z forward), whose pinhole model `intrinsics` is.
    valid_a, valid_b   int8 / uint8 / bool [G,N] / [N]: which slots hold a point.  A slot is a correspondence when both bytes are
                 nonzero, all six numbers are finite and at most 2^20 in magnitude and b's depth is > 0.
    intrinsics   (fx, fy, cx, cy), four Python floats: the camera of b's frame, in whose pixels tol is stated.
    mask         int8 / uint8 / bool [G,N] / [N] or None: the correspondences that may take part in the fit; all are classified.
    Each of the `hypotheses` candidates is the similarity that three sampled correspondences fix (the scale from the two triangles'
    sides, the rotation from their frames); the last candidate is the identity.  A point is within tolerance when s R a + t lies in
    front of the camera, within tol pixels of b's projection and within depth_tol of b's depth (relative); the candidate with most
    such points wins, the lowest on ties, and is refined by three Gauss-Newton rounds on those two errors.  Returns (sim float32
    [G,3,4]: row r = (s R[r], t[r]), apply_similarity applies it; all zero where there is no fit; scale float32 [G]: s, 0 where there
    is no fit; label int8 [G,N]: 1 within tolerance, 0 not, -1 no correspondence; error float32 [G,N]: the squared pixel distance,
    +inf behind the camera, -1 without a correspondence or a fit; stats int32 [G,4] = (points fitted on, points labelled 1, the
    winning candidate or -1, bits: 1 a round kept its transform, 2 an entry was left out, 3 more than 4096 points, 5 the sets are
    identical: exactly (1, I, 0))); `out`: such a tuple to write into.  A fit needs min_points (>= 3) points within tolerance.
    Limits: one similarity per pair; at least three non-collinear common points; no covariance; a degenerate inlier set keeps the
    candidate's transform (bit 1)."""
    return _align_fit(a, valid_a, b, valid_b, intrinsics, mask, tol, depth_tol, hypotheses, min_points, seed, out, "fit_align")


def apply_similarity(sim: torch.Tensor, points: torch.Tensor) -> torch.Tensor:
    """sim [...,3,4] = (s R | t) of fit_align on points [...,N,3] -> s R X + t, [...,N,3] (elementwise torch, no wait)."""
    return points @ sim[..., :3].transpose(-1, -2) + sim[..., None, :, 3]


def compose_similarity(pose: torch.Tensor, sim: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """A pose [...,3,4] = (R_p | t_p) against a's world, X_f = R_p X_a + t_p in a's unit, stated against b's world and in b's unit,
    with sim [...,3,4] = (s R | t) and scale [...] = s of fit_align(a, b) (elementwise torch, no wait).
    X_b = s R X_a + t gives X_a = R^T (X_b - t) / s, so X_f = R_p R^T (X_b - t) / s + t_p; times s, the same camera point in b's unit:
    s X_f = (R_p R^T) X_b + (s t_p - R_p R^T t).  Hence R' = R_p R^T and t' = s t_p - R' t.  Where there is no fit (scale 0) the
    result is not finite."""
    s = scale[..., None, None]
    Rn = pose[..., :3] @ (sim[..., :3] / s).transpose(-1, -2)
    return torch.cat([Rn, s * pose[..., 3:] - Rn @ sim[..., 3:]], dim=-1)


def camera_centre(pose: torch.Tensor) -> torch.Tensor:
    """Where the camera of a pose [...,3,4] = (M | t) with X_f = M X_w + t stands in the world's coordinates and unit: -M^-1 t, [...,3]
    (a 3 x 3 solve in torch, no wait).  For a rigid pose this is -R^T t; it also holds for what world_pose() returns against a structure
    of merge_structures, whose left block is a rotation times the scale between the two units -- there -R^T t would be off by s^2."""
    return -torch.linalg.solve(pose[..., :3], pose[..., 3])


def merge_structures(a: "Structure", b: "Structure", sim: torch.Tensor, label: torch.Tensor) -> "Structure":
    """Two structures of one stream as one, on b's anchor, in b's unit and b's camera, from what fit_align(a.points, a.valid, b.points,
    b.valid) returned for them (sim [3,4], label [N]; elementwise torch, no wait): b's points where b has one; where b has none and a
    has one, a's point carried over by sim -- if there is a fit (a slot labelled 1) and the carried point lies in front of b's
    camera.  origin = (s R | t) composed with a.origin, the map from the first world of a's chain into b's camera and unit, so that
    world_pose() of a pose against the merged structure keeps answering in that first world: its left block is a rotation times s
    (the two units differ), so the camera's centre is camera_centre(pose) = -M^-1 t, in the first world's unit -- NOT -R^T t --, and
    (M | t) / s is the rigid pose there."""
    if not (isinstance(a, Structure) and isinstance(b, Structure)):
        raise ValueError("merge_structures: a and b must be ops.Structure")
    carried = apply_similarity(sim, a.points)
    take = (a.valid != 0) & (b.valid == 0) & (label == 1).any() & (carried[:, 2] > 0) & torch.isfinite(carried).all(dim=-1)
    points = torch.where(take[:, None], carried, b.points)
    valid = torch.where(take, torch.ones_like(b.valid), b.valid)
    origin = sim if a.origin is None else torch.cat([sim[:, :3] @ a.origin[:, :3], sim[:, :3] @ a.origin[:, 3:] + sim[:, 3:]], dim=-1)
    return Structure(points, valid, b.anchor, b.intrinsics, origin)


# ------------------------------------------------------------------------------------------
# fit structure (csrc/structure.hip; include/ctk.h, "fit structure")
# ------------------------------------------------------------------------------------------
def min_sin2_of(min_parallax: float) -> float:
    """min_parallax in degrees -> the squared sine the kernel compares with (the float32 of sin^2), in (0, 1]."""
    deg = float(min_parallax)
    if not (math.isfinite(deg) and 0.0 < deg <= 90.0):
        raise ValueError("min_parallax must lie in (0, 90] degrees")
    s2 = struct.unpack("f", struct.pack("f", math.sin(math.radians(deg)) ** 2))[0]
    if not 0.0 < s2 <= 1.0:
        raise ValueError("min_parallax is too small: its squared sine is no positive float32")
    return s2


def _structure_fit(src, intrinsics, pose, pose_stats, structure, valid, source_frame, origin, into, tol, min_views, min_parallax, refine, out):
    a, who, dev, G, F_ = _FITS["structure"].args(), src.who, src.device, src.G, src.F
    min_views, into = int(min_views), -1 if into is None else int(into)
    if not 1 <= F_ <= L.Structure3D.VIEWS_MAX:
        raise ValueError(f"{who}: between 1 and {L.Structure3D.VIEWS_MAX} frames are views, got {F_}")
    if not L.Structure3D.MIN_VIEWS <= min_views <= L.Structure3D.VIEWS_MAX:
        raise ValueError(f"{who}: min_views must lie in {L.Structure3D.MIN_VIEWS}..{L.Structure3D.VIEWS_MAX}")
    if not -1 <= into < F_:
        raise ValueError(f"{who}: into must be one of the {F_} views, or None")
    if int(source_frame) < 0:
        raise ValueError(f"{who}: source_frame must be a frame >= 0")
    try:
        a.min_sin2 = min_sin2_of(min_parallax)
    except ValueError as e:
        raise ValueError(f"{who}: {e}") from None
    _intrinsics(a, intrinsics, who)
    a.into, a.source_frame, a.min_views, a.refine, a.tol, a.reserved = into, int(source_frame), min_views, 1 if refine else 0, _positive_tol(tol, who), 0
    a.pose = _tensor_ptr(pose, _F32, (G, F_, 3, 4), "pose", dev, who, " (fit_resection's)")
    a.pose_stats = None if pose_stats is None else _tensor_ptr(pose_stats, _I32, (G, F_, 4), "pose_stats", dev, who, " (fit_resection's)")
    if (structure is None) != (valid is None):
        raise ValueError(f"{who}: structure and valid come both or neither")
    a.structure_in = a.valid_in = None
    if structure is not None:
        a.structure_in = _tensor_ptr(structure, _F32, (G, src.N, 3), "structure", dev, who)
        a.valid_in = _tensor_ptr(valid, _BYTES, (G, src.N), "valid", dev, who)
    a.origin_in = None if origin is None else _tensor_ptr(origin, _F32, (G, 3, 4), "origin", dev, who)
    src.bind(a)
    return _fit_launch("structure", a, out, dev, who)


def fit_structure(tracks: torch.Tensor, visible: torch.Tensor, intrinsics, pose: torch.Tensor, *, pose_stats: Optional[torch.Tensor] = None,
                  structure: Optional[torch.Tensor] = None, valid: Optional[torch.Tensor] = None, source_frame: int = 0,
                  origin: Optional[torch.Tensor] = None, into: Optional[int] = None, tol: float = 2.0, min_views: int = 3,
                  min_parallax: float = 1.0, refine: bool = False, first_row: Optional[torch.Tensor] = None, scale=(1, 1), out=None):
    """Points added to a 3-D structure: every point tracked on several LOCALISED frames becomes a 3-D point in the structure's unit, by
    one launch and without a wait (ctk_fit_structure; include/ctk.h and csrc/structure_math.h have the rules).  Works on any result of
    any predictor here, offline ones included.

    tracks, visible, first_row, scale   as in fit_resection; all T <= 256 frames are views.
    intrinsics   (fx, fy, cx, cy), four Python floats: one pinhole camera in the pixels of tracks * scale.
    pose, pose_stats   float32 [G,T,3,4] / [T,3,4] and int32 [G,T,4] / [T,4] as fit_resection returned them for these frames; a frame
             whose pose is not finite, is no rotation, or (with pose_stats) had no fit is no view.  Only read.
    structure, valid, source_frame   the old structure (float32 [G,N,3] / [N,3], int8 / uint8 / bool [G,N] / [N]) and the frame it is
             stated in, or neither: its points are carried along (label 2) unless first_row says the slot was reassigned after
             source_frame; refine: they are triangulated too, and a new point that is accepted wins.
    origin   float32 [G,3,4] / [3,4]: the old structure's own origin (None: the identity).
    into     a view k (a row of tracks): every point that is written is stated in the camera of that frame, and the returned origin is
             (R_k R_o | R_k t_o + t_k); None: points stay in the coordinates the poses map from, the origin is copied.
    Per point: a linear midpoint start over its observations, three Gauss-Newton rounds on the reprojection error with gates of 4, 2
    and 1 x tol pixels, then accepted when at least min_views (2..256) views and at least half of its observations lie within tol
    and the first of them shows a parallax of at least min_parallax degrees against another.  Returns (points float32 [G,N,3], zero where label < 1; label int8 [G,N]: -1 fewer
    than two observations and not carried, 0 rejected, 1 accepted, 2 carried; error float32 [G,N]: the mean squared reprojection error
    over the counted views in px^2, -1 where the label is not 1; stats int32 [G,N,4] = (observations, counted views, the first
    counted view or -1, bits 0 / 1 / 2: round 1 / 2 / 3 fell back, bit 3: no start, bit 4: no parallax, bit 5: the `into` view is no
    view: no structure at all, bit 6: fewer than half of the observations are counted); origin float32 [G,3,4]); `out`: such a tuple to write into.  No bundle adjustment; the parallax test
    looks at the first counted view against the others only; one pinhole camera without distortion."""
    src = _TensorSource("fit_structure", tracks, visible, first_row=first_row, scale=scale, points_max=L.Structure3D.POINTS_MAX)
    return _structure_fit(src, intrinsics, _group_axis(pose, 3), _group_axis(pose_stats, 2), _group_axis(structure, 2), _group_axis(valid, 1),
                          source_frame, _group_axis(origin, 2), into, tol, min_views, min_parallax, refine, out)


# ------------------------------------------------------------------------------------------
# CoTracker2 iteration (cotracker.py:86-173): row kernels + the general update former
# ------------------------------------------------------------------------------------------
def sample_features4d(map_hwc: torch.Tensor, coords: torch.Tensor) -> torch.Tensor:
    """sample_features4d (model_utils.py:258-290): channels-last map [H,W,C] sampled at coords [N,2]=(x,y) -> [N,C]."""
    _chk_f32(map_hwc, coords)
    H, W, Cc = map_hwc.shape
    N = coords.shape[0]
    out = torch.empty(N, Cc, device=coords.device, dtype=torch.float32)
    L.check(L.load().ctk_sample_features4d(_ptr(map_hwc), H, W, Cc, _ptr(coords), N, _ptr(out), _stream()), "ctk_sample_features4d")
    return out


def bilinear_sampler(input: torch.Tensor, coords: torch.Tensor, align_corners: bool = True, padding_mode: str = "border") -> torch.Tensor:
    """Op D: bilinear_sampler (model_utils.py:191-255), the reference's signature and layouts -- input [B,C,H,W] with coords
    [B,Ho,Wo,2] = (x, y) -> [B,C,Ho,Wo], or input [B,C,T,H,W] with coords [B,Do,Ho,Wo,3] = (t, x, y) -> [B,C,Do,Ho,Wo].
    Bit-identical to the reference's F.grid_sample on the CPU (ctk_bilinear_sampler, csrc/sampler.hip)."""
    input, coords = input.contiguous(), coords.contiguous()  # (the reference's own unit test hands over permuted coordinates)
    _chk_f32(input, coords)
    if padding_mode not in ("zeros", "border"):
        raise NotImplementedError(f"padding_mode={padding_mode!r}: the HIP sampler implements 'zeros' and 'border'")
    sizes = input.shape[2:]
    assert len(sizes) in (2, 3), "input must be [B,C,H,W] or [B,C,T,H,W]"
    nd = len(sizes)
    assert coords.dim() == nd + 2 and coords.shape[-1] == nd and coords.shape[0] == input.shape[0]
    B, Cc = input.shape[:2]
    D = sizes[0] if nd == 3 else 0
    H, W = sizes[-2], sizes[-1]
    inner = tuple(coords.shape[1:-1])
    P = 1
    for d in inner:
        P *= d
    out = torch.empty((B, Cc) + inner, device=input.device, dtype=torch.float32)
    if P > 0:
        L.check(L.load().ctk_bilinear_sampler(_ptr(input), B, Cc, D, H, W, _ptr(coords), P, int(bool(align_corners)),
                                              L.PAD_BORDER if padding_mode == "border" else L.PAD_ZEROS, _ptr(out), _stream()),
                "ctk_bilinear_sampler")
    return out


def v2_assemble(coords, fcorrs, track_feat, track_mask, vis, pos, in_ld: int, out_split: bool) -> torch.Tensor:
    """Transformer input of CoTracker2 (cotracker.py:135-150 without the time embedding): [N*S, in_ld] f32 or SH."""
    _chk_f32(coords, fcorrs, track_feat, track_mask, vis, pos)
    S, N = coords.shape[0], coords.shape[1]
    assert fcorrs.shape == (N, S, 196) and track_feat.shape == (S, N, 128) and pos.shape == (N, 456)
    assert track_mask.shape == (S, N) and vis.shape == (S, N)
    x = (torch.empty(N * S, in_ld // 32, 2, 32, device=coords.device, dtype=torch.float16) if out_split
         else torch.empty(N * S, in_ld, device=coords.device, dtype=torch.float32))
    L.check(L.load().ctk_v2_assemble(S, N, _ptr(coords), _ptr(fcorrs), _ptr(track_feat), _ptr(track_mask), _ptr(vis), _ptr(pos),
                                     in_ld, _ptr(x), int(out_split), _stream()), "ctk_v2_assemble")
    return x


def v2_apply_delta(delta: torch.Tensor, coords: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5):
    """coords [S,N,2] += delta[:, :2] in place; returns GroupNorm(1,128)(delta[:, 2:130]) as [S*N,128] (row t*N+n)."""
    _chk_f32(delta, coords, gamma, beta)
    S, N = coords.shape[0], coords.shape[1]
    assert delta.shape[0] == N * S
    normed = torch.empty(S * N, 128, device=coords.device, dtype=torch.float32)
    L.check(L.load().ctk_v2_apply_delta(S, N, _ptr(delta), delta.shape[1], _ptr(coords), _ptr(gamma), _ptr(beta), float(eps),
                                        _ptr(normed), _stream()), "ctk_v2_apply_delta")
    return normed


def v2_vis_head(track_feat: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """vis_predictor (cotracker.py:172): track_feat [S,N,128] -> logits [S,N]."""
    _chk_f32(track_feat, w, b)
    S, N, _ = track_feat.shape
    out = torch.empty(S, N, device=track_feat.device, dtype=torch.float32)
    L.check(L.load().ctk_v2_vis_head(_ptr(track_feat), S * N, _ptr(w), _ptr(b), _ptr(out), _stream()), "ctk_v2_vis_head")
    return out


def update_former_ex(x: torch.Tensor, x_split: bool, S: int, N: int, fw: "L.FormerWeights", point_mask: Optional[torch.Tensor]) -> torch.Tensor:
    """General EfficientUpdateFormer.forward (cotracker.py:483-531) with the CoTracker2 attention mask:
    x [N*S, in_ld] (f32 or SH) -> delta [N*S, out_ld] f32."""
    ws = _workspace(_query_bytes("ctk_update_former_workspace_bytes", S, N), x.device)
    delta = torch.empty(N * S, fw.out_ld, device=x.device, dtype=torch.float32)
    if point_mask is not None:
        assert point_mask.dtype == torch.uint8 and point_mask.shape == (N,) and point_mask.is_cuda
    L.check(L.load().ctk_update_former_ex(S, N, _ptr(x), int(x_split), C.byref(fw), _ptr(point_mask), _ptr(delta), _ptr(ws), ws.numel(),
                                     _stream()), "ctk_update_former_ex")
    return delta


# One CoTracker3 window as a host model asks for it: Window's tensors in the order of Window.keep, and whether the window may
# overwrite coords / vis / conf (`owned`; if not, the caller still needs them -- the sliding carry-over -- and the window gets clones).
WindowRequest = namedtuple("WindowRequest", "fmaps support coords vis conf mask owned")


def window_tensors(parts) -> List[torch.Tensor]:
    """The tensors of a window's `keep`, or of a request in that order, as one flat list (per-level lists expanded; no None, no flag)."""
    return [t_ for p_ in parts for t_ in (p_ if isinstance(p_, list) else [p_]) if torch.is_tensor(t_)]


class _WindowTensors:
    """What Window and V2Window know about the tensors behind their ctypes struct.  keep: the constructor's tensor arguments in
    its order, held alive; state: those the window call updates in place, which a graph warm-up must save and restore."""

    def inputs(self) -> List[torch.Tensor]:  # every tensor a graph replay must refresh, in the one fixed order of `keep`
        return window_tensors(self.keep)

    def clone(self):
        """A window of the same arguments on private copies of all inputs: the static buffers of a captured graph."""
        return self._like(*[[t_.clone() for t_ in p_] if isinstance(p_, list) else p_ if p_ is None else p_.clone() for p_ in self.keep])

    def refresh(self, src) -> None:
        """copy_ every input from `src`: a window of the same shape, or a request (its tensors in the order of `keep`)."""
        for d, s_ in zip(self.inputs(), window_tensors(getattr(src, "keep", src))):
            d.copy_(s_)


class V2Window(_WindowTensors):
    """ctypes ctk_v2_window_args of one CoTracker2 window plus the tensors it points to (coords / track_feat are
    updated in place by forward_window_v2, vis_out receives the visibility logits)."""

    def __init__(self, pyr: Sequence[torch.Tensor], coords: torch.Tensor, track_feat: torch.Tensor, vis: torch.Tensor,
                 track_mask: torch.Tensor, point_mask: Optional[torch.Tensor], iters: int):
        _chk_f32(*pyr, coords, track_feat, vis, track_mask)
        S, N = coords.shape[0], coords.shape[1]
        assert coords.shape == (S, N, 2) and track_feat.shape == (S, N, 128) and vis.shape == (S, N) and track_mask.shape == (S, N)
        a = L.V2WindowArgs()
        a.S, a.N, a.iters = S, N, iters
        for l in range(L.LEVELS):
            assert pyr[l].shape[0] == S and pyr[l].shape[3] == 128
            a.H[l], a.W[l], a.fmaps[l] = pyr[l].shape[1], pyr[l].shape[2], _ptr(pyr[l])
        if point_mask is not None:
            assert point_mask.dtype == torch.uint8 and point_mask.is_cuda and point_mask.shape == (N,)
        self.vis_out = torch.empty(S, N, device=coords.device, dtype=torch.float32)
        a.coords, a.track_feat, a.vis, a.track_mask = _ptr(coords), _ptr(track_feat), _ptr(vis), _ptr(track_mask)
        a.point_mask, a.vis_out = _ptr(point_mask), _ptr(self.vis_out)
        self.args = a
        self.S, self.N = S, N
        self.keep = (list(pyr), coords, track_feat, vis, track_mask, point_mask)
        self.state = (coords, track_feat)
        self._like = lambda *parts: V2Window(*parts, iters)
        self.device = coords.device

    def result(self):  # what the host code consumes after the call: (coords, visibility logits)
        return self.state[0], self.vis_out


# ------------------------------------------------------------------------------------------
# window-level ops
# ------------------------------------------------------------------------------------------
class Window(_WindowTensors):
    """Holds the ctypes ctk_window_args plus the tensors it points to."""

    def __init__(self, fmaps: Sequence[torch.Tensor], support: Sequence[torch.Tensor], coords: torch.Tensor,
                 vis: torch.Tensor, conf: torch.Tensor, scale_xy, iters: int = 6,
                 point_mask: Optional[torch.Tensor] = None, max_corr_rows: int = 262144, use_aux_stream: bool = True,
                 space_attn: bool = True):
        _chk_f32(*fmaps, *support, coords, vis, conf)
        S, N = coords.shape[0], coords.shape[1]
        assert coords.shape == (S, N, 2) and vis.shape == (S, N) and conf.shape == (S, N)
        a = L.WindowArgs()
        a.S, a.N, a.iters = S, N, iters
        for l in range(L.LEVELS):
            assert fmaps[l].shape[0] == S and fmaps[l].shape[3] == 128
            assert support[l].shape == (N, 49, 128)
            a.H[l], a.W[l] = fmaps[l].shape[1], fmaps[l].shape[2]
            a.fmaps[l] = _ptr(fmaps[l])
            a.support[l] = _ptr(support[l])
        if point_mask is not None:
            assert point_mask.dtype == torch.uint8 and point_mask.is_cuda and point_mask.shape == (N,)
        a.point_mask = _ptr(point_mask)
        a.coords, a.vis, a.conf = _ptr(coords), _ptr(vis), _ptr(conf)
        a.scale_x, a.scale_y = float(scale_xy[0]), float(scale_xy[1])
        a.points_per_chunk = max(1, min(N, max_corr_rows // S))
        a.aux_stream = aux_stream(coords.device).cuda_stream if use_aux_stream else None
        a.flags = 0 if space_attn else L.WINDOW_NO_SPACE_ATTN  # add_space_attn=False (cotracker.py:496-502)
        self.args = a
        self.S, self.N = S, N
        self.keep = (list(fmaps), list(support), coords, vis, conf, point_mask)
        self.state = (coords, vis, conf)
        self._like = lambda fm, sup, c, v, f, m: Window(fm, sup, c, v, f, scale_xy, iters, m, max_corr_rows, use_aux_stream, space_attn)
        self.device = coords.device

    def result(self):  # what the host code consumes after the call: the state, updated in place
        return self.state


_ws_cache = {}
_aux_streams = {}


def aux_stream(device) -> torch.cuda.Stream:
    """The per-device auxiliary stream handed to ctk_forward_window (ctk_window_args.aux_stream): the library forks
    independent launches onto it and joins it back, so callers never synchronise with it themselves."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _aux_streams:
        _aux_streams[key] = torch.cuda.Stream(device=device)
    return _aux_streams[key]


def _workspace(nbytes: int, device) -> torch.Tensor:
    key = (device.index if device.index is not None else torch.cuda.current_device())
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _ws_cache[key] = None  # (the old buffer is released before the larger one is allocated)
        buf = _ws_cache[key] = torch.empty(nbytes, device=device, dtype=torch.uint8)
    return buf


def _run_window(name: str, args, wstruct, nbytes: int, device) -> None:
    """The direct window calls: entry point `name` on the argument and weight structs with the shared workspace of `nbytes`."""
    ws = _workspace(nbytes, device)
    L.check(getattr(L.load(), name)(C.byref(args), C.byref(wstruct), _ptr(ws), ws.numel(), _stream()), name)


def forward_window(win: Window, weights) -> None:
    """`iters` update iterations in place on win's coords/vis/conf (cotracker3_online.py:171-264)."""
    nbytes = _query_bytes("ctk_forward_window_workspace_bytes", C.byref(win.args))
    _run_window("ctk_forward_window", win.args, weights.struct_for(win.S, folded=True), nbytes, win.device)


def forward_window_v2(win: V2Window, weights) -> None:
    """CoTracker2.forward_window (cotracker.py:86-173) as one C call: `iters` iterations in place on win's coords /
    track_feat, visibility logits into win.vis_out."""
    _run_window("ctk_forward_window_v2", win.args, weights.struct, _v2_workspace_bytes(win, weights), win.device)


def _v2_workspace_bytes(win: V2Window, weights) -> int:
    return _query_bytes("ctk_forward_window_v2_workspace_bytes", C.byref(win.args), C.byref(weights.struct))


class WindowGraph:
    """hipGraph of one whole window (all `iters` iterations, ~190 launches each) captured once by
    ctk_window_graph_create and replayed with ONE graph launch per call (BASELINE.json configs[3]).

    The graph bakes in the pointers of ``win``'s tensors, of the weights and of a private workspace, so the
    caller refreshes the CONTENTS of win's tensors in place (``copy_``) and calls ``launch()``."""

    def __init__(self, win: Window, weights):
        self.wins = [win]
        self._capture("ctk_forward_window", "ctk_window_graph_create", win.args, weights, weights.struct_for(win.S, folded=True),
                      _query_bytes("ctk_forward_window_workspace_bytes", C.byref(win.args)), win.state, [win.args], win.device)

    def _capture(self, direct: str, create: str, args, weights, wstruct, nbytes: int, state, iter_slots, device) -> None:
        """The capture protocol of every window graph.  direct / create: the C entry points of the direct call and of the
        capture (same arguments: `args`, the weights' struct); state: the tensors the window updates in place; iter_slots: the
        argument structs whose `iters` the warm-up call patches to 1."""
        lib = L.load()
        self.weights = weights                      # keeps every weight tensor (and in_bias_t for this S) alive
        self.ws = torch.empty(nbytes, device=device, dtype=torch.uint8)  # private: its address is baked in
        call = (C.byref(args), C.byref(wstruct), _ptr(self.ws), self.ws.numel())
        # One direct iteration first: every kernel of the window is resident (HIP loads code objects lazily, which
        # is not allowed inside a capture); the state it touched is restored afterwards.
        saved = [t_.clone() for t_ in state]
        iters = iter_slots[0].iters
        for a in iter_slots:
            a.iters = 1
        L.check(getattr(lib, direct)(*call, _stream()), direct)
        for a in iter_slots:
            a.iters = iters
        for t_, s_ in zip(state, saved):
            t_.copy_(s_)
        torch.cuda.synchronize(device)              # weight packing / input copies issued so far are complete
        h = C.c_void_p()
        L.check(getattr(lib, create)(*call, C.byref(h)), create)
        self._h = h
        n = C.c_int64(0)
        L.check(lib.ctk_window_graph_nodes(self._h, C.byref(n)), "ctk_window_graph_nodes")
        self.nodes = n.value

    def launch(self) -> None:
        L.check(L.load().ctk_window_graph_launch(self._h, _stream()), "ctk_window_graph_launch")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                L.load().ctk_window_graph_destroy(h)
            except Exception:
                pass


class V2WindowGraph(WindowGraph):
    """hipGraph of one CoTracker2 window (ctk_v2_window_graph_create): the contract of WindowGraph."""

    def __init__(self, win: V2Window, weights):
        self.wins = [win]
        self._capture("ctk_forward_window_v2", "ctk_v2_window_graph_create", win.args, weights, weights.struct,
                      _v2_workspace_bytes(win, weights), win.state, [win.args], win.device)


class WindowBatch:
    """ctk_window_batch over B Windows of equal shape (S, N, iters, level sizes, scale, flags, mask presence): the
    argument of the joint calls.  ``points_per_chunk`` counts points of the STACKED list of B*N tracks (default: what
    ``max_corr_rows`` rows of correlation volume hold, as for one window) and is written into wins[0]'s slot of the array.
    ``shared``: the windows are query groups of ONE video (ctk_window_batch.flags = CTK_BATCH_SHARED_FMAPS) -- the same fmaps
    in every window, state / support / mask as consecutive slices of one allocation each, which is what ``group_windows``
    builds; the library checks it and answers anything else with CTK_E_SHAPE."""

    def __init__(self, wins: Sequence[Window], max_corr_rows: int = 262144, points_per_chunk: Optional[int] = None,
                 shared: bool = False):
        B = len(wins)
        if not 1 <= B <= L.MAX_BATCH:
            raise ValueError(f"a joint window takes 1..{L.MAX_BATCH} videos, got {B}")
        self.wins = list(wins)
        self.arr = (L.WindowArgs * B)()
        for b, w_ in enumerate(wins):
            C.memmove(C.byref(self.arr[b]), C.byref(w_.args), C.sizeof(L.WindowArgs))
        if B > 1:
            S, N = wins[0].S, wins[0].N
            ppc = points_per_chunk if points_per_chunk is not None else max(1, min(B * N, max_corr_rows // S))
            for b in range(B):
                self.arr[b].points_per_chunk = int(ppc)
        elif points_per_chunk is not None:
            self.arr[0].points_per_chunk = int(points_per_chunk)
        self.struct = L.WindowBatch(B, L.BATCH_SHARED_FMAPS if shared else 0, C.cast(self.arr, C.POINTER(L.WindowArgs)))
        self.B, self.S, self.N = B, wins[0].S, wins[0].N
        self.device = wins[0].device

    def workspace_bytes(self) -> int:
        return _query_bytes("ctk_forward_window_batch_workspace_bytes", C.byref(self.struct))


def group_windows(fmaps: Sequence[torch.Tensor], support: Sequence[torch.Tensor], coords: torch.Tensor, vis: torch.Tensor,
                  conf: torch.Tensor, scale_xy, point_mask: Optional[torch.Tensor] = None, **window_kw) -> List[Window]:
    """The G windows of G query groups over ONE video, as ``WindowBatch(..., shared=True)`` takes them: every window points at
    the same fmaps and at its slice of support[l] [G*N,49,128], coords [G,S,N,2], vis / conf [G,S,N] and point_mask [G,N]."""
    G, _, N = coords.shape[:3]
    assert all(s_.shape[0] == G * N for s_ in support) and (point_mask is None or point_mask.shape == (G, N))
    return [Window(fmaps, [s_[g * N:(g + 1) * N] for s_ in support], coords[g], vis[g], conf[g], scale_xy,
                   point_mask=None if point_mask is None else point_mask[g], **window_kw) for g in range(G)]


def forward_windows(wins: Sequence[Window], weights, max_corr_rows: int = 262144, points_per_chunk: Optional[int] = None,
                    shared: bool = False) -> None:
    """ONE joint window call for B videos (ctk_forward_window_batch): `iters` update iterations in place on every
    win's coords / vis / conf.  One video: exactly forward_window(wins[0]).  shared: B query groups of one video (WindowBatch)."""
    batch = WindowBatch(wins, max_corr_rows, points_per_chunk, shared)
    _run_window("ctk_forward_window_batch", batch.struct, weights.struct_for(batch.S, folded=True), batch.workspace_bytes(), batch.device)


class WindowBatchGraph(WindowGraph):
    """hipGraph of one joint window of B videos (ctk_window_batch_graph_create): the contract of WindowGraph for every win."""

    def __init__(self, wins: Sequence[Window], weights, max_corr_rows: int = 262144, points_per_chunk: Optional[int] = None,
                 shared: bool = False):
        self.batch = batch = WindowBatch(wins, max_corr_rows, points_per_chunk, shared)
        self.wins = batch.wins
        self._capture("ctk_forward_window_batch", "ctk_window_batch_graph_create", batch.struct, weights,
                      weights.struct_for(batch.S, folded=True),
                      batch.workspace_bytes(), [t_ for w_ in batch.wins for t_ in w_.state], list(batch.arr), batch.device)


# ------------------------------------------------------------------------------------------
# stream state of G query groups over one live video (include/ctk.h: ctk_stream_begin / _support / _commit / _assign)
# ------------------------------------------------------------------------------------------
# the query frame of an empty slot: finite, exact in float32, .long() of it is defined, and no stream reaches it -- so the row is never
# inside a sample range and never below ind + S (never sampled, point_mask 0: the blank track of a query that has not arrived)
EMPTY_FRAME = L.STREAM_EMPTY_FRAME


def history_span(committed: int, T_cap: int, ring: bool, f0: int, F: int, back: int = 0, fwd: int = 0, to: int = -1):
    """The one range rule of the readers of a stream's history (StreamGroups.draw, motion, field, objects, planes, epipolar): may a call for frames
    [f0, f0 + F) be served by a history of T_cap rows, `committed` frames in, a ring or not?  Besides its own frames the call reads
    the `back` frames before each (a trail, a positive lag; those >= 0), the frame `fwd` after each (a negative lag), and the fixed
    frame `to` (>= 0); an anchor reads nothing more.  -> None, or what is wrong with the frames [lo, hi] that are read:
    ("beyond", lo, hi): not all committed yet; ("left", lo, hi): a ring has overwritten some; ("span", lo, hi): more rows than one
    call may span -- the C-ABI keeps F + back + fwd <= T_cap and the rows that are read apart, for the rows of a ring must not alias."""
    if f0 < 0 or F < 1 or f0 + F > committed:
        return "beyond", f0, f0 + F - 1
    lo, hi = max(f0 - back, 0), f0 + F - 1 + fwd
    if to >= 0:
        lo, hi = min(lo, to), max(hi, to)
    if hi >= committed:
        return "beyond", lo, hi
    oldest = max(committed - T_cap, 0) if ring else 0
    if lo < oldest:
        return "left", lo, hi
    if max(hi - lo + 1, F + back + fwd) > T_cap:
        return "span", lo, hi
    return None


class StreamGroups:
    """The device-resident state of G query groups streamed over ONE video, in the layouts the shared joint window wants, and
    the three launches that step it (csrc/stream.hip).  Everything a window call reads or writes lives here and keeps its
    address for the life of the object -- the pyramid [S,H_l,W_l,128], the window state coords [G,S,N,2] / vis / conf [G,S,N],
    point_mask [G,N], the support accumulators support[l] [G*N,49,128] -- so captured window graphs bake these pointers in and
    nothing is stacked or copied per call.  The history [G,T_cap,N,.] is a capacity buffer outside the graphs, grown
    geometrically.  ``serial`` changes whenever the baked-in buffers are re-allocated (graph cache key).

    Slots: a row of the query table whose frame is EMPTY_FRAME (and whose position is (0, 0)) is an empty slot, and assign() /
    release() hand slots to new queries or empty them between two calls -- writes into the resident buffers: no address, no
    shape and therefore no captured graph changes.  The bookkeeping lives on the host: ``occupied`` [G,N] (bool) and
    ``first_row`` [G,N] (the history row from which the rows belong to the present occupant); ``committed`` counts the history
    rows written so far and ``next_ind`` is the first frame of the next call's window (both follow commit()).

    Ring (``ring_rows`` = R >= S, for streams without an end): the history holds R rows, frame f in row f % R, allocated once --
    reserve() never grows it, the ring forms of the four entry points step it (ctk_stream_*_ring), and an assign clears all R rows
    of a slot.  A wrapped range of frames is not a view: history() raises, emit() copies any [f0, f1) of the last R frames out in
    frame order with one launch (it serves the linear layout too), and frame_rows() names the rows of a range as slices."""

    _serial = 0
    ring_rows = None  # (a state pickled before the attribute existed)
    _stab = None

    def __init__(self, queries: torch.Tensor, S: int, step: int, stride: float, level_sizes, ring_rows: Optional[int] = None):
        if ring_rows is not None and (int(ring_rows) != ring_rows or ring_rows < S):
            raise ValueError(f"ring_rows must be an integer >= the window length {S}, got {ring_rows!r}")
        self.ring_rows = None if ring_rows is None else int(ring_rows)
        G, N = queries.shape[:2]
        dev = queries.device
        self.G, self.N, self.S, self.step, self.stride = G, N, S, step, float(stride)
        self.level_sizes = tuple(level_sizes)
        self.queries = queries.reshape(G * N, 3).float().contiguous().clone()
        self.pyr = [torch.empty(S, h, w, 128, device=dev) for h, w in level_sizes]
        self.coords = torch.empty(G, S, N, 2, device=dev)
        self.vis = torch.empty(G, S, N, device=dev)
        self.conf = torch.empty(G, S, N, device=dev)
        self.mask = torch.empty(G, N, device=dev, dtype=torch.uint8)
        self.support = [torch.zeros(G * N, 49, 128, device=dev) for _ in level_sizes]
        self.nonfinite = torch.zeros(1, device=dev, dtype=torch.int32)
        self.T_cap = 0
        self.hist = None
        self.reserve(4 * S if self.ring_rows is None else self.ring_rows)
        self.closed = False  # a chunk shorter than the window ends the stream
        self.live = True     # False: the stream it carried is over, the buffers wait for restart()
        StreamGroups._serial += 1
        self.serial = StreamGroups._serial
        self._wins = {}
        self._new_book()

    def _new_book(self) -> None:
        self.committed, self.next_ind = 0, 0
        self._stab = {}  # stabilize(): {group: (next frame, state tensor [1,6], alpha, ((H, W, zoom), post tensor or None))}
        self._occupied = None  # read from the query table when it is first asked for: the calls of a stream never wait for it
        self.first_row = torch.zeros(self.G, self.N, dtype=torch.long)

    @property
    def occupied(self) -> torch.Tensor:
        """[G,N] bool, on the host: which slots hold a query.  The first look copies the frame column of the resident table to
        the host (one small device-to-host copy per stream); assign() and release() keep it up to date from then on."""
        if self._occupied is None:
            self._occupied = (self.queries[:, 0].cpu() != EMPTY_FRAME).reshape(self.G, self.N)
        return self._occupied

    def fits(self, queries: torch.Tensor, S: int, step: int, stride: float, level_sizes, ring_rows: Optional[int] = None) -> bool:
        return (tuple(queries.shape[:2]) == (self.G, self.N) and queries.device == self.queries.device and ring_rows == self.ring_rows and
                (S, step, float(stride), tuple(level_sizes)) == (self.S, self.step, self.stride, self.level_sizes))

    def restart(self, queries: torch.Tensor) -> None:
        """A new stream on the same buffers (same shapes: the captured graphs stay valid)."""
        self.queries.copy_(queries.reshape(self.G * self.N, 3))
        for s_ in self.support:
            s_.zero_()
        for h_ in self.hist:
            h_.zero_()
        self.nonfinite.zero_()
        self.closed, self.live = False, True
        self._new_book()

    def reserve(self, T: int) -> None:
        """History capacity of at least T frames: doubled when it runs out (one copy per doubling, not per call); rows past the
        committed ones are zero.  A ring is allocated once, by the constructor, and never grows."""
        if T <= self.T_cap or (self.ring_rows is not None and self.hist is not None):
            return
        cap = max(T, 2 * self.T_cap)
        dev = self.queries.device
        new = [torch.zeros(self.G, cap, self.N, 2, device=dev), torch.zeros(self.G, cap, self.N, device=dev),
               torch.zeros(self.G, cap, self.N, device=dev)]
        if self.hist is not None:
            for n_, o_ in zip(new, self.hist):
                n_[:, :self.T_cap].copy_(o_)
        self.hist, self.T_cap = new, cap

    def history(self, T: int):
        """Views of the first T history rows: (coords [G,T,N,2] pixels, vis logits [G,T,N], conf logits [G,T,N])."""
        if self.ring_rows is not None:
            raise RuntimeError("a ring history has no view of a range of frames (it may wrap): use emit()")
        return tuple(h_[:, :T] for h_ in self.hist)

    def frame_rows(self, f0: int, f1: int) -> List[slice]:
        """The history rows of frames [f0, f1) as slices in frame order: one, or two where a ring wraps (f1 - f0 <= T_cap)."""
        if self.ring_rows is None:
            return [slice(f0, f1)]
        R = self.ring_rows
        assert 0 <= f1 - f0 <= R
        r0, r1 = f0 % R, f0 % R + (f1 - f0)
        return [slice(r0, r1)] if r1 <= R else [slice(r0, R), slice(0, r1 - R)]

    # -- readers of the history: emit, health, draw and the fit readers.  What they share is stated here, once: whom a call reads
    # (_reader), which frames it may read (_held: history_span) and the source fields of its args (_bind_history).  emit, health and
    # draw hold their own options, struct fields and launch; a fit reader is _HistorySource and the body it shares with its tensor form.
    def _reader(self, who: str, N_out, group, first_row, points_max: Optional[int] = None, need_row: bool = False):
        """Whom a reader reads -> (N_out, g0, G): the first N_out points (default: all N; at most points_max) of the G groups from g0
        on (`group` alone, or None: all), and first_row checked as what emit takes: int32 [self.G, self.N] on the device, or None."""
        N_out = self.N if N_out is None else int(N_out)
        top = self.N if points_max is None else min(self.N, points_max)
        if not 1 <= N_out <= top:
            raise ValueError(f"{who}: N_out must lie in [1, {top}]")
        g0, G = (0, self.G) if group is None else (int(group), 1)
        if not 0 <= g0 < self.G:
            raise ValueError(f"{who}: group must lie in [0, {self.G})")
        dev = self.queries.device
        if (first_row is not None or need_row) and not (isinstance(first_row, torch.Tensor) and first_row.dtype == torch.int32 and
                                                        tuple(first_row.shape) == (self.G, self.N) and first_row.device == dev and
                                                        first_row.is_contiguous()):
            raise ValueError(f"{who}: first_row must be a contiguous int32 tensor [{self.G},{self.N}] on {dev}")
        return N_out, g0, G

    def _held(self, who: str, f0: int, F: int, *, back: int = 0, fwd: int = 0, to: int = -1, hint: str = "") -> None:
        """ValueError unless the history still holds every frame a call for [f0, f0 + F) reads (back, fwd, to: history_span's); hint:
        what to do about a call that spans too many rows."""
        bad = history_span(self.committed, self.T_cap, self.ring_rows is not None, f0, F, back, fwd, to)
        if bad is None:
            return
        kind, lo, hi = bad
        if kind == "beyond":
            raise ValueError(f"{who}: frames [{lo}, {hi + 1}) lie beyond what has been tracked ({self.committed} frames)")
        if kind == "left":
            pin = " (pin the source frame while it is there)" if to >= 0 else ""
            raise ValueError(f"{who}: frames [{lo}, {hi + 1}) have left the history: it holds the last {self.T_cap} of {self.committed} "
                             f"frames{pin}")
        raise ValueError(f"{who}: frames [{lo}, {hi + 1}) need more than the {self.T_cap} history rows one call may span{hint}")

    def _bind_history(self, a, g0: int, G: int, N_out: int, f0: int, F: Optional[int], scale, thresh: float, first_row) -> None:
        """The source fields of a reader's args: the history and logits of the groups from g0 on (F None: the args have no F)."""
        a.G, a.N, a.N_out, a.R, a.f0 = G, self.N, N_out, self.T_cap, f0
        if F is not None:
            a.F = F
        a.sx, a.sy, a.thresh = float(scale[0]), float(scale[1]), float(thresh)
        a.hist_coords, a.hist_vis, a.hist_conf = [_ptr_at(h_, g0) for h_ in self.hist]
        a.visible = None
        a.first_row = None if first_row is None else _ptr_at(first_row, g0)

    def emit(self, f0: int, f1: int, N_out: Optional[int] = None, scale=(1.0, 1.0), logits: bool = True, thresh: Optional[float] = None,
             first_row: Optional[torch.Tensor] = None):
        """History frames [f0, f1) of the first N_out points of every group, copied out in frame order by ONE launch
        (ctk_stream_emit): tracks [G,f1-f0,N_out,2] = history coords * scale (one float32 multiplication; (1, 1): a copy), then the
        two logit tensors [G,f1-f0,N_out] if `logits`, then -- `thresh` given -- visibility (bool) = sigmoid(vis) * sigmoid(conf) >
        thresh, ANDed with frame >= first_row[g, n] (int32 [G,N] on the device, INT32_MAX: an empty slot) when that is given.  The
        frames must be among the last T_cap committed ones (a ring keeps no more).  Returns the tuple of what was asked for."""
        if history_span(self.committed, self.T_cap, self.ring_rows is not None, f0, f1 - f0) is not None:
            raise ValueError(f"emit: frames [{f0}, {f1}) are not among the {min(self.committed, self.T_cap)} frames the history holds "
                             f"(it ends at frame {self.committed})")
        if thresh is None:
            first_row = None  # (it gates the visibility only)
        N_out, _, _ = self._reader("emit", N_out, None, first_row)
        dev, F_ = self.queries.device, f1 - f0
        a = L.StreamEmit.Args()
        a.G, a.N, a.N_out, a.R, a.f0, a.f1 = self.G, self.N, N_out, self.T_cap, f0, f1
        a.sx, a.sy, a.thresh, a.reserved = float(scale[0]), float(scale[1]), 0.0 if thresh is None else float(thresh), 0
        a.hist_coords, a.hist_vis, a.hist_conf = (_ptr(h_) for h_ in self.hist)
        out = [torch.empty(self.G, F_, N_out, 2, device=dev)]
        a.tracks = _ptr(out[0])
        if logits:
            out += [torch.empty(self.G, F_, N_out, device=dev), torch.empty(self.G, F_, N_out, device=dev)]
            a.vis_logit, a.conf_logit = _ptr(out[1]), _ptr(out[2])
        if thresh is not None:
            out.append(torch.empty(self.G, F_, N_out, device=dev, dtype=torch.bool))  # (one byte per element, written as 0 / 1)
            a.visible, a.first_row = _ptr(out[-1]), _ptr(first_row)
        L.check(L.load().ctk_stream_emit(C.byref(a), _stream()), "ctk_stream_emit")
        return tuple(out)

    HEALTH_CELLS_MAX = 4096  # (csrc/stream.hip: the cover of a group is counted in LDS)

    def health(self, look: int, grid, thresh: float, N_out: Optional[int], first_row: torch.Tensor, bounds):
        """The slots of every group judged over the last `look` committed frames by ONE launch (ctk_stream_health; include/ctk.h
        has the rules): -> (lost [G,N_out] int32: frames lost, newest first, -1 for an empty slot and 0 for one whose occupant has
        not been tracked yet; cell [G,N_out] int32: the slot's cell cy * gw + cx of the grid = (gh, gw) laid over bounds = (x_lo,
        x_hi, y_lo, y_hi), model-resolution pixels, inclusive, or -1; cover [G,gh*gw] int32: slots per cell).  alive is emit's
        sigmoid(vis) * sigmoid(conf) > thresh inside the bounds.  first_row: int32 [G,N] on the device, INT32_MAX for an empty slot
        (what emit takes).  f1 = committed, ind_next = next_ind.  The three results are views of ONE allocation, in this order
        (``lost._base``: one copy brings all of them to the host).  No wait."""
        gh, gw = (int(v) for v in grid)
        look = int(look)
        dev = self.queries.device
        if self.committed <= 0:
            raise ValueError("health: no frame has been committed yet")
        if not 1 <= look <= min(self.T_cap, self.committed):
            raise ValueError(f"health: look must lie in [1, {min(self.T_cap, self.committed)}] (frames so far: {self.committed}, history "
                             f"rows: {self.T_cap})")
        N_out, _, _ = self._reader("health", N_out, None, first_row, need_row=True)
        if gh < 1 or gw < 1 or gh * gw > self.HEALTH_CELLS_MAX:
            raise ValueError(f"health: the grid must have between 1 and {self.HEALTH_CELLS_MAX} cells, got {gh} x {gw}")
        a = L.StreamHealth.Args()
        a.G, a.N, a.N_out, a.R, a.f1, a.look, a.ind_next = self.G, self.N, N_out, self.T_cap, self.committed, look, self.next_ind
        a.thresh, a.reserved, a.gh, a.gw = float(thresh), 0, gh, gw
        a.x_lo, a.x_hi, a.y_lo, a.y_hi = (float(v) for v in bounds)
        if not (a.x_hi > a.x_lo and a.y_hi > a.y_lo):
            raise ValueError(f"health: empty bounds {tuple(bounds)}")
        # float32 operands, float32 quotient (the struct fields hold the float32 bounds the kernel compares with)
        a.inv_cw, a.inv_ch = (float(torch.tensor(float(n_), dtype=torch.float32) / (torch.tensor(hi, dtype=torch.float32) -
                                                                                   torch.tensor(lo, dtype=torch.float32)))
                              for n_, lo, hi in ((gw, a.x_lo, a.x_hi), (gh, a.y_lo, a.y_hi)))
        a.queries = _ptr(self.queries)
        a.hist_coords, a.hist_vis, a.hist_conf = (_ptr(h_) for h_ in self.hist)
        a.first_row = _ptr(first_row)
        k = self.G * N_out
        flat = torch.empty(2 * k + self.G * gh * gw, device=dev, dtype=torch.int32)
        lost, cell, cover = flat[:k].view(self.G, N_out), flat[k:2 * k].view(self.G, N_out), flat[2 * k:].view(self.G, gh * gw)
        a.lost, a.cell, a.cover = _ptr(lost), _ptr(cell), _ptr(cover)
        L.check(L.load().ctk_stream_health(C.byref(a), _stream()), "ctk_stream_health")
        return lost, cell, cover

    def draw(self, frames: torch.Tensor, f0: int, colors: torch.Tensor, *, N_out: Optional[int] = None, scale=(1.0, 1.0),
             thresh: float = 0.6, first_row: Optional[torch.Tensor] = None, trail: int = 8, radius: int = 4, half_width: int = 1,
             alpha=None, max_jump: int = 256, out: Optional[torch.Tensor] = None, layout: Optional[str] = None,
             group: Optional[int] = None) -> torch.Tensor:
        """The first N_out points of every group (or of `group` alone) drawn onto uint8 frames straight from the stream's own
        history and logits -- no emit in between --, by the two launches of ctk_draw_tracks (draw_tracks has the picture): picture j
        of `frames` shows frame f0 + j, visibility is emit's sigmoid(vis) * sigmoid(conf) > thresh, positions are history coords *
        scale (emit's multiplication).  colors uint8 [G,N,3] and first_row int32 [G,N] (what emit takes) on the device, over all N
        slots.  The frames f0 - trail .. f0 + F - 1 (those >= 0) must be among the committed ones the history still holds:
        ValueError otherwise.  No wait."""
        who = "draw"
        N_out, g0, G = self._reader(who, N_out, group, first_row)
        if not (isinstance(frames, torch.Tensor) and frames.dim() == 4):
            raise ValueError(f"{who}: frames must be a uint8 device tensor [F,H,W,3] or [F,3,H,W]")
        dev = self.queries.device
        if not (isinstance(colors, torch.Tensor) and colors.dtype == torch.uint8 and tuple(colors.shape) == (self.G, self.N, 3) and
                colors.device == dev and colors.is_contiguous()):
            raise ValueError(f"{who}: colors must be a contiguous uint8 tensor [{self.G},{self.N},3] on {dev}")
        a = L.Draw.Args()
        _draw_style(a, trail, radius, half_width, alpha, max_jump, who)
        f0 = int(f0)
        self._held(who, f0, frames.shape[0], back=a.trail, hint=": draw fewer frames per call")
        self._bind_history(a, g0, G, N_out, f0, None, scale, thresh, first_row)  # (_draw_launch has the F of the surface)
        a.colors = _ptr_at(colors, g0)
        return _draw_launch(a, frames, out, layout, who)

    def motion(self, f0: int, F: int, *, N_out: Optional[int] = None, scale=(1.0, 1.0), thresh: float = 0.6,
               first_row: Optional[torch.Tensor] = None, lag: int = 1, model: str = "similarity", tol: float = 2.0, hypotheses: int = 128,
               min_base: float = 16.0, seed: int = 0, group: Optional[int] = None, out=None):
        """The camera motion of frames f0 .. f0 + F - 1 (each against the frame `lag` before it) fitted to the first N_out points of
        every group (or of `group` alone) straight from the stream's own history and logits -- no emit in between --, by the one
        launch of ctk_fit_motion (fit_motion has the picture): visibility is emit's sigmoid(vis) * sigmoid(conf) > thresh, positions
        are history coords * scale (emit's multiplication), tol and min_base are in those pixels.  first_row int32 [G,N] (what emit
        takes) on the device.  The frames f0 - lag .. f0 + F - 1 (those >= 0) must be among the committed ones the history still
        holds: ValueError otherwise.  -> (motion [G,F,2,3], inlier [G,F,N_out], stats [G,F,4]) on the device.  No wait."""
        src = _HistorySource(self, "motion", f0, F, N_out, group, first_row, scale, thresh)
        return _motion_fit(src, lag, model, tol, hypotheses, min_base, seed, out)

    def stabilize(self, frames: torch.Tensor, f0: int, *, group: int = 0, reset: bool = False, alpha: float = 0.1, zoom: float = 1.0,
                  border: str = "fill", fill=(0, 0, 0), out: Optional[torch.Tensor] = None, layout: Optional[str] = None,
                  N_out: Optional[int] = None, scale=(1.0, 1.0), thresh: float = 0.6, first_row: Optional[torch.Tensor] = None,
                  model: str = "similarity", tol: float = 2.0, hypotheses: int = 128, min_base: float = 16.0, seed: int = 0):
        """uint8 `frames` (picture j shows frame f0 + j) steadied by the camera motion of `group`, straight from the stream's own
        history and logits: self.motion(lag = 1), smooth_path, warp_frames -- three launches, no wait (ops.stabilize has the
        picture).  The path state is kept here, one per group: the first call for a group, or reset=True, locks onto frame f0 (its
        matrix is the identity, or the zoom alone: the motion from frame f0 - 1 into it is not part of the path); any other call must
        go on where the last one ended (f0 = its f0 + F) with the same alpha: ValueError otherwise.  restart() drops the states.  Range errors are those of motion().  -> (out, warp float32 [F,2,3]) on the device."""
        who = "stabilize"
        if not (isinstance(frames, torch.Tensor) and frames.dim() == 4):
            raise ValueError(f"{who}: frames must be a uint8 device tensor [F,H,W,3] or [F,3,H,W]")
        f0, F_, group, alpha = int(f0), frames.shape[0], int(group), float(alpha)
        if not 0 <= group < self.G:
            raise ValueError(f"{who}: group must lie in [0, {self.G})")
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"{who}: alpha must lie in [0, 1], got {alpha!r}")
        if self._stab is None:
            self._stab = {}
        held = None if reset else self._stab.get(group)
        if held is not None and (held[0] != f0 or held[2] != alpha):
            raise ValueError(f"{who}: group {group} has been steadied up to frame {held[0]} with alpha = {held[2]}; a call for frame {f0} "
                             f"with alpha = {alpha} does not go on from there: pass reset=True to lock onto frame {f0} afresh")
        a, out = _warp_args(frames, out, border, fill, layout, who)  # (everything that can be refused is, before the state moves)
        key = (a.H, a.W, float(zoom))
        if held is not None and held[3][0] == key:
            post = held[3][1]
        else:
            post = None if key[2] == 1.0 else zoom_matrix(a.H, a.W, zoom).to(frames.device)
        motion = self.motion(f0, F_, N_out=N_out, scale=scale, thresh=thresh, first_row=first_row, lag=1, model=model, tol=tol,
                             hypotheses=hypotheses, min_base=min_base, seed=seed, group=group)[0]
        if held is None:  # frame f0 is the one locked onto: the motion INTO it is not part of the path
            motion[0, 0] = 0.0
            motion[0, 0, 0, 0] = 1.0
            motion[0, 0, 1, 1] = 1.0
        state = _path_state(1, self.queries.device) if held is None else held[1]
        warp, state = smooth_path(motion, state, alpha=alpha, post=post)
        _warp_launch(a, warp, frames.device, who)
        self._stab[group] = (f0 + F_, state, alpha, (key, post))
        return out, warp[0]

    def field(self, f0: int, F: int, *, size, cell: int = 16, radius: int = 2, to: Optional[int] = None, lag: Optional[int] = None,
              anchor: Optional[FieldAnchor] = None, N_out: Optional[int] = None, scale=(1.0, 1.0), thresh: float = 0.6,
              first_row: Optional[torch.Tensor] = None, group: Optional[int] = None, out=None):
        """The displacement fields of frames f0 .. f0 + F - 1 towards a frame "to" (one of `to`, `lag`, `anchor`: track_field has the
        picture) interpolated from the first N_out points of every group (or of `group` alone) straight from the stream's own history
        and logits -- no emit in between --, by the three launches of ctk_track_field: visibility is emit's sigmoid(vis) *
        sigmoid(conf) > thresh, positions are history coords * scale, size = (H, W) is in those pixels.  first_row int32 [G,N] (what
        emit takes) on the device.  Every frame that is read (those >= 0) must be among the committed ones the history still holds:
        ValueError otherwise; an anchor needs no frame but its own copy.  -> (field [G,F,gh,gw,2], level [G,F,gh,gw], stats [G,F,4])
        on the device.  No wait."""
        src = _HistorySource(self, "field", f0, F, N_out, group, first_row, scale, thresh, L.Field.POINTS_MAX)
        return _field_fit(src, size, cell, radius, to, lag, anchor, out)

    def objects(self, f0: int, F: int, *, labels: Optional[torch.Tensor] = None, objects: int = 4, lag: int = 1, to: Optional[int] = None,
                anchor: Optional[FieldAnchor] = None, N_out: Optional[int] = None, scale=(1.0, 1.0), thresh: float = 0.6,
                first_row: Optional[torch.Tensor] = None, model: str = "similarity", tol: float = 2.0, hypotheses: int = 128,
                min_base: float = 16.0, min_points: int = 8, seed: int = 0, group: Optional[int] = None):
        """Up to `objects` fits per frame f0 .. f0 + F - 1 over the first N_out points of every group (or of `group` alone), each frame
        against a source frame (f - lag, a fixed `to`, or an `anchor`: fit_objects has the picture), straight from the stream's own
        history and logits -- no emit in between --, by the one launch of ctk_fit_objects: visibility is emit's sigmoid(vis) *
        sigmoid(conf) > thresh, positions are history coords * scale, tol and min_base are in those pixels.  labels int8 [G,N] (of
        the groups asked for) on the device: labels mode; None: split mode.  first_row int32 [G,N] (what emit takes) on the device.
        Every frame that is read (those >= 0) must be among the committed ones the history still holds: ValueError otherwise; an anchor
        needs no frame but its own copy.  -> (motion [G,F,objects,2,3], label [G,F,N_out], stats [G,F,objects,4], box
        [G,F,objects,4]) on the device.  No wait."""
        src = _HistorySource(self, "objects", f0, F, N_out, group, first_row, scale, thresh)
        return _objects_fit(src, labels, objects, lag, to, anchor, model, tol, hypotheses, min_base, min_points, seed)

    def planes(self, f0: int, F: int, *, labels: Optional[torch.Tensor] = None, planes: int = 1, lag: int = 1, to: Optional[int] = None,
               anchor: Optional[FieldAnchor] = None, inverse: bool = False, N_out: Optional[int] = None, scale=(1.0, 1.0),
               thresh: float = 0.6, first_row: Optional[torch.Tensor] = None, tol: float = 2.0, hypotheses: int = 128,
               min_base: float = 16.0, min_points: int = 8, seed: int = 0, group: Optional[int] = None):
        """Up to `planes` homography fits per frame f0 .. f0 + F - 1 over the first N_out points of every group (or of `group` alone),
        each frame against a source frame (f - lag, a fixed `to`, or an `anchor`: fit_planes has the picture), straight from the
        stream's own history and logits -- no emit in between --, by the one launch of ctk_fit_planes: visibility is emit's sigmoid(vis)
        * sigmoid(conf) > thresh, positions are history coords * scale, tol and min_base are in those pixels.  labels int8 [G,N] (of the
        groups asked for) on the device, or None: one plane of all points.  first_row int32 [G,N] (what emit takes) on the device.
        Every frame that is read (those >= 0) must be among the committed ones the history still holds: ValueError otherwise; an anchor
        needs no frame but its own copy.  -> (homography [G,F,planes,3,3], label [G,F,N_out], stats [G,F,planes,4], box
        [G,F,planes,4]) on the device.  No wait."""
        src = _HistorySource(self, "planes", f0, F, N_out, group, first_row, scale, thresh)
        return _planes_fit(src, labels, planes, lag, to, anchor, inverse, tol, hypotheses, min_base, min_points, seed)

    def epipolar(self, f0: int, F: int, *, mask: Optional[torch.Tensor] = None, lag: int = 1, to: Optional[int] = None,
                 anchor: Optional[FieldAnchor] = None, N_out: Optional[int] = None, scale=(1.0, 1.0), thresh: float = 0.6,
                 first_row: Optional[torch.Tensor] = None, tol: float = 1.0, hypotheses: int = 512, min_base: float = 16.0,
                 min_points: int = 16, seed: int = 0, group: Optional[int] = None, out=None):
        """One fundamental matrix per frame f0 .. f0 + F - 1 over the first N_out points of every group (or of `group` alone), each
        frame against a source frame (f - lag, a fixed `to`, or an `anchor`: fit_epipolar has the picture), straight from the stream's
        own history and logits -- no emit in between --, by the one launch of ctk_fit_epipolar: visibility is emit's sigmoid(vis) *
        sigmoid(conf) > thresh, positions are history coords * scale, tol and min_base are in those pixels.  mask int8 / uint8 / bool
        [G,N] (of the groups asked for) on the device, or None: every point may be fitted on.  first_row int32 [G,N] (what emit takes) on
        the device.  Every frame that is read (those >= 0) must be among the committed ones the history still holds: ValueError
        otherwise; an anchor needs no frame but its own copy.  -> (fundamental [G,F,3,3], label [G,F,N_out], error [G,F,N_out], stats
        [G,F,4]) on the device.  No wait."""
        src = _HistorySource(self, "epipolar", f0, F, N_out, group, first_row, scale, thresh)
        return _epipolar_fit(src, mask, lag, to, anchor, tol, hypotheses, min_base, min_points, seed, out)

    def pose(self, f0: int, F: int, intrinsics, fundamental: torch.Tensor, label: torch.Tensor, *, mask: Optional[torch.Tensor] = None,
             lag: int = 1, to: Optional[int] = None, anchor: Optional[FieldAnchor] = None, N_out: Optional[int] = None,
             scale=(1.0, 1.0), thresh: float = 0.6, first_row: Optional[torch.Tensor] = None, min_points: int = 8,
             group: Optional[int] = None, out=None):
        """One camera pose per frame f0 .. f0 + F - 1 and two depths per point over the first N_out points of every group (or of `group`
        alone), from what epipolar() returned for the same frames, source form, N_out, scale, thresh, first_row and group
        (fundamental [G,F,3,3], label [G,F,N_out]; only read) and the intrinsics (fx, fy, cx, cy: four Python floats, in the pixels of
        history coords * scale), straight from the stream's own history and logits by the one launch of ctk_fit_pose: fit_pose has the
        picture.  mask int8 / uint8 / bool [G,N] (of the groups asked for) on the device, or None.  Every frame that is read (those
        >= 0) must be among the committed ones the history still holds: ValueError otherwise.  -> (pose [G,F,3,4], depth
        [G,F,N_out,2], stats [G,F,4]) on the device.  No wait."""
        src = _HistorySource(self, "pose", f0, F, N_out, group, first_row, scale, thresh)
        return _pose_fit(src, intrinsics, fundamental, label, mask, lag, to, anchor, min_points, out)

    def focal(self, f0: int, F: int, fundamental: torch.Tensor, label: torch.Tensor, *, focals=None, size=None, candidates: int = 64,
              span=(0.25, 4.0), principal=None, mask: Optional[torch.Tensor] = None, lag: int = 1, to: Optional[int] = None,
              anchor: Optional[FieldAnchor] = None, N_out: Optional[int] = None, scale=(1.0, 1.0), thresh: float = 0.6,
              first_row: Optional[torch.Tensor] = None, tol: float = 1.0, min_points: int = 16, min_frames: int = 1,
              contrast: float = 1.5, curve: Optional[torch.Tensor] = None, group: Optional[int] = None, out=None):
        """The focal length of the camera from the frames f0 .. f0 + F - 1 over the first N_out points of every group (or of `group`
        alone), from what epipolar() returned for the same frames, source form, N_out, scale, thresh, first_row and group (fundamental
        [G,F,3,3], label [G,F,N_out]; only read), straight from the stream's own history and logits by the two launches of
        ctk_fit_focal: fit_focal has the picture, the candidates (focals / size, candidates, span), the principal point (in the pixels
        of history coords * scale; None: the centre of `size`), the contrast rule and `curve`, the running sum an earlier call
        returned.  Every frame that is read (those >= 0) must be among the committed ones the history still holds: ValueError
        otherwise.  -> (focal [G], curve [G,K+2], cost [G,F,K], stats [G,4], focals [K]) on the device.  No wait."""
        src = _HistorySource(self, "focal", f0, F, N_out, group, first_row, scale, thresh)
        return _focal_fit(src, fundamental, label, focals, size, candidates, span, principal, mask, lag, to, anchor, tol, min_points,
                          min_frames, contrast, curve, out)

    def resection(self, f0: int, F: int, intrinsics, structure: torch.Tensor, valid: torch.Tensor, seed_pose: torch.Tensor, *,
                  lag: int = 1, to: Optional[int] = None, anchor: Optional[FieldAnchor] = None, N_out: Optional[int] = None,
                  scale=(1.0, 1.0), thresh: float = 0.6, first_row: Optional[torch.Tensor] = None, tol: float = 2.0, hypotheses: int = 256,
                  min_points: int = 16, seed: int = 0, group: Optional[int] = None, out=None):
        """One camera pose per frame f0 .. f0 + F - 1 against a 3-D structure (structure float32 [G,N,3] in the source camera's
        coordinates, valid int8 / uint8 / bool [G,N], of the groups asked for; only read), started from seed_pose float32 [G,F,3,4]
        (pose()'s for the same frames and source form; only read), over the first N_out points of every group (or of `group` alone),
        straight from the stream's own history and logits by the one launch of ctk_fit_resection: fit_resection has the picture.
        intrinsics: (fx, fy, cx, cy), four Python floats, in the pixels of history coords * scale.  Every frame that is read (those
        >= 0) must be among the committed ones the history still holds: ValueError otherwise.  -> (pose [G,F,3,4], label
        [G,F,N_out], error [G,F,N_out], stats [G,F,4]) on the device.  No wait."""
        src = _HistorySource(self, "resection", f0, F, N_out, group, first_row, scale, thresh)
        return _resection_fit(src, intrinsics, structure, valid, seed_pose, lag, to, anchor, tol, hypotheses, min_points, seed, out)

    def p3p(self, f0: int, F: int, intrinsics, structure: torch.Tensor, valid: torch.Tensor, *, lag: int = 1, to: Optional[int] = None,
            anchor: Optional[FieldAnchor] = None, N_out: Optional[int] = None, scale=(1.0, 1.0), thresh: float = 0.6,
            first_row: Optional[torch.Tensor] = None, tol: float = 2.0, hypotheses: int = 256, min_points: int = 16, seed: int = 0,
            group: Optional[int] = None, out=None):
        """One camera pose per frame f0 .. f0 + F - 1 against a 3-D structure (structure float32 [G,N,3] in the source camera's
        coordinates, valid int8 / uint8 / bool [G,N], of the groups asked for; only read) WITHOUT a seed pose, over the first N_out
        points of every group (or of `group` alone), straight from the stream's own history and logits by the one launch of
        ctk_fit_p3p: fit_p3p has the picture.  intrinsics: (fx, fy, cx, cy), four Python floats, in the pixels of history coords *
        scale.  Every frame that is read (those >= 0) must be among the committed ones the history still holds: ValueError
        otherwise.  -> (pose [G,F,3,4], label [G,F,N_out], error [G,F,N_out], stats [G,F,4]) on the device.  No wait."""
        src = _HistorySource(self, "p3p", f0, F, N_out, group, first_row, scale, thresh)
        return _resection_fit(src, intrinsics, structure, valid, None, lag, to, anchor, tol, hypotheses, min_points, seed, out, kind="p3p")

    def align(self, a: torch.Tensor, valid_a: torch.Tensor, b: torch.Tensor, valid_b: torch.Tensor, intrinsics, *,
              mask: Optional[torch.Tensor] = None, tol: float = 2.0, depth_tol: float = 0.1, hypotheses: int = 256, min_points: int = 8,
              seed: int = 0, out=None):
        """The similarity b ~ s R a + t between two point sets over this stream's slots (a, b float32 [G,N,3] / [N,3] with their
        validity bytes [G,N] / [N], N the stream's slots per group, on the stream's device; only read) by the one launch of
        ctk_fit_align: fit_align has the picture.  The call reads no history, so no frame has to be held by the ring; nothing of the
        stream is touched.  -> (sim [G,3,4], scale [G], label [G,N], error [G,N], stats [G,4]) on the device.  No wait."""
        if not (isinstance(a, torch.Tensor) and a.device == self.coords.device and a.shape[-2:] == (self.N, 3)):
            raise ValueError(f"align: a must be a float32 tensor [{self.N},3] or [G,{self.N},3] on {self.coords.device}")
        return _align_fit(a, valid_a, b, valid_b, intrinsics, mask, tol, depth_tol, hypotheses, min_points, seed, out, "align")

    def structure(self, f0: int, F: int, intrinsics, pose: torch.Tensor, *, pose_stats: Optional[torch.Tensor] = None,
                  structure: Optional[torch.Tensor] = None, valid: Optional[torch.Tensor] = None, source_frame: int = 0,
                  origin: Optional[torch.Tensor] = None, into: Optional[int] = None, N_out: Optional[int] = None, scale=(1.0, 1.0),
                  thresh: float = 0.6, first_row: Optional[torch.Tensor] = None, tol: float = 2.0, min_views: int = 3,
                  min_parallax: float = 1.0, refine: bool = False, group: Optional[int] = None, out=None):
        """One 3-D point per slot from the frames f0 .. f0 + F - 1 (F <= 256 views) under pose float32 [G,F,3,4] and pose_stats int32
        [G,F,4] (resection()'s for the same frames; only read), over the first N_out points of every group (or of `group` alone),
        straight from the stream's own history and logits by the one launch of ctk_fit_structure: fit_structure has the picture.
        structure float32 [G,N,3], valid int8 / uint8 / bool [G,N] and origin float32 [G,3,4] (of the groups asked for; only read) are
        the old structure, stated in frame source_frame; into: a view 0 .. F - 1 or None.  intrinsics: (fx, fy, cx, cy), four Python
        floats, in the pixels of history coords * scale.  Every frame that is read must be among the committed ones the history still
        holds: ValueError otherwise.  -> (points [G,N_out,3], label [G,N_out], error [G,N_out], stats [G,N_out,4], origin [G,3,4]) on
        the device.  No wait."""
        src = _HistorySource(self, "structure", f0, F, N_out, group, first_row, scale, thresh, L.Structure3D.POINTS_MAX)
        return _structure_fit(src, intrinsics, pose, pose_stats, structure, valid, source_frame, origin, into, tol, min_views, min_parallax,
                              refine, out)

    def _args(self, ind: int, T_valid: int = 0, flag: bool = False) -> "L.StreamArgs":
        a = L.StreamArgs()
        a.G, a.N, a.S, a.step, a.ind, a.T_valid, a.T_cap, a.stride = self.G, self.N, self.S, self.step, ind, T_valid, self.T_cap, self.stride
        a.queries = _ptr(self.queries)
        a.hist_coords, a.hist_vis, a.hist_conf = (_ptr(h_) for h_ in self.hist)
        a.coords, a.vis, a.conf, a.point_mask = _ptr(self.coords), _ptr(self.vis), _ptr(self.conf), _ptr(self.mask)
        for l, f_ in enumerate(self.pyr):
            a.H[l], a.W[l], a.fmaps[l], a.support[l] = f_.shape[1], f_.shape[2], _ptr(f_), _ptr(self.support[l])
        a.nonfinite = _ptr(self.nonfinite) if flag else None
        return a

    def set_pyramid(self, f0: torch.Tensor) -> None:
        """Level-0 features [T <= S, H, W, 128] of this call's chunk into the resident pyramid: the last frame repeated up to S
        frames (cotracker3_online.py:321-328 pads the video; the encoder is per frame), then the pooled levels."""
        T = f0.shape[0]
        self.pyr[0][:T].copy_(f0)
        if T < self.S:
            self.pyr[0][T:].copy_(f0[-1:].expand(self.S - T, -1, -1, -1))
        for l in range(1, len(self.pyr)):
            avg_pool2_nhwc(self.pyr[l - 1], out=self.pyr[l])

    def advance_pyramid(self, f_new: torch.Tensor, T_valid: int) -> None:
        """The counterpart of set_pyramid for a stream that keeps its overlap: this call's window is the previous one advanced by
        `step` frames, so on every level rows [step, S) move to [0, S - step) (the halves do not overlap: step == S // 2), the
        level-0 features f_new [n <= step, H, W, 128] of the NEW frames land behind them, the last of them repeated up to S rows
        when the chunk is short (T_valid = S - step + n < S, as set_pyramid pads), and the pooled levels are computed for rows
        [S - step, S) only.  The pooling is per frame, so every row holds the bits set_pyramid would have put there.  No address
        changes: captured graphs and ``serial`` are untouched."""
        S, step = self.S, self.step
        ov = S - step
        assert 2 * step == S and ov == step, "advance_pyramid: the window halves must not overlap (step == window_len // 2)"
        n = f_new.shape[0]
        assert 1 <= n <= step and T_valid == ov + n, (n, T_valid)
        for p_ in self.pyr:
            p_[:ov].copy_(p_[step:])
        self.pyr[0][ov:ov + n].copy_(f_new)
        if n < step:
            self.pyr[0][ov + n:].copy_(f_new[-1:].expand(step - n, -1, -1, -1))
        for l in range(1, len(self.pyr)):
            avg_pool2_nhwc(self.pyr[l - 1][ov:], out=self.pyr[l][ov:])

    def begin(self, ind: int) -> None:
        self.reserve(ind + self.S)
        name = "ctk_stream_begin" if self.ring_rows is None else "ctk_stream_begin_ring"
        L.check(getattr(L.load(), name)(C.byref(self._args(ind)), _stream()), name)

    def sample_support(self, ind: int) -> None:
        self.reserve(ind + self.S)
        name = "ctk_stream_support" if self.ring_rows is None else "ctk_stream_support_ring"
        L.check(getattr(L.load(), name)(C.byref(self._args(ind)), _stream()), name)

    def commit(self, ind: int, T_valid: int, flag: bool) -> None:
        name = "ctk_stream_commit" if self.ring_rows is None else "ctk_stream_commit_ring"
        L.check(getattr(L.load(), name)(C.byref(self._args(ind, T_valid, flag)), _stream()), name)
        self.committed, self.next_ind = ind + T_valid, ind + self.step

    @property
    def resident_frames(self):
        """(first, last + 1) of the frames the resident pyramid holds between two calls: the window just tracked, [next_ind - step,
        next_ind - step + S).  None before the first call of a stream."""
        if self.next_ind < self.step:
            return None
        return (self.next_ind - self.step, self.next_ind - self.step + self.S)

    def assign(self, slots, queries: torch.Tensor, rows: Optional[int] = None, min_frame: Optional[int] = None,
               resident: bool = False) -> None:
        """Between two calls: slot slots[m] (flat index g*N + n) gets the query queries[m] = (frame, x, y) in model-resolution
        pixels, its support accumulators and its history rows [0, rows) are cleared (rows: default every row committed so far; a ring:
        all its rows, always), and
        the bookkeeping follows (first_row = next_ind).  One launch (ctk_stream_assign); the slot list reaches the device with one
        non-blocking copy, and so do queries given on the host.  The frame column is checked HERE, on the host -- for queries on
        the device that is one small device-to-host copy; the positions never leave the device --: a frame that is not finite, or
        whose integer part lies below `min_frame` (the caller's rule: the first frame no support call has handed out yet), raises
        ValueError, like a slot out of range, a slot listed twice or a wrong shape; nothing is written then.  Touches neither
        ``serial`` nor the windows, the pyramid or any buffer address.

        resident=True (ctk_stream_assign_resident, still one launch): query frames of the window just tracked are admitted too --
        trunc(frame) >= next_ind - step, the first frame of the resident pyramid; this rule is checked here whatever the caller's
        `min_frame` says (which still applies when given).  Such a slot gets its support patch sampled from the resident pyramid
        (the bits ctk_stream_support would have added) and, instead of zeros, (x, y) with zero logits in the history rows of frames
        [next_ind, next_ind + S - step), from which the next begin starts it as a fresh point; later frames are assigned as
        without the keyword.  Needs a tracked window (next_ind >= step) and a stream no short chunk has closed: RuntimeError.
        The linear history is reserved up to next_ind + S first, as the next begin would do: it may grow (new history addresses;
        no address a captured graph has baked in changes -- the history lies outside the graphs)."""
        if resident:
            if self.closed:
                raise RuntimeError("assign: a chunk shorter than the window has ended the stream")
            if self.next_ind < self.step:
                raise RuntimeError("assign: resident=True needs a tracked window: no call of this stream has been made yet")
        idx = torch.as_tensor(slots).detach().cpu().reshape(-1)
        M = idx.numel()
        if M == 0 or idx.dtype.is_floating_point or idx.dtype.is_complex or idx.dtype == torch.bool:
            raise ValueError("assign: slots must be a non-empty list of integer slot indices g*N + n")
        idx = idx.long()
        if int(idx.min()) < 0 or int(idx.max()) >= self.G * self.N:
            raise ValueError(f"assign: slot index outside [0, {self.G * self.N})")
        if torch.unique(idx).numel() != M:
            raise ValueError("assign: a slot is listed twice")
        if not isinstance(queries, torch.Tensor) or tuple(queries.shape) != (M, 3) or not queries.dtype.is_floating_point:
            raise ValueError(f"assign: queries must be a float tensor [{M},3] = (frame, x, y), one row per listed slot")
        ring = getattr(self, "ring_rows", None) is not None
        rows = (self.T_cap if ring else self.committed) if rows is None else int(rows)
        if not 0 <= rows <= self.T_cap:
            raise ValueError(f"assign: rows must lie in [0, {self.T_cap}]")
        dev = self.queries.device
        frames = queries[:, 0].detach().float().cpu()
        if not bool((torch.isfinite(frames) & (frames <= EMPTY_FRAME)).all()):
            raise ValueError("assign: a query frame is not finite (or lies beyond EMPTY_FRAME)")
        if min_frame is not None and int(frames.long().min()) < min_frame:
            raise ValueError(f"assign: query frame {int(frames.long().min())} lies before frame {min_frame}: its features have left "
                             "the stream")
        if resident and int(frames.long().min()) < self.next_ind - self.step:
            raise ValueError(f"assign: query frame {int(frames.long().min())} lies before frame {self.next_ind - self.step}, the first "
                             f"the resident pyramid holds (frames [{self.next_ind - self.step}, {self.next_ind - self.step + self.S}) "
                             "and later ones are admitted)")
        if queries.device == dev:
            q = queries.detach().float().contiguous()
        else:
            q = queries.detach().float().contiguous().pin_memory().to(dev, non_blocking=True)
        s32 = idx.to(torch.int32).pin_memory().to(dev, non_blocking=True)
        _ = self.occupied  # (the bookkeeping is read from the table BEFORE this assign changes it)
        if resident:  # ind = next_ind: the pyramid's first frame is next_ind - step, the carry rows start at next_ind
            self.reserve(self.next_ind + self.S)  # (what the next begin reserves: the carry rows lie inside the buffer)
            name = "ctk_stream_assign_resident_ring" if ring else "ctk_stream_assign_resident"
            L.check(getattr(L.load(), name)(C.byref(self._args(self.next_ind)), _ptr(s32), _ptr(q), M, *(() if ring else (rows,)),
                                            _stream()), name)
        elif not ring:
            L.check(L.load().ctk_stream_assign(C.byref(self._args(0)), _ptr(s32), _ptr(q), M, rows, _stream()), "ctk_stream_assign")
        else:  # every row of the ring, whatever `rows` says: after a wrap a slot's rows hold frames of any age
            L.check(L.load().ctk_stream_assign_ring(C.byref(self._args(0)), _ptr(s32), _ptr(q), M, _stream()), "ctk_stream_assign_ring")
        self._occupied.view(-1)[idx] = frames != EMPTY_FRAME
        self.first_row.view(-1)[idx] = self.next_ind

    def release(self, slots) -> None:
        """Empty the listed slots: assign of (EMPTY_FRAME, 0, 0).  No frame rule."""
        self.assign(slots, torch.tensor([[EMPTY_FRAME, 0.0, 0.0]]).expand(torch.as_tensor(slots).numel(), 3))

    def windows(self, g0: int, g1: int, scale_xy, **window_kw) -> List[Window]:
        """The windows of groups g0 .. g1-1 on the resident buffers (slices of one allocation each: WindowBatch(shared=True)).
        Cached: a captured graph keeps the very Window objects it was captured on."""
        key = (g0, g1, tuple(scale_xy), tuple(sorted(window_kw.items())))
        if key not in self._wins:
            N = self.N
            self._wins[key] = group_windows(self.pyr, [s_[g0 * N:g1 * N] for s_ in self.support], self.coords[g0:g1], self.vis[g0:g1],
                                            self.conf[g0:g1], scale_xy, point_mask=self.mask[g0:g1], use_aux_stream=False, **window_kw)
        return self._wins[key]

    def __getstate__(self):  # ctypes structs with raw pointers are rebuilt on demand
        return {**self.__dict__, "_wins": {}}

    def __deepcopy__(self, memo):
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = {} if k == "_wins" else copy.deepcopy(v, memo)
        StreamGroups._serial += 1
        new.serial = StreamGroups._serial  # other buffers: graphs captured on the original do not apply
        return new

    def __setstate__(self, state):
        self.__dict__.update(state)
        StreamGroups._serial += 1
        self.serial = StreamGroups._serial


def corr_volume(win: Window) -> torch.Tensor:
    out = torch.empty(L.LEVELS, win.N * win.S, L.CORR_LD, device=win.device, dtype=torch.float32)
    L.check(L.load().ctk_corr_volume(C.byref(win.args), _ptr(out), _stream()), "ctk_corr_volume")
    return out


def corr_volume_sh(win: Window) -> torch.Tensor:
    """Split-half sampler: SH volumes [4, N*S, 76, 2, 32] float16 (use unsplit on a level to compare)."""
    lib = L.load()
    out = torch.empty(L.LEVELS, win.N * win.S, L.CORR_LD // 32, 2, 32, device=win.device, dtype=torch.float16)
    ws = _workspace(_query_bytes("ctk_corr_volume_sh_workspace_bytes", C.byref(win.args)), win.device)
    L.check(lib.ctk_corr_volume_sh(C.byref(win.args), _ptr(out), _ptr(ws), ws.numel(), _stream()), "ctk_corr_volume_sh")
    return out


def corr_embed(win: Window, weights, x: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = L.load()
    if x is None:
        x = torch.zeros(win.N * win.S, L.X_LD, device=win.device, dtype=torch.float32)
    ws = _workspace(_query_bytes("ctk_corr_embed_workspace_bytes", C.byref(win.args)), win.device)
    mw = weights.struct_for(win.S)
    L.check(lib.ctk_corr_embed(C.byref(win.args), C.byref(mw), _ptr(x), _ptr(ws), ws.numel(), _stream()), "ctk_corr_embed")
    return x


def corr_embed_batch(wins: Sequence[Window], weights, points_per_chunk: Optional[int] = None, shared: bool = False) -> torch.Tensor:
    """corr_embed of a joint window (ctk_corr_embed_batch): x [B*N*S, 1120] f32, row (b*N + n)*S + t, columns [0,1024) written."""
    batch = WindowBatch(wins, points_per_chunk=points_per_chunk, shared=shared)
    x = torch.zeros(batch.B * batch.N * batch.S, L.X_LD, device=batch.device, dtype=torch.float32)
    ws = _workspace(_query_bytes("ctk_corr_embed_batch_workspace_bytes", C.byref(batch.struct)), batch.device)
    mw = weights.struct_for(batch.S)
    L.check(L.load().ctk_corr_embed_batch(C.byref(batch.struct), C.byref(mw), _ptr(x), _ptr(ws), ws.numel(), _stream()),
            "ctk_corr_embed_batch")
    return x


def window_tokens(wins: Sequence[Window], weights, points_per_chunk: Optional[int] = None, shared: bool = False,
                  folded: bool = True) -> torch.Tensor:
    """The tokens [B*N*S, 384] one iteration of the joint window call hands to the update former (ctk_window_tokens_batch): the
    correlation stage, token assembly and input projection as the window runs them -- with fc2 folded into the projection, or
    (folded=False) by the unfolded launches.  The windows' state is not changed."""
    batch = WindowBatch(wins, points_per_chunk=points_per_chunk, shared=shared)
    tokens = torch.empty(batch.B * batch.N * batch.S, L.HID, device=batch.device, dtype=torch.float32)
    ws = _workspace(batch.workspace_bytes(), batch.device)
    mw = weights.struct_for(batch.S, folded=folded)
    L.check(L.load().ctk_window_tokens_batch(C.byref(batch.struct), C.byref(mw), _ptr(tokens), _ptr(ws), ws.numel(), _stream()),
            "ctk_window_tokens_batch")
    return tokens


def assemble_tokens(win: Window, x: torch.Tensor) -> torch.Tensor:
    L.check(L.load().ctk_assemble_tokens(C.byref(win.args), _ptr(x), 0, _stream()), "ctk_assemble_tokens")
    return x


def tap_indices(win: Window) -> torch.Tensor:
    out = torch.empty(win.S, win.N, L.LEVELS, 2, 7, device=win.device, dtype=torch.int32)
    L.check(L.load().ctk_tap_indices(C.byref(win.args), _ptr(out), _stream()), "ctk_tap_indices")
    return out


def update_former(x: torch.Tensor, S: int, N: int, weights) -> torch.Tensor:
    """x [N*S, 1120] (our column layout) -> delta [N*S,4]."""
    _chk_f32(x)
    lib = L.load()
    ws = _workspace(_query_bytes("ctk_update_former_workspace_bytes", S, N), x.device)
    delta = torch.empty(N * S, 4, device=x.device, dtype=torch.float32)
    mw = weights.struct_for(S)
    L.check(lib.ctk_update_former(S, N, _ptr(x), C.byref(mw), _ptr(delta), _ptr(ws), ws.numel(), _stream()), "ctk_update_former")
    return delta


# ------------------------------------------------------------------------------------------
# opt-in per-kernel timing (bench.py)
# ------------------------------------------------------------------------------------------
def profile_enable(on: bool) -> None:
    L.check(L.load().ctk_profile_enable(1 if on else 0), "ctk_profile_enable")


def profile_read():
    rows = (L.ProfileRow * 64)()
    n = C.c_int(0)
    L.check(L.load().ctk_profile_read(rows, 64, C.byref(n)), "ctk_profile_read")
    return [dict(name=rows[i].name.decode(), launches=rows[i].launches, total_ms=rows[i].total_ms, flops=rows[i].flops,
                 bytes=rows[i].bytes) for i in range(n.value)]
