"""Argument validation of the encoder's pixel entry points and the CoTracker2 row entry points (include/ctk.h:
ctk_enc_stem_im2col, ctk_enc_inorm_workspace_bytes, ctk_enc_inorm_stats, ctk_enc_inorm_apply, ctk_enc_fuse, ctk_enc_l2norm,
ctk_v2_assemble, ctk_v2_apply_delta, ctk_v2_vis_head) and of the CoTracker3 row entry points (ctk_layernorm, ctk_layernorm_dual,
ctk_assemble_tokens, ctk_assemble_tokens_batch, ctk_virtual_init, ctk_heads_update, and what of the weights reaches their kernels
through ctk_forward_window / ctk_update_former), without a GPU: every rule the header documents is refused with its
CTK_E_* code BEFORE any HIP call.  The pointers below are made-up addresses: every call in this file is invalid in exactly
one way, so none of them may reach a launch.  The file runs only where no device is visible: there a call that slipped through
a missing check returns a positive hipError_t, which no assertion here accepts, instead of launching on these addresses."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up device addresses: only where a stray launch cannot run")

from ctk_support import lib  # noqa: E402,F401

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
P = 0x10000        # a "pointer": non-NULL, 16-byte aligned, never dereferenced
ODD = P + 8        # 8-byte aligned only
ODD4 = P + 4       # 4-byte aligned only


def _each_missing(call, good, required):
    """call(*args) with each required pointer (by position) set to None in turn -> CTK_E_NULL."""
    for i in required:
        args = list(good)
        args[i] = None
        assert call(*args) == E_NULL, (call.__name__, i)


def _with(good, **at):
    args = list(good)
    for i, v in at.items():
        args[int(i[1:])] = v
    return args


def test_abi_version_is_unchanged(lib):
    assert lib.ctk_abi_version() == 9
    assert b"aligned" in lib.ctk_error_string(E_ALIGN)


def test_stem_im2col_arguments(lib):
    f = lib.ctk_enc_stem_im2col
    good = [P, 2, 64, 96, P, None]          # frames, F, H, W, out_sh, stream
    _each_missing(f, good, (0, 4))
    for bad in (_with(good, _1=0), _with(good, _1=-1), _with(good, _2=6), _with(good, _3=6), _with(good, _2=0), _with(good, _3=-7)):
        assert f(*bad) == E_SHAPE, bad
    assert f(*_with(good, _4=ODD)) == E_ALIGN                   # f16x8 stores
    assert f(*_with(good, _0=None, _2=6)) == E_NULL             # NULL is reported before the shape


def test_inorm_workspace_bytes_arguments(lib):
    f = lib.ctk_enc_inorm_workspace_bytes
    n = C.c_size_t(77)
    assert f(3, 1536, 64, None) == E_NULL
    for F, HW, Cn in ((0, 1536, 64), (-1, 1536, 64), (65536, 1536, 64), (3, 0, 64), (3, -5, 64), (3, 1536, 0), (3, 1536, 60),
                      (3, 1536, 1032), (3, 1536, 2048)):
        assert f(F, HW, Cn, C.byref(n)) == E_SHAPE and n.value == 77, (F, HW, Cn)
    # the query itself needs no device: F * ceil(HW / 512) * C * 16 bytes (f64 sum and sum of squares per partial block)
    for F, HW, Cn in ((1, 1, 8), (3, 511, 64), (3, 512, 96), (2, 513, 128), (16, 49152, 256), (65535, 7, 1024)):
        assert f(F, HW, Cn, C.byref(n)) == 0 and n.value == F * ((HW + 511) // 512) * Cn * 16, (F, HW, Cn, n.value)


def test_inorm_stats_arguments(lib):
    f = lib.ctk_enc_inorm_stats
    good = [P, 3, 1536, 64, 1e-5, P, P, None]   # x, F, HW, C, eps, stats, workspace, stream
    _each_missing(f, good, (0, 5, 6))
    for bad in (_with(good, _1=0), _with(good, _1=65536), _with(good, _2=0), _with(good, _2=-1), _with(good, _3=0), _with(good, _3=-8),
                _with(good, _3=4), _with(good, _3=68), _with(good, _3=1032), _with(good, _3=4096)):
        assert f(*bad) == E_SHAPE, bad
    assert f(*_with(good, _0=ODD)) == E_ALIGN                   # f32x4 loads
    assert f(*_with(good, _6=ODD)) == E_ALIGN                   # the f64 partial sums


def test_inorm_apply_arguments(lib):
    f = lib.ctk_enc_inorm_apply
    good = [P, P, P, P, 3, 1536, 64, P, P, None]   # x, stats, skip, skip_stats, F, HW, C, out_sh, out_f32, stream
    _each_missing(f, good, (0, 1))
    assert f(*_with(good, _7=None, _8=None)) == E_NULL           # neither output given
    assert f(*_with(good, _2=None)) == E_NULL                    # skip statistics without a skip
    for bad in (_with(good, _4=0), _with(good, _5=0), _with(good, _6=0), _with(good, _6=8), _with(good, _6=16), _with(good, _6=48),
                _with(good, _6=-32)):
        assert f(*bad) == E_SHAPE, bad
    for i in (0, 2, 7, 8):                                       # x, skip, out_sh, out_f32: 16-byte vector accesses
        assert f(*_with(good, **{f"_{i}": ODD})) == E_ALIGN, i
    assert f(*_with(good, _2=None, _3=None, _8=None, _6=40)) == E_SHAPE   # the optional ones left out: the rest is still checked


def test_fuse_arguments(lib):
    f = lib.ctk_enc_fuse

    def args(src=(P, P, P, P), H=(32, 16, 8, 4), W=(48, 24, 12, 6), Cs=(64, 96, 128, 128), F=2, Ho=16, Wo=24, out=P,
             null=None):
        a = [(C.c_void_p * 4)(*src), (C.c_int32 * 4)(*H), (C.c_int32 * 4)(*W), (C.c_int32 * 4)(*Cs), F, Ho, Wo, out, None]
        if null is not None:
            a[null] = None
        return a

    for i in (0, 1, 2, 3, 7):
        assert f(*args(null=i)) == E_NULL, i
    for k in range(4):
        src = [P] * 4
        src[k] = None
        assert f(*args(src=src)) == E_NULL, k                    # a NULL source
        src[k] = ODD
        assert f(*args(src=src)) == E_ALIGN, k
        for name, val in (("H", 0), ("W", 0), ("Cs", 0), ("Cs", 4), ("Cs", 100)):
            v = list(args.__defaults__[("H", "W", "Cs").index(name) + 1])
            v[k] = val
            assert f(*args(**{name: v})) == E_SHAPE, (k, name, val)
    assert f(*args(Cs=(64, 96, 128, 120))) == E_SHAPE            # every C_k % 8 == 0 but the total (408) % 32 != 0
    assert f(*args(Cs=(8, 8, 8, 16))) == E_SHAPE                 # total 40
    for kw in ({"F": 0}, {"Ho": 0}, {"Wo": 0}, {"F": -2}):
        assert f(*args(**kw)) == E_SHAPE, kw
    assert f(*args(out=ODD)) == E_ALIGN


def test_l2norm_arguments(lib):
    f = lib.ctk_enc_l2norm
    good = [P, 100, P, None]
    _each_missing(f, good, (0, 2))
    assert f(*_with(good, _1=0)) == E_SHAPE and f(*_with(good, _1=-4)) == E_SHAPE


def test_v2_assemble_arguments(lib):
    f = lib.ctk_v2_assemble
    good = [8, 5, P, P, P, P, P, P, 480, P, 0, None]   # S, N, coords, fcorrs, track_feat, track_mask, vis, pos, in_ld, x, x_split, stream
    _each_missing(f, good, (2, 3, 4, 5, 6, 7, 9))
    for bad in (_with(good, _0=0), _with(good, _1=0), _with(good, _0=-8), _with(good, _8=448), _with(good, _8=455), _with(good, _8=456),
                _with(good, _8=470), _with(good, _8=496 + 8), _with(good, _8=0)):
        assert f(*bad) == E_SHAPE, bad
    assert f(*_with(good, _8=456, _10=1)) == E_SHAPE            # 456 % 32 != 0 for the SH output too


def test_v2_apply_delta_arguments(lib):
    f = lib.ctk_v2_apply_delta
    good = [8, 5, P, 192, P, P, P, 1e-5, P, None]   # S, N, delta, out_ld, coords, gamma, beta, eps, normed, stream
    _each_missing(f, good, (2, 4, 5, 6, 8))
    for bad in (_with(good, _0=0), _with(good, _1=0), _with(good, _1=-5), _with(good, _3=129), _with(good, _3=128), _with(good, _3=0)):
        assert f(*bad) == E_SHAPE, bad
    assert f(*_with(good, _8=ODD4)) == E_ALIGN                   # float2 stores of the normalised rows: 8 bytes


def test_v2_vis_head_arguments(lib):
    f = lib.ctk_v2_vis_head
    good = [P, 40, P, P, P, None]   # track_feat, R, w, b, out, stream
    _each_missing(f, good, (0, 2, 3, 4))
    assert f(*_with(good, _1=0)) == E_SHAPE and f(*_with(good, _1=-1)) == E_SHAPE
    assert f(*_with(good, _0=ODD4)) == E_ALIGN and f(*_with(good, _2=ODD4)) == E_ALIGN   # float2 loads: 8 bytes


def test_v2_window_refuses_what_its_last_call_would_refuse(lib):
    """ctk_forward_window_v2 ends with the visibility head; a track_feat or vis_w it would refuse is refused by the window's own
    validation (shared by the workspace query, the direct call and the graph capture), before an iteration has updated anything."""
    from cotracker_amd import _lib as L
    a, w, n = L.V2WindowArgs(), L.V2Weights(), C.c_size_t(0)
    a.S, a.N, a.iters = 8, 10, 4
    for l in range(L.LEVELS):
        a.H[l], a.W[l], a.fmaps[l] = 16 >> l, 24 >> l, P
    a.coords = a.track_feat = a.vis = a.track_mask = a.vis_out = P
    w.former.in_dim, w.former.in_ld, w.former.out_dim, w.former.out_ld = 456, 480, 130, 192
    w.pos_hwc, w.pos_h, w.pos_w = P, 16, 24
    w.norm_w = w.norm_b = w.upd_w = w.upd_b = w.vis_w = w.vis_b = P
    query = lib.ctk_forward_window_v2_workspace_bytes
    a.track_feat = ODD4
    assert query(C.byref(a), C.byref(w), C.byref(n)) == E_ALIGN
    assert lib.ctk_forward_window_v2(C.byref(a), C.byref(w), P, 1 << 40, None) == E_ALIGN
    h = C.c_void_p()
    assert lib.ctk_v2_window_graph_create(C.byref(a), C.byref(w), P, 1 << 40, C.byref(h)) == E_ALIGN and not h.value
    a.track_feat, w.vis_w = P, ODD4
    assert query(C.byref(a), C.byref(w), C.byref(n)) == E_ALIGN
    assert lib.ctk_forward_window_v2(C.byref(a), C.byref(w), P, 1 << 40, None) == E_ALIGN
    w.vis_w = ODD        # 8-byte aligned is enough for the float2 loads
    rc = query(C.byref(a), C.byref(w), C.byref(n))      # a query: no launch
    assert rc != E_ALIGN


# ---- the CoTracker3 row entry points (csrc/rowops.hip) ----------------------------------------------------------------------------------
def _state_batch(B=1, **at):
    """ctk_window_batch of made-up state pointers, S = 8 and N = 5; at: field=value on video B - 1 (the last one) alone."""
    from cotracker_amd import _lib as L
    arr = (L.WindowArgs * max(B, 1))()
    for a in arr:
        a.S, a.N, a.coords, a.vis, a.conf, a.scale_x, a.scale_y = 8, 5, P, P, P, 1.0, 1.0
    for k, v in at.items():
        setattr(arr[max(B, 1) - 1], k, v)
    return L.WindowBatch(B, 0, C.cast(arr, C.POINTER(L.WindowArgs))), arr


def test_new_row_symbols_are_declared_bound_and_exported(lib):
    import os
    from cotracker_amd import _lib as L
    from ctk_support import ROOT
    header = open(os.path.join(ROOT, "include", "ctk.h")).read()
    for name in ("ctk_layernorm_dual", "ctk_virtual_init", "ctk_assemble_tokens_batch", "ctk_heads_update"):
        assert f"int {name}(" in header and name in L.SYMBOLS and hasattr(lib, name), name
    assert lib.ctk_abi_version() == L.ABI_VERSION == 9


def test_layernorm_and_assemble_tokens_alignment(lib):
    f = lib.ctk_layernorm
    good = [P, P, 40, P, P, 1e-5, 0, None]      # x, y, R, gamma, beta, eps, out_split, stream
    _each_missing(f, good, (0, 1, 3, 4))        # (gamma without beta, beta without gamma)
    assert f(*_with(good, _2=0)) == E_SHAPE and f(*_with(good, _2=-3)) == E_SHAPE
    for i in (0, 1, 3, 4):                      # f32x4 loads, f32x4 / f16x8 stores
        for odd in (ODD, ODD4):
            for split in (0, 1):
                assert f(*_with(good, **{f"_{i}": odd, "_6": split})) == E_ALIGN, (i, odd, split)
    assert f(*_with(good, _0=ODD, _3=None, _4=None)) == E_ALIGN      # without the affine part too
    assert f(*_with(good, _0=None, _2=0)) == E_NULL and f(*_with(good, _0=ODD, _2=0)) == E_SHAPE   # NULL, then shape, then alignment
    from cotracker_amd import _lib as L
    a = L.WindowArgs()
    a.S, a.N, a.coords, a.vis, a.conf, a.scale_x, a.scale_y = 8, 5, P, P, P, 1.0, 1.0
    g = lib.ctk_assemble_tokens
    assert g(None, P, 0, None) == E_NULL and g(C.byref(a), None, 0, None) == E_NULL
    for split in (0, 1):
        assert g(C.byref(a), ODD, split, None) == E_ALIGN and g(C.byref(a), ODD4, split, None) == E_ALIGN
    a.N = 0
    assert g(C.byref(a), ODD, 0, None) == E_SHAPE


def test_layernorm_dual_arguments(lib):
    f = lib.ctk_layernorm_dual
    good = [P, P, P, 40, P, P, 1e-5, 1e-6, 0, None]   # x, y, y2, R, gamma, beta, eps, eps2, out_split, stream
    _each_missing(f, good, (0, 1, 2, 4, 5))
    assert f(*_with(good, _3=0)) == E_SHAPE and f(*_with(good, _3=-1)) == E_SHAPE
    for i in (0, 1, 2, 4, 5):
        for split in (0, 1):
            assert f(*_with(good, **{f"_{i}": ODD, "_8": split})) == E_ALIGN, (i, split)
    assert f(*_with(good, _2=ODD4, _4=None, _5=None)) == E_ALIGN
    assert f(*_with(good, _2=None, _3=0)) == E_NULL and f(*_with(good, _2=ODD, _3=0)) == E_SHAPE


def test_virtual_init_arguments(lib):
    f = lib.ctk_virtual_init
    good = [P, 8, 2, P, None]                   # virtual_tokens, S, B, dst, stream
    _each_missing(f, good, (0, 3))
    for bad in (_with(good, _1=0), _with(good, _1=-8), _with(good, _2=0), _with(good, _2=-1), _with(good, _2=17)):
        assert f(*bad) == E_SHAPE, bad
    for i in (0, 3):
        assert f(*_with(good, **{f"_{i}": ODD})) == E_ALIGN and f(*_with(good, **{f"_{i}": ODD4})) == E_ALIGN, i
    assert f(*_with(good, _0=None, _2=17)) == E_NULL and f(*_with(good, _0=ODD, _2=17)) == E_SHAPE


def test_assemble_tokens_batch_arguments(lib):
    f = lib.ctk_assemble_tokens_batch

    def call(batch, x=P, split=0, ld=1120, base=1024):
        return f(C.byref(batch[0]) if batch is not None else None, x, split, ld, base, None)

    for B in (1, 2, 16):
        assert call(_state_batch(B), x=None) == E_NULL
        for field in ("coords", "vis", "conf"):
            assert call(_state_batch(B, **{field: None})) == E_NULL, (B, field)
        for kw in ({"S": 0}, {"N": 0}, {"S": -8}, {"scale_x": 0.0}, {"scale_y": -1.0}, {"scale_x": float("nan")}):
            assert call(_state_batch(B, **kw)) == E_SHAPE, (B, kw)
        for ld, base in ((1120, 1056), (1120, 1000), (1100, 992), (1120, -32), (96, 32), (1632, 1568), (0, 0)):
            assert call(_state_batch(B), ld=ld, base=base) == E_SHAPE, (B, ld, base)
        for ld, base in ((1120, 1024), (1632, 1536), (96, 0)):       # the two layouts of the window and the smallest one
            for split in (0, 1):
                assert call(_state_batch(B), x=ODD, split=split, ld=ld, base=base) == E_ALIGN, (B, ld, base, split)
                assert call(_state_batch(B), x=ODD4, split=split, ld=ld, base=base) == E_ALIGN
    assert call(None) == E_NULL
    from cotracker_amd import _lib as L
    assert f(C.byref(L.WindowBatch(2, 0, None)), P, 0, 1120, 1024, None) == E_NULL
    assert call(_state_batch(0)) == E_SHAPE and call(_state_batch(17)) == E_SHAPE and call(_state_batch(-1)) == E_SHAPE
    for kw in ({"S": 7}, {"N": 6}, {"scale_x": 2.0}, {"scale_y": 0.5}):      # the videos of a joint call agree
        assert call(_state_batch(3, **kw)) == E_SHAPE, kw
    assert call(_state_batch(2, coords=None), x=ODD) == E_NULL and call(_state_batch(2, S=0), x=ODD) == E_SHAPE


def test_heads_update_arguments(lib):
    f = lib.ctk_heads_update

    def call(batch, tokens=P, hw=P, hb=P, delta=None):
        return f(C.byref(batch[0]) if batch is not None else None, tokens, hw, hb, delta, None)

    for B in (1, 2, 16):
        for kw in ({"tokens": None}, {"hw": None}, {"hb": None}):
            assert call(_state_batch(B), **kw) == E_NULL, (B, kw)
        for field in ("coords", "vis", "conf"):
            assert call(_state_batch(B, **{field: None})) == E_NULL, (B, field)      # the state: all three
        for kw in ({"S": 0}, {"N": 0}, {"N": -5}):
            assert call(_state_batch(B, **kw)) == E_SHAPE, (B, kw)
        for kw in ({"tokens": ODD}, {"hw": ODD}, {"tokens": ODD4}, {"hw": ODD4}):    # f32x4 loads
            assert call(_state_batch(B), **kw) == E_ALIGN, (B, kw)
    assert call(None) == E_NULL
    assert call(_state_batch(0)) == E_SHAPE and call(_state_batch(17)) == E_SHAPE
    assert call(_state_batch(2, S=7)) == E_SHAPE and call(_state_batch(2, N=4)) == E_SHAPE
    # B == 1: delta and / or the state; delta is one 16-byte store per row
    none = dict(coords=None, vis=None, conf=None)
    assert call(_state_batch(1, **none)) == E_NULL                                   # neither
    assert call(_state_batch(1, **none), delta=ODD) == E_ALIGN and call(_state_batch(1), delta=ODD4) == E_ALIGN
    assert call(_state_batch(1, coords=None, vis=None), delta=P) == E_NULL           # a part of the state
    assert call(_state_batch(1, **none), delta=P, hw=ODD) == E_ALIGN
    # B > 1: the joint kernel has no delta
    assert call(_state_batch(2), delta=P) == E_SHAPE and call(_state_batch(16), delta=P) == E_SHAPE
    assert call(_state_batch(2), tokens=None, delta=P) == E_NULL                     # NULL first


def _model_weights():
    """A ctk_model_weights (f32 back end, unfolded) of made-up pointers that passes every NULL rule."""
    from cotracker_amd import _lib as L
    w = L.ModelWeights()
    for n in ("corr_fc1_w", "corr_fc1_b", "corr_fc2_w", "corr_fc2_b", "in_w", "in_bias_t", "virtual_tokens", "head_w", "head_b"):
        setattr(w, n, P)
    for blocks in (w.time_blocks, w.virtual2point, w.virtual_self, w.point2virtual):
        for b in blocks:
            for n in ("wq", "bq", "wkv", "bkv", "wo", "bo", "w1", "b1", "w2", "b2", "ctx_gamma", "ctx_beta"):
                setattr(b, n, P)
    return w


def test_windows_refuse_what_their_row_kernels_would_misread(lib):
    """head_w, virtual_tokens and norm_context's gamma / beta reach heads_kernel, virtual_init_kernel and layernorm_kernel through
    the window and update-former calls: refused with the weights' validation, before the workspace is looked at or anything runs."""
    from cotracker_amd import _lib as L
    a = L.WindowArgs()
    a.S, a.N, a.iters, a.coords, a.vis, a.conf, a.scale_x, a.scale_y = 8, 5, 1, P, P, P, 1.0, 1.0
    batch = L.WindowBatch(1, 0, C.pointer(a))
    h = C.c_void_p()

    def every_entry(w):
        return (lib.ctk_update_former(8, 5, P, C.byref(w), P, P, 1 << 40, None),
                lib.ctk_forward_window(C.byref(a), C.byref(w), P, 1 << 40, None),
                lib.ctk_forward_window_batch(C.byref(batch), C.byref(w), P, 1 << 40, None),
                lib.ctk_window_tokens_batch(C.byref(batch), C.byref(w), P, P, 1 << 40, None),
                lib.ctk_window_graph_create(C.byref(a), C.byref(w), P, 1 << 40, C.byref(h)))

    for odd in (ODD, ODD4):
        for name in ("head_w", "virtual_tokens"):
            w = _model_weights()
            setattr(w, name, odd)
            assert every_entry(w) == (E_ALIGN,) * 5 and not h.value, name
        for blocks in ("virtual2point", "point2virtual"):
            for i in (0, L.DEPTH - 1):
                for name in ("ctx_gamma", "ctx_beta"):
                    w = _model_weights()
                    setattr(getattr(w, blocks)[i], name, odd)
                    assert every_entry(w) == (E_ALIGN,) * 5 and not h.value, (blocks, i, name)
    w = _model_weights()
    assert lib.ctk_update_former(8, 5, P, C.byref(w), ODD, P, 1 << 40, None) == E_ALIGN      # delta: one 16-byte store per row
    w.head_w = None
    assert lib.ctk_update_former(8, 5, P, C.byref(w), ODD, P, 1 << 40, None) == E_NULL
    fw = L.FormerWeights()                                                                  # CoTracker2's former: the same kernels
    fw.depth, fw.in_dim, fw.in_ld, fw.out_dim, fw.out_ld = 1, 456, 480, 130, 192
    blocks = [L.BlockWeights() for _ in range(4)]
    for b in blocks:
        for n in ("wq", "bq", "wkv", "bkv", "wo", "bo", "w1", "b1", "w2", "b2", "ctx_gamma", "ctx_beta"):
            setattr(b, n, P)
    fw.in_w = fw.in_b = fw.virtual_tokens = fw.head_w = fw.head_b = P
    fw.time_blocks, fw.virtual2point, fw.virtual_self, fw.point2virtual = (C.pointer(b) for b in blocks)
    ex = lambda: lib.ctk_update_former_ex(8, 5, P, 0, C.byref(fw), None, P, P, 1 << 40, None)  # noqa: E731
    fw.virtual_tokens = ODD
    assert ex() == E_ALIGN
    fw.virtual_tokens, blocks[1].ctx_gamma = P, ODD4
    assert ex() == E_ALIGN
    blocks[1].ctx_gamma, blocks[3].ctx_beta = P, ODD
    assert ex() == E_ALIGN
