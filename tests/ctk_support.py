"""What the test modules share: `from ctk_support import ...` (tests/ is on sys.path; this is a plain module -- not a conftest, not a
plugin).  Helpers that used to be pasted from file to file live here once; where the copies differed, the difference is an argument
and every module passes what its own copy did.  A fixture is shared by importing it under the name the module uses
(`from ctk_support import precision_default as precision  # noqa: F401`).  Tolerances and bars stay in the module that asserts them."""
import copy
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, STEP, STRIDE = 8, 4, 4  # window length, step and stride of the small models; their resolution
HW = (64, 96)


# ---- small things ---------------------------------------------------------------------------------------------------------------
def dev():
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def maxdiff(a, b):
    """max |a - b| in float64; tensors (any device) and arrays."""
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max())


def logit(p):
    p = p.detach().cpu().double() if torch.is_tensor(p) else torch.from_numpy(np.asarray(p)).double()
    return torch.log(p / (1 - p))


def bits(x):
    """A tensor of 1- or 4-byte elements as integers (NaN patterns compare like any other)."""
    return x.view(torch.uint8) if x.dtype == torch.uint8 else x.contiguous().view(torch.int32)


def same_bits(a, b):
    """Bit-for-bit equality (torch.equal would let -0 pass for +0 and fail NaN against NaN)."""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    iv = {torch.float32: torch.int32, torch.float16: torch.int16, torch.float64: torch.int64}[a.dtype]
    return torch.equal(a.contiguous().view(iv).cpu(), b.contiguous().view(iv).cpu())


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from cotracker_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


# ---- ctk_gemm as the C-ABI sees it (tests/test_gpu_gemm_matrix.py, test_gpu_parity.py, test_cabi_and_host.py) --------------------------
def gemm_raw(A, lda, M, N, K, out, ldc, W=None, ldw=0, Wp=None, bias=None, bias_rows=None, period=0, resid=None, ldr=0, act=0,
             batch=1, a_bs=0, c_bs=0, a_split=False, c_split=False):
    """Fills ctk_gemm_args field by field (ops.gemm fixes lda = K, batch = 1 and the base pointers) and calls ctk_gemm on the
    current stream -> its return code.  Pointers: tensors (a view passes the address of its first element), integers or None."""
    from cotracker_amd import _lib as L

    def p(x):
        return x.data_ptr() if torch.is_tensor(x) else x

    g = L.GemmArgs()
    g.A, g.lda, g.M = p(A), lda, M
    g.W, g.ldw, g.N, g.K = p(W), ldw, N, K
    g.Wp = p(Wp)
    g.C, g.ldc = p(out), ldc
    g.bias, g.bias_rows, g.bias_period = p(bias), p(bias_rows), period
    g.resid, g.ldr = p(resid), ldr
    g.act, g.batch, g.a_bs, g.c_bs, g.k_valid = act, batch, a_bs, c_bs, 0
    g.a_split, g.c_split = int(a_split), int(c_split)
    stream = torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else None
    return L.load().ctk_gemm(C.byref(g), stream)


# ---- ctk_conv2d_sh as the C-ABI sees it (tests/test_gpu_conv_matrix.py, test_cabi_and_host.py) -------------------------------------------
def conv_raw(in_sh, F, H, W, Cin, wp, bias, n_out, n_pad, KH, KW, stride, pad, out, zeros):
    """ctk_conv2d_sh on the current stream with every argument the caller's (HipEncoder._conv allocates the output itself and takes
    the rest from a _Conv) -> its return code.  Pointers: tensors (a view passes the address of its first element), integers or None."""
    from cotracker_amd import _lib as L

    def p(x):
        return x.data_ptr() if torch.is_tensor(x) else x

    stream = torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else None
    return L.load().ctk_conv2d_sh(p(in_sh), F, H, W, Cin, p(wp), p(bias), n_out, n_pad, KH, KW, stride, pad, p(out), p(zeros), stream)


# ---- ctk_attention_ex as the C-ABI sees it (tests/test_gpu_attention_matrix.py) ----------------------------------------------------------
def attention_raw(q, q_ld, q_bs, q_is, k, v, kv_ld, kv_bs, kv_is, out, o_ld, o_bs, o_is, nbatch, n1, n2, splits=1, partial=None,
                  o_split=False, key_mask=None, query_mask=None, batch2=None):
    """Fills ctk_attn_args field by field (ops.attention fixes the leading dimensions at 384, o_bs = q_bs and the base pointers)
    and calls ctk_attention_ex on the current stream -> its return code.  batch2: None (b2 == NULL, the single-level call) or a
    dict with the fields of ctk_attn_batch2 (inner, q_os, kv_os, o_os, key_mask_os, query_mask_os).  Pointers: tensors (a view
    passes the address of its first element), integers or None."""
    from cotracker_amd import _lib as L

    def p(x):
        return x.data_ptr() if torch.is_tensor(x) else x

    a = L.AttnArgs()
    a.q, a.q_ld, a.q_bs, a.q_is = p(q), q_ld, q_bs, q_is
    a.k, a.v, a.kv_ld, a.kv_bs, a.kv_is = p(k), p(v), kv_ld, kv_bs, kv_is
    a.out, a.o_ld, a.o_bs, a.o_is = p(out), o_ld, o_bs, o_is
    a.nbatch, a.n1, a.n2 = nbatch, n1, n2
    a.splits, a.partial, a.o_split = splits, p(partial), int(o_split)
    a.key_mask, a.query_mask = p(key_mask), p(query_mask)
    b2 = None
    if batch2 is not None:
        b2 = L.AttnBatch2()
        b2.inner, b2.reserved = batch2["inner"], 0
        b2.q_os, b2.kv_os, b2.o_os = batch2["q_os"], batch2["kv_os"], batch2["o_os"]
        b2.key_mask_os, b2.query_mask_os = batch2.get("key_mask_os", 0), batch2.get("query_mask_os", 0)
    stream = torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else None
    return L.load().ctk_attention_ex(C.byref(a), None if b2 is None else C.byref(b2), stream)


# ---- the correlation samplers as the C-ABI sees them (tests/test_gpu_corr_matrix.py) ---------------------------------------------------------
CORR_K, CORR_LD = 2401, 2432  # 49 x 49 volume columns and the row length (K padding of corr_mlp.fc1), in 4-byte units


NAN_PATTERN = 0x7FC17FC1  # NaN as one f32 and as two f16


def nan_framed(x, pad=8192, pattern=None, whole=False):
    """A copy of x (f32) in the middle of a NaN-filled allocation on the GPU, `pad` elements on either side (a multiple of 4: the
    view keeps the 16-byte alignment of the allocation) -> the contiguous view.  A read that leaves the operand reads NaN.
    pattern: the bits of the NaN (NAN_PATTERN reads as NaN in either number format; default: torch's).  whole=True -> (view, the
    whole allocation), for `frame_intact` after a launch that writes the view."""
    assert pad % 4 == 0 and x.dtype == torch.float32
    if pattern is None:
        flat = torch.full((x.numel() + 2 * pad,), float("nan"), device=dev())
    else:
        flat = torch.full((x.numel() + 2 * pad,), pattern, dtype=torch.int32, device=dev()).view(torch.float32)
    view = flat[pad:pad + x.numel()].view(x.shape)
    view.copy_(x)
    return (view, flat) if whole else view


def frame_intact(flat, view, pattern=NAN_PATTERN):
    """Whether the `pattern` words around `view` inside its allocation `flat` (nan_framed(..., pattern, whole=True)) kept their bits."""
    pad = (flat.numel() - view.numel()) // 2
    w = flat.view(torch.int32)
    return bool((w[:pad] == pattern).all()) and bool((w[pad + view.numel():] == pattern).all())


# ---- the row kernels as the C-ABI sees them (tests/test_gpu_rowop_matrix.py): every pointer the caller's ------------------------------------
def _addr(x):
    return x.data_ptr() if torch.is_tensor(x) else x


def _current_stream():
    return torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else None


def layernorm_raw(x, y, R, gamma, beta, eps, out_split, y2=None, eps2=0.0):
    """ctk_layernorm, or with y2 ctk_layernorm_dual, on the current stream -> its return code (ops.layernorm allocates y itself).
    Pointers here and below: tensors (a view passes the address of its first element), integers or None."""
    from cotracker_amd import _lib as L
    if y2 is None:
        return L.load().ctk_layernorm(_addr(x), _addr(y), R, _addr(gamma), _addr(beta), eps, int(out_split), _current_stream())
    return L.load().ctk_layernorm_dual(_addr(x), _addr(y), _addr(y2), R, _addr(gamma), _addr(beta), eps, eps2, int(out_split),
                                       _current_stream())


def virtual_init_raw(virtual_tokens, S, B, dst):
    from cotracker_amd import _lib as L
    return L.load().ctk_virtual_init(_addr(virtual_tokens), S, B, _addr(dst), _current_stream())


def assemble_raw(states, S, N, scale_xy, x, x_split, ld, base):
    """ctk_assemble_tokens_batch over states = [(coords, vis, conf)] per video -> its return code."""
    from cotracker_amd import _lib as L
    from cotracker_amd import ops
    batch, keep = ops.state_batch(states, S, N, scale_xy)
    return L.load().ctk_assemble_tokens_batch(C.byref(batch), _addr(x), int(x_split), ld, base, _current_stream())


def heads_raw(states, S, N, tokens, head_w, head_b, delta):
    """ctk_heads_update over states = [(coords, vis, conf)] per video ((None, None, None): delta only) -> its return code."""
    from cotracker_amd import _lib as L
    from cotracker_amd import ops
    batch, keep = ops.state_batch(states, S, N)
    return L.load().ctk_heads_update(C.byref(batch), _addr(tokens), _addr(head_w), _addr(head_b), _addr(delta), _current_stream())


def corr_volume_raw(win, sh, canary, guard=4):
    """ctk_corr_volume (sh=False) or ctk_corr_volume_sh of a whole window into caller-owned memory (ops.corr_volume* allocate their
    own): [guard rows | 4 levels x N*S rows | guard rows] x CORR_LD 4-byte units, pre-filled with `canary`.  The entry points fix
    the level stride at N*S rows, so guard rows lie in front of level 0 and behind level 3 only.
    -> (the volume f32 [4][N*S][CORR_LD] or SH f16 [4][N*S][76][2][32], whether every guard row kept its bits)."""
    from cotracker_amd import _lib as L
    from cotracker_amd import ops
    rows = L.LEVELS * win.N * win.S
    buf = torch.full((rows + 2 * guard, CORR_LD), canary, dtype=torch.int32, device=win.device)
    body = buf[guard:guard + rows]
    stream = torch.cuda.current_stream().cuda_stream
    if sh:
        ws = ops._workspace(ops._query_bytes("ctk_corr_volume_sh_workspace_bytes", C.byref(win.args)), win.device)
        L.check(L.load().ctk_corr_volume_sh(C.byref(win.args), body.data_ptr(), ws.data_ptr(), ws.numel(), stream), "ctk_corr_volume_sh")
        vol = body.view(torch.float16).view(L.LEVELS, win.N * win.S, CORR_LD // 32, 2, 32)
    else:
        L.check(L.load().ctk_corr_volume(C.byref(win.args), body.data_ptr(), stream), "ctk_corr_volume")
        vol = body.view(torch.float32).view(L.LEVELS, win.N * win.S, CORR_LD)
    intact = bool((buf[:guard] == canary).all()) and bool((buf[guard + rows:] == canary).all())
    return vol, intact


def sampler_taps(coords, sizes):
    """The tap tables of a window on the host, from the numpy restatement of the reference's float32 coordinate arithmetic
    (oracle/cotracker_oracle.py: sampler_indices_weights): coords [S,N,2] float32 in level-0 units, sizes [(H, W)] per level ->
    per level a dict of [S,N,7] arrays for either axis a in "xy": a+"0" the floor index, a+"1" its clamped upper neighbour,
    "w"+a+"0" / "w"+a+"1" their float32 weights."""
    from oracle import cotracker_oracle as O
    f32 = np.float32
    out = []
    d = np.arange(-3, 4).astype(f32)
    for l, (H, W) in enumerate(sizes):
        cl = (np.asarray(coords, f32) * f32(1.0 / 2 ** l)).astype(f32)  # coords / 2**l: exact
        tab = {}
        for k, (a, size) in enumerate((("x", W), ("y", H))):
            i0, w0, w1 = O.sampler_indices_weights((cl[..., k:k + 1] + d).astype(f32), size)
            tab[a + "0"], tab[a + "1"], tab["w" + a + "0"], tab["w" + a + "1"] = i0, np.minimum(i0 + 1, size - 1), w0, w1
        out.append(tab)
    return out


def recorded(call):
    """-> (call(), {recorder row name: launches}) of the library launches `call` made.  The recorder is one per process."""
    from cotracker_amd import ops
    ops.profile_enable(True)
    try:
        out = call()
        rows = {r["name"]: r["launches"] for r in ops.profile_read()}
    finally:
        ops.profile_enable(False)
    return out, rows


# ---- the two Linear back ends ---------------------------------------------------------------------------------------------------
PRECISIONS = ["f16x3", "f32"]


@pytest.fixture(params=PRECISIONS)
def precision_param(request):
    """Hands out the back end's name; the test passes it on."""
    return request.param


def _as_default(request):
    from cotracker_amd import model
    old = model.DEFAULT_PRECISION
    model.DEFAULT_PRECISION = request.param
    yield request.param
    model.DEFAULT_PRECISION = old


@pytest.fixture(params=PRECISIONS)
def precision_default(request):
    """Also makes the back end model.DEFAULT_PRECISION for the test."""
    yield from _as_default(request)


@pytest.fixture(autouse=True, params=PRECISIONS)
def precision_default_autouse(request):
    """precision_default for every test of the importing module, asked for or not."""
    yield from _as_default(request)


# ---- models ---------------------------------------------------------------------------------------------------------------------
SWITCHES = ("batch_mode", "hip_graph", "range_guard", "online_feature_cache", "stream_range_check", "stream_groups", "stream_slots")


def small_model(cache, precision, kind="online", seed=1, window_len=8, model_resolution=(64, 96), **switches):
    """A small synthetic-weight model on the GPU, built once per `cache` -- the calling module's own dict: tests count graph captures
    and encoder calls and hold on to the stream state, so modules do not share instances.  kind: "online" / "offline" / "v2".
    `switches` are set on EVERY hand-out, in the order given (a test that flipped one does not leak into the next)."""
    from cotracker_amd.build_cotracker import build_cotracker
    from cotracker_amd.model import CoTrackerThreeOffline, CoTrackerThreeOnline
    from cotracker_amd.weights import fill_synthetic_
    assert set(switches) <= set(SWITCHES), set(switches) - set(SWITCHES)
    key = (precision, kind, seed, window_len, model_resolution)
    if key not in cache:
        if kind == "v2":
            m = build_cotracker(None, v2=True, window_len=window_len).eval()
        else:
            cls = {"online": CoTrackerThreeOnline, "offline": CoTrackerThreeOffline}[kind]
            m = cls(stride=STRIDE, corr_radius=3, window_len=window_len, model_resolution=model_resolution).eval()
        fill_synthetic_(m, seed=seed)
        m.precision = precision
        cache[key] = m.to(dev())
    m = cache[key]
    for name, value in switches.items():
        setattr(m, name, value)
    return m


def overflow_model(precision, **switches):
    """tests/test_gpu_range.py: an MLP whose hidden activations leave the f16 range.  A fresh model per call."""
    from cotracker_amd.model import CoTrackerThreeOnline
    from cotracker_amd.weights import fill_synthetic_
    m = CoTrackerThreeOnline(stride=STRIDE, corr_radius=3, window_len=S, model_resolution=HW).eval()
    fill_synthetic_(m, seed=1)
    with torch.no_grad():
        m.updateformer.time_blocks[0].mlp.fc1.weight.mul_(3e5)
        m.updateformer.time_blocks[0].mlp.fc2.weight.mul_(1e-5)
    m.invalidate_packed_weights()
    m.precision = precision
    for name, value in switches.items():
        setattr(m, name, value)
    return m.to(dev())


def copy_without_stream_state(m, stream_slots):
    """A deep copy of the model that starts without a stream state of its own, with the slot switch as given."""
    held, m._gstream = m._gstream, None
    try:
        ref = copy.deepcopy(m)
    finally:
        m._gstream = held
    ref.stream_slots = stream_slots
    return ref


def count_encodes(m):
    """-> a list that grows by the frame count of every encoder call of m, until the caller does `del m._encode`."""
    calls = []
    orig = m._encode

    def counted(frames, *a, **k):
        calls.append(int(frames.shape[0]))
        return orig(frames, *a, **k)
    m._encode = counted
    return calls


# ---- streams (tests/test_gpu_stream_groups.py, _slots.py, _push.py) -----------------------------------------------------------------
def stream_inputs(G, N, T, seed=0, frames=None):
    """One video of T frames and G query sets.  frames: the query frames to draw from, a list or a function of T; by default they
    lie in the first, a middle and the last chunk.  Every group keeps a point at frame 0."""
    g = torch.Generator().manual_seed(seed)
    video = (torch.rand(1, T, 3, *HW, generator=g) * 255).to(dev())
    q = torch.rand(G, N, 3, generator=g) * torch.tensor([1.0, HW[1] - 1.0, HW[0] - 1.0])
    if callable(frames):
        frames = frames(T)
    frames = frames or [0, 0, 2, 3, T // 2 - 1, T // 2, T // 2 + 1, T - STEP - 1, T - 3, T - 2]
    q[..., 0] = torch.tensor(frames, dtype=torch.float32)[torch.randint(0, len(frames), (G, N), generator=g)]
    q[:, 0, 0] = 0.0
    return video, q.to(dev())


def chunks(T):
    """The chunk starts of a stream over T frames (T = S + k * STEP: full chunks only)."""
    return list(range(0, T - S + 1, STEP))


def run_stream(m, video, q, iters=2, between=None, starts=None, lengths=None):
    """-> the (coords, vis, conf) clones after every call.  between(k) runs before call k >= 1 (assigns and releases); starts /
    lengths: the chunks, where they are not the full ones."""
    m.init_video_online_processing()
    outs = []
    for k, t0 in enumerate(starts if starts is not None else chunks(video.shape[1])):
        if k and between is not None:
            between(k)
        n = S if lengths is None else lengths[k]
        c, v, f, _ = m(video[:, t0:t0 + n], q, iters=iters, is_online=True)
        outs.append((c.clone(), v.clone(), f.clone()))
    return outs


# ---- frame ingest (tests/test_gpu_stream_push.py, test_ingest_host.py) --------------------------------------------------------------
def source(dtype, layout, Fn, H, W, seed, pad=(0, 0), device="cpu"):
    """A random source on `device`; pad = (extra rows, extra columns) of the allocation it is a cropped view of."""
    g = torch.Generator().manual_seed(seed)
    full = (Fn, H + pad[0], W + pad[1], 3) if layout == "hwc" else (Fn, 3, H + pad[0], W + pad[1])
    x = torch.randint(0, 256, full, dtype=torch.uint8, generator=g)
    if dtype == torch.float32:
        x = x.float() + torch.rand(full, generator=g)  # not integer-valued: every product rounds
    x = x.to(device)
    return x[:, :H, :W] if layout == "hwc" else x[:, :, :H, :W]


def nchw(src, layout, contiguous=False):
    x = (src.permute(0, 3, 1, 2) if layout == "hwc" else src).float()
    return x.contiguous() if contiguous else x


def fp64_resize(x, size):
    """x [F,3,H,W] (any dtype, any device) -> float64 [F,3,h,w]: tap indices and weights from the float32 coordinate arithmetic of
    ATen (area_pixel_compute_scale / _source_index, align_corners=True), values and blend in float64 (the rule of
    oracle/window_fp64.py for tap positions)."""
    H, W = x.shape[-2:]

    def axis(n_in, n_out):
        r = torch.tensor(float(n_in - 1), dtype=torch.float32) / torch.tensor(float(n_out - 1), dtype=torch.float32) if n_out > 1 \
            else torch.tensor(0.0)
        s = r.to(x.device) * torch.arange(n_out, dtype=torch.float32, device=x.device)
        i0 = s.long()
        i1 = i0 + (i0 < n_in - 1).long()
        l1 = s - i0.float()
        l0 = 1.0 - l1
        return i0, i1, l0.double(), l1.double()

    y0, y1, ly0, ly1 = axis(H, size[0])
    x0, x1, lx0, lx1 = axis(W, size[1])
    v = x.double()
    top = v[:, :, y0][:, :, :, x0] * lx0 + v[:, :, y0][:, :, :, x1] * lx1
    bot = v[:, :, y1][:, :, :, x0] * lx0 + v[:, :, y1][:, :, :, x1] * lx1
    return top * ly0[:, None] + bot * ly1[:, None]


def ulps(got, want):
    """|got - want| in units of the float32 ulp of the value."""
    want = want.double()
    mag = want.abs().float().clamp_min(2.0 ** -20)
    ulp = (torch.nextafter(mag, torch.full_like(mag, float("inf"))) - mag).double()
    return float(((got.double() - want).abs() / ulp).max())


def host_library(tmp_path_factory, name):
    """tests/host/<name>_host.cpp -- a csrc/*_math.h header behind a plain loop -- built with g++ under -ffp-contract=off, the flag
    the device translation unit is built with -> the loaded library."""
    so = os.path.join(str(tmp_path_factory.mktemp(name)), f"lib{name}_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                    os.path.join(ROOT, "tests", "host", f"{name}_host.cpp")], check=True)
    return C.CDLL(so)


# ---- the encoder chain (tests/test_encoder_fp64_reference.py, test_gpu_encoder_stages.py) -------------------------------------------
# name: (H, W, frames).  halo: every 3 x 3 / stride-1 layer is tile-aligned (Hout % 8 == 0 and Wout % 32 == 0: conv3x3_halo_kernel);
# mixed: layer4 (8 x 16) falls back to conv_pp128_kernel; odd: 35 x 51, 18 x 26, 9 x 13, 5 x 7 maps, fused to 17 x 25
ENC_CASES = {"halo": (128, 512, 2), "mixed": (128, 256, 2), "odd": (70, 102, 3)}
# fault hooks of oracle/encoder_fp64.py: name -> (case it is planted on, the stage it must move and no other, the hook).
# Planted where the fault means something: the tap on the map that has a halo tile seam at columns 31 | 32 (layer3 of `halo` is
# 16 x 64), the frame statistics where frames 0 and 1 are both textured (`odd`).
ENC_FAULTS = {
    "dropped_tap_at_a_tile_seam": ("halo", "layer3.1", {"drop_tap": ("layer3.1.conv2", 0, 2, 31, 33)}),
    "skip_with_main_branch_stats": ("halo", "layer2.0", {"skip_stats": "layer2.0"}),
    "unbiased_variance": ("halo", "layer4.0", {"unbiased": "layer4.0.norm2"}),
    "fuse_level_align_corners_false": ("halo", "fused", {"fuse_corners": 3}),
    "norm1_stats_of_another_frame": ("odd", "norm1", {"norm1_frame": (1, 0)}),
}


def encoder_model():
    """The model whose `fnet` the encoder stage tests run: fill_synthetic_(seed=3) weights, on the CPU."""
    from cotracker_amd.model import CoTrackerThreeOnline
    from cotracker_amd.weights import fill_synthetic_
    m = CoTrackerThreeOnline(stride=STRIDE, corr_radius=3, window_len=16).eval()
    fill_synthetic_(m, seed=3)
    return m


def encoder_frames(case):
    """[F,3,H,W] float32 in 0..255 on the CPU: synthetic_video(seed=9) frames, then ONE CONSTANT frame of 127.5 -- 0 after
    2 * (x / 255) - 1, so every convolution of that frame returns its bias at every pixel and every instance norm of the chain sees a
    variance of exactly 0: the eps path, (x - mean) * 1 / sqrt(1e-5)."""
    from cotracker_amd.synthetic import synthetic_video
    H, W, Fn = ENC_CASES[case]
    return torch.cat([synthetic_video(Fn - 1, H, W, seed=9)[0], torch.full((1, 3, H, W), 127.5)]).float().contiguous()


# ---- include/ctk.h as the C compiler sees it ----------------------------------------------------------------------------------------
def abi_structs():
    """C name -> ctypes mirror, for every struct that crosses the boundary."""
    from cotracker_amd import _lib as L
    return {"ctk_block_weights": L.BlockWeights, "ctk_model_weights": L.ModelWeights, "ctk_window_args": L.WindowArgs,
            "ctk_gemm_args": L.GemmArgs, "ctk_attn_args": L.AttnArgs, "ctk_attn_batch2": L.AttnBatch2,
            "ctk_window_batch": L.WindowBatch, "ctk_stream_args": L.StreamArgs, "ctk_ingest_args": L.IngestArgs,
            "ctk_former_weights": L.FormerWeights, "ctk_v2_window_args": L.V2WindowArgs, "ctk_v2_weights": L.V2Weights,
            "ctk_profile_row": L.ProfileRow}


@functools.lru_cache(maxsize=None)
def header_layout():
    """ONE C program, generated from the ctypes classes of cotracker_amd._lib (their field names are the C field names), compiled
    against include/ctk.h and run once per session ->
      "sizeof"    {C struct name: bytes},
      "offsetof"  {C struct name: {field: bytes}} for every field of every mirror,
      "constants" {"CTK_X": value} for every CTK_* #define / enumerator of the header that _lib mirrors as the number X, in the
                  number type _lib uses, and "as_long" the same values converted with (long)."""
    from cotracker_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "ctk.h")).read()
    defined = re.findall(r"#define (CTK_\w+)", header) + re.findall(r"\b(CTK_\w+) = -?\d", header)  # macros and enumerators
    names = sorted({n for n in defined if type(getattr(L, n[4:], None)) in (int, float)})
    lines = []
    for cname, cls in abi_structs().items():
        lines.append(f'printf("S {cname} - %zu\\n", sizeof({cname}));')
        lines += [f'printf("F {cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));' for f in cls._fields_]
    lines += [f'printf("K {n} %ld %.17g\\n", (long)({n}), (double)({n}));' for n in names]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "ctk.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    lay = {"sizeof": {}, "offsetof": {c: {} for c in abi_structs()}, "constants": {}, "as_long": {}}
    for kind, a, b, *v in (ln.split() for ln in out.splitlines()):
        if kind == "S":
            lay["sizeof"][a] = int(v[0])
        elif kind == "F":
            lay["offsetof"][a][b] = int(v[0])
        else:
            lay["as_long"][a] = int(b)
            lay["constants"][a] = float(v[0]) if isinstance(getattr(L, a[4:]), float) else int(b)
    return lay
