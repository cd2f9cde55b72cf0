"""ctk_track_field and ctk_warp_field on the GPU (csrc/field.hip) against the numpy restatement of tests/field_reference.py: every byte
of field, level, stats, of the poisoned, fenced destination (pitch padding included) and every flow bit.  The shapes are the smallest
that reach each path: one node tile and several, one LDS chunk of pairs and 32, every "to" form, a ring that has wrapped, logits and
the visible tensor, first_row, a hole; bytes, whole dwords and row tails, three pixel formats, strided source and destination, a
source box that fits the LDS and one that does not; then 1080p for the multi-tile path and 64-bit offsets, the ops layer, and the
predictor on a pushed ring stream."""
import ctypes as C

import numpy as np
import pytest
import torch

import field_reference as R
from ctk_support import HW, S, STEP, STRIDE, dev, recorded, t

pytestmark = pytest.mark.gpu

GUARD, POISON, FENCE = 64, 0x5A, 0xA5
TRACK_ROWS = {"field_accum": 1, "field_pyramid": 1, "field_resolve": 1}
ALL_ROWS = dict(TRACK_ROWS, warp_field=1)


def fenced(nbytes):
    """A poisoned device buffer of nbytes between two fences, 256-byte aligned -> (whole tensor with fences, the view between them)."""
    whole = torch.empty(256 + nbytes + 2 * GUARD, dtype=torch.uint8, device=dev())
    base = (-(whole.data_ptr() + GUARD)) % 256
    buf = whole[base:base + nbytes + 2 * GUARD]
    buf.fill_(FENCE)
    buf[GUARD:GUARD + nbytes].fill_(POISON)
    return buf, buf[GUARD:GUARD + nbytes]


def fences_hold(buf):
    b = buf.cpu().numpy()
    return (b[:GUARD] == FENCE).all() and (b[-GUARD:] == FENCE).all()


def raw_track(coords, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1, size=(1, 1), cs=4, radius=2,
              to=-1, lag=0, anchor=None, sx=1.0, sy=1.0):
    """The C-ABI call itself on fenced, poisoned outputs and workspace; checks every byte against the restatement and returns it."""
    from cotracker_amd import _lib as L
    coords = np.asarray(coords, dtype=np.float32)
    G, Rr, N, _ = coords.shape
    gh, gw = R.grid(size[0], cs), R.grid(size[1], cs)
    a = L.Field.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.F = G, N, N if N_out is None else N_out, Rr, f0, F
    a.H, a.W, a.cs, a.radius, a.to, a.lag, a.anchor_frame = size[0], size[1], cs, radius, to, lag, 0 if anchor is None else anchor[2]
    a.sx, a.sy, a.thresh, a.reserved = sx, sy, thresh, 0
    keep = [t(coords)]
    a.hist_coords = keep[0].data_ptr()
    for name, arr, dt in (("visible", visible, np.uint8), ("hist_vis", vis, np.float32), ("hist_conf", conf, np.float32), ("first_row", first_row, np.int32),
                          ("anchor_coords", None if anchor is None else anchor[0], np.float32),
                          ("anchor_visible", None if anchor is None else anchor[1], np.uint8)):
        if arr is not None:
            keep.append(t(np.asarray(arr, dtype=dt)))
            setattr(a, name, keep[-1].data_ptr())
    need = C.c_size_t(0)
    L.check(L.load().ctk_track_field_workspace_bytes(C.byref(a), C.byref(need)), "ctk_track_field_workspace_bytes")
    n = G * F * gh * gw
    bufs = [fenced(nb) for nb in (n * 8, n, G * F * 16, need.value)]
    a.field, a.level, a.stats = (b[1].data_ptr() for b in bufs[:3])
    res, rows = recorded(lambda: L.load().ctk_track_field(C.byref(a), bufs[3][1].data_ptr(), need.value, torch.cuda.current_stream().cuda_stream))
    L.check(res, "ctk_track_field")
    torch.cuda.synchronize()
    assert rows == TRACK_ROWS
    want = R.track_field(coords, visible=visible, vis=vis, conf=conf, thresh=thresh, first_row=first_row, N_out=N_out, f0=f0, F=F, size=size,
                         cs=cs, radius=radius, to=to, lag=lag, anchor=anchor, sx=sx, sy=sy)
    got = (bufs[0][1].cpu().numpy().view(np.int32).reshape(G, F, gh, gw, 2), bufs[1][1].cpu().numpy().reshape(G, F, gh, gw),
           bufs[2][1].cpu().numpy().view(np.int32).reshape(G, F, 4))
    for name, g_, w_ in zip(("field", "level", "stats"), got, want):
        bad = np.argwhere(g_ != w_)
        assert bad.size == 0, (name, bad[:4].tolist(), g_[tuple(bad[0])], w_[tuple(bad[0])])
    assert all(fences_hold(b[0]) for b in bufs)
    return want


def scene(seed, G, T, N, hw, p_visible=0.9):
    rng = np.random.default_rng(seed)
    H, W = hw
    p0 = rng.uniform(-0.1, 1.1, (G, 1, N, 2)) * np.array([W, H])
    coords = (p0 + np.cumsum(rng.normal(0, 1.5, (G, T, N, 2)), axis=1)).astype(np.float32)
    visible = (rng.uniform(size=(G, T, N)) < p_visible).astype(np.uint8)
    return coords, visible, rng


# hw, N, cs, radius, G, what
TRACK_CASES = [
    ((29, 37), 1, 2, 1, 1, "to"),         # one pair, one tile, most nodes from the pyramid
    ((29, 37), 5, 3, 2, 3, "ring"),       # logits on a ring that has wrapped, lag 1
    ((45, 70), 300, 4, 4, 1, "forward"),  # first_row, a negative lag, a scale
    ((45, 70), 5, 2, 4, 3, "anchor"),     # an anchor with a reassigned slot; 2 x 2 node tiles
    ((67, 130), 300, 3, 1, 3, "ring"),    # logits + first_row on the ring, 2 chunks of pairs
    ((67, 130), 300, 2, 2, 1, "hole"),    # 3 x 2 node tiles, a hole that needs levels >= 2
    ((67, 130), 8192, 4, 2, 1, "to"),     # 32 chunks of pairs
    ((29, 37), 300, 4, 1, 1, "nothing"),  # no pair at all
]


@pytest.mark.parametrize("hw,N,cs,radius,G,what", TRACK_CASES)
def test_track_field_equals_the_restatement(hw, N, cs, radius, G, what):
    T = 7
    coords, visible, rng = scene(N + cs, G, T, N, hw)
    kw = dict(size=hw, cs=cs, radius=radius)
    if what == "to":
        want = raw_track(coords, visible=visible, to=2, f0=0, F=T, **kw)
        assert want[2][..., 0].max() > 0 and (want[0][:, 2] == 0).all()  # the field of frame 2 against itself is zero
    elif what == "ring":
        K = 5  # rows of frames 9 .. 13, frame f in row f % 5
        vis, conf = rng.normal(1.0, 2.0, (G, K, N)).astype(np.float32), rng.normal(1.0, 2.0, (G, K, N)).astype(np.float32)
        first = rng.integers(8, 13, (G, N)).astype(np.int32) if N > 5 else None
        want = raw_track(coords[:, :K], vis=vis, conf=conf, thresh=0.6, first_row=first, f0=11, F=3, lag=1, N_out=max(N - 3, 1), sx=0.75, sy=1.25, **kw)
        assert N <= 5 or want[2][..., 0].max() > 0
    elif what == "forward":
        first = rng.integers(0, 4, (G, N)).astype(np.int32)
        first[:, 3] = R.INT32_MAX
        want = raw_track(coords, visible=visible, first_row=first, f0=0, F=5, lag=-2, sx=1.5, sy=0.5, **kw)
        assert want[2][..., 0].min() > 20
    elif what == "anchor":
        first = np.zeros((G, N), dtype=np.int32)
        first[:, 1] = 5  # reassigned after the anchor was taken on frame 3
        visible[:] = 1
        anchor = (coords[:, 3].copy(), visible[:, 3].copy(), 3)
        want = raw_track(coords, visible=visible, first_row=first, anchor=anchor, f0=4, F=3, **kw)
        assert (want[2][..., 0] == 4).all()  # 4 of the 5 slots: the anchor's frame lies below slot 1's first row
    elif what == "hole":
        p = rng.uniform(0, 1, (N, 2)) * np.array([130, 67])
        p[(np.abs(p[:, 0] - 65) < 30) & (np.abs(p[:, 1] - 33) < 22)] = (-500.0, -500.0)  # moved out of everyone's reach
        coords = np.stack([p, p + np.array([1.5, 0.25])]).astype(np.float32)[None]
        want = raw_track(coords, visible=np.ones((1, 2, N), dtype=np.uint8), to=1, **kw)
        assert want[1][0, 0, 8, 16] >= 2 and want[2][0, 0, 2] >= 2 and (want[1] == 0).sum() > 100
    else:
        want = raw_track(coords, visible=np.zeros_like(visible), lag=1, f0=1, F=2, **kw)
        assert (want[0] == 0).all() and (want[1] == R.NO_LEVEL).all() and (want[2] == (0, 0, R.NO_LEVEL, 0)).all()


def rows_view(buf, offset, F, rows, row_bytes, frame_stride, row_stride):
    assert offset + (F - 1) * frame_stride + (rows - 1) * row_stride + row_bytes <= buf.size
    return np.lib.stride_tricks.as_strided(buf[offset:], shape=(F, rows, row_bytes), strides=(frame_stride, row_stride, 1))


def raw_warp(pics, field, cs, border, fill, layout, src_pad=(0, 0), dst_pad=(0, 0), dst_off=0, flow=True, one_source=False):
    """The C-ABI call itself: pics uint8 [F,H,W,3] / [F,3,H,W] / [F,H,W] laid out with rows padded by pad[0] and frames by pad[1]
    elements, the destination poisoned, fenced and dst_off bytes off its 256-byte aligned allocation.  Checks every byte of the
    destination against the restatement (padding: still the poison), the fences, the source and every flow bit."""
    from cotracker_amd import _lib as L
    F = field.shape[0]
    C_ = 1 if pics.ndim == 3 else 3
    H, W = pics.shape[1:3] if (pics.ndim == 3 or layout == R.HWC) else pics.shape[2:4]
    planar = C_ == 3 and layout == R.CHW
    rows, row_bytes = (C_ * H, W) if planar else (H, C_ * W)
    (srs, sfs), (drs, dfs) = [(row_bytes + pad[0], rows * (row_bytes + pad[0]) + pad[1]) for pad in (src_pad, dst_pad)]
    Fs = 1 if one_source else F
    rng = np.random.default_rng(F * H + W)
    src = rng.integers(0, 256, Fs * sfs, dtype=np.uint8)  # (what lies between the rows is noise: it must not be read)
    rows_view(src, 0, Fs, rows, row_bytes, sfs, srs)[...] = pics[:Fs].reshape(Fs, rows, row_bytes)
    nd = (F - 1) * dfs + (rows - 1) * drs + row_bytes
    whole, dst = fenced(dst_off + nd)
    wf, fl = fenced(F * H * W * 8)
    src_d, f_d = t(src), t(np.ascontiguousarray(field, dtype=np.int32))
    a = L.Field.WarpArgs()
    a.F, a.H, a.W, a.C, a.layout, a.border, a.cs, a.reserved = F, H, W, C_, layout, border, cs, 0
    for k in range(3):
        a.fill[k] = fill[k]
    a.src_frame_stride, a.src_row_stride, a.dst_frame_stride, a.dst_row_stride = 0 if one_source else sfs, srs, dfs, drs
    a.field, a.src, a.dst, a.flow = f_d.data_ptr(), src_d.data_ptr(), dst.data_ptr() + dst_off, fl.data_ptr() if flow else None
    res, rows_ = recorded(lambda: L.load().ctk_warp_field(C.byref(a), torch.cuda.current_stream().cuda_stream))
    L.check(res, "ctk_warp_field")
    torch.cuda.synchronize()
    assert rows_ == {"warp_field": 1}
    ref = R.warp_field(pics[:Fs], field, cs, border, fill, layout)
    want = np.full(dst_off + nd, POISON, dtype=np.uint8)
    rows_view(want, dst_off, F, rows, row_bytes, dfs, drs)[...] = ref.reshape(F, rows, row_bytes)
    got = dst.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert fences_hold(whole) and fences_hold(wf) and np.array_equal(src_d.cpu().numpy(), src)
    got_flow = fl.cpu().numpy().view(np.int32).reshape(F, H, W, 2)
    if flow:
        assert np.array_equal(got_flow, R.flow(field, H, W, cs).view(np.int32))
    else:
        assert (fl.cpu().numpy() == POISON).all()
    return ref


def four_fields(rng, H, W, cs):
    """Zero, a smooth sub-pixel field, a rough one of +-9 pixels (its tiles' boxes still fit the LDS), one that leads mostly outside."""
    gh, gw = R.grid(H, cs), R.grid(W, cs)
    f = np.zeros((4, gh, gw, 2), dtype=np.int32)
    f[1] = rng.integers(-200, 200, (gh, gw, 2))
    f[2] = rng.integers(-9 * 256, 9 * 256, (gh, gw, 2))
    f[3] = f[1]
    f[3, ..., 0] += (W - 6) * 256
    return f


# H, W, cs, dst row padding, dst frame padding, dst offset in bytes
WARP_SHAPES = [
    (29, 37, 2, 0, 0, 0),    # rows of 111 / 37 bytes: the byte path, a row tail of one pixel
    (40, 64, 3, 8, 4, 0),    # padded rows: whole dwords, no tail
    (45, 70, 4, 2, 8, 0),    # whole dwords plus a tail of two pixels; 2 x 3 tiles of 64 x 16, partial in x and y
    (40, 64, 3, 8, 4, 1),    # the same surface one byte off: the byte path
    (67, 130, 3, 2, 0, 0),   # 3 x 5 tiles
]


@pytest.mark.parametrize("fmt", ("hwc", "chw", "one"))
@pytest.mark.parametrize("H,W,cs,row_pad,frame_pad,off", WARP_SHAPES)
def test_warp_field_equals_the_restatement(H, W, cs, row_pad, frame_pad, off, fmt):
    rng = np.random.default_rng(H + W + cs)
    field = four_fields(rng, H, W, cs)
    shape = {"hwc": (4, H, W, 3), "chw": (4, 3, H, W), "one": (4, H, W)}[fmt]
    pics = rng.integers(0, 256, shape, dtype=np.uint8)
    layout = R.CHW if fmt == "chw" else R.HWC
    for border in (R.FILL, R.EDGE):
        ref = raw_warp(pics, field, cs, border, (7, 200, 90), layout, src_pad=(3, 5), dst_pad=(row_pad, frame_pad), dst_off=off)
        assert np.array_equal(ref[0], pics[0])  # a zero field copies
    if fmt == "one":  # one source for every field; the flow not asked for
        raw_warp(pics, field, cs, R.FILL, (9, 9, 9), layout, dst_pad=(row_pad, frame_pad), dst_off=off, flow=False, one_source=True)


def test_warp_field_wild_fields_and_the_box_that_does_not_fit():
    """A field whose tiles' source boxes exceed the LDS (+-60 pixels from node to node): the fallback to memory; and one that holds
    the extremes of int32: every tap is clamped, nothing outside the picture is read (the fences and the noise between the rows)."""
    rng = np.random.default_rng(8)
    H, W, cs = 67, 130, 2
    gh, gw = R.grid(H, cs), R.grid(W, cs)
    field = rng.integers(-60 * 256, 60 * 256, (3, gh, gw, 2)).astype(np.int32)
    field[1, ::3, ::2] = np.iinfo(np.int32).min
    field[1, 1::3, 1::2] = np.iinfo(np.int32).max
    field[2] = rng.integers(-(2 ** 31), 2 ** 31, (gh, gw, 2), dtype=np.int64).astype(np.int32)
    for fmt, shape, layout in (("hwc", (3, H, W, 3), R.HWC), ("chw", (3, 3, H, W), R.CHW), ("one", (3, H, W), R.HWC)):
        pics = rng.integers(0, 256, shape, dtype=np.uint8)
        for border in (R.FILL, R.EDGE):
            raw_warp(pics, field, cs, border, (1, 2, 3), layout, src_pad=(1, 0), dst_pad=(2, 0))


def test_full_hd_multi_tile():
    """One 1080 x 1920 single-channel picture, 1024 points, c = 16: 8 x 5 node tiles, 30 x 68 pixel tiles."""
    rng = np.random.default_rng(1)
    H, W, N = 1080, 1920, 1024
    p = rng.uniform(0, 1, (N, 2)) * np.array([W, H])
    p[(np.abs(p[:, 0] - 900) < 250) & (np.abs(p[:, 1] - 500) < 200)] += 4000.0  # a hole
    q = (p - np.array([W / 2, H / 2])) * 1.01 + np.array([W / 2 + 3.0, H / 2 - 2.0])
    coords = np.stack([p, q]).astype(np.float32)[None]
    want = raw_track(coords, visible=np.ones((1, 2, N), dtype=np.uint8), to=1, size=(H, W), cs=4, radius=2)
    assert want[2][0, 0, 0] > 900 and want[2][0, 0, 2] >= 2
    pic = rng.integers(0, 256, (1, H, W), dtype=np.uint8)
    raw_warp(pic, want[0][0], 4, R.FILL, (0, 0, 0), R.HWC, dst_pad=(64, 0))


def test_ops_layer():
    from cotracker_amd import ops
    H, W, T, N = 45, 70, 6, 80
    coords, visible, rng = scene(4, 2, T, N, (H, W))
    tr, vi = t(coords), t(visible)
    first = rng.integers(0, 3, (2, N)).astype(np.int32)
    (field, level, stats), rows = recorded(lambda: ops.track_field(tr, vi.bool(), size=(H, W), cell=8, radius=2, lag=1, first_row=t(first).long()))
    assert rows == TRACK_ROWS
    want = R.track_field(coords, visible=visible, first_row=first, f0=0, F=T, size=(H, W), cs=3, radius=2, lag=1)
    assert all(np.array_equal(g_.cpu().numpy(), w_) for g_, w_ in zip((field, level, stats), want))
    # forward flow past the last frame: rows are appended, frame T - 1 has nothing to lead to
    fwd = ops.track_field(tr[0], vi[0], size=(H, W), cell=8, lag=-1, first_frame=2, frames=4, N_out=50)
    want = R.track_field(np.concatenate([coords[:1], np.zeros((1, 1, N, 2), np.float32)], 1), visible=np.concatenate([visible[:1], np.zeros((1, 1, N), np.uint8)], 1),
                         N_out=50, f0=2, F=4, size=(H, W), cs=3, radius=2, lag=-1)
    assert all(np.array_equal(g_.cpu().numpy(), w_) for g_, w_ in zip(fwd, want)) and want[2][0, 3, 0] == 0 and want[2][0, 2, 0] > 0
    # propagate = track_field(to) + warp_field, four launches; a mask, planar and channels-last pictures; a view as destination
    mask = t(rng.integers(0, 2, (H, W), dtype=np.uint8) * 255)
    out, rows = recorded(lambda: ops.propagate(mask, tr[0], vi[0], src_frame=1, frames=(2, 3), cell=8, radius=2))
    assert rows == ALL_ROWS and tuple(out.shape) == (3, H, W)
    f_to = R.track_field(coords[:1], visible=visible[:1], f0=2, F=3, size=(H, W), cs=3, radius=2, to=1)[0][0]
    assert np.array_equal(out.cpu().numpy(), R.warp_field(mask.cpu().numpy()[None], f_to, 3))
    pic = t(rng.integers(0, 256, (3, H, W), dtype=np.uint8))
    big = torch.full((3, 3, H, W + 8), POISON, dtype=torch.uint8, device=dev())
    res = ops.propagate(pic, tr[0], vi[0], src_frame=1, frames=(2, 3), cell=8, border="edge", out=big[..., 4:W + 4])
    b = big.cpu().numpy()
    assert res.data_ptr() == big[..., 4:W + 4].data_ptr() and (b[..., :4] == POISON).all() and (b[..., W + 4:] == POISON).all()
    assert np.array_equal(b[..., 4:W + 4], R.warp_field(pic.cpu().numpy()[None], f_to, 3, R.EDGE, layout=R.CHW))
    # warp_field with the flow, dense_flow
    src = t(rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8))
    out, flow = ops.warp_field(src, field[0], cell=8, fill=(5, 6, 7), flow=True)
    want_field = field[0].cpu().numpy()
    assert np.array_equal(out.cpu().numpy(), R.warp_field(src.cpu().numpy(), want_field, 3, R.FILL, (5, 6, 7)))
    assert np.array_equal(flow.cpu().numpy().view(np.int32), R.flow(want_field, H, W, 3).view(np.int32))
    dflow, rows = recorded(lambda: ops.dense_flow(tr[1], vi[1], size=(H, W), lag=1, cell=8, first_row=t(first[1])))
    assert rows == ALL_ROWS and np.array_equal(dflow.cpu().numpy().view(np.int32), R.flow(field[1].cpu().numpy(), H, W, 3).view(np.int32))
    for bad in (dict(lag=0), dict(lag=1, to=2), dict(), dict(to=T), dict(to=-1), dict(lag=1, cell=12), dict(lag=1, radius=5), dict(lag=1, N_out=N + 1),
                dict(lag=1, frames=T + 1), dict(anchor=ops.FieldAnchor(tr[:, 0], vi[:, 0], 0))):  # (the anchor's tensors are views: not contiguous)
        with pytest.raises(ValueError):
            ops.track_field(tr, vi, size=(H, W), **bad)
    for bad in (dict(out=src), dict(border="wrap"), dict(fill=(0, 0)), dict(fill=(0, 0, 256)), dict(cell=16)):
        with pytest.raises(ValueError):
            ops.warp_field(src, field[0], **dict(dict(cell=8), **bad))


# ---- the predictor ------------------------------------------------------------------------------------------------------------------
RAW = (100, 140)


def small_predictor(history, spare):
    from cotracker_amd.model import CoTrackerThreeOnline
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    from cotracker_amd.weights import fill_synthetic_
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=S)
    model = CoTrackerThreeOnline(stride=STRIDE, corr_radius=3, window_len=S, model_resolution=HW).eval()
    fill_synthetic_(model, seed=5)
    model.hip_graph, model.batch_mode = True, "loop"
    p.model, p.interp_shape, p.step = model, HW, STEP
    p.spare_points, p.history_frames = spare, history
    return p.to(dev())


def test_pin_propagate_and_dense_flow_on_a_push_stream(monkeypatch):
    """Ring (16 rows) + graph on, frames pushed as uint8; a twin on the same ring that never asks, and a stream without a ring whose
    rows are the reference.  The tracks are bit-identical with and without the calls and nothing is re-captured; what propagate and
    dense_flow return equals the restatement on the history as recent() emits it; a picture carried through an anchor pinned K + 8
    frames before equals ops.propagate on the unbounded stream's rows.  The small model's weights are synthetic and follow nothing,
    so the exact-shift property is checked on a planted history at the end: the ring's rows are overwritten with points that move
    by whole pixels, and the propagated mask is the shifted mask exactly."""
    from cotracker_amd import ops
    from cotracker_amd.synthetic import synthetic_video
    K, G, N, spare = 16, 2, 6, 2
    T = S + 9 * STEP  # 44 frames
    video = synthetic_video(T, *RAW, seed=11)[0].permute(0, 2, 3, 1).round().to(torch.uint8).contiguous().to(dev())
    g = torch.Generator().manual_seed(2)
    q = torch.rand(G, N, 3, generator=g) * torch.tensor([1.0, RAW[1] - 1.0, RAW[0] - 1.0])
    q[..., 0] = torch.tensor([0.0, 0.0, 2.0, 5.0, 9.0, 30.0])
    q = q.to(dev())
    captures = []
    orig = ops.WindowGraph._capture

    def counting(self, *a, **k):
        captures.append(1)
        return orig(self, *a, **k)
    monkeypatch.setattr(ops.WindowGraph, "_capture", counting)
    p, twin, free = small_predictor(K, spare), small_predictor(K, spare), small_predictor(None, spare)
    for x in (p, twin, free):
        x(torch.zeros(1, 1, 3, *RAW, device=dev()), is_first_step=True, queries=q, add_support_grid=True)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.pin()
    Nu = N + spare
    rng = np.random.default_rng(0)
    mask = t(rng.integers(0, 2, RAW, dtype=np.uint8) * 255)
    pic = t(rng.integers(0, 256, (*RAW, 3), dtype=np.uint8))

    def ring():
        done = p.model._gstream.committed
        tr, vi = p.recent(min(done, K))
        base = done - tr.shape[1]
        ring_c, ring_v = np.zeros((G, K, Nu, 2), dtype=np.float32), np.zeros((G, K, Nu), dtype=np.uint8)
        for i in range(tr.shape[1]):
            ring_c[:, (base + i) % K], ring_v[:, (base + i) % K] = tr[:, i].cpu().numpy(), vi[:, i].cpu().numpy()
        first = None if p._first_row is None else np.clip(p._first_row.cpu().numpy(), 0, R.INT32_MAX).astype(np.int32)
        return ring_c, ring_v, first
    kept, calls = {}, 0
    for k, t0 in enumerate(range(0, T - S + 1, STEP)):
        new = video[:S] if k == 0 else video[t0 + S - STEP:t0 + S]
        c0 = len(captures)
        got = p.push_frames(new, add_support_grid=True)
        c1 = len(captures)
        ref = twin.push_frames(new, add_support_grid=True)
        assert len(captures) - c1 == c1 - c0, (k, c0, c1, len(captures))  # nothing is re-captured: the twin, which never asks, captures as often
        free.push_frames(new, add_support_grid=True)
        c3 = len(captures)
        assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(got[1], ref[1]), k
        done = p.model._gstream.committed
        if k == 4:  # done = 24: frame 16 is the oldest of the window just tracked, the next window starts behind it: it is final
            anchor = p.pin(frame=done - S)
            assert anchor.frame == done - S == 16 and anchor.group == 0 and len(captures) == c3
            assert tuple(anchor.coords.shape) == (1, p.queries.shape[1], 2) and anchor.visible.dtype == torch.uint8
            kept["anchor"] = anchor
            calls += 1
        if k in (1, 3, 5):  # a frame of the ring as the source: the window just tracked, group 0, a mask
            c, v, first = ring()
            src_frame = done - 6
            out, rows = recorded(lambda: p.propagate(mask, src_frame, cell=8, radius=2))
            assert rows == ALL_ROWS and len(captures) == c3 and tuple(out.shape) == (STEP, *RAW) and out.dtype == torch.uint8
            f_ = R.track_field(c[:1], visible=v[:1], first_row=None if first is None else first[:1], f0=done - STEP, F=STEP, size=RAW, cs=3,
                               radius=2, to=src_frame)
            assert np.array_equal(out.cpu().numpy(), R.warp_field(mask.cpu().numpy()[None], f_[0][0], 3))
            kept["pairs"] = kept.get("pairs", 0) + int(f_[2][..., 0].sum())
            flow, rows = recorded(lambda: p.dense_flow(lag=2, cell=8, group=1))
            assert rows == ALL_ROWS and tuple(flow.shape) == (STEP, *RAW, 2)
            f_ = R.track_field(c[1:], visible=v[1:], first_row=None if first is None else first[1:], f0=done - STEP, F=STEP, size=RAW, cs=3,
                               radius=2, lag=2)
            assert np.array_equal(flow.cpu().numpy().view(np.int32), R.flow(f_[0][0], *RAW, 3).view(np.int32))
            calls += 2
        if k == 3:
            for x in (p, twin, free):
                x.add_queries(torch.tensor([[float(t0 + S + 1), 60.0, 50.0]], device=dev()), group=1)
        if k == 9:  # done = 44, the ring holds frames 28 .. 43: frame 16 left it long ago
            a = kept["anchor"]
            first_frame = a.frame + K + 8
            with pytest.raises(ValueError, match="left the history"):
                p.propagate(pic, a.frame, first_frame=first_frame, n=STEP)
            with pytest.raises(ValueError, match="pinned on group"):
                p.propagate(pic, a, first_frame=first_frame, n=STEP, group=1)
            out, rows = recorded(lambda: p.propagate(pic, a, first_frame=first_frame, n=STEP, border="edge"))
            assert rows == ALL_ROWS and tuple(out.shape) == (STEP, *RAW, 3)
            tr, vi = free._emit_result(0, done)  # the unbounded stream's rows: raw-video pixels, thresholded visibility
            want = ops.propagate(pic, tr[0], vi[0], src_frame=a.frame, frames=(first_frame, STEP), border="edge")
            assert torch.equal(out, want)
            # not vacuous: points of the anchor are still followed 24 frames on (the synthetic weights move them by less than the
            # 1/16 pixel of a position, so the pictures themselves say little here: the planted history below moves)
            pairs = ops.track_field(tr[0], vi[0], size=RAW, to=a.frame, first_frame=first_frame, frames=STEP)[2][0, :, 0]
            assert int(pairs.min()) >= 2
            one = p.propagate(pic.permute(2, 0, 1).contiguous(), a, first_frame=first_frame + 1, n=1, border="edge")
            assert torch.equal(one[0].permute(1, 2, 0), want[1])
            with pytest.raises(ValueError, match="beyond what has been tracked"):
                p.propagate(pic, a, first_frame=done - 1, n=2)
            with pytest.raises(ValueError, match="beyond what has been tracked"):
                p.dense_flow(lag=-1)  # forward flow of the newest frames needs frames not tracked yet
            p.dense_flow(n=2, first_frame=done - 4, lag=-2)
            assert len(captures) == c3
            calls += 3
    assert calls == 10 and kept["pairs"] > 0
    # the planted history: every point of group 0 moves by whole raw-video pixels from frame to frame
    gs = p.model._gstream
    done = gs.committed
    (Hr, Wr), (ih, iw) = RAW, HW
    sx, sy = np.float32((Wr - 1) / (iw - 1)), np.float32((Hr - 1) / (ih - 1))
    off = np.cumsum(rng.integers(-3, 4, (done, 2)), axis=0)
    base = rng.integers(20, 80, (gs.N, 2)).astype(np.float64)
    for f in range(done - K, done):
        raw = base + off[f]
        gs.hist[0][0, f % K] = t((raw / np.array([sx, sy], dtype=np.float64)).astype(np.float32))
    gs.hist[1][0].fill_(20.0)
    gs.hist[2][0].fill_(20.0)
    src_frame = done - 7
    out = p.propagate(mask, src_frame, first_frame=done - 5, n=5, cell=16, radius=1).cpu().numpy()
    m = mask.cpu().numpy()
    moved = 0
    for j, f in enumerate(range(done - 5, done)):
        dx, dy = (off[src_frame] - off[f]).tolist()  # out(x, y) = mask(x + dx, y + dy), the fill where that lies outside
        want = np.zeros_like(m)
        ys, xs = np.arange(Hr)[:, None] + dy, np.arange(Wr)[None, :] + dx
        inside = (ys >= 0) & (ys < Hr) & (xs >= 0) & (xs < Wr)
        want[inside] = m[np.clip(ys, 0, Hr - 1), np.clip(xs, 0, Wr - 1)][inside]
        assert np.array_equal(out[j], want), (f, dx, dy)
        moved += abs(dx) + abs(dy)
    assert moved > 0
    # the same through an anchor pinned on the planted source frame
    assert np.array_equal(p.propagate(mask, p.pin(frame=src_frame), first_frame=done - 5, n=5, cell=16, radius=1).cpu().numpy(), out)
    for x in (p, twin, free):
        x.finish()
