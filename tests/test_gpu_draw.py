"""Draw tracks (-m gpu): the two kernels behind ops.draw_tracks, ops.StreamGroups.draw and CoTrackerOnlinePredictor.draw
(csrc/draw.hip: ctk_draw_tracks) against the numpy restatement of tests/draw_reference.py, which tests/test_draw_host.py also holds a
g++ build of csrc/draw_math.h against.

Every comparison is np.array_equal on EVERY byte of the buffer the frames lie in: the bytes of the row pitch beyond W pixels and a
guard after the last frame are random sentinels that must survive."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import draw_reference as R
from ctk_support import HW, S, STEP, STRIDE, dev, recorded, t

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
GUARD = 64


# ---- surfaces -------------------------------------------------------------------------------------------------------------------
def surface(layout, F, H, W, row_stride, seed):
    """-> (flat uint8 numpy buffer of random bytes with a guard behind the last frame, shape, strides) of F frames in `layout`."""
    rows = H if layout == "hwc" else 3 * H
    fs = rows * row_stride
    buf = np.random.RandomState(seed).randint(0, 256, F * fs + GUARD).astype(np.uint8)
    if layout == "hwc":
        return buf, (F, H, W, 3), (fs, row_stride, 3, 1)
    return buf, (F, 3, H, W), (fs, H * row_stride, row_stride, 1)


def np_view(buf, shape, strides):
    return np.lib.stride_tricks.as_strided(buf, shape, strides)


def expected(buf, shape, strides, layout, **kw):
    """The whole buffer after draw_reference.draw on the frames in it."""
    want = buf.copy()
    v = np_view(want, shape, strides)
    pics = v if layout == "hwc" else v.transpose(0, 2, 3, 1)
    out = R.draw(np.ascontiguousarray(pics), **kw)
    v[...] = out if layout == "hwc" else out.transpose(0, 3, 1, 2)
    return want


def raw_draw(frames, out, layout, hist, colors, *, f0, trail, alpha, radius, half_width, max_jump, sx, sy, N_out, visible=None,
             logits=None, thresh=0.6, first_row=None):
    """ctk_draw_tracks as the C-ABI sees it: hist [G,R,N,2] read by f % R, N_out <= N, either form of visibility."""
    from cotracker_amd import _lib as L
    from cotracker_amd import ops
    a = L.Draw.Args()
    ops._draw_style(a, trail, radius, half_width, alpha, max_jump, "test")
    a.G, a.R, a.N = hist.shape[:3]
    a.N_out, a.f0, a.sx, a.sy, a.thresh = N_out, f0, sx, sy, thresh
    keep = [hist, colors, visible, first_row] + list(logits or ())
    a.hist_coords, a.colors = hist.data_ptr(), colors.data_ptr()
    if visible is not None:
        a.visible = visible.data_ptr()
    else:
        a.hist_vis, a.hist_conf = (x.data_ptr() for x in logits)
    if first_row is not None:
        a.first_row = first_row.data_ptr()
    res = ops._draw_launch(a, frames, out, layout, "test")
    del keep
    return res


# ---- 1. the small ring case: every rule, by hand ----------------------------------------------------------------------------------------
H1, W1, F1, G1, N1, NOUT1, R1, L1 = 37, 53, 3, 2, 5, 4, 8, 3
SX, SY = 1.37, 0.81
MAX_JUMP = 20
ALPHA1 = [200, 143, 63, 15]
COLORS1 = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [9, 9, 9]],
                    [[0, 255, 255], [255, 0, 255], [128, 64, 32], [10, 200, 90], [7, 7, 7]]], dtype=np.uint8)
FIRST1 = np.array([[0, 0, 0, INT32_MAX, 0], [5, 0, 0, 0, 0]], dtype=np.int32)


def hand_point(g, n, f):
    """-> (pixel x, pixel y, visible) of slot (g, n) on frame f; None for x: a NaN coordinate."""
    if g == 0:
        return [(3 * f - 18, 8, True),                                  # frame 6: pixel (0, 8), a tile corner; early frames outside
                ((-40, 80, True) if f == 7 else (51 + f % 2, 35 + f % 3, True)),  # half outside; frame 7 wholly outside (and two jumps)
                ((None, 20, True) if f == 7 else (20 + f, 20, True)),   # a NaN coordinate on frame 7
                (25, 25, True),                                         # an empty slot (first_row = INT32_MAX)
                (30, 30, True)][n]                                      # n >= N_out: never drawn
    return [(5 + 2 * f, 12 + f, True),                                  # first_row = 5: in the middle of the trail of pictures 6 .. 8
            (40 - f, 5 + 2 * f, f not in (2, 6)),                       # an invisible middle frame: a ring, two segments dropped
            ({7: 10 + MAX_JUMP + 1, 8: 10 + 2 * MAX_JUMP + 1}.get(f, 10), 30, True),  # 6 -> 7 jumps max_jump + 1, 7 -> 8 max_jump
            (3, 8, True),                                               # static (dd == 0), on the pixel of (0, 0) at frame 7: order
            (33, 33, True)][n]


def hand_history(last):
    """The ring after frame `last`: rows f % R of frames last - R + 1 .. last (those >= 0); the other rows hold NaN."""
    hist = np.full((G1, R1, N1, 2), np.nan, dtype=np.float32)
    vis = np.zeros((G1, R1, N1), dtype=np.uint8)
    for f in range(max(last - R1 + 1, 0), last + 1):
        for g in range(G1):
            for n in range(N1):
                x, y, v = hand_point(g, n, f)
                hist[g, f % R1, n] = (np.nan if x is None else np.float32(x) / np.float32(SX), np.float32(y) / np.float32(SY))
                vis[g, f % R1, n] = v
    return hist, vis


@functools.lru_cache(maxsize=None)
def ring_case(f0, layout, row_stride):
    """-> (buffer, shape, strides, history, visibility, the expected buffer): the reference is computed once per case."""
    hist, vis = hand_history(f0 + F1 - 1)
    buf, shape, strides = surface(layout, F1, H1, W1, row_stride, seed=f0 + row_stride)
    want = expected(buf, shape, strides, layout, tracks=hist, visible=vis, colors=COLORS1, f0=f0, trail=L1, alpha=ALPHA1 + [0] * 61, radius=4,
                    half_width=1, max_jump=MAX_JUMP, sx=SX, sy=SY, first_row=FIRST1, N_out=NOUT1)
    return buf, shape, strides, hist, vis, want


def test_hand_history_hits_the_rules():
    """The case is what its comments say: quantised pixels, the tile corner, the shared pixel, the exact jumps."""
    hist, vis = hand_history(8)
    q = lambda g, n, f: (R.quant(hist[g, f % R1, n, 0], SX), R.quant(hist[g, f % R1, n, 1], SY))  # noqa: E731
    assert q(0, 0, 6) == ((True, 0), (True, 8)) and q(0, 0, 7) == ((True, 3), (True, 8)) == q(1, 3, 7)
    assert q(0, 1, 7) == ((True, -40), (True, 80)) and q(0, 1, 8) == ((True, 51), (True, 37)) and not q(0, 2, 7)[0][0]
    assert q(1, 2, 7)[0][1] - q(1, 2, 6)[0][1] == MAX_JUMP + 1 and q(1, 2, 8)[0][1] - q(1, 2, 7)[0][1] == MAX_JUMP
    assert not vis[1, 6 % R1, 1] and vis[1, 5, 1] and vis[1, 7, 1]
    for f0 in (6, 1):
        *_, want = ring_case(f0, "hwc", W1 * 3 + 5)
        buf = ring_case(f0, "hwc", W1 * 3 + 5)[0]
        assert (want != buf).sum() > 300  # something is drawn


@pytest.mark.parametrize("f0", [6, 1], ids=["wrap", "before0"])  # frames 6, 7, 8 in rows 6, 7, 0; frames 1 .. 3 with f0 - L < 0
@pytest.mark.parametrize("layout,pad", [("hwc", 5), ("hwc", 7), ("chw", 5), ("chw", 7)])  # pitches 164 / 166 and 58 / 60: dwords or bytes
def test_small_ring_case(layout, pad, f0):
    row_stride = (W1 * 3 if layout == "hwc" else W1) + pad
    buf, shape, strides, hist, vis, want = ring_case(f0, layout, row_stride)
    kw = dict(f0=f0, trail=L1, alpha=ALPHA1, radius=4, half_width=1, max_jump=MAX_JUMP, sx=SX, sy=SY, N_out=NOUT1, visible=t(vis),
              first_row=t(FIRST1))
    hist_d, colors_d = t(hist), t(COLORS1)
    # in place
    flat = t(buf)
    got = raw_draw(torch.as_strided(flat, shape, strides), None, layout, hist_d, colors_d, **kw)
    assert got.data_ptr() == flat.data_ptr()
    assert np.array_equal(flat.cpu().numpy(), want)
    # src -> dst: the same pictures; src untouched; dst's own padding and guard (other random bytes) survive
    src, other = t(buf), surface(layout, F1, H1, W1, row_stride, seed=99)[0]
    dst = t(other)
    raw_draw(torch.as_strided(src, shape, strides), torch.as_strided(dst, shape, strides), layout, hist_d, colors_d, **kw)
    assert np.array_equal(src.cpu().numpy(), buf)
    want_dst = other.copy()
    np_view(want_dst, shape, strides)[...] = np_view(want, shape, strides)
    assert np.array_equal(dst.cpu().numpy(), want_dst)
    assert np.array_equal(np_view(dst.cpu().numpy(), shape, strides), np_view(flat.cpu().numpy(), shape, strides))


# ---- 2. the list machinery: more than one chunk of records, a tile whose list exceeds a chunk ----------------------------------------
H2, W2, N2 = 70, 130, 300


CLUSTER_SURFACES = [("hwc", 0), ("chw", 0), ("hwc", 2), ("chw", 2)]


@functools.lru_cache(maxsize=None)
def cluster_case():
    rng = np.random.RandomState(5)
    T = 3
    tracks = np.empty((T, N2, 2), dtype=np.float32)
    start = np.concatenate([rng.uniform([124, 5], [132, 11], (285, 2)),     # around the tile corner (128, 8)
                            rng.uniform([-6, -6], [W2 + 6, H2 + 6], (15, 2))])  # and anywhere, the border included
    for f in range(T):
        tracks[f] = start + f * rng.uniform(-2, 2, (N2, 2))
    visible = rng.rand(T, N2) < 0.8
    colors = rng.randint(0, 256, (N2, 3)).astype(np.uint8)
    alpha = [180, 90]
    want = {}
    for layout, pad in CLUSTER_SURFACES:  # dense rows of 390 / 130 bytes: the byte path; pitches of 392 / 132: the dword path
        buf, shape, strides = surface(layout, 2, H2, W2, (W2 * 3 if layout == "hwc" else W2) + pad, seed=7)
        want[layout, pad] = (buf, shape, strides, expected(buf, shape, strides, layout, tracks=tracks[None], visible=visible[None], colors=colors[None],
                                                      f0=1, trail=1, alpha=alpha + [0] * 63, radius=3, half_width=1, max_jump=256))
    return tracks, visible, colors, alpha, want


@pytest.mark.parametrize("layout,pad", CLUSTER_SURFACES)
def test_list_machinery(layout, pad):
    from cotracker_amd import ops
    tracks, visible, colors, alpha, want = cluster_case()
    buf, shape, strides, exp = want[layout, pad]
    assert (strides[1 if layout == "hwc" else 2] % 4 == 0) == (pad == 2) and strides[0] % 4 == 0
    # 600 records per picture (three chunks); the tile [0, 127] x [0, 7] at the corner meets more than 256 of them in both pictures
    q = np.rint(tracks).astype(np.int64)
    for f in (1, 2):
        lo, hi = np.minimum(q[f - 1], q[f]), np.maximum(q[f - 1], q[f])
        marks = (q[f, :, 0] - 3 <= 127) & (q[f, :, 0] + 3 >= 0) & (q[f, :, 1] - 3 <= 7) & (q[f, :, 1] + 3 >= 0)
        segs = visible[f] & visible[f - 1] & (lo[:, 0] - 1 <= 127) & (hi[:, 0] + 1 >= 0) & (lo[:, 1] - 1 <= 7) & (hi[:, 1] + 1 >= 0)
        assert int(marks.sum()) + int(segs.sum()) > 256 and 2 * N2 > 512
    flat = t(buf)
    ops.draw_tracks(torch.as_strided(flat, shape, strides), t(tracks), t(visible), t(colors), trail=1, radius=3, half_width=1, alpha=alpha,
                    first_frame=1)
    assert np.array_equal(flat.cpu().numpy(), exp)
    assert (exp != buf).sum() > 2000


# ---- 3. the logits form ---------------------------------------------------------------------------------------------------------
def test_logits_form_equals_the_visible_form_on_the_emitted_visibility():
    """Logits from {-6, +6}: the products are 0.995 or at most 0.0025, so no expf difference moves a point across 0.6."""
    from cotracker_amd import _lib as L
    from cotracker_amd import ops
    f0 = 6
    buf, shape, strides, hist, vis, want = ring_case(f0, "hwc", W1 * 3 + 5)
    rng = np.random.RandomState(3)
    both = rng.rand(*vis.shape) < 0.5  # a visible point: both logits + 6; an invisible one: one of them, or both, - 6
    hv = np.where(vis.astype(bool) | ~both, 6.0, -6.0).astype(np.float32)
    hf = np.where(vis.astype(bool) | both, 6.0, -6.0).astype(np.float32)
    hf[~vis.astype(bool) & (rng.rand(*vis.shape) < 0.3)] = -6.0
    assert np.array_equal(R.visible_from_logits(hv, hf, 0.6), vis.astype(bool))
    hist_d, hv_d, hf_d, colors_d, first_d = t(hist), t(hv), t(hf), t(COLORS1), t(FIRST1)
    kw = dict(trail=L1, alpha=ALPHA1, radius=4, half_width=1, max_jump=MAX_JUMP)
    flat = t(buf)
    raw_draw(torch.as_strided(flat, shape, strides), None, "hwc", hist_d, colors_d, f0=f0, sx=SX, sy=SY, N_out=NOUT1, logits=(hv_d, hf_d),
             thresh=0.6, first_row=first_d, **kw)
    assert np.array_equal(flat.cpu().numpy(), want)
    # the emit launch over frames [f0 - L, f0 + F): scaled tracks and thresholded visibility, then the visible form on them at scale 1
    e = L.StreamEmit.Args()
    e.G, e.N, e.N_out, e.R, e.f0, e.f1, e.sx, e.sy, e.thresh, e.reserved = G1, N1, NOUT1, R1, f0 - L1, f0 + F1, SX, SY, 0.6, 0
    n = F1 + L1
    tracks = torch.empty(G1, n, NOUT1, 2, device=dev())
    visible = torch.empty(G1, n, NOUT1, device=dev(), dtype=torch.bool)
    e.hist_coords, e.hist_vis, e.hist_conf, e.first_row = hist_d.data_ptr(), hv_d.data_ptr(), hf_d.data_ptr(), first_d.data_ptr()
    e.tracks, e.visible = tracks.data_ptr(), visible.data_ptr()
    L.check(L.load().ctk_stream_emit(C.byref(e), torch.cuda.current_stream().cuda_stream), "ctk_stream_emit")
    rel = np.clip(FIRST1[:, :NOUT1].astype(np.int64) - (f0 - L1), 0, INT32_MAX).astype(np.int32)
    flat2 = t(buf)
    ops.draw_tracks(torch.as_strided(flat2, shape, strides), tracks, visible, colors_d[:, :NOUT1].contiguous(), first_frame=L1, first_row=t(rel), **kw)
    assert np.array_equal(flat2.cpu().numpy(), want)


# ---- 4. determinism and launch count ----------------------------------------------------------------------------------------------
def test_two_runs_are_identical_and_a_call_is_two_launches(monkeypatch):
    from cotracker_amd import _lib as L
    from cotracker_amd import ops
    tracks, visible, colors, alpha, want = cluster_case()
    buf, shape, strides, exp = want["hwc", 0]
    args = (t(tracks), t(visible), t(colors))
    kw = dict(trail=1, radius=3, half_width=1, alpha=alpha, first_frame=1)
    outs = []
    for _ in range(2):
        flat = t(buf)
        ops.draw_tracks(torch.as_strided(flat, shape, strides), *args, **kw)
        outs.append(flat.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], exp)
    # the library's launch recorder: one row per kernel, one launch each
    flat = t(buf)
    _, rows = recorded(lambda: ops.draw_tracks(torch.as_strided(flat, shape, strides), *args, **kw))
    assert rows == {"draw_prepare": 1, "draw_raster": 1}
    assert np.array_equal(flat.cpu().numpy(), exp)
    # and the entry points of the library the call goes through: the query and the one call
    lib, seen = L.load(), []
    for name in L.SYMBOLS:
        if name != "ctk_error_string":
            def counted(*a, _fn=getattr(lib, name), _name=name):
                seen.append(_name)
                return _fn(*a)
            monkeypatch.setattr(lib, name, counted)
    ops.draw_tracks(torch.as_strided(t(buf), shape, strides), *args, **kw)
    assert seen == ["ctk_draw_tracks_workspace_bytes", "ctk_draw_tracks"]


def test_ops_refusals():
    from cotracker_amd import ops
    frames = torch.zeros(2, 16, 24, 3, dtype=torch.uint8, device=dev())
    tracks, vis = torch.zeros(4, 3, 2, device=dev()), torch.ones(4, 3, dtype=torch.bool, device=dev())
    for bad in (dict(trail=65), dict(trail=-1), dict(radius=0), dict(radius=33), dict(half_width=17), dict(max_jump=0), dict(max_jump=4096),
                dict(first_frame=3), dict(first_frame=-1), dict(alpha=[255]), dict(alpha=[256, 0, 0]), dict(out=frames[:1]),
                dict(out=torch.zeros(2, 16, 24, 4, dtype=torch.uint8, device=dev())[..., :3]), dict(layout="chw")):
        with pytest.raises(ValueError):
            ops.draw_tracks(frames, tracks, vis, **{"trail": 2, **bad})
    for f_, t_, v_ in ((frames.float(), tracks, vis), (frames[:, :, ::2], tracks, vis), (frames, tracks.double(), vis), (frames, tracks, vis.float()),
                       (frames, tracks, vis[:3])):
        with pytest.raises(ValueError):
            ops.draw_tracks(f_, t_, v_)
    assert not frames.any()  # nothing was drawn by a refused call
    # every frame of a result with a trail longer than what is left: rows are appended for the C-ABI's F + trail <= R, none is read
    full = torch.zeros(4, 16, 24, 3, dtype=torch.uint8, device=dev())
    tracks = torch.tensor([[[4.0, 4.0]], [[8.0, 4.0]], [[12.0, 8.0]], [[16.0, 8.0]]], device=dev())
    ops.draw_tracks(full, tracks, torch.ones(4, 1, dtype=torch.bool, device=dev()), trail=3, radius=2)
    want = R.draw(np.zeros((4, 16, 24, 3), dtype=np.uint8), tracks.cpu().numpy()[None], np.ones((1, 4, 1), dtype=bool),
                  ops.rainbow_colors(tracks[0, :, 1][None]).cpu().numpy(), trail=3, radius=2)
    assert np.array_equal(full.cpu().numpy(), want) and want.any()


# ---- 5. the predictor ---------------------------------------------------------------------------------------------------------------
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


def test_predictor_draw_on_a_push_stream():
    from cotracker_amd.synthetic import synthetic_video
    K, G, N, spare, L_ = 32, 2, 6, 2, 4
    T = S + 9 * STEP  # 44 frames: the ring of 32 rows has wrapped
    video = synthetic_video(T, *RAW, seed=11)[0].permute(0, 2, 3, 1).round().to(torch.uint8).contiguous().to(dev())  # [T,H,W,3]
    g = torch.Generator().manual_seed(2)
    q = torch.rand(G, N, 3, generator=g) * torch.tensor([1.0, RAW[1] - 1.0, RAW[0] - 1.0])
    q[..., 0] = torch.tensor([0.0, 0.0, 2.0, 5.0, 9.0, 30.0])
    q = q.to(dev())
    p, twin = small_predictor(K, spare), small_predictor(K, spare)
    for x in (p, twin):
        x(torch.zeros(1, 1, 3, *RAW, device=dev()), is_first_step=True, queries=q, add_support_grid=True)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.draw(video[:1].clone())
    Nu = N + spare
    drawn = 0
    for k, t0 in enumerate(range(0, T - S + 1, STEP)):
        new = video[:S] if k == 0 else video[t0 + S - STEP:t0 + S]
        got, ref = p.push_frames(new, add_support_grid=True), twin.push_frames(new, add_support_grid=True)
        # the tracks of the stream are bit-identical with and without the draw calls in between
        assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(got[1], ref[1]), k
        if k not in (0, 3, 4, 8):
            continue
        done = p.model._gstream.committed
        assert done == t0 + S
        F_ = STEP if k else 6  # (k == 0: the stream is 8 frames old, the trail of its first pictures reaches below frame 0)
        frames = video[done - F_:done].clone()
        tr, vi = p.recent(F_ + L_) if done >= F_ + L_ else p.recent(done)
        base = done - tr.shape[1]
        assert (base == 0) == (k == 0)
        colors_before = p._colors
        out = p.draw(frames, trail=L_)
        assert out.data_ptr() == frames.data_ptr()
        first = None if p._first_row is None else np.clip(p._first_row.cpu().numpy() - base, 0, INT32_MAX)
        colors = p._colors[2][:, :Nu].cpu().numpy()
        want = R.draw(video[done - F_:done].cpu().numpy(), tr.cpu().numpy(), vi.cpu().numpy(), colors, f0=tr.shape[1] - F_, trail=L_,
                      first_row=first)
        assert np.array_equal(frames.cpu().numpy(), want), k
        assert (want != video[done - F_:done].cpu().numpy()).any()
        drawn += 1
        # the default colours are rebuilt only when the query table changed (the add before call 4)
        assert (p._colors is colors_before) == (k not in (0, 4)), k
        if k == 3:  # a point added in mid-stream: its first row lies inside the trail of what is drawn after the next call
            for x in (p, twin):
                x.add_queries(torch.tensor([[float(t0 + S + 1), 60.0, 50.0]], device=dev()), group=1)
        if k == 8:
            assert done > K  # the ring has wrapped
            # planar frames, one query set, an older range, colours of the caller's, into `out`
            planar = video[done - 10:done - 6].permute(0, 3, 1, 2).contiguous()
            mine = torch.randint(0, 256, (Nu, 3), dtype=torch.uint8, generator=g)
            dst = torch.empty_like(planar)
            assert p.draw(planar, first_frame=done - 10, trail=2, radius=3, half_width=0, colors=mine, out=dst, group=1) is dst
            tr, vi = p.recent(12)
            first = np.clip(p._first_row.cpu().numpy() - (done - 12), 0, INT32_MAX)
            want = R.draw(video[done - 10:done - 6].cpu().numpy(), tr[1:].cpu().numpy(), vi[1:].cpu().numpy(), mine.numpy()[None], f0=2, trail=2,
                          radius=3, half_width=0, first_row=first[1:])
            assert np.array_equal(dst.permute(0, 2, 3, 1).cpu().numpy(), want)
            assert torch.equal(planar, video[done - 10:done - 6].permute(0, 3, 1, 2))
            # the trail has left the ring; pictures beyond what has been tracked
            with pytest.raises(ValueError, match="left the history"):
                p.draw(frames, first_frame=done - K + 2, trail=L_)
            # the oldest picture whose trail the ring still holds, byte for byte against recent(K); one frame older is refused
            oldest = video[done - K + L_:done - K + L_ + 1].clone()
            p.draw(oldest, first_frame=done - K + L_, trail=L_)
            tr, vi = p.recent(K)
            first = np.clip(p._first_row.cpu().numpy() - (done - K), 0, INT32_MAX)
            want = R.draw(video[done - K + L_:done - K + L_ + 1].cpu().numpy(), tr.cpu().numpy(), vi.cpu().numpy(),
                          p._colors[2][:, :Nu].cpu().numpy(), f0=L_, trail=L_, first_row=first)
            assert np.array_equal(oldest.cpu().numpy(), want) and (want != video[done - K + L_:done - K + L_ + 1].cpu().numpy()).any()
            with pytest.raises(ValueError, match="left the history"):
                p.draw(oldest, first_frame=done - K + L_ - 1, trail=L_)
            with pytest.raises(ValueError, match="beyond what has been tracked"):
                p.draw(frames, first_frame=done - F_ + 1)
            with pytest.raises(ValueError, match="expected"):
                p.draw(frames[:, :50])
    assert drawn == 4
    for x in (p, twin):
        x.finish()


def test_predictor_draw_on_a_chunk_fed_group_stream():
    """G = 2 query sets over one video fed in chunks through forward, no spare_points, no history_frames: the stream runs on the device
    state without slots and on a linear history, and returns everything since frame 0."""
    from cotracker_amd import ops
    from cotracker_amd.synthetic import synthetic_video
    G, N, L_, F_ = 2, 5, 3, 4
    T = S + 2 * STEP
    video = synthetic_video(T, *RAW, seed=12).to(dev())  # [1,T,3,H,W] float
    frames_u8 = video[0].permute(0, 2, 3, 1).round().to(torch.uint8).contiguous()
    g = torch.Generator().manual_seed(4)
    q = torch.rand(G, N, 3, generator=g) * torch.tensor([1.0, RAW[1] - 1.0, RAW[0] - 1.0])
    q[..., 0] = torch.tensor([0.0, 0.0, 1.0, 3.0, 6.0])
    p = small_predictor(None, 0)
    p(video[:, :1], is_first_step=True, queries=q.to(dev()), add_support_grid=True)
    scale = ((RAW[1] - 1) / (HW[1] - 1), (RAW[0] - 1) / (HW[0] - 1))
    for t0 in range(0, T - S + 1, STEP):
        tracks, vis = p(video[:, t0:t0 + S], add_support_grid=True)
        done = t0 + S
        assert tracks.shape == (G, done, N, 2) and p._first_row is None
        assert p.model.stream_groups and not p.model.stream_slots and p.model._gstream.ring_rows is None
        frames = frames_u8[done - F_:done].clone()
        assert p.draw(frames, trail=L_) is frames
        assert torch.equal(p._colors[2], ops.rainbow_colors(p.queries[..., 2]))
        # the returned tracks are the history times the scale, the product draw rounds; the visibility is emit's expression on the
        # history logits (the returned one thresholds torch's sigmoids: equal outside a hair's breadth of 0.6)
        n = F_ + L_
        etr, evi = p.model.stream_emit(done - n, done, N_out=N, scale=scale, logits=False, thresh=0.6)
        assert torch.equal(tracks[:, done - n:].contiguous().view(torch.int32), etr.view(torch.int32))
        assert int((evi != vis[:, done - n:]).sum()) <= 1
        want = R.draw(frames_u8[done - F_:done].cpu().numpy(), tracks[:, done - n:].cpu().numpy(), evi.cpu().numpy(),
                      p._colors[2][:, :N].cpu().numpy(), f0=L_, trail=L_)
        assert np.array_equal(frames.cpu().numpy(), want) and (want != frames_u8[done - F_:done].cpu().numpy()).any()
    # a linear history refuses nothing for age; what one call may span is said as such
    with pytest.raises(ValueError, match="draw fewer frames per call"):
        gs = p.model._gstream
        assert gs.committed == T and gs.T_cap == 2 * T
        gs.draw(torch.zeros(T, 8, 8, 3, dtype=torch.uint8, device=dev()), 0, p._colors[2], trail=T + 1)
    p.finish()
