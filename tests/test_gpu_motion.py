"""ctk_fit_motion on the GPU (csrc/motion.hip) against the numpy restatement of tests/motion_reference.py: every output exactly, the
float32 matrices bit for bit.  The shapes are the smallest at which the kernel takes each of its paths: fewer slots than a wave, one
compaction chunk, two with the second nearly empty, several, the full LDS list; one, several and a partial last round of hypotheses."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_reference as R
from ctk_support import HW, S, STEP, STRIDE, dev, recorded, t

pytestmark = pytest.mark.gpu

GUARD, POISON, FENCE = 64, 0x5A, 0xA5


def fenced(nbytes):
    """A poisoned output of nbytes between two fences: -> (whole buffer, the output's view)."""
    buf = torch.full((nbytes + 2 * GUARD,), FENCE, dtype=torch.uint8, device=dev())
    buf[GUARD:GUARD + nbytes] = POISON
    return buf, buf[GUARD:GUARD + nbytes]


def raw_fit(coords, *, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1, lag=1, model=1, tol=2.0, K=128,
            min_base=16.0, seed=0, scale=(1.0, 1.0)):
    """The C-ABI call itself on poisoned, fenced outputs -> (motion, inlier, stats) as numpy; the fences are checked here."""
    from cotracker_amd import _lib as L
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    keep = [t(coords)] + [None if x is None else t(np.ascontiguousarray(x)) for x in (visible, vis, conf, first_row)]
    a = L.Motion.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.F, a.lag, a.model, a.K, a.seed = G, N, N_out, R_, f0, F, lag, model, K, seed
    a.tol, a.min_base, a.sx, a.sy, a.thresh, a.reserved = tol, min_base, scale[0], scale[1], thresh, 0
    a.hist_coords, a.visible, a.hist_vis, a.hist_conf, a.first_row = (None if x is None else x.data_ptr() for x in keep)
    outs = [fenced(G * F * 24), fenced(G * F * N_out), fenced(G * F * 16)]
    a.motion, a.inlier, a.stats = (o[1].data_ptr() for o in outs)
    n = C.c_size_t(99)
    L.check(L.load().ctk_fit_motion_workspace_bytes(C.byref(a), C.byref(n)), "ctk_fit_motion_workspace_bytes")
    assert n.value == 0
    L.check(L.load().ctk_fit_motion(C.byref(a), None, 0, torch.cuda.current_stream().cuda_stream), "ctk_fit_motion")
    torch.cuda.synchronize()
    for whole, _ in outs:  # the bytes next to each output
        assert bool((whole[:GUARD] == FENCE).all()) and bool((whole[-GUARD:] == FENCE).all())
    m, i, s = (o[1].cpu().numpy() for o in outs)
    return m.view(np.float32).reshape(G, F, 2, 3), i.view(np.int8).reshape(G, F, N_out), s.view(np.int32).reshape(G, F, 4)


def same(got, want):
    for g_, w_, name in zip(got, want, ("motion", "inlier", "stats")):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        eq = (g_.view(np.int32) if g_.dtype == np.float32 else g_) == (w_.view(np.int32) if w_.dtype == np.float32 else w_)
        assert eq.all(), (name, np.argwhere(~eq)[:5].tolist(), g_[~eq][:5], w_[~eq][:5])


def both(coords, **kw):
    """Every byte of the three poisoned outputs equals the restatement's (no value of which is the poison pattern)."""
    got, want = raw_fit(coords, **kw), R.fit_motion(coords, **kw)
    same(got, want)
    return want


def spoil(coords, visible, N_out):
    """Positions that are not valid, an empty slot, a late first row, and frames with M = 2, 1 and 0 at the end."""
    G, T, N, _ = coords.shape
    coords[0, 2, 1] = np.nan
    coords[0, 3, 2, 1] = np.inf
    coords[-1, 4, 3, 0] = -9000.0
    coords[-1, 1, 0] = (8192.0, -8192.0)
    first = np.zeros((G, N), dtype=np.int32)
    first[0, 4] = R.INT32_MAX
    first[-1, min(5, N_out - 1)] = 3
    visible[:, T - 7:, :2] = 1  # (slots 0 and 1 are seen on every source frame of the three)
    visible[:, T - 3, 2:] = 0  # frame T - 3: 2 points seen
    visible[:, T - 2, 1:] = 0  # frame T - 2: 1
    visible[:, T - 1, :] = 0   # frame T - 1: 0
    return first


# N_out, G, F, K, model, lag, form ("linear": R = T rows; "ring": R < frames, f - lag and f straddle the wrap), logits
CASES = [
    (5, 1, 1, 1, 1, 1, "linear", False),
    (5, 2, 9, 64, 0, 3, "linear", True),
    (64, 2, 9, 64, 1, 3, "ring", False),
    (64, 1, 9, 300, 0, 1, "ring", True),
    (257, 1, 9, 256, 1, 1, "ring", True),
    (257, 2, 1, 1024, 0, 1, "linear", False),
    (257, 1, 9, 300, 1, 3, "linear", False),
    (1088, 2, 9, 64, 1, 1, "ring", False),
    (1088, 1, 1, 1024, 1, 1, "linear", True),
    (1088, 1, 9, 256, 0, 3, "ring", False),
]


@pytest.mark.parametrize("N_out,G,F,K,model,lag,form,logits", CASES)
def test_kernel_against_the_restatement(N_out, G, F, K, model, lag, form, logits):
    N, T = N_out + 3, 14  # the last 3 slots of a group are never read
    coords, visible, _ = R.scene(N_out + K, G, T, N, hw=(384, 512) if N_out > 64 else HW)
    first = spoil(coords, visible, N_out)
    if form == "ring":  # 12 rows after 14 frames hold frames 2 .. 13, frame 12 in row 0
        R_, f0 = 12, T - F
        coords, visible = R.fold(coords, R_, T), R.fold(visible, R_, T)
        assert F + lag <= R_ and (f0 - lag) % R_ > (T - 1) % R_
    else:
        f0 = 0 if F == 9 else T - 4  # F = 9 from frame 0: f0 < lag; F = 1: the last frame on which every point may be seen
    kw = dict(first_row=first, N_out=N_out, f0=f0, F=F, lag=lag, model=model, K=K, seed=K + 7, min_base=8.0, scale=(1.37, 0.81))
    if logits:  # away from the threshold: products of 0.98 or below 0.02 against 0.6, so that expf cannot decide
        rng = np.random.default_rng(K)
        kw.update(vis=np.where(visible != 0, 5.0, -5.0).astype(np.float32) + rng.uniform(-1, 1, visible.shape).astype(np.float32),
                  conf=np.full(visible.shape, 6.0, dtype=np.float32), thresh=0.6)
        kw["vis"][0, 1, 0] = np.nan
    else:
        kw.update(visible=visible)
    m, inl, st = both(coords, **kw)
    assert (inl[0, :, 4] == -1).all() and st[:, :, 0].max() > min(N_out, 60) // 2
    if F == 9:
        assert form != "ring" or (st[:, -3:, 0] == [2, 1, 0]).all()
        assert N_out < 64 or ((inl == 1).any() and (inl == 0).any())
        if f0 == 0:
            assert (st[:, :lag, 0] == 0).all() and (st[:, :lag, 2] == -1).all()


def test_full_lds_list():
    """N_out = 8192: 128 KiB of dynamic LDS, 32 compaction chunks."""
    N = 8192 + 3
    coords, visible, _ = R.scene(1, 1, 2, N, hw=(2000, 3000), p_visible=0.97)
    m, inl, st = both(coords, visible=visible, N_out=8192, f0=1, F=1, K=64, seed=3, min_base=64.0)
    assert st[0, 0, 0] > 7000 and st[0, 0, 1] > 4000 and st[0, 0, 2] >= 0


@pytest.mark.parametrize("model", (0, 1))
def test_few_points_close_pairs_and_ties(model):
    N = 6
    coords = np.zeros((2, 6, N, 2), dtype=np.float32)  # (6 rows: F + lag <= R for the 5 frames)
    coords[:, :, :, 0] = np.arange(N) * 20.0 + np.arange(6)[:, None] * 3.0  # everything shifts by (3, 1) px a frame
    coords[:, :, :, 1] = (np.arange(N) % 2) * 30.0 + np.arange(6)[:, None] * 1.0
    visible = np.zeros((2, 6, N), dtype=np.uint8)
    visible[:, :2, :] = 1   # frame 1: M = 6
    visible[:, 2, :2] = 1   # frame 2: M = 2
    visible[:, 3, :1] = 1   # frame 3: M = 1;  frame 4: M = 0
    m, inl, st = both(coords, visible=visible, model=model, K=64, seed=1, f0=0, F=5)
    assert st[0, :, 0].tolist() == [0, 6, 2, 1, 0]
    assert st[1, 1].tolist() == [6, 6, 0, 0] and st[1, 2].tolist() == [2, 2, 0, 0]  # every hypothesis ties: the lowest k wins
    assert np.array_equal(m[0, 1], np.array([[1, 0, 3], [0, 1, 1]], dtype=np.float32))
    m, inl, st = both(coords, visible=visible, model=model, K=300, seed=1, f0=1, F=1, min_base=200.0)  # every pair too close
    assert st[0, 0].tolist() == ([6, 6, 0, 0] if model == 0 else [6, 0, -1, 0]) and (model == 0 or (inl[0, 0] == 0).all())
    m, inl, st = both(coords, visible=visible, model=model, K=64, seed=1, f0=1, F=1, min_base=50.0)    # the lowest admissible k
    assert st[0, 0, 1] == 6 and (model == 0) == (st[0, 0, 2] == 0)
    # the corners of the position range: the products at their stated bounds
    c = np.array([[-8192, -8192], [8192, -8192], [8192, 8192], [-8192, 8192]], dtype=np.float32)
    corners = np.zeros((1, 2, 512, 2), dtype=np.float32)
    corners[0, 0] = c[np.arange(512) % 4]
    corners[0, 1, :, 0], corners[0, 1, :, 1] = -corners[0, 0, :, 1], corners[0, 0, :, 0]
    both(corners, visible=np.ones((1, 2, 512), dtype=np.uint8), model=model, K=8, seed=4, f0=1, F=1, tol=256.0, min_base=8192.0)


def test_one_launch_two_runs_and_the_ops_layer(monkeypatch):
    from cotracker_amd import _lib as L
    from cotracker_amd import ops
    coords, visible, _ = R.scene(21, 2, 6, 70)
    tr, vi = t(coords), t(visible)
    kw = dict(lag=2, model="similarity", hypotheses=300, seed=9, scale=(1.37, 0.81))
    want = R.fit_motion(coords, visible=visible, f0=0, F=6, lag=2, K=300, seed=9, scale=(1.37, 0.81))
    outs = [tuple(x.cpu().numpy() for x in ops.fit_motion(tr, vi, **kw)) for _ in range(2)]  # (T + lag rows: the result is padded)
    same(outs[0], want), same(outs[1], want)
    # bool visibility, one group as [T,N,2], a range, into `out`
    out = (torch.empty(1, 3, 2, 3, device=dev()), torch.empty(1, 3, 70, device=dev(), dtype=torch.int8),
           torch.empty(1, 3, 4, device=dev(), dtype=torch.int32))
    res, rows = recorded(lambda: ops.fit_motion(tr[1], vi[1].bool(), first_frame=2, frames=3, out=out, model="translation", hypotheses=64))
    assert rows == {"fit_motion": 1} and all(x is y for x, y in zip(res, out))
    same(tuple(x.cpu().numpy() for x in res), R.fit_motion(coords[1:], visible=visible[1:], f0=2, F=3, model=0, K=64))
    # the entry points of the library the call goes through: the query and the one call
    lib, seen = L.load(), []
    for name in L.SYMBOLS:
        if name != "ctk_error_string":
            def counted(*a, _fn=getattr(lib, name), _name=name):
                seen.append(_name)
                return _fn(*a)
            monkeypatch.setattr(lib, name, counted)
    ops.fit_motion(tr, vi, **kw)
    assert seen == ["ctk_fit_motion_workspace_bytes", "ctk_fit_motion"]
    for bad in (dict(lag=0), dict(model="affine"), dict(hypotheses=0), dict(hypotheses=4097), dict(seed=-1), dict(first_frame=6), dict(frames=7),
                dict(out=out)):
        with pytest.raises(ValueError):
            ops.fit_motion(tr, vi, **bad)
    with pytest.raises(RuntimeError, match="ctk_fit_motion"):  # the C-ABI's own refusal, through the query
        ops.fit_motion(tr, vi, tol=0.0)


def test_logits_form_equals_the_visible_form_on_the_emitted_visibility():
    """Kernel against kernel, random logits on both sides of the threshold: the visibility expression is ctk_stream_emit's bit for bit."""
    from cotracker_amd import _lib as L
    from cotracker_amd import ops
    G, T, N, N_out, lag = 2, 10, 203, 200, 2
    coords, _, _ = R.scene(5, G, T, N)
    rng = np.random.default_rng(8)
    hv, hf = (rng.normal(1.0, 2.0, (G, T, N)).astype(np.float32) for _ in range(2))
    first = np.zeros((G, N), dtype=np.int32)
    first[0, :3] = (4, R.INT32_MAX, 9)
    sx, sy = 1.37, 0.81
    got = raw_fit(coords, vis=hv, conf=hf, thresh=0.6, first_row=first, N_out=N_out, f0=0, F=T - lag, lag=lag, K=64, seed=2, scale=(sx, sy))
    hist_d, hv_d, hf_d, first_d = t(coords), t(hv), t(hf), t(first)
    e = L.StreamEmit.Args()
    e.G, e.N, e.N_out, e.R, e.f0, e.f1, e.sx, e.sy, e.thresh, e.reserved = G, N, N_out, T, 0, T, sx, sy, 0.6, 0
    tracks = torch.empty(G, T, N_out, 2, device=dev())
    visible = torch.empty(G, T, N_out, device=dev(), dtype=torch.bool)
    e.hist_coords, e.hist_vis, e.hist_conf, e.first_row = hist_d.data_ptr(), hv_d.data_ptr(), hf_d.data_ptr(), first_d.data_ptr()
    e.tracks, e.visible = tracks.data_ptr(), visible.data_ptr()
    L.check(L.load().ctk_stream_emit(C.byref(e), torch.cuda.current_stream().cuda_stream), "ctk_stream_emit")
    assert 0.2 < float(visible.float().mean()) < 0.8
    again = ops.fit_motion(tracks, visible, lag=lag, hypotheses=64, seed=2, first_frame=0, frames=T - lag)
    same(tuple(x.cpu().numpy() for x in again), got)
    assert (got[2][:, lag:, 0] > 4).all()  # (not vacuous: about 16 of 200 points are seen on both frames)


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


def test_camera_motion_on_a_push_stream(monkeypatch):
    """Ring + graph on, frames pushed as uint8.  camera_motion reads the stream's own history and logits; what it is compared with is
    the restatement run on the history as recent() emits it -- positions by the same float32 multiplication, visibility by the emit
    kernel's expression, frame f in row f % K as in the ring --, so the scale arithmetic is the same and the frame numbers, which seed
    the hypotheses, are the stream's."""
    from cotracker_amd import ops
    from cotracker_amd.synthetic import synthetic_video
    K, G, N, spare = 32, 2, 6, 2
    T = S + 9 * STEP  # 44 frames: the ring of 32 rows has wrapped
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
    p, twin = small_predictor(K, spare), small_predictor(K, spare)
    for x in (p, twin):
        x(torch.zeros(1, 1, 3, *RAW, device=dev()), is_first_step=True, queries=q, add_support_grid=True)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.camera_motion()
    Nu, fitted = N + spare, 0

    def want(f0, F_, **kw):
        done = p.model._gstream.committed
        tr, vi = p.recent(min(done, K))
        base = done - tr.shape[1]
        ring_c, ring_v = np.zeros((G, K, Nu, 2), dtype=np.float32), np.zeros((G, K, Nu), dtype=np.uint8)
        for i in range(tr.shape[1]):
            ring_c[:, (base + i) % K], ring_v[:, (base + i) % K] = tr[:, i].cpu().numpy(), vi[:, i].cpu().numpy()
        first = None if p._first_row is None else np.clip(p._first_row.cpu().numpy(), 0, R.INT32_MAX)
        return R.fit_motion(ring_c, visible=ring_v, first_row=first, f0=f0, F=F_, **kw)
    for k, t0 in enumerate(range(0, T - S + 1, STEP)):
        new = video[:S] if k == 0 else video[t0 + S - STEP:t0 + S]
        c0 = len(captures)
        got = p.push_frames(new, add_support_grid=True)
        c1 = len(captures)
        ref = twin.push_frames(new, add_support_grid=True)
        assert len(captures) - c1 == c1 - c0, (k, c0, c1, len(captures))  # nothing is re-captured: the twin, which never asks, captures as often
        # the tracks of the stream are bit-identical with and without the camera_motion calls in between
        assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(got[1], ref[1]), k
        if k not in (0, 3, 4, 8):
            continue
        done = p.model._gstream.committed
        res, rows = recorded(lambda: p.camera_motion(tol=4.0, min_base=4.0, hypotheses=64, seed=k))
        assert rows == {"fit_motion": 1} and len(captures) == c1 + (c1 - c0)
        assert [tuple(x.shape) for x in res] == [(G, STEP, 2, 3), (G, STEP, Nu), (G, STEP, 4)]
        same(tuple(x.cpu().numpy() for x in res), want(done - STEP, STEP, tol=4.0, min_base=4.0, K=64, seed=k))
        fitted += 1
        one = p.camera_motion(1, lag=3, model="translation", group=1, seed=5)  # the newest frame only, one query set
        same(tuple(x.cpu().numpy() for x in one), tuple(x[1:] for x in want(done - 1, 1, lag=3, model=0, K=128, seed=5)))
        if k == 3:
            for x in (p, twin):
                x.add_queries(torch.tensor([[float(t0 + S + 1), 60.0, 50.0]], device=dev()), group=1)
        if k == 8:
            assert done > K  # the ring has wrapped: the oldest frame whose source it still holds, and one older
            old = p.camera_motion(2, first_frame=done - K + 1, hypotheses=32)
            same(tuple(x.cpu().numpy() for x in old), want(done - K + 1, 2, K=32))
            with pytest.raises(ValueError, match="left the history"):
                p.camera_motion(2, first_frame=done - K)
            with pytest.raises(ValueError, match="beyond what has been tracked"):
                p.camera_motion(2, first_frame=done - 1)
    assert fitted == 4
    for x in (p, twin):
        x.finish()
