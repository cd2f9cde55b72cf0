"""ctk_fit_focal on the GPU (csrc/focal.hip) against the numpy restatement of tests/focal_reference.py: every byte of the four arrays it
writes (the fifth value ops.fit_focal returns, the candidates, is an input and is checked unchanged), on outputs that are poisoned
with NaN words and framed by them (nan_framed / frame_intact; the int64 outputs are framed as pairs of words).  The inputs
`fundamental` and `label` come from the restatement of ctk_fit_epipolar, so this file tests the focal kernels alone; one case chains
the two entry points.  The shapes are the smallest at which the kernels take each of their paths: a list shorter than a wave, one
chunk less one slot, one chunk and one slot, several chunks, the full LDS list; candidate blocks that are full, partly filled and
single, with a wave left without a candidate; the three source forms across a ring wrap; with and without a mask; logits; frames
that do not take part next to ones that do."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import epipolar_reference as ER
import focal_reference as FR
import motion_reference as R
import objects_reference as O
from ctk_support import HW, NAN_PATTERN, S, STEP, STRIDE, dev, frame_intact, host_library, nan_framed, recorded, t

pytestmark = pytest.mark.gpu

NAMES = ("focal", "curve", "cost", "stats")
CENTRE = (240.0, 135.0)  # of epipolar_reference.history at its default size


def framed(words, dtype):
    """A NaN-poisoned output of `words` 4-byte words inside a NaN frame -> (the output's view as dtype, the words' view, the allocation)."""
    view, flat = nan_framed(torch.full((words,), float("nan")).view(torch.int32).fill_(NAN_PATTERN).view(torch.float32), pattern=NAN_PATTERN,
                            whole=True)
    return view.view(dtype), view, flat


def raw_fit(coords, fundamental, label, focals, principal, *, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None,
            f0=0, F=1, to=None, lag=None, anchor=None, mask=None, min_points=16, scale=(1.0, 1.0), tol=1.0, contrast=1.5, min_frames=1,
            curve_in=None):
    """The C-ABI call itself on poisoned, framed outputs -> (focal, curve, cost, stats) as numpy; the frames and the inputs are checked
    here."""
    from cotracker_amd import _lib as L_
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    focals = np.asarray(focals, dtype=np.float32)
    K = focals.shape[0]
    given = (visible, vis, conf, first_row, None if anchor is None else anchor[0], None if anchor is None else anchor[1],
             None if mask is None else np.asarray(mask, dtype=np.int8), np.asarray(fundamental, dtype=np.float32),
             np.asarray(label, dtype=np.int8), focals, None if curve_in is None else np.asarray(curve_in, dtype=np.int64))
    keep = [t(coords)] + [None if x is None else t(np.ascontiguousarray(x)) for x in given]
    before = [None if x is None else x.clone() for x in keep]
    a = L_.Focal.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.F = G, N, N_out, R_, f0, F
    a.to, a.lag, a.anchor_frame = -1 if to is None else to, 0 if lag is None else lag, 0 if anchor is None else anchor[2]
    a.min_points, a.K, a.min_frames = min_points, K, min_frames
    a.cx, a.cy = principal
    a.sx, a.sy, a.thresh, a.tol, a.contrast, a.reserved = scale[0], scale[1], thresh, tol, contrast, 0
    (a.hist_coords, a.visible, a.hist_vis, a.hist_conf, a.first_row, a.anchor_coords, a.anchor_visible, a.mask, a.fundamental,
     a.label, a.focals, a.curve_in) = (None if x is None else x.data_ptr() for x in keep)
    outs = [framed(G, torch.float32), framed(G * (K + 2) * 2, torch.int64), framed(G * F * K * 2, torch.int64), framed(G * 4, torch.int32)]
    a.focal, a.curve, a.cost, a.stats = (o[0].data_ptr() for o in outs)
    n = C.c_size_t(99)
    L_.check(L_.load().ctk_fit_focal_workspace_bytes(C.byref(a), C.byref(n)), "ctk_fit_focal_workspace_bytes")
    assert n.value == 0
    L_.check(L_.load().ctk_fit_focal(C.byref(a), None, 0, torch.cuda.current_stream().cuda_stream), "ctk_fit_focal")
    torch.cuda.synchronize()
    for _, view, flat in outs:  # the words next to each output
        assert frame_intact(flat, view)
    for x, b in zip(keep, before):  # the kernels only read their inputs
        assert x is None or torch.equal(x.view(torch.uint8), b.view(torch.uint8))
    fo, cu, co, st = (o[0].cpu().numpy() for o in outs)
    return fo.reshape(G), cu.reshape(G, K + 2), co.reshape(G, F, K), st.reshape(G, 4)


def same(got, want):
    for g_, w_, name in zip(got, want, NAMES):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        eq = (g_.view(np.int32) if g_.dtype == np.float32 else g_) == (w_.view(np.int32) if w_.dtype == np.float32 else w_)
        assert eq.all(), (name, np.argwhere(~eq)[:5].tolist(), g_[~eq][:5], w_[~eq][:5])


def both(coords, fundamental, label, focals, principal, **kw):
    """Every byte of the four poisoned outputs equals the restatement's."""
    got, want = raw_fit(coords, fundamental, label, focals, principal, **kw), FR.fit_focal(coords, fundamental, label, focals, principal, **kw)
    same(got, want)
    return want


@functools.lru_cache(maxsize=None)
def scene(N_out, G, F, form):
    """A history and the epipolar restatement's matrices and labels for it, made once per shape.  form: "lag" linear rows; "ring": 12
    rows after 14 frames, f - lag and f straddle the wrap, logits; "to", with a mask; "anchor": a ring that has dropped the anchor's
    frame and a slot released after it, with a mask."""
    N, T = N_out + 3, 14  # the last 3 slots of a group are never read
    coords, visible, mover = ER.history(N_out + G, G, T, N, movers=0.25 if N_out > 16 else 0.0)
    first = O.spoil(coords, N_out) if N_out > 16 else np.zeros((G, N), dtype=np.int32)  # NaN, inf and outside positions, first rows
    if N_out <= 16:
        visible[:] = 1
    mask = None
    if form in ("to", "anchor"):
        mask = (~mover).astype(np.int8)
        mask[0, :4] = (-1, 20, 0, -128)
    src = dict(first_row=first, N_out=N_out, F=F, scale=(1.37, 1.37))
    if form == "lag":
        src.update(f0=T - F, lag=3)
    elif form == "to":
        src.update(f0=T - F, to=T - 6)
    elif form == "ring":
        coords, visible = R.fold(coords, 12, T), R.fold(visible, 12, T)
        src.update(f0=T - F, lag=3)
        assert (src["f0"] - 3) % 12 > (T - 1) % 12
    else:
        anchor = (coords[:, 1].copy(), visible[:, 1].copy(), 1)
        first[-1, 7] = 2
        coords, visible = R.fold(coords, 12, T), R.fold(visible, 12, T)
        src.update(f0=T - F, anchor=anchor)
    if form == "ring":  # away from the threshold: products of 0.98 or below 0.02 against 0.6, so that expf cannot decide
        rng = np.random.default_rng(N_out)
        src.update(vis=np.where(visible != 0, 5.0, -5.0).astype(np.float32) + rng.uniform(-1, 1, visible.shape).astype(np.float32),
                   conf=np.full(visible.shape, 6.0, dtype=np.float32), thresh=0.6)
    else:
        src.update(visible=visible)
    fu, lab, _, est = ER.fit_epipolar(coords, mask=mask, min_points=8, K=64, seed=N_out, min_base=3.0, tol=1.0, **src)
    assert (est[..., 2] >= 0).all()
    if N_out <= 16:
        lab[lab == 0] = 1  # the labels are an input: a fit list of exactly N_out entries
    return coords, fu, lab, mask, src


FORMS = {16: "lag", 255: "to", 257: "anchor", 600: "ring"}


@pytest.mark.parametrize("K", (1, 3, 4, 5, 63, 64, 65, 256))
@pytest.mark.parametrize("N_out", (16, 255, 257, 600))
def test_fit_against_the_restatement(N_out, K):
    """Small K: two groups, three frames, the first of which is swapped for one that does not take part on one group; large K: one
    frame of one group (the restatement walks every candidate in Python)."""
    G, F = (2, 3) if K <= 5 else (1, 1)
    coords, fu, lab, mask, src = scene(N_out, G, F, FORMS[N_out])
    focals = FR.candidates(480 * 1.37, K=K)
    centre = (CENTRE[0] * 1.37, CENTRE[1] * 1.37)
    if K == 5:
        focals[3] = np.nan  # a bad candidate value in a partly filled block
    if K == 65:
        focals[64] = -1.0
    fu = fu.copy()
    if G == 2:
        fu[1, 0] = (0.0, np.nan, np.inf)[K % 3]  # zero / NaN / infinite matrix rows next to fitted ones
    fo, cu, co, st = both(coords, fu, lab, focals, centre, mask=mask, min_points=8, contrast=1.0, **src)
    assert (st[:, 0] == (F if G == 1 else np.array([F, F - 1]))).all() and (co[0] > 0).all()
    if G == 2:
        assert (co[1, 0] == 0).all()
        again = both(coords, fu, lab, focals, centre, mask=mask, min_points=8, contrast=1.0, curve_in=cu, min_frames=2 * F - 1, **src)
        assert np.array_equal(again[1][:, :K], 2 * cu[:, :K]) and again[3][0, 1] >= 0 and again[3][1, 1] == -1  # 2 F - 2 frames on group 1
    if K in (5, 65):
        bad = co[..., 3 if K == 5 else 64]  # the candidate that does not stand costs M 2^32 on every frame that takes part
        assert (st[:, 3] & FR.BIT_CANDIDATE).all() and (bad % FR.ONE == 0).all() and (bad[0] >= 8 * FR.ONE).all()
    else:
        assert not (st[:, 3] & FR.BIT_CANDIDATE).any()


def test_full_lds_list():
    """N_out = 8192: 144 KiB of dynamic LDS, 32 chunks; K = 4: one full candidate block."""
    N = 8192 + 3
    coords, visible, _ = ER.history(1, 1, 4, N, hw=(2000, 4000))
    src = dict(visible=visible, N_out=8192, f0=3, F=1, lag=3)
    fu, lab, _, est = ER.fit_epipolar(coords, K=16, seed=3, min_base=32.0, min_points=16, **src)
    assert est[0, 0, 2] >= 0
    fo, cu, co, st = both(coords, fu, lab, FR.candidates(4000, K=4), (2000.0, 1000.0), contrast=1.0, **src)
    assert st[0, 0] == 1 and st[0, 2] > 4000 and st[0, 1] >= 0


def test_frames_that_do_not_take_part():
    """Labels all 0; lists of 12, 8, 7, 1 and 0 entries under min_points 8; no source frame; min_frames above what took part; a
    contrast the curve misses."""
    N = 12
    coords, _, _ = ER.history(9, 2, 7, N, movers=0.0)
    visible = np.zeros((2, 7, N), dtype=np.uint8)
    visible[:, 0] = 1
    for f, count in enumerate((12, 8, 7, 1, 0, 9), start=1):
        visible[:, f, :count] = 1
    src = dict(visible=visible, f0=0, F=7, to=0)
    fu, lab, _, _ = ER.fit_epipolar(coords, K=64, seed=1, min_base=2.0, min_points=8, **src)
    lab[lab == 0] = 1
    fu[:, 3] = fu[:, 1]  # a matrix where epipolar had none: M = 7 alone decides
    focals = FR.candidates(480, K=6)
    fo, cu, co, st = both(coords, fu, lab, focals, CENTRE, min_points=8, contrast=1.0, **src)
    assert (st[:, 0] == 4).all() and (co[:, 3:6] == 0).all() and (cu[:, 7] == 12 + 12 + 8 + 9).all()
    both(coords, fu, lab, focals, CENTRE, min_points=8, contrast=1.0, min_frames=5, **src)
    both(coords, fu, lab, focals, CENTRE, min_points=8, contrast=float(np.float32(1e6)), **src)
    fo, cu, co, st = both(coords, fu, np.zeros_like(lab), focals, CENTRE, min_points=8, **src)
    assert (st == np.array([0, -1, 0, 0])).all() and (co == 0).all() and (fo.view(np.int32) == 0).all()
    src = dict(visible=visible, f0=0, F=2, lag=3)  # no source frame yet
    fo, cu, co, st = both(coords, fu[:, :2], lab[:, :2], focals, CENTRE, min_points=8, **src)
    assert (st[:, 1] == -1).all() and (co == 0).all()


def test_the_two_entry_points_chained_on_a_stream_shaped_history(tmp_path_factory):
    """One planted scene as a stream holds it -- a ring of 12 rows after 14 frames, logits, first rows, the default fit at lag 8 --
    through ctk_fit_epipolar and then ctk_fit_focal on its outputs, and through the g++ builds of the two headers: every bit is equal,
    and the fit is accepted at the default contrast (checked on the CPU first: contrast 6.2, candidate 26 of 64, 827 entries over four
    frames).  What comes out is 760.7 px for a planted 864: the scene turns by at most 0.024 rad over the lag, and its matrices are
    fitted at 0.1 px noise on a 960 x 540 picture -- tests/test_focal_host.py measures the accuracy on scenes made for it."""
    from test_gpu_epipolar import raw_fit as raw_epipolar
    host_e, host_f = host_library(tmp_path_factory, "epipolar"), host_library(tmp_path_factory, "focal")
    host_e.host_fit_epipolar.restype = C.c_int
    host_e.host_fit_epipolar.argtypes = [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 5 + [C.c_void_p] * 12
    host_f.host_fit_focal.restype = C.c_int
    host_f.host_fit_focal.argtypes = [C.c_int] * 12 + [C.c_float] * 7 + [C.c_void_p] * 16
    G, T, N, F, lag, K = 1, 14, 300, 4, 8, 64
    coords, visible, mover = ER.history(21, G, T, N, hw=(540, 960), noise=0.1)
    ring_c = np.ascontiguousarray(R.fold(coords, 12, T))
    ring_v = R.fold(visible, 12, T)
    vis = np.ascontiguousarray(np.where(ring_v != 0, 5.0, -5.0).astype(np.float32))
    conf = np.full(vis.shape, 6.0, dtype=np.float32)
    first = np.zeros((G, N), dtype=np.int32)
    first[0, 5] = T - 2
    focals = FR.candidates(960, K=K)
    src = dict(vis=vis, conf=conf, thresh=0.6, first_row=first, f0=T - F, F=F, lag=lag)
    fu, lab, _, est = raw_epipolar(ring_c, **src)
    got = raw_fit(ring_c, fu, lab, focals, (479.5, 269.5), **src)
    we = [np.full((G, F, 3, 3), np.nan, dtype=np.float32), np.full((G, F, N), 77, dtype=np.int8), np.full((G, F, N), np.nan, dtype=np.float32),
          np.full((G, F, 4), -99, dtype=np.int32)]
    assert host_e.host_fit_epipolar(G, N, N, 12, T - F, F, -1, lag, 0, 16, 512, 0, 1.0, 16.0, 1.0, 1.0, 0.6, ring_c.ctypes.data, None,
                                    vis.ctypes.data, conf.ctypes.data, first.ctypes.data, None, None, None, *(w.ctypes.data for w in we)) == 0
    want = [np.full(G, np.nan, dtype=np.float32), np.full((G, K + 2), -7, dtype=np.int64), np.full((G, F, K), -7, dtype=np.int64),
            np.full((G, 4), -99, dtype=np.int32)]
    assert host_f.host_fit_focal(G, N, N, 12, T - F, F, -1, lag, 0, 16, K, 1, 479.5, 269.5, 1.0, 1.0, 0.6, 1.0, 1.5, ring_c.ctypes.data, None,
                                 vis.ctypes.data, conf.ctypes.data, first.ctypes.data, None, None, None, we[0].ctypes.data, we[1].ctypes.data,
                                 focals.ctypes.data, None, *(w.ctypes.data for w in want)) == 0
    same(got, want)
    fo, cu, co, st = got
    assert st[0].tolist() == [F, 26, 827, 0] and fo[0] > 0


def test_the_ops_layer():
    """ops.fit_focal after ops.fit_epipolar equals the raw call's restatement: two launches, `out`, the cached candidates, two
    accumulated calls equal one, and the refusals."""
    from cotracker_amd import ops
    T, N, K = 8, 150, 12
    coords, visible, mover = ER.history(5, 2, T, N)
    fit = dict(K=64, seed=4, min_base=4.0, min_points=10)
    mask = (~mover).astype(np.int8)
    fu, lab, _, _ = ER.fit_epipolar(coords, visible=visible, f0=0, F=T, lag=3, mask=mask, **fit)
    focals = FR.candidates(480, K=K)
    centre = ((480 - 1) * 0.5, (270 - 1) * 0.5)
    want = FR.fit_focal(coords, fu, lab, focals, centre, visible=visible, f0=0, F=T, lag=3, mask=mask, min_points=10)
    tr, vi, mk = t(coords), t(visible).bool(), t(~mover)
    e = ops.fit_epipolar(tr, vi, mask=mk, lag=3, hypotheses=64, seed=4, min_base=4.0, min_points=10)
    kw = dict(size=(270, 480), candidates=K, mask=mk, lag=3, min_points=10)
    got, rows = recorded(lambda: ops.fit_focal(tr, vi, e[0], e[1], **kw))
    assert rows == {"fit_focal_sweep": 1, "fit_focal_choose": 1}
    assert np.array_equal(got[4].cpu().numpy().view(np.int32), focals.view(np.int32)) and len(got) == 5
    same([g_.cpu().numpy() for g_ in got[:4]], want)
    assert [tuple(g_.shape) for g_ in got] == [(2,), (2, K + 2), (2, T, K), (2, 4)] + [(K,)] and (want[3][:, 0] == T - 3).all()
    assert ops.fit_focal(tr, vi, e[0], e[1], **kw)[4] is got[4]  # the candidates are kept per (span, K, W, device)
    out = tuple(torch.empty_like(g_) for g_ in got[:4])
    again = ops.fit_focal(tr, vi, e[0], e[1], focals=[float(v) for v in focals], principal=centre, mask=mk.to(torch.int8), lag=3, min_points=10,
                          out=out)
    assert all(a_ is b_ for a_, b_ in zip(again, out))
    same([g_.cpu().numpy() for g_ in again[:4]], want)
    # two accumulated calls (frames 0..4, then 5..7 of the same tracks) equal one
    e1 = [x[:, :5].contiguous() for x in e[:2]]
    first = ops.fit_focal(tr[:, :5].contiguous(), vi[:, :5].contiguous(), e1[0], e1[1], **kw)
    rest_want = FR.fit_focal(coords, fu[:, 5:], lab[:, 5:], focals, centre, visible=visible, f0=5, F=3, lag=3, mask=mask, min_points=10,
                             curve_in=first[1].cpu().numpy())
    assert np.array_equal(rest_want[1], want[1]) and np.array_equal(rest_want[0].view(np.int32), want[0].view(np.int32))
    two = ops.fit_focal(tr, vi, e[0], e[1], focals=first[4], principal=centre, mask=mk, lag=3, min_points=10, curve=first[1])
    assert torch.equal(two[1][:, :K], first[1][:, :K] + got[1][:, :K])
    for bad in (dict(min_points=7), dict(lag=0), dict(to=T), dict(mask=mk.float()), dict(out=out[:2]), dict(candidates=0), dict(candidates=257),
                dict(span=(0.0, 4.0)), dict(span=(2.0, 1.0)), dict(size=None), dict(focals=[300.0, 200.0]), dict(focals=[0.0, 200.0]),
                dict(focals=[float("nan")]), dict(focals=t(focals).double()), dict(principal=(float("inf"), 1.0)), dict(tol=0.0),
                dict(min_frames=0), dict(contrast=0.5), dict(contrast=float("nan")), dict(curve=got[1][:, :5]), dict(curve=got[1].int())):
        with pytest.raises(ValueError):
            ops.fit_focal(tr, vi, e[0], e[1], **{**kw, **bad})
    for f_, l_ in ((e[0].double(), e[1]), (e[0][:, :3], e[1]), (e[0], e[1].to(torch.uint8)), (e[0], e[1][..., :5]), (e[0].cpu(), e[1])):
        with pytest.raises(ValueError):
            ops.fit_focal(tr, vi, f_, l_, **kw)


# ---- the predictor --------------------------------------------------------------------------------------------------------------------
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


def test_calibrate_on_a_push_stream(monkeypatch):
    """Ring + graph on, frames pushed as uint8.  calibrate() reads the stream's own history and logits by three launches; what it is
    compared with is ops.fit_epipolar and then ops.fit_focal on the tracks as recent() emits them, accumulated the same way.  The
    stream's tracks are bit-identical to a twin's that never asks, nothing is re-captured, and the stream's state is not
    re-allocated.  intrinsics() feeds pose(), and raises on a zero focal length."""
    from cotracker_amd import ops
    from cotracker_amd.synthetic import synthetic_video
    K, G, N, spare, g = 16, 2, 24, 2, 1
    T = S + 4 * STEP
    video = synthetic_video(T, *RAW, seed=11)[0].permute(0, 2, 3, 1).round().to(torch.uint8).contiguous().to(dev())
    gen = torch.Generator().manual_seed(2)
    q = torch.rand(G, N, 3, generator=gen) * torch.tensor([0.0, RAW[1] - 1.0, RAW[0] - 1.0])
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
        p.calibrate()
    Nu = N + spare
    # synthetic weights track nothing real: the bounds are wide, so that some frames take part; contrast 1 accepts any curve
    fit = dict(tol=6.0, min_base=1.0, hypotheses=64, min_points=8, seed=3)
    lag, checked, fitted, cand = 3, 0, 0, 9
    state, cal, want_curve = None, None, None
    centre = ((RAW[1] - 1) * 0.5, (RAW[0] - 1) * 0.5)
    for k, t0 in enumerate(range(0, T - S + 1, STEP)):
        new = video[:S] if k == 0 else video[t0 + S - STEP:t0 + S]
        c0 = len(captures)
        got = p.push_frames(new, add_support_grid=True)
        c1 = len(captures)
        ref = twin.push_frames(new, add_support_grid=True)
        assert len(captures) - c1 == c1 - c0, (k, c0, c1, len(captures))  # nothing is re-captured: the twin, which never asks, captures as often
        assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(got[1], ref[1]), k
        gs = p.model._gstream
        done = gs.committed
        ptrs = tuple(h_.data_ptr() for h_ in gs.hist) + (gs.queries.data_ptr(),)
        assert state is None or state == ptrs  # the stream's state stays where it is
        state = ptrs
        first = None if p._first_row is None else p._first_row[g]
        if k >= 2:
            tr, vi = p.recent(min(done, K))
            full_t, full_v = torch.zeros(done, Nu, 2, device=dev()), torch.zeros(done, Nu, dtype=torch.bool, device=dev())
            full_t[done - tr.shape[1]:], full_v[done - tr.shape[1]:] = tr[g], vi[g]
            (focal, cal), rows = recorded(lambda: p.calibrate(lag=lag, candidates=cand, group=g, contrast=1.0, state=cal, **fit))
            assert rows == {"fit_epipolar": 1, "fit_focal_sweep": 1, "fit_focal_choose": 1} and len(captures) == c1 + (c1 - c0)  # three launches
            assert focal.shape == () and tuple(cal[0].shape) == (cand + 2,) and tuple(cal[1].shape) == (cand,) and cal[2] == centre
            e = ops.fit_epipolar(full_t, full_v, lag=lag, first_row=first, **fit)
            # the frames of this window alone, accumulated onto the earlier windows' curve
            want = ops.fit_focal(full_t, full_v, e[0], e[1], size=RAW, candidates=cand, lag=lag, first_row=first, tol=fit["tol"],
                                 min_points=fit["min_points"], contrast=1.0)
            new_cost = want[2][0, done - STEP:].sum(dim=0)
            want_curve = new_cost if want_curve is None else want_curve + new_cost
            assert torch.equal(cal[0][:cand], want_curve)
            fitted += int(focal.item() > 0)
            checked += 1
            with pytest.raises(ValueError, match="beyond what has been tracked"):
                p.calibrate(2, first_frame=done - 1, lag=lag)
            with pytest.raises(ValueError, match="history"):
                p.calibrate(1, done - 1, lag=K)
            with pytest.raises(ValueError, match="state"):
                p.calibrate(lag=lag, state=(1, 2))
    assert checked == 3 and fitted > 0  # (not vacuous: a focal length came out)
    cam = p.intrinsics(focal, cal)
    assert cam == (float(focal.item()), float(focal.item())) + centre and p.intrinsics(focal) == cam and p.intrinsics(focal, (1.0, 2.0))[2:] == (1.0, 2.0)
    res = p.pose(cam, lag=lag, group=g, **fit)  # intrinsics() feeds pose()
    assert tuple(res[0].shape) == (STEP, 3, 4)
    with pytest.raises(ValueError, match="no fit yet"):
        p.intrinsics(torch.zeros((), device=dev()))
    with pytest.raises(ValueError, match="no fit yet"):
        p.intrinsics(0.0)
    same_tracks = twin.recent(4)
    mine = p.recent(4)
    assert torch.equal(mine[0].view(torch.int32), same_tracks[0].view(torch.int32)) and torch.equal(mine[1], same_tracks[1])
    for x in (p, twin):
        x.finish()
