"""ctk_fit_epipolar on the GPU (csrc/epipolar.hip) against the numpy restatement of tests/epipolar_reference.py: every byte of poisoned,
fenced outputs, the float32 matrices and errors bit for bit.  The shapes are the smallest at which the kernel takes each of its paths:
exactly eight slots, nine, one chunk less one slot, one chunk and one slot, the full LDS list; one hypothesis, one full pass, one
more, a partial second pass; a fit list with and without a mask; the three source forms; frames with 0 and 7 correspondences."""
import ctypes as C

import numpy as np
import pytest
import torch

import epipolar_reference as ER
import motion_reference as R
import objects_reference as O
from ctk_support import HW, S, STEP, STRIDE, dev, host_library, recorded, t

pytestmark = pytest.mark.gpu

GUARD, POISON, FENCE = 64, 0x5A, 0xA5
NAMES = ("fundamental", "label", "error", "stats")


def fenced(nbytes):
    """A poisoned output of nbytes between two fences: -> (whole buffer, the output's view)."""
    buf = torch.full((nbytes + 2 * GUARD,), FENCE, dtype=torch.uint8, device=dev())
    buf[GUARD:GUARD + nbytes] = POISON
    return buf, buf[GUARD:GUARD + nbytes]


def raw_fit(coords, *, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1, to=None, lag=None, anchor=None,
            mask=None, min_points=16, tol=1.0, K=512, min_base=16.0, seed=0, scale=(1.0, 1.0)):
    """The C-ABI call itself on poisoned, fenced outputs -> (fundamental, label, error, stats) as numpy; the fences are checked here."""
    from cotracker_amd import _lib as L_
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    given = (visible, vis, conf, first_row, None if anchor is None else anchor[0], None if anchor is None else anchor[1],
             None if mask is None else np.asarray(mask, dtype=np.int8))
    keep = [t(coords)] + [None if x is None else t(np.ascontiguousarray(x)) for x in given]
    a = L_.Epipolar.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.F = G, N, N_out, R_, f0, F
    a.to, a.lag, a.anchor_frame = -1 if to is None else to, 0 if lag is None else lag, 0 if anchor is None else anchor[2]
    a.min_points, a.K, a.seed = min_points, K, seed
    a.tol, a.min_base, a.sx, a.sy, a.thresh, a.reserved = tol, min_base, scale[0], scale[1], thresh, 0
    (a.hist_coords, a.visible, a.hist_vis, a.hist_conf, a.first_row, a.anchor_coords, a.anchor_visible,
     a.mask) = (None if x is None else x.data_ptr() for x in keep)
    outs = [fenced(G * F * 36), fenced(G * F * N_out), fenced(G * F * N_out * 4), fenced(G * F * 16)]
    a.fundamental, a.label, a.error, a.stats = (o[1].data_ptr() for o in outs)
    n = C.c_size_t(99)
    L_.check(L_.load().ctk_fit_epipolar_workspace_bytes(C.byref(a), C.byref(n)), "ctk_fit_epipolar_workspace_bytes")
    assert n.value == 0
    L_.check(L_.load().ctk_fit_epipolar(C.byref(a), None, 0, torch.cuda.current_stream().cuda_stream), "ctk_fit_epipolar")
    torch.cuda.synchronize()
    for whole, _ in outs:  # the bytes next to each output
        assert bool((whole[:GUARD] == FENCE).all()) and bool((whole[-GUARD:] == FENCE).all())
    m, la, er, s = (o[1].cpu().numpy() for o in outs)
    return (m.view(np.float32).reshape(G, F, 3, 3), la.view(np.int8).reshape(G, F, N_out), er.view(np.float32).reshape(G, F, N_out),
            s.view(np.int32).reshape(G, F, 4))


def same(got, want):
    for g_, w_, name in zip(got, want, NAMES):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        eq = (g_.view(np.int32) if g_.dtype == np.float32 else g_) == (w_.view(np.int32) if w_.dtype == np.float32 else w_)
        assert eq.all(), (name, np.argwhere(~eq)[:5].tolist(), g_[~eq][:5], w_[~eq][:5])


def both(coords, **kw):
    """Every byte of the four poisoned outputs equals the restatement's (no value of which is the poison pattern)."""
    got, want = raw_fit(coords, **kw), ER.fit_epipolar(coords, **kw)
    same(got, want)
    return want


# N_out, G, F, K, a mask given, form ("lag": linear rows; "ring": R < frames, f - lag and f straddle the wrap; "to"; "anchor": a ring that
# has dropped the anchor's frame, and a slot released after it), logits
CASES = [
    (8, 1, 1, 1, False, "lag", False),
    (9, 2, 3, 256, True, "ring", True),
    (255, 2, 3, 257, True, "to", False),
    (257, 2, 3, 300, True, "anchor", False),
    (257, 1, 2, 256, False, "ring", True),
    (600, 2, 3, 1, False, "lag", False),
]


@pytest.mark.parametrize("N_out,G,F,K,masked,form,logits", CASES)
def test_fit_against_the_restatement(N_out, G, F, K, masked, form, logits):
    N, T = N_out + 3, 14  # the last 3 slots of a group are never read
    coords, visible, mover = ER.history(N_out + K, G, T, N)
    first = O.spoil(coords, N_out) if N_out > 9 else np.zeros((G, N), dtype=np.int32)  # NaN, inf and outside positions, first rows
    if N_out <= 9:
        visible[:] = 1
    mask = None
    if masked:
        mask = (~mover).astype(np.int8)
        mask[0, :4] = (-1, 20, 0, -128)
    kw = dict(first_row=first, N_out=N_out, F=F, mask=mask, min_points=8, K=K, seed=K + 7, min_base=3.0, scale=(1.37, 0.81), tol=1.0)
    if form == "lag":
        kw.update(f0=T - F - 1, lag=2)
    elif form == "to":
        kw.update(f0=T - F, to=T - 6)
    elif form == "ring":  # 12 rows after 14 frames hold frames 2 .. 13, frame 12 in row 0
        coords, visible = R.fold(coords, 12, T), R.fold(visible, 12, T)
        kw.update(f0=T - F, lag=3)
        assert (kw["f0"] - 3) % 12 > (T - 1) % 12
    else:  # the anchor was taken on frame 1, which the ring of 12 rows has dropped; slot 7 was released and reassigned after it
        anchor = (coords[:, 1].copy(), visible[:, 1].copy(), 1)
        first[-1, 7] = 2
        coords, visible = R.fold(coords, 12, T), R.fold(visible, 12, T)
        kw.update(f0=T - F, anchor=anchor)
    if logits:  # away from the threshold: products of 0.98 or below 0.02 against 0.6, so that expf cannot decide
        rng = np.random.default_rng(K)
        kw.update(vis=np.where(visible != 0, 5.0, -5.0).astype(np.float32) + rng.uniform(-1, 1, visible.shape).astype(np.float32),
                  conf=np.full(visible.shape, 6.0, dtype=np.float32), thresh=0.6)
    else:
        kw.update(visible=visible)
    fu, lab, er, st = both(coords, **kw)
    if N_out > 9:
        assert (lab[0, :, 4] == -1).all() and (er[0, :, 4] == -1).all()
    if form == "anchor":
        assert (lab[-1, :, 7] == -1).all()
    if N_out >= 255 and K >= 256:
        assert (st[:, :, 1] >= 8).all() and (st[:, :, 2] >= 0).all() and (lab == 0).any() and (lab == 1).any() and (st[..., 3] == 0).all()
        if masked:  # what the mask keeps out of the fit is classified all the same
            out_of_fit = (mask[:, None, :N_out] == 0) & (lab >= 0)
            assert out_of_fit.any() and (er[out_of_fit] >= 0).all() and (st[:, :, 0] < (lab >= 0).sum(axis=-1)).all()


def test_full_lds_list():
    """N_out = 8192: 144 KiB of dynamic LDS, 32 chunks; two passes of hypotheses, the second with one lane."""
    N = 8192 + 3
    coords, visible, _ = ER.history(1, 1, 2, N, hw=(2000, 4000))
    fu, lab, er, st = both(coords, visible=visible, N_out=8192, f0=1, F=1, lag=1, K=257, seed=3, min_base=32.0, min_points=16)
    assert st[0, 0, 0] > 6000 and st[0, 0, 1] > 4000 and st[0, 0, 2] >= 0 and st[0, 0, 3] == 0


def test_few_correspondences_and_lists_that_fit_nothing():
    """Frames with 0, 1, 7, 8 and 12 correspondences; a mask that leaves 7; too few inliers for min_points; all points on one line; a
    static camera."""
    N = 12
    coords, _, _ = ER.history(9, 2, 7, N, movers=0.0)
    visible = np.zeros((2, 7, N), dtype=np.uint8)
    visible[:, 0] = 1
    for f, count in enumerate((12, 8, 7, 1, 0, 9), start=1):
        visible[:, f, :count] = 1
    kw = dict(visible=visible, K=64, seed=1, f0=0, F=7, to=0, min_base=2.0, min_points=8)
    fu, lab, er, st = both(coords, **kw)
    assert st[0, :, 0].tolist() == [12, 12, 8, 7, 1, 0, 9] and (st[:, 3:6, 1] == 0).all() and (st[:, 3:6, 2] == -1).all()
    assert (lab[:, 5] == -1).all() and (lab[:, 3, :7] == 0).all() and (er[:, 3] == -1).all() and (fu[:, 3:6] == 0).all()
    mask = np.ones((2, N), dtype=np.int8)
    mask[:, 7:] = 0
    fu, lab, er, st = both(coords, mask=mask, **kw)
    assert (st[:, :, 0] <= 7).all() and (st[:, :, 2] == -1).all() and (lab[:, 1] == 0).all()
    both(coords, **{**kw, "min_points": 13})
    x = np.arange(40, dtype=np.float32) * 7.0
    line = np.stack([x, 2.0 * x + 3.0], axis=1)
    both(np.stack([line, line + 5.0])[None], visible=np.ones((1, 2, 40), dtype=np.uint8), f0=1, F=1, lag=1, K=128, seed=2, min_points=8,
         min_base=0.0)
    still, _, _ = ER.history(4, 1, 2, 80, movers=0.0)
    still[0, 1] = still[0, 0]
    both(still, visible=np.ones((1, 2, 80), dtype=np.uint8), f0=1, F=1, lag=1, K=64, seed=2, min_points=8, min_base=2.0)


def test_label_equals_the_host_build_on_a_stream_shaped_history(tmp_path_factory):
    """One planted scene as a stream holds it -- a ring of 12 rows after 14 frames, logits, first rows, the default fit -- through the
    kernel and through the g++ build of the same header: the labels, and everything else, are equal."""
    host = host_library(tmp_path_factory, "epipolar")
    host.host_fit_epipolar.restype = C.c_int
    host.host_fit_epipolar.argtypes = [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 5 + [C.c_void_p] * 12
    G, T, N, F, lag = 1, 14, 300, 4, 8
    coords, visible, mover = ER.history(21, G, T, N, hw=(540, 960), noise=0.1)
    ring_c = np.ascontiguousarray(R.fold(coords, 12, T))
    ring_v = R.fold(visible, 12, T)
    vis = np.ascontiguousarray(np.where(ring_v != 0, 5.0, -5.0).astype(np.float32))
    conf = np.full(vis.shape, 6.0, dtype=np.float32)
    first = np.zeros((G, N), dtype=np.int32)
    first[0, 5] = T - 2
    kw = dict(vis=vis, conf=conf, thresh=0.6, first_row=first, f0=T - F, F=F, lag=lag)
    got = raw_fit(ring_c, **kw)
    want = [np.full((G, F, 3, 3), np.nan, dtype=np.float32), np.full((G, F, N), 77, dtype=np.int8), np.full((G, F, N), np.nan, dtype=np.float32),
            np.full((G, F, 4), -99, dtype=np.int32)]
    rc = host.host_fit_epipolar(G, N, N, 12, T - F, F, -1, lag, 0, 16, 512, 0, 1.0, 16.0, 1.0, 1.0, 0.6, ring_c.ctypes.data, None,
                                vis.ctypes.data, conf.ctypes.data, first.ctypes.data, None, None, None, *(w.ctypes.data for w in want))
    assert rc == 0
    assert np.array_equal(got[1], want[1])
    same(got, want)
    lab = got[1][0]
    static = ~mover[0]
    assert (got[3][0, :, 2] >= 0).all() and (lab[:, 5][: F - 2] == -1).all()
    assert ((lab[:, static] == 0).sum(axis=1) <= 0.01 * static.sum()).all()  # the static scene stays, whatever its depth
    assert ((lab[:, ~static] == 0).sum(axis=1) >= 0.5 * ((lab[:, ~static] >= 0).sum(axis=1))).all()  # and most movers are told apart


def test_the_ops_layer():
    """ops.fit_epipolar: one launch, `out`, the mask forms, and the refusals."""
    from cotracker_amd import ops
    T, N = 6, 150
    coords, visible, mover = ER.history(5, 2, T, N)
    want = ER.fit_epipolar(np.concatenate([coords, np.zeros((2, 2, N, 2), dtype=np.float32)], axis=1),
                           visible=np.concatenate([visible, np.zeros((2, 2, N), dtype=np.uint8)], axis=1), f0=0, F=T, lag=2, K=64, seed=4,
                           min_base=4.0, min_points=10, mask=(~mover).astype(np.int8))
    tr, vi, mk = t(coords), t(visible).bool(), t(~mover)
    fit = dict(lag=2, hypotheses=64, seed=4, min_base=4.0, min_points=10)
    got, rows = recorded(lambda: ops.fit_epipolar(tr, vi, mask=mk, **fit))
    assert rows == {"fit_epipolar": 1}
    same([g_.cpu().numpy() for g_ in got], want)
    assert [tuple(g_.shape) for g_ in got] == [(2, T, 3, 3), (2, T, N), (2, T, N), (2, T, 4)]
    out = tuple(torch.empty_like(g_) for g_ in got)
    again = ops.fit_epipolar(tr, vi, mask=mk.to(torch.int8), out=out, **fit)
    assert all(a_ is b_ for a_, b_ in zip(again, out))
    same([g_.cpu().numpy() for g_ in again], want)
    one = ops.fit_epipolar(tr[0], vi[0], mask=mk[0].to(torch.uint8), **fit)  # [T,N,2]: one group
    same([g_.cpu().numpy() for g_ in one], [w[:1] for w in want])
    for bad in (dict(min_points=7), dict(hypotheses=0), dict(lag=0), dict(to=1, anchor=ops.FieldAnchor(tr[:, 0].contiguous(), vi[:, 0].contiguous(), 0)),
                dict(to=T), dict(mask=mk.float()), dict(mask=mk[:, :5]), dict(out=out[:3])):
        with pytest.raises(ValueError):
            ops.fit_epipolar(tr, vi, **{**fit, **bad})


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


def test_epipolar_and_split_scene_on_a_push_stream(monkeypatch):
    """Ring + graph on, frames pushed as uint8.  epipolar() and split_scene() read the stream's own history and logits; what they are
    compared with is ops.fit_epipolar on the tracks as recent() emits them.  The stream's tracks are bit-identical to a twin's that never
    asks, nothing is re-captured, the stream's state is not re-allocated, each call makes one launch, and split_scene's ObjectSet goes
    through follow() and follow_planes() as it is."""
    from cotracker_amd import ops
    from cotracker_amd.synthetic import synthetic_video
    K, G, N, spare, g = 16, 2, 24, 2, 1
    T = S + 5 * STEP
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
        p.epipolar()
    Nu = N + spare
    # synthetic weights track nothing real: the bounds are wide, so that some frames have a fit and both label values occur
    fit = dict(tol=6.0, min_base=1.0, hypotheses=64, min_points=8, seed=3)
    lag, checked, fitted, followed = 3, 0, 0, 0
    state = None
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
            mask = torch.ones(gs.N, dtype=torch.int8, device=dev())
            mask[1] = 0
            for m_ in (None, mask):
                res, rows = recorded(lambda: p.epipolar(lag=lag, mask=m_, group=g, **fit))
                assert rows == {"fit_epipolar": 1} and len(captures) == c1 + (c1 - c0)
                assert [tuple(x.shape) for x in res] == [(STEP, 3, 3), (STEP, Nu), (STEP, Nu), (STEP, 4)]
                want = ops.fit_epipolar(full_t, full_v, mask=None if m_ is None else m_[:Nu].contiguous(), lag=lag, first_row=first, **fit)
                for a_, b_ in zip(res, want):
                    b_ = b_[0, done - STEP:]
                    assert torch.equal(a_.view(torch.int32) if a_.dtype == torch.float32 else a_,
                                       b_.view(torch.int32) if b_.dtype == torch.float32 else b_)
                fitted += int((res[3][:, 2] >= 0).sum())
                checked += 1
            scene, rows = recorded(lambda: p.split_scene(lag=lag, group=g, **fit))
            assert rows.get("fit_epipolar") == 1 and len(captures) == c1 + (c1 - c0)
            assert isinstance(scene, ops.ObjectSet) and scene.objects == 2 and scene.anchor.frame == done - 1 and scene.anchor.group == g
            lab = p.epipolar(1, done - 1, lag=lag, group=g, **fit)[1][0]
            assert tuple(scene.labels.shape) == (gs.N,) and scene.labels.dtype == torch.int8 and bool((scene.labels[Nu:] == -1).all())
            assert torch.equal(scene.labels[:Nu], torch.where(lab < 0, lab, 1 - lab))
            motion, la, st, bx = p.follow(scene, min_points=2, tol=8.0, min_base=1.0)
            assert tuple(motion.shape) == (STEP, 2, 2, 3) and tuple(la.shape) == (STEP, Nu) and tuple(st.shape) == (STEP, 2, 4)
            hom = p.follow_planes(scene, min_points=4, tol=8.0, min_base=1.0)[0]
            assert tuple(hom.shape) == (STEP, 2, 3, 3)
            followed += 1
            with pytest.raises(ValueError, match="beyond what has been tracked"):
                p.epipolar(2, first_frame=done - 1, lag=lag)
            with pytest.raises(ValueError, match="must both have been tracked"):
                p.split_scene(frame=done, lag=lag)
            with pytest.raises(ValueError, match="history"):
                p.epipolar(1, done - 1, lag=K)
    assert checked == 8 and followed == 4 and fitted > 0  # (not vacuous: some frame had a fit)
    same_tracks = twin.recent(4)
    mine = p.recent(4)
    assert torch.equal(mine[0].view(torch.int32), same_tracks[0].view(torch.int32)) and torch.equal(mine[1], same_tracks[1])
    for x in (p, twin):
        x.finish()
