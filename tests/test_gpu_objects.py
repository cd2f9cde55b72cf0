"""ctk_fit_objects on the GPU (csrc/objects.hip) against the numpy restatement of tests/objects_reference.py: every byte of the four
poisoned, fenced outputs, the float32 matrices bit for bit.  The shapes are the smallest at which the kernel takes each of its paths:
fewer slots than a wave, exactly one chunk, two with the second nearly empty, several, the full LDS list; one round, several, all
sixteen; one, several and a partial last pass of hypotheses; both modes, both models, the three source forms."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_reference as R
import objects_reference as O
from ctk_support import HW, S, STEP, STRIDE, dev, recorded, t

pytestmark = pytest.mark.gpu

GUARD, POISON, FENCE = 64, 0x5A, 0xA5
NAMES = ("motion", "label", "stats", "box")


def fenced(nbytes):
    """A poisoned output of nbytes between two fences: -> (whole buffer, the output's view)."""
    buf = torch.full((nbytes + 2 * GUARD,), FENCE, dtype=torch.uint8, device=dev())
    buf[GUARD:GUARD + nbytes] = POISON
    return buf, buf[GUARD:GUARD + nbytes]


def raw_fit(coords, *, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1, to=None, lag=None, anchor=None,
            labels=None, L=4, min_points=8, model=1, tol=2.0, K=128, min_base=16.0, seed=0, scale=(1.0, 1.0)):
    """The C-ABI call itself on poisoned, fenced outputs -> (motion, label, stats, box) as numpy; the fences are checked here."""
    from cotracker_amd import _lib as L_
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    given = (visible, vis, conf, first_row, None if anchor is None else anchor[0], None if anchor is None else anchor[1],
             None if labels is None else np.asarray(labels, dtype=np.int8))
    keep = [t(coords)] + [None if x is None else t(np.ascontiguousarray(x)) for x in given]
    a = L_.Objects.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.F = G, N, N_out, R_, f0, F
    a.to, a.lag, a.anchor_frame = -1 if to is None else to, 0 if lag is None else lag, 0 if anchor is None else anchor[2]
    a.L, a.min_points, a.model, a.K, a.seed = L, min_points, model, K, seed
    a.tol, a.min_base, a.sx, a.sy, a.thresh, a.reserved = tol, min_base, scale[0], scale[1], thresh, 0
    (a.hist_coords, a.visible, a.hist_vis, a.hist_conf, a.first_row, a.anchor_coords, a.anchor_visible,
     a.labels) = (None if x is None else x.data_ptr() for x in keep)
    outs = [fenced(G * F * L * 24), fenced(G * F * N_out), fenced(G * F * L * 16), fenced(G * F * L * 16)]
    a.motion, a.label, a.stats, a.box = (o[1].data_ptr() for o in outs)
    n = C.c_size_t(99)
    L_.check(L_.load().ctk_fit_objects_workspace_bytes(C.byref(a), C.byref(n)), "ctk_fit_objects_workspace_bytes")
    assert n.value == 0
    L_.check(L_.load().ctk_fit_objects(C.byref(a), None, 0, torch.cuda.current_stream().cuda_stream), "ctk_fit_objects")
    torch.cuda.synchronize()
    for whole, _ in outs:  # the bytes next to each output
        assert bool((whole[:GUARD] == FENCE).all()) and bool((whole[-GUARD:] == FENCE).all())
    m, la, s, b = (o[1].cpu().numpy() for o in outs)
    return (m.view(np.float32).reshape(G, F, L, 2, 3), la.view(np.int8).reshape(G, F, N_out), s.view(np.int32).reshape(G, F, L, 4),
            b.view(np.int32).reshape(G, F, L, 4))


def same(got, want):
    for g_, w_, name in zip(got, want, NAMES):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        eq = (g_.view(np.int32) if g_.dtype == np.float32 else g_) == (w_.view(np.int32) if w_.dtype == np.float32 else w_)
        assert eq.all(), (name, np.argwhere(~eq)[:5].tolist(), g_[~eq][:5], w_[~eq][:5])


def both(coords, **kw):
    """Every byte of the four poisoned outputs equals the restatement's (no value of which is the poison pattern)."""
    got, want = raw_fit(coords, **kw), O.fit_objects(coords, **kw)
    same(got, want)
    return want


# N_out, G, F, L, K, model, mode, form ("lag": linear rows; "ring": R < frames, f - lag and f straddle the wrap; "to"; "anchor": a ring
# that has dropped the anchor's frame, and a slot released after it), logits
CASES = [
    (5, 1, 1, 1, 1, 1, "split", "lag", False),
    (5, 2, 3, 3, 128, 0, "labels", "ring", True),
    (256, 1, 5, 3, 128, 1, "split", "ring", False),
    (256, 2, 3, 16, 300, 0, "labels", "to", False),
    (257, 1, 5, 16, 128, 1, "split", "anchor", True),
    (257, 2, 3, 3, 1, 1, "labels", "lag", False),
    (700, 1, 5, 3, 300, 1, "labels", "anchor", False),
    (700, 2, 3, 16, 128, 0, "split", "to", True),
    (700, 1, 3, 1, 128, 1, "split", "lag", False),
    (700, 1, 3, 1, 128, 0, "labels", "ring", False),
]


@pytest.mark.parametrize("N_out,G,F,L,K,model,mode,form,logits", CASES)
def test_kernel_against_the_restatement(N_out, G, F, L, K, model, mode, form, logits):
    N, T = N_out + 3, 14  # the last 3 slots of a group are never read
    coords, visible, who = O.objects_scene(N_out + K + L, G, T, N)
    if N_out > 64:  # a larger picture: the points of a set are further apart than min_base
        coords *= np.float32(4.0)
    first = O.spoil(coords, N_out)
    labels = None
    if mode == "labels":
        labels = who.astype(np.int8)
        labels[0, :4] = (-1, 20, 16, L)  # no round's
    kw = dict(first_row=first, N_out=N_out, F=F, labels=labels, L=L, min_points=3, model=model, K=K, seed=K + 7, min_base=8.0,
              scale=(1.37, 0.81), tol=2.0)
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
    m, lab, st, bx = both(coords, **kw)
    assert (lab[0, :, 4] == -1).all() and (lab >= 0).sum(axis=-1).min() >= min(N_out, 60) // 3
    if form == "anchor":
        assert (lab[-1, :, 7] == -1).all()
    if N_out >= 256:
        assert (lab == 0).any() and (lab == O.NONE).any() and (L == 1 or (st[:, :, 1, 1] >= 3).all())
        if mode == "labels":
            assert (lab[0, :, :4][lab[0, :, :4] >= 0] == O.NONE).all()


@pytest.mark.parametrize("mode", ("split", "labels"))
def test_full_lds_list(mode):
    """N_out = 8192: 144 KiB of dynamic LDS, 32 chunks."""
    N = 8192 + 3
    coords, visible, who = O.objects_scene(1, 1, 2, N)
    coords *= np.float32(30.0)
    m, lab, st, bx = both(coords, visible=visible, N_out=8192, f0=1, F=1, lag=1, L=3, K=8, seed=3, min_base=64.0,
                          labels=who.astype(np.int8) if mode == "labels" else None)
    assert st[0, 0, 0, 0] > 3000 and st[0, 0, :, 1].sum() > 5000 and (st[0, 0, :, 2] >= 0).all()


@pytest.mark.parametrize("model", (0, 1))
def test_few_points_and_rounds_that_stop(model):
    """Frames with M = 12, 2, 1, 0; a split that stops at round 1; labels mode with an empty label, one point, too few, a fit."""
    N = 12
    coords = np.zeros((2, 6, N, 2), dtype=np.float32)
    coords[:, :, :, 0] = np.arange(N) * 20.0 + np.arange(6)[:, None] * 3.0  # everything shifts by (3, 1) px a frame ...
    coords[:, :, :, 1] = (np.arange(N) % 2) * 30.0 + np.arange(6)[:, None] * 1.0
    coords[:, :, 8:, 1] += np.arange(6)[:, None] * 40.0                      # ... but the last four, which also sink by 40
    visible = np.zeros((2, 6, N), dtype=np.uint8)
    visible[:, :2, :] = 1   # frame 1: M = 12
    visible[:, 2, :2] = 1   # frame 2: M = 2
    visible[:, 3, :1] = 1   # frame 3: M = 1;  frame 4: M = 0
    kw = dict(visible=visible, model=model, K=64, seed=1, f0=0, F=5, lag=1, min_base=16.0)
    m, lab, st, bx = both(coords, L=4, min_points=3, **kw)
    assert st[1, :, 0, 0].tolist() == [0, 12, 2, 1, 0] and st[1, 1, :, :2].tolist() == [[12, 8], [4, 4], [0, 0], [0, 0]]
    assert st[0, 2].tolist() == [[2, 0, -1, 0]] * 4 and lab[0, 2, :3].tolist() == [O.NONE, O.NONE, -1]
    m, lab, st, bx = both(coords, L=3, min_points=5, **kw)  # the second set is too small: the split stops at round 1
    assert st[0, 1, :, :2].tolist() == [[12, 8], [4, 0], [4, 0]] and lab[0, 1].tolist() == [0] * 8 + [O.NONE] * 4
    both(coords, L=2, min_points=1, **kw)
    labels = np.array([[2] * 8 + [3, 3, 3, 1]] * 2, dtype=np.int8)
    m, lab, st, bx = both(coords, L=4, min_points=2, labels=labels, **kw)
    assert st[0, 1, :, 0].tolist() == [0, 1, 8, 3] and lab[1, 1].tolist() == [2] * 8 + [3, 3, 3, O.NONE]
    both(coords, L=2, min_points=1, **{**kw, "min_base": 400.0})  # every pair too close
    # the corners of the position range: the products and the box at their stated bounds
    c = np.array([[-8192, -8192], [8192, -8192], [8192, 8192], [-8192, 8192]], dtype=np.float32)
    corners = np.zeros((1, 2, 512, 2), dtype=np.float32)
    corners[0, 0] = c[np.arange(512) % 4]
    corners[0, 1, :, 0], corners[0, 1, :, 1] = -corners[0, 0, :, 1], corners[0, 0, :, 0]
    both(corners, visible=np.ones((1, 2, 512), dtype=np.uint8), model=model, L=2, min_points=1, K=8, seed=4, f0=1, F=1, lag=1, tol=256.0,
         min_base=8192.0)


@pytest.mark.parametrize("model", (0, 1))
def test_round_0_is_fit_motion_on_the_device(model):
    """Split mode, the lag form, min_points = 1: round 0's matrix and stats and (label == 0) are ctk_fit_motion's, kernel against kernel."""
    from cotracker_amd import ops
    coords, visible, _ = R.scene(31, 2, 9, 300, hw=(384, 512))
    got = raw_fit(coords, visible=visible, f0=0, F=7, lag=2, L=3, min_points=1, model=model, K=128, seed=9, scale=(1.37, 0.81))
    mm, inl, ms = (x.cpu().numpy() for x in ops.fit_motion(t(coords), t(visible), lag=2, model=("translation", "similarity")[model],
                                                           hypotheses=128, seed=9, scale=(1.37, 0.81), frames=7))
    assert np.array_equal(got[0][:, :, 0].view(np.int32), mm.view(np.int32)) and np.array_equal(got[2][:, :, 0], ms)
    assert np.array_equal(got[1] == 0, inl == 1) and np.array_equal(got[1] == -1, inl == -1)
    assert (ms[:, 2:, 1] > (5 if model == 0 else 40)).all()  # (not vacuous; a translation fits little of a turning scene)


def test_the_ops_layer(monkeypatch):
    from cotracker_amd import _lib as L_
    from cotracker_amd import ops
    coords, visible, who = O.objects_scene(21, 2, 6, 70)
    tr, vi = t(coords), t(visible)
    kw = dict(model="similarity", hypotheses=300, seed=9, scale=(1.37, 0.81), min_points=3, min_base=8.0)
    ref = dict(K=300, seed=9, scale=(1.37, 0.81), min_points=3, min_base=8.0)
    # split mode, the default lag (T + lag rows: the result is padded), twice
    want = O.fit_objects(coords, visible=visible, f0=0, F=6, lag=1, L=4, **ref)
    for _ in range(2):
        same(tuple(x.cpu().numpy() for x in ops.fit_objects(tr, vi, **kw)), want)
    # labels mode: int8 [G,N]; a fixed frame; a range; one launch
    labels = who.astype(np.int8)
    res, rows = recorded(lambda: ops.fit_objects(tr, vi, labels=t(labels), objects=3, to=1, frames=(2, 3), **kw))
    assert rows == {"fit_objects": 1}
    same(tuple(x.cpu().numpy() for x in res), O.fit_objects(coords, visible=visible, labels=labels, f0=2, F=3, to=1, L=3, **ref))
    # one group as [T,N,2] with bool visibility, labels [N], an anchor, first rows
    first = np.zeros(70, dtype=np.int64)
    first[:3] = (2, 2 ** 40, 0)
    anchor = ops.FieldAnchor(t(coords[1:, 0]), t(visible[1:, 0]), 0)
    got = ops.fit_objects(tr[1], vi[1].bool(), labels=t(labels[1]), anchor=anchor, first_row=torch.from_numpy(first), frames=(1, 5), **kw)
    same(tuple(x.cpu().numpy() for x in got),
         O.fit_objects(coords[1:], visible=visible[1:], labels=labels[1:], anchor=(coords[1:, 0], visible[1:, 0], 0), f0=1, F=5, L=4,
                       first_row=np.clip(first, 0, R.INT32_MAX)[None], **ref))
    # the entry points of the library the call goes through: the query and the one call
    lib, seen = L_.load(), []
    for name in L_.SYMBOLS:
        if name != "ctk_error_string":
            def counted(*a, _fn=getattr(lib, name), _name=name):
                seen.append(_name)
                return _fn(*a)
            monkeypatch.setattr(lib, name, counted)
    ops.fit_objects(tr, vi, **kw)
    assert seen == ["ctk_fit_objects_workspace_bytes", "ctk_fit_objects"]
    for bad in (dict(lag=0), dict(model="affine"), dict(hypotheses=0), dict(seed=-1), dict(objects=0), dict(objects=17), dict(min_points=0),
                dict(to=6), dict(to=-1), dict(to=1, anchor=anchor), dict(frames=(5, 2)), dict(labels=t(labels).to(torch.int32)),
                dict(anchor=anchor)):  # (the anchor holds one group, the tracks two)
        with pytest.raises(ValueError):
            ops.fit_objects(tr, vi, **bad)
    with pytest.raises(RuntimeError, match="ctk_fit_objects"):  # the C-ABI's own refusal, through the query
        ops.fit_objects(tr, vi, tol=0.0)


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


def test_split_label_follow_on_a_push_stream(monkeypatch):
    """Ring + graph on, frames pushed as uint8.  split_objects, label_objects and follow read the stream's own history and logits; what
    they are compared with is ops.fit_objects on the tracks as recent() emits them -- positions by the same float32 multiplication,
    visibility by the emit kernel's expression, every frame in the row of its own number, so the frame numbers, which seed the
    hypotheses, are the stream's.  By the last call the ring has dropped the frame the objects were chosen on."""
    from cotracker_amd import ops
    from cotracker_amd.synthetic import synthetic_video
    K, G, N, spare, g = 16, 2, 12, 2, 1
    T = S + 7 * STEP  # 36 frames: the ring of 16 rows has wrapped, and dropped the frame the objects are chosen on
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
        p.split_objects()
    Nu = N + spare
    fit = dict(tol=4.0, min_base=4.0, hypotheses=64, min_points=2, seed=3)
    boxes = torch.tensor([[-50.0, -50.0, 70.0, 150.0], [50.0, -50.0, 200.0, 150.0], [500.0, 500.0, 600.0, 600.0]])  # left, right (they overlap), nothing
    first = None

    def history():
        """-> (tracks [done,Nu,2], visible [done,Nu]) of group g, zeros where the ring has dropped the frame."""
        done = p.model._gstream.committed
        tr, vi = p.recent(min(done, K))
        full_t, full_v = torch.zeros(done, Nu, 2, device=dev()), torch.zeros(done, Nu, dtype=torch.bool, device=dev())
        full_t[done - tr.shape[1]:], full_v[done - tr.shape[1]:] = tr[g], vi[g]
        return full_t, full_v
    sets, followed = None, 0
    for k, t0 in enumerate(range(0, T - S + 1, STEP)):
        new = video[:S] if k == 0 else video[t0 + S - STEP:t0 + S]
        c0 = len(captures)
        got = p.push_frames(new, add_support_grid=True)
        c1 = len(captures)
        ref = twin.push_frames(new, add_support_grid=True)
        assert len(captures) - c1 == c1 - c0, (k, c0, c1, len(captures))  # nothing is re-captured: the twin, which never asks, captures as often
        # the tracks of the stream are bit-identical with and without the calls in between
        assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(got[1], ref[1]), k
        done = p.model._gstream.committed
        first = None if p._first_row is None else p._first_row[g]
        if k == 3:  # (on the synthetic weights few points are visible before, and on the newest frames of a window)
            at = done - 3
            full_t, full_v = history()
            split, rows = recorded(lambda: p.split_objects(at, lag=4, objects=3, group=g, **fit))
            assert rows == {"fit_objects": 1} and len(captures) == c1 + (c1 - c0)  # (the pin's emit is not a recorded launch)
            want = ops.fit_objects(full_t, full_v, objects=3, lag=4, frames=(at, 1), first_row=first, **fit)[1][0, 0]
            assert split.objects == 3 and split.anchor.frame == at and split.anchor.group == g and split.labels.dtype == torch.int8
            assert torch.equal(split.labels[:Nu], torch.where(want == ops.OBJECT_NONE, torch.full_like(want, -1), want))
            assert bool((split.labels[Nu:] == -1).all()) and bool((split.labels[:N] >= 0).any())
            boxed = p.label_objects(boxes, at, group=g)
            x, y, seen = full_t[at, :, 0], full_t[at, :, 1], full_v[at]
            expect = torch.full((Nu,), -1, dtype=torch.int8, device=dev())
            for r in (2, 1, 0):  # the lowest r wins
                b = boxes[r].to(dev())
                expect[(x >= b[0]) & (x <= b[2]) & (y >= b[1]) & (y <= b[3]) & seen] = r
            assert torch.equal(boxed.labels[:Nu], expect) and bool((boxed.labels[Nu:] == -1).all()) and boxed.objects == 3
            assert bool((expect == 0).any()) and bool((expect == 1).any()) and not bool((expect == 2).any())
            anchor_row = ops.FieldAnchor(full_t[at][None].contiguous(), full_v[at][None].contiguous(), at)
            sets = (split, boxed)
        if k in (4, 7):
            assert (k == 7) == (done - K > sets[0].anchor.frame)  # by the last call the ring has dropped the anchor's frame
            full_t, full_v = history()
            for chosen in sets:
                res, rows = recorded(lambda: p.follow(chosen, **fit))
                assert rows == {"fit_objects": 1} and len(captures) == c1 + (c1 - c0)
                assert [tuple(x.shape) for x in res] == [(STEP, 3, 2, 3), (STEP, Nu), (STEP, 3, 4), (STEP, 3, 4)]
                m, la, st, bx = ops.fit_objects(full_t, full_v, labels=chosen.labels[:Nu].contiguous(), objects=3, anchor=anchor_row,
                                                frames=(done - STEP, STEP), first_row=first, **fit)
                assert torch.equal(res[0].view(torch.int32), m[0].view(torch.int32)) and torch.equal(res[1], la[0])
                assert torch.equal(res[2], st[0]) and torch.equal(res[3], bx[0].float() / 16.0) and res[3].dtype == torch.float32
                assert int(st[0, :, :, 0].sum()) > 0
                followed += 1
            one = p.follow(sets[1], 1, model="translation")  # the newest frame only
            assert one[0].shape == (1, 3, 2, 3) and one[1].shape == (1, Nu)
            with pytest.raises(ValueError, match="beyond what has been tracked"):
                p.follow(sets[0], 2, first_frame=done - 1)
    assert followed == 4
    with pytest.raises(ValueError, match="left the history"):
        p.split_objects(frame=done - K + 2, lag=4)
    with pytest.raises(ValueError, match="ObjectSet"):
        p.follow(None)
    for x in (p, twin):
        x.finish()
