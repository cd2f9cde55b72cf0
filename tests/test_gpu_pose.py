"""ctk_fit_pose on the GPU (csrc/pose.hip) against the numpy restatement of tests/pose_reference.py: every byte of poisoned, fenced
outputs, the float32 poses and depths bit for bit.  The inputs `fundamental` and `label` come from the restatement of ctk_fit_epipolar,
so this file tests the pose kernel alone; one case chains the two kernels.  The shapes are the smallest at which the kernel takes each
of its paths: a fit list of exactly min_points entries, one more, one chunk less one slot, one chunk and one slot, several chunks, the
full LDS list; the three source forms; with and without a mask; logits; a no-fit frame next to a fitted one."""
import ctypes as C

import numpy as np
import pytest
import torch

import epipolar_reference as ER
import motion_reference as R
import objects_reference as O
import pose_reference as PZ
from ctk_support import HW, S, STEP, STRIDE, dev, host_library, recorded, t

pytestmark = pytest.mark.gpu

GUARD, POISON, FENCE = 64, 0x5A, 0xA5
NAMES = ("pose", "depth", "stats")
CAM = (0.9 * 480, 0.9 * 480, 240.0, 135.0)  # the camera of epipolar_reference.history at its default size


def fenced(nbytes):
    """A poisoned output of nbytes between two fences: -> (whole buffer, the output's view)."""
    buf = torch.full((nbytes + 2 * GUARD,), FENCE, dtype=torch.uint8, device=dev())
    buf[GUARD:GUARD + nbytes] = POISON
    return buf, buf[GUARD:GUARD + nbytes]


def raw_fit(coords, cam, fundamental, label, *, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1,
            to=None, lag=None, anchor=None, mask=None, min_points=8, scale=(1.0, 1.0)):
    """The C-ABI call itself on poisoned, fenced outputs -> (pose, depth, stats) as numpy; the fences and the inputs are checked here."""
    from cotracker_amd import _lib as L_
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    given = (visible, vis, conf, first_row, None if anchor is None else anchor[0], None if anchor is None else anchor[1],
             None if mask is None else np.asarray(mask, dtype=np.int8), np.asarray(fundamental, dtype=np.float32),
             np.asarray(label, dtype=np.int8))
    keep = [t(coords)] + [None if x is None else t(np.ascontiguousarray(x)) for x in given]
    before = [None if x is None else x.clone() for x in keep]
    a = L_.Pose.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.F = G, N, N_out, R_, f0, F
    a.to, a.lag, a.anchor_frame = -1 if to is None else to, 0 if lag is None else lag, 0 if anchor is None else anchor[2]
    a.min_points = min_points
    a.fx, a.fy, a.cx, a.cy = cam
    a.sx, a.sy, a.thresh, a.reserved = scale[0], scale[1], thresh, 0
    (a.hist_coords, a.visible, a.hist_vis, a.hist_conf, a.first_row, a.anchor_coords, a.anchor_visible, a.mask, a.fundamental,
     a.label) = (None if x is None else x.data_ptr() for x in keep)
    outs = [fenced(G * F * 48), fenced(G * F * N_out * 8), fenced(G * F * 16)]
    a.pose, a.depth, a.stats = (o[1].data_ptr() for o in outs)
    n = C.c_size_t(99)
    L_.check(L_.load().ctk_fit_pose_workspace_bytes(C.byref(a), C.byref(n)), "ctk_fit_pose_workspace_bytes")
    assert n.value == 0
    L_.check(L_.load().ctk_fit_pose(C.byref(a), None, 0, torch.cuda.current_stream().cuda_stream), "ctk_fit_pose")
    torch.cuda.synchronize()
    for whole, _ in outs:  # the bytes next to each output
        assert bool((whole[:GUARD] == FENCE).all()) and bool((whole[-GUARD:] == FENCE).all())
    for x, b in zip(keep, before):  # the kernel only reads its inputs, fundamental and label among them
        assert x is None or torch.equal(x.view(torch.uint8), b.view(torch.uint8))
    po, de, st = (o[1].cpu().numpy() for o in outs)
    return po.view(np.float32).reshape(G, F, 3, 4), de.view(np.float32).reshape(G, F, N_out, 2), st.view(np.int32).reshape(G, F, 4)


def same(got, want):
    for g_, w_, name in zip(got, want, NAMES):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        eq = (g_.view(np.int32) if g_.dtype == np.float32 else g_) == (w_.view(np.int32) if w_.dtype == np.float32 else w_)
        assert eq.all(), (name, np.argwhere(~eq)[:5].tolist(), g_[~eq][:5], w_[~eq][:5])


def both(coords, cam, fundamental, label, **kw):
    """Every byte of the three poisoned outputs equals the restatement's (no value of which is the poison pattern)."""
    got, want = raw_fit(coords, cam, fundamental, label, **kw), PZ.fit_pose(coords, cam, fundamental, label, **kw)
    same(got, want)
    return want


# N_out, G, F, a mask given, form ("lag": linear rows; "ring": R < frames, f - lag and f straddle the wrap; "to"; "anchor": a ring that
# has dropped the anchor's frame, and a slot released after it), logits
CASES = [
    (8, 1, 1, False, "lag", False),
    (9, 2, 3, False, "ring", True),
    (255, 2, 3, True, "to", False),
    (257, 2, 3, True, "anchor", False),
    (257, 1, 2, False, "ring", True),
    (600, 2, 3, False, "lag", False),
]


@pytest.mark.parametrize("N_out,G,F,masked,form,logits", CASES)
def test_fit_against_the_restatement(N_out, G, F, masked, form, logits):
    N, T = N_out + 3, 14  # the last 3 slots of a group are never read
    coords, visible, mover = ER.history(N_out + G, G, T, N, movers=0.25 if N_out > 9 else 0.0)
    first = O.spoil(coords, N_out) if N_out > 9 else np.zeros((G, N), dtype=np.int32)  # NaN, inf and outside positions, first rows
    if N_out <= 9:
        visible[:] = 1
    mask = None
    if masked:
        mask = (~mover).astype(np.int8)
        mask[0, :4] = (-1, 20, 0, -128)
    src = dict(first_row=first, N_out=N_out, F=F, scale=(1.37, 0.81))
    cam = (1.37 * CAM[0], 0.81 * CAM[1], 1.37 * CAM[2], 0.81 * CAM[3])
    if form == "lag":
        src.update(f0=T - F - 1, lag=2)
    elif form == "to":
        src.update(f0=T - F, to=T - 6)
    elif form == "ring":  # 12 rows after 14 frames hold frames 2 .. 13, frame 12 in row 0
        coords, visible = R.fold(coords, 12, T), R.fold(visible, 12, T)
        src.update(f0=T - F, lag=3)
        assert (src["f0"] - 3) % 12 > (T - 1) % 12
    else:  # the anchor was taken on frame 1, which the ring of 12 rows has dropped; slot 7 was released and reassigned after it
        anchor = (coords[:, 1].copy(), visible[:, 1].copy(), 1)
        first[-1, 7] = 2
        coords, visible = R.fold(coords, 12, T), R.fold(visible, 12, T)
        src.update(f0=T - F, anchor=anchor)
    if logits:  # away from the threshold: products of 0.98 or below 0.02 against 0.6, so that expf cannot decide
        rng = np.random.default_rng(N_out)
        src.update(vis=np.where(visible != 0, 5.0, -5.0).astype(np.float32) + rng.uniform(-1, 1, visible.shape).astype(np.float32),
                   conf=np.full(visible.shape, 6.0, dtype=np.float32), thresh=0.6)
    else:
        src.update(visible=visible)
    fu, lab, _, est = ER.fit_epipolar(coords, mask=mask, min_points=8, K=64, seed=N_out, min_base=3.0, tol=1.0, **src)
    assert (est[..., 2] >= 0).all()
    if N_out <= 9:
        lab[lab == 0] = 1  # the labels are an input: a fit list of exactly N_out entries
    po, de, st = both(coords, cam, fu, lab, mask=mask, min_points=8, **src)
    assert (st[..., 2] >= 0).all() and (np.isnan(de[..., 0]) == (lab < 0)).all()  # every correspondence has depths, a label of 0 included
    if N_out <= 9:  # (a matrix through eight or nine points obeys them all and is far from rank 2: a pose comes out, not a good one)
        assert (st[..., 0] == N_out).all()
    if N_out > 9:
        assert np.isnan(de[0, :, 4]).all() and (lab == 0).any() and (st[..., 1] >= 0.8 * st[..., 0]).all()
    if form == "anchor":
        assert np.isnan(de[-1, :, 7]).all()
    if masked:  # what the mask keeps out of the fit list has depths all the same
        ones = (lab == 1).sum(axis=-1)
        assert (st[..., 0] <= ones).all() and (st[..., 0] < ones).any()
    if form == "lag" and N_out == 600:  # a no-fit frame (epipolar's zero row) next to fitted ones; min_points one above a list's length
        fu[0, 1] = 0.0
        po, de, st = both(coords, cam, fu, lab, mask=mask, min_points=8, **src)
        assert st[0, 1].tolist()[1:] == [0, -1, 0] and st[0, 0, 2] >= 0 and st[0, 2, 2] >= 0 and st[1, 1, 2] >= 0
        assert (de[0, 1].view(np.uint32) == PZ.NAN_BITS).all() and np.array_equal(po[0, 1], np.eye(3, 4, dtype=np.float32))
        po, de, st = both(coords, cam, fu, lab, min_points=int(st[1, 2, 0]) + 1, **src)
        assert st[1, 2, 2] == -1


def test_full_lds_list():
    """N_out = 8192: 144 KiB of dynamic LDS, 32 chunks."""
    N = 8192 + 3
    coords, visible, _ = ER.history(1, 1, 2, N, hw=(2000, 4000))
    src = dict(visible=visible, N_out=8192, f0=1, F=1, lag=1)
    fu, lab, _, est = ER.fit_epipolar(coords, K=16, seed=3, min_base=32.0, min_points=16, **src)
    assert est[0, 0, 2] >= 0
    po, de, st = both(coords, (0.9 * 4000, 0.9 * 4000, 2000.0, 1000.0), fu, lab, min_points=16, **src)
    assert st[0, 0, 0] > 4000 and st[0, 0, 1] > 0.95 * st[0, 0, 0] and st[0, 0, 2] >= 0


def test_lists_that_fit_nothing_and_the_entry_the_cap_leaves_out():
    """Frames with 12, 8, 7, 1 and 0 correspondences under min_points 8; matrices that are no fit; a static camera; the ray through the
    epipole of tests/test_pose_host.py (stats[3] bit 2)."""
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
    po, de, st = both(coords, CAM, fu, lab, min_points=8, **src)
    assert st[0, :, 0].tolist() == [12, 12, 8, 7, 1, 0, 9] and (st[:, 3:6, 2] == -1).all() and (st[:, (0, 1, 2, 6), 2] >= 0).all()
    fu[0, 2] = np.nan
    fu[1, 2] = 0.0
    fu[1, 6, 0, 0] = np.inf
    po, de, st = both(coords, CAM, fu, lab, min_points=8, **src)
    assert (st[:, 2, 2] == -1).all() and st[1, 6, 2] == -1 and st[0, 6, 2] >= 0
    still, _, _ = ER.history(4, 1, 2, 80, movers=0.0)
    still[0, 1] = still[0, 0]
    ones = dict(visible=np.ones((1, 2, 80), dtype=np.uint8), f0=1, F=1, lag=1)
    fu, lab, _, _ = ER.fit_epipolar(still, K=64, seed=2, min_points=8, min_base=2.0, **ones)
    both(still, CAM, fu, lab, **ones)
    both(still, CAM, np.eye(3, dtype=np.float32)[None, None], np.ones((1, 1, 80), dtype=np.int8), **ones)
    f, cx, cy = 1024.0, 960.0, 540.0
    rng = np.random.default_rng(3)
    n = 60
    P = np.stack([rng.uniform(100, 1820, n), rng.uniform(60, 1020, n)], axis=1)
    Z = rng.uniform(3.0, 12.0, n)
    Q = np.array([cx, cy]) + (P - np.array([cx, cy])) * (Z / (Z - 0.3))[:, None]
    P[0] = Q[0] = (cx, cy)
    Ki = np.array([[1 / f, 0, -cx / f], [0, 1 / f, -cy / f], [0, 0, 1]])
    fu = (Ki.T @ np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 0]]) @ Ki).astype(np.float32)[None, None]
    po, de, st = both(np.stack([P, Q])[None].astype(np.float32), (f, f, cx, cy), fu, np.ones((1, 1, n), dtype=np.int8),
                      visible=np.ones((1, 2, n), dtype=np.uint8), f0=1, lag=1)
    assert st[0, 0, 2] >= 0 and st[0, 0, 3] & 4


def test_the_two_kernels_chained_on_a_stream_shaped_history(tmp_path_factory):
    """One planted scene as a stream holds it -- a ring of 12 rows after 14 frames, logits, first rows, the default fit -- through
    ctk_fit_epipolar and then ctk_fit_pose on its outputs, and through the g++ builds of the two headers: every bit is equal, the camera
    that the scene was planted with comes out, and the static scene lies in front of it."""
    from test_gpu_epipolar import raw_fit as raw_epipolar
    host_e, host_p = host_library(tmp_path_factory, "epipolar"), host_library(tmp_path_factory, "pose")
    host_e.host_fit_epipolar.restype = C.c_int
    host_e.host_fit_epipolar.argtypes = [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 5 + [C.c_void_p] * 12
    host_p.host_fit_pose.restype = C.c_int
    host_p.host_fit_pose.argtypes = [C.c_int] * 10 + [C.c_float] * 7 + [C.c_void_p] * 13
    G, T, N, F, lag = 1, 14, 300, 4, 8
    coords, visible, mover = ER.history(21, G, T, N, hw=(540, 960), noise=0.1)
    cam = (0.9 * 960, 0.9 * 960, 480.0, 270.0)
    ring_c = np.ascontiguousarray(R.fold(coords, 12, T))
    ring_v = R.fold(visible, 12, T)
    vis = np.ascontiguousarray(np.where(ring_v != 0, 5.0, -5.0).astype(np.float32))
    conf = np.full(vis.shape, 6.0, dtype=np.float32)
    first = np.zeros((G, N), dtype=np.int32)
    first[0, 5] = T - 2
    src = dict(vis=vis, conf=conf, thresh=0.6, first_row=first, f0=T - F, F=F, lag=lag)
    fu, lab, _, est = raw_epipolar(ring_c, **src)
    got = raw_fit(ring_c, cam, fu, lab, min_points=16, **src)
    we = [np.full((G, F, 3, 3), np.nan, dtype=np.float32), np.full((G, F, N), 77, dtype=np.int8), np.full((G, F, N), np.nan, dtype=np.float32),
          np.full((G, F, 4), -99, dtype=np.int32)]
    assert host_e.host_fit_epipolar(G, N, N, 12, T - F, F, -1, lag, 0, 16, 512, 0, 1.0, 16.0, 1.0, 1.0, 0.6, ring_c.ctypes.data, None,
                                    vis.ctypes.data, conf.ctypes.data, first.ctypes.data, None, None, None, *(w.ctypes.data for w in we)) == 0
    want = [np.full((G, F, 3, 4), np.nan, dtype=np.float32), np.full((G, F, N, 2), 77.0, dtype=np.float32), np.full((G, F, 4), -99, dtype=np.int32)]
    assert host_p.host_fit_pose(G, N, N, 12, T - F, F, -1, lag, 0, 16, *cam, 1.0, 1.0, 0.6, ring_c.ctypes.data, None, vis.ctypes.data,
                                conf.ctypes.data, first.ctypes.data, None, None, None, we[0].ctypes.data, we[1].ctypes.data,
                                *(w.ctypes.data for w in want)) == 0
    same(got, want)
    po, de, st = got
    assert (st[0, :, 2] >= 0).all() and (st[0, :, 3] == 0).all() and (st[0, :, 1] >= 0.9 * st[0, :, 0]).all()
    static_in = (lab[0] == 1) & ~mover[0]
    assert (de[0][static_in] > 0).all()
    step = np.array([0.05, 0.004, 0.01])  # epipolar_reference.history: the camera's step per frame, and a turn of at most 0.003 rad
    for j in range(F):
        tt = po[0, j, :, 3].astype(np.float64)
        assert np.degrees(np.arccos(np.dot(tt, step) / np.linalg.norm(step))) < 3.0
        assert np.abs(po[0, j, :, :3] - np.eye(3)).max() < 0.05


def test_the_ops_layer():
    """ops.fit_pose after ops.fit_epipolar: one launch each, `out`, the mask forms, and the refusals."""
    from cotracker_amd import ops
    T, N = 6, 150
    coords, visible, mover = ER.history(5, 2, T, N)
    pad_c = np.concatenate([coords, np.zeros((2, 2, N, 2), dtype=np.float32)], axis=1)
    pad_v = np.concatenate([visible, np.zeros((2, 2, N), dtype=np.uint8)], axis=1)
    fit = dict(K=64, seed=4, min_base=4.0, min_points=10)
    mask = (~mover).astype(np.int8)
    fu, lab, _, _ = ER.fit_epipolar(pad_c, visible=pad_v, f0=0, F=T, lag=2, mask=mask, **fit)
    want = PZ.fit_pose(pad_c, CAM, fu, lab, visible=pad_v, f0=0, F=T, lag=2, mask=mask, min_points=10)
    tr, vi, mk = t(coords), t(visible).bool(), t(~mover)
    e = ops.fit_epipolar(tr, vi, mask=mk, lag=2, hypotheses=64, seed=4, min_base=4.0, min_points=10)
    got, rows = recorded(lambda: ops.fit_pose(tr, vi, CAM, e[0], e[1], mask=mk, lag=2, min_points=10))
    assert rows == {"fit_pose": 1}
    same([g_.cpu().numpy() for g_ in got], want)
    assert [tuple(g_.shape) for g_ in got] == [(2, T, 3, 4), (2, T, N, 2), (2, T, 4)]
    assert (want[2][:, 2:, 2] >= 0).all()
    out = tuple(torch.empty_like(g_) for g_ in got)
    again = ops.fit_pose(tr, vi, CAM, e[0], e[1], mask=mk.to(torch.int8), lag=2, min_points=10, out=out)
    assert all(a_ is b_ for a_, b_ in zip(again, out))
    same([g_.cpu().numpy() for g_ in again], want)
    one = ops.fit_pose(tr[0], vi[0], list(CAM), e[0][:1].contiguous(), e[1][:1].contiguous(), mask=mk[0].to(torch.uint8), lag=2, min_points=10)
    same([g_.cpu().numpy() for g_ in one], [w[:1] for w in want])
    for bad in (dict(min_points=7), dict(lag=0), dict(to=1, anchor=ops.FieldAnchor(tr[:, 0].contiguous(), vi[:, 0].contiguous(), 0)),
                dict(to=T), dict(mask=mk.float()), dict(mask=mk[:, :5]), dict(out=out[:2])):
        with pytest.raises(ValueError):
            ops.fit_pose(tr, vi, CAM, e[0], e[1], **{**dict(lag=2, min_points=10), **bad})
    for cam in ((0.0, 1.0, 2.0, 3.0), (1.0, float("nan"), 2.0, 3.0), (1.0, 1.0, float("inf"), 3.0), (1.0, 2.0, 3.0), t(np.array(CAM))):
        with pytest.raises(ValueError, match="intrinsics"):
            ops.fit_pose(tr, vi, cam, e[0], e[1], lag=2)
    for f_, l_ in ((e[0].double(), e[1]), (e[0][:, :3], e[1]), (e[0], e[1].to(torch.uint8)), (e[0], e[1][..., :5]), (e[0].cpu(), e[1])):
        with pytest.raises(ValueError):
            ops.fit_pose(tr, vi, CAM, f_, l_, lag=2)


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


def test_pose_on_a_push_stream(monkeypatch):
    """Ring + graph on, frames pushed as uint8.  pose() reads the stream's own history and logits by two launches; what it is compared
    with is ops.fit_epipolar and then ops.fit_pose on the tracks as recent() emits them.  The stream's tracks are bit-identical to a
    twin's that never asks, nothing is re-captured, and the stream's state is not re-allocated."""
    from cotracker_amd import ops
    from cotracker_amd.synthetic import synthetic_video
    K, G, N, spare, g = 16, 2, 24, 2, 1
    T = S + 4 * STEP
    cam = (120.0, 118.0, 70.0, 50.0)
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
        p.pose(cam)
    Nu = N + spare
    # synthetic weights track nothing real: the bounds are wide, so that some frames have a fit
    fit = dict(tol=6.0, min_base=1.0, hypotheses=64, min_points=8, seed=3)
    lag, checked, fitted = 3, 0, 0
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
                res, rows = recorded(lambda: p.pose(cam, lag=lag, mask=m_, group=g, **fit))
                assert rows == {"fit_epipolar": 1, "fit_pose": 1} and len(captures) == c1 + (c1 - c0)  # two launches, no capture
                assert [tuple(x.shape) for x in res] == [(STEP, 3, 4), (STEP, Nu, 2), (STEP, Nu), (STEP, 4)]
                mu = None if m_ is None else m_[:Nu].contiguous()
                e = ops.fit_epipolar(full_t, full_v, mask=mu, lag=lag, first_row=first, **fit)
                want = ops.fit_pose(full_t, full_v, cam, e[0], e[1], mask=mu, lag=lag, first_row=first, min_points=fit["min_points"])
                for a_, b_ in zip(res, (want[0], want[1], e[1], want[2])):
                    b_ = b_[0, done - STEP:]
                    assert torch.equal(a_.view(torch.int32) if a_.dtype == torch.float32 else a_,
                                       b_.view(torch.int32) if b_.dtype == torch.float32 else b_)
                assert torch.equal(res[2], p.epipolar(lag=lag, mask=m_, group=g, **fit)[1])  # the labels are epipolar()'s
                fitted += int((res[3][:, 2] >= 0).sum())
                checked += 1
            with pytest.raises(ValueError, match="beyond what has been tracked"):
                p.pose(cam, 2, first_frame=done - 1, lag=lag)
            with pytest.raises(ValueError, match="history"):
                p.pose(cam, 1, done - 1, lag=K)
            with pytest.raises(ValueError, match="intrinsics"):
                p.pose((0.0, 1.0, 2.0, 3.0), lag=lag)
    assert checked == 6 and fitted > 0  # (not vacuous: some frame had a pose)
    same_tracks = twin.recent(4)
    mine = p.recent(4)
    assert torch.equal(mine[0].view(torch.int32), same_tracks[0].view(torch.int32)) and torch.equal(mine[1], same_tracks[1])
    for x in (p, twin):
        x.finish()
