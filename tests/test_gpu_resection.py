"""ctk_fit_resection on the GPU (csrc/resection.hip) against the numpy restatement of tests/resection_reference.py: every byte of
poisoned, fenced outputs, the float32 poses and errors bit for bit, the inputs unchanged.  The shapes are resection_reference.cases():
the smallest at which the kernel takes each of its paths -- a fit list of exactly min_points entries and of one less, one chunk less
one slot, one chunk and one slot, several chunks, the list cap (bit 3) and the largest N_out; 1, 256, 257 and 1024 hypotheses; the
three source forms; logits; spoiled positions, structure points, validity bytes and seeds; ties between candidates; the frame that
is the source frame itself.  One case chains the three kernels as localize() does; the last ones hold the host layers to them."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_reference as R
import resection_reference as RR
from ctk_support import HW, S, STEP, STRIDE, dev, host_library, recorded, t

pytestmark = pytest.mark.gpu

GUARD, POISON, FENCE = 64, 0x5A, 0xA5
NAMES = ("pose", "label", "error", "stats")


def fenced(nbytes):
    """A poisoned output of nbytes between two fences: -> (whole buffer, the output's view)."""
    buf = torch.full((nbytes + 2 * GUARD,), FENCE, dtype=torch.uint8, device=dev())
    buf[GUARD:GUARD + nbytes] = POISON
    return buf, buf[GUARD:GUARD + nbytes]


def raw_fit(coords, cam, structure, valid, seeds, *, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1,
            to=None, lag=None, anchor=None, tol=2.0, hypotheses=256, seed=0, min_points=16, scale=(1.0, 1.0)):
    """The C-ABI call itself on poisoned, fenced outputs -> (pose, label, error, stats) as numpy; the fences and the inputs are checked
    here."""
    from cotracker_amd import _lib as L_
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    given = (visible, vis, conf, first_row, None if anchor is None else anchor[0], None if anchor is None else anchor[1],
             np.asarray(structure, dtype=np.float32), np.asarray(valid, dtype=np.int8), np.asarray(seeds, dtype=np.float32))
    keep = [t(coords)] + [None if x is None else t(np.ascontiguousarray(x)) for x in given]
    before = [None if x is None else x.clone() for x in keep]
    a = L_.Resection.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.F = G, N, N_out, R_, f0, F
    a.to, a.lag, a.anchor_frame = -1 if to is None else to, 0 if lag is None else lag, 0 if anchor is None else anchor[2]
    a.min_points, a.hypotheses, a.seed = min_points, hypotheses, seed
    a.fx, a.fy, a.cx, a.cy = cam
    a.sx, a.sy, a.thresh, a.tol = scale[0], scale[1], thresh, tol
    (a.hist_coords, a.visible, a.hist_vis, a.hist_conf, a.first_row, a.anchor_coords, a.anchor_visible, a.structure, a.valid,
     a.seed_pose) = (None if x is None else x.data_ptr() for x in keep)
    outs = [fenced(G * F * 48), fenced(G * F * N_out), fenced(G * F * N_out * 4), fenced(G * F * 16)]
    a.pose, a.label, a.error, a.stats = (o[1].data_ptr() for o in outs)
    n = C.c_size_t(99)
    L_.check(L_.load().ctk_fit_resection_workspace_bytes(C.byref(a), C.byref(n)), "ctk_fit_resection_workspace_bytes")
    assert n.value == 0
    L_.check(L_.load().ctk_fit_resection(C.byref(a), None, 0, torch.cuda.current_stream().cuda_stream), "ctk_fit_resection")
    torch.cuda.synchronize()
    for whole, _ in outs:  # the bytes next to each output
        assert bool((whole[:GUARD] == FENCE).all()) and bool((whole[-GUARD:] == FENCE).all())
    for x, b in zip(keep, before):  # the kernel only reads its inputs, the structure and the seeds among them
        assert x is None or torch.equal(x.view(torch.uint8), b.view(torch.uint8))
    po, la, er, st = (o[1].cpu().numpy() for o in outs)
    return (po.view(np.float32).reshape(G, F, 3, 4), la.view(np.int8).reshape(G, F, N_out), er.view(np.float32).reshape(G, F, N_out),
            st.view(np.int32).reshape(G, F, 4))


def same(got, want):
    for g_, w_, name in zip(got, want, NAMES):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        eq = (g_.view(np.int32) if g_.dtype == np.float32 else g_) == (w_.view(np.int32) if w_.dtype == np.float32 else w_)
        assert eq.all(), (name, np.argwhere(~eq)[:5].tolist(), g_[~eq][:5], w_[~eq][:5])


CASES = {name: (args, kw) for name, args, kw in RR.cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_against_the_restatement(name):
    """Every byte of the four poisoned outputs equals the restatement's (no value of which is the poison pattern)."""
    args, kw = CASES[name]
    same(raw_fit(*args, **kw), RR.fit_resection(*args, **kw))


def test_the_three_kernels_chained_on_a_stream_shaped_history(tmp_path_factory):
    """One planted camera path as a stream holds it -- a ring of 8 rows after 14 frames, logits, first rows, an anchor on frame 3, which
    the ring has dropped -- through ctk_fit_epipolar, ctk_fit_pose and ctk_fit_resection as localize() chains them, and through the g++
    builds of the three headers: every bit is equal.  The structure comes from a planted reconstruct on the pair (0, 3) through the g++
    builds.  The planted path comes back: the camera positions lie within a tenth of the distance travelled and the rotations within
    0.2 degrees (the structure is one noisy pair's: tests/test_pose_host.py measured up to 0.6 degrees of direction and 1.6 % of
    depth on such pairs, which is what its scale, and with it every later position, inherits)."""
    from test_gpu_epipolar import raw_fit as raw_epipolar
    from test_gpu_pose import raw_fit as raw_pose
    hosts = {n: host_library(tmp_path_factory, n) for n in ("epipolar", "pose", "resection")}
    hosts["epipolar"].host_fit_epipolar.restype = C.c_int
    hosts["epipolar"].host_fit_epipolar.argtypes = [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 5 + [C.c_void_p] * 12
    hosts["pose"].host_fit_pose.restype = C.c_int
    hosts["pose"].host_fit_pose.argtypes = [C.c_int] * 10 + [C.c_float] * 7 + [C.c_void_p] * 13
    hosts["resection"].host_fit_resection.restype = C.c_int
    hosts["resection"].host_fit_resection.argtypes = [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 8 + [C.c_void_p] * 14
    G, T, N, F, Rr, at = 1, 14, 300, 4, 8, 3
    sc = RR.scene(21, G, T, N, src=at, hw=(540, 960), noise=0.1, p_visible=2.0)
    coords, cam, mover = sc["coords"], sc["cam"], sc["mover"]
    ones = np.ones((G, T, N), dtype=np.uint8)

    def host_epipolar(c, rows, f0, F_, lag, anchor, mask, vis=None, conf=None, first=None, visible=None):
        out = [np.full((G, F_, 3, 3), np.nan, dtype=np.float32), np.full((G, F_, N), 77, dtype=np.int8),
               np.full((G, F_, N), np.nan, dtype=np.float32), np.full((G, F_, 4), -99, dtype=np.int32)]
        ptr = [None if x is None else x.ctypes.data for x in (visible, vis, conf, first, None if anchor is None else anchor[0],
                                                              None if anchor is None else anchor[1], mask)]
        assert hosts["epipolar"].host_fit_epipolar(G, N, N, rows, f0, F_, -1, lag, 0 if anchor is None else anchor[2], 16, 512, 0, 1.0, 16.0,
                                                   1.0, 1.0, 0.6, c.ctypes.data, *ptr, *(w.ctypes.data for w in out)) == 0
        return out

    def host_pose(c, rows, f0, F_, lag, anchor, mask, fu, lab, vis=None, conf=None, first=None, visible=None):
        out = [np.full((G, F_, 3, 4), np.nan, dtype=np.float32), np.full((G, F_, N, 2), 77.0, dtype=np.float32),
               np.full((G, F_, 4), -99, dtype=np.int32)]
        ptr = [None if x is None else x.ctypes.data for x in (visible, vis, conf, first, None if anchor is None else anchor[0],
                                                              None if anchor is None else anchor[1], mask)]
        assert hosts["pose"].host_fit_pose(G, N, N, rows, f0, F_, -1, lag, 0 if anchor is None else anchor[2], 16, *cam, 1.0, 1.0, 0.6,
                                           c.ctypes.data, *ptr, fu.ctypes.data, lab.ctypes.data, *(w.ctypes.data for w in out)) == 0
        return out
    # the planted reconstruct: the pair (0, 3) of the linear history
    fu, lab, _, est = host_epipolar(coords, T, at, 1, at, None, None, visible=ones)
    assert est[0, 0, 2] >= 0
    de = host_pose(coords, T, at, 1, at, None, None, fu, lab, visible=ones)[1]
    pts, valid = RR.structure_from_pose(coords[0, at], cam, de[0, 0], lab[0, 0])
    pts, valid = np.ascontiguousarray(pts[None]), np.ascontiguousarray(valid[None])
    assert valid.sum() > 0.5 * N  # (the movers are out, and what lies deeper than 64 of the pair's short baselines)
    # the stream's view: a ring, logits, a slot released after the anchor was taken
    ring_c = np.ascontiguousarray(R.fold(coords, Rr, T))
    vis = np.ascontiguousarray(np.where(R.fold(ones, Rr, T) != 0, 5.0, -5.0).astype(np.float32))
    conf = np.full(vis.shape, 6.0, dtype=np.float32)
    first = np.zeros((G, N), dtype=np.int32)
    first[0, 5] = at + 1
    anchor = (np.ascontiguousarray(coords[:, at]), np.ascontiguousarray(ones[:, at]), at)
    src = dict(vis=vis, conf=conf, thresh=0.6, first_row=first, f0=T - F, F=F, anchor=anchor)
    fu, lab, _, _ = raw_epipolar(ring_c, mask=valid, **src)
    seeds = raw_pose(ring_c, cam, fu, lab, mask=valid, min_points=16, **src)[0]
    got = raw_fit(ring_c, cam, pts, valid, seeds, tol=2.0, hypotheses=256, seed=0, min_points=16, **src)
    we = host_epipolar(ring_c, Rr, T - F, F, 0, anchor, valid, vis=vis, conf=conf, first=first)
    assert np.array_equal(we[0].view(np.int32), fu.view(np.int32)) and np.array_equal(we[1], lab)
    wp = host_pose(ring_c, Rr, T - F, F, 0, anchor, valid, we[0], we[1], vis=vis, conf=conf, first=first)
    assert np.array_equal(wp[0].view(np.int32), seeds.view(np.int32))
    want = [np.full((G, F, 3, 4), np.nan, dtype=np.float32), np.full((G, F, N), 77, dtype=np.int8), np.full((G, F, N), 77.0, dtype=np.float32),
            np.full((G, F, 4), -99, dtype=np.int32)]
    assert hosts["resection"].host_fit_resection(G, N, N, Rr, T - F, F, -1, 0, at, 16, 256, 0, *cam, 1.0, 1.0, 0.6, 2.0, ring_c.ctypes.data, None,
                                                 vis.ctypes.data, conf.ctypes.data, first.ctypes.data, anchor[0].ctypes.data,
                                                 anchor[1].ctypes.data, pts.ctypes.data, valid.ctypes.data, wp[0].ctypes.data,
                                                 *(w.ctypes.data for w in want)) == 0
    same(got, want)
    po, la, er, st = got
    assert (st[0, :, 2] >= 0).all() and (st[0, :, 3] == 0).all() and (la[0, :, 5] == -1).all()
    static = (valid[0] == 1) & ~mover[0]
    assert (la[0][:, static] == 1).mean() > 0.99 and (la[0][:, (valid[0] == 1) & mover[0]] == 0).all()
    base = float(np.linalg.norm(sc["truth"][0, 0, :, 3]))  # the pair (0, 3): frame 0 seen from the structure's frame
    for j in range(F):
        Rt, tt = sc["truth"][0, T - F + j, :, :3], sc["truth"][0, T - F + j, :, 3] / base
        Rm, tm = po[0, j, :, :3].astype(np.float64), po[0, j, :, 3].astype(np.float64)
        Ct, Cm = -Rt.T @ tt, -Rm.T @ tm
        assert np.linalg.norm(Cm - Ct) <= 0.1 * np.linalg.norm(Ct), (j, Cm, Ct)
        assert np.degrees(2.0 * np.arcsin(min(1.0, np.linalg.norm(Rm - Rt) / (2.0 * np.sqrt(2.0))))) <= 0.2


def test_the_ops_layer():
    """ops.fit_resection: one launch, `out`, one group without its axis, and the refusals."""
    from cotracker_amd import ops
    G, T, N = 2, 6, 150
    sc = RR.scene(5, G, T, N, src=1)
    coords, visible, cam = sc["coords"], sc["visible"], sc["cam"]
    valid = (~sc["mover"]).astype(np.int8)
    seeds = RR.unit_seeds(sc["truth"], range(T))
    seeds[1, 4] = np.nan
    fit = dict(tol=2.0, hypotheses=64, seed=4, min_points=10)
    want = RR.fit_resection(coords, cam, sc["structure"], valid, seeds, visible=visible, f0=0, F=T, to=1, **fit)
    k = want[3][:, :, 2]  # every row has a fit but the one whose seed is NaN: (I | 0) is too far off; the source frame itself is exact
    assert (k >= 0).sum() == G * T - 1 and k[1, 4] == -1 and (want[3][:, 1, 3] == 32).all()
    tr, vi, st, va, se = t(coords), t(visible).bool(), t(sc["structure"]), t(valid), t(seeds)
    got, rows = recorded(lambda: ops.fit_resection(tr, vi, cam, st, va, se, to=1, **fit))
    assert rows == {"fit_resection": 1}
    same([g_.cpu().numpy() for g_ in got], want)
    assert [tuple(g_.shape) for g_ in got] == [(G, T, 3, 4), (G, T, N), (G, T, N), (G, T, 4)]
    out = tuple(torch.empty_like(g_) for g_ in got)
    again = ops.fit_resection(tr, vi, cam, st, va.bool(), se, to=1, out=out, **fit)
    assert all(a_ is b_ for a_, b_ in zip(again, out))
    same([g_.cpu().numpy() for g_ in again], want)
    one = ops.fit_resection(tr[0], vi[0], list(cam), st[0], va[0].to(torch.uint8), se[0], to=1, **fit)
    same([g_.cpu().numpy() for g_ in one], [w[:1] for w in want])
    anchor = ops.FieldAnchor(tr[:, 1].contiguous(), vi[:, 1].contiguous(), 1)
    anchored = ops.fit_resection(tr, vi, cam, st, va, se, anchor=anchor, **fit)  # the same source, as an anchor
    same([g_.cpu().numpy() for g_ in anchored], want)
    for bad in (dict(min_points=5), dict(hypotheses=0), dict(hypotheses=1025), dict(tol=0.0), dict(tol=float("nan")), dict(to=None, lag=0),
                dict(anchor=anchor), dict(to=T), dict(out=out[:3])):
        with pytest.raises(ValueError):
            ops.fit_resection(tr, vi, cam, st, va, se, **{**dict(to=1), **fit, **bad})
    for bad_cam in ((0.0, 1.0, 2.0, 3.0), (1.0, float("nan"), 2.0, 3.0), (1.0, 2.0, 3.0), t(np.array(cam))):
        with pytest.raises(ValueError, match="intrinsics"):
            ops.fit_resection(tr, vi, bad_cam, st, va, se, to=1)
    for s_, v_, p_ in ((st.double(), va, se), (st[:, :5], va, se), (st, va.float(), se), (st, va[:, :5], se), (st, va, se[:, :3]),
                       (st, va, se.cpu()), (st, va, se.double())):
        with pytest.raises(ValueError):
            ops.fit_resection(tr, vi, cam, s_, v_, p_, to=1)


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


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def test_reconstruct_and_localize_on_a_push_stream(monkeypatch):
    """Ring + graph on, frames pushed as uint8.  reconstruct() is pose() for the one pair, ops.structure_from_pose and a pin;
    localize() is three launches on the stream's own history and logits, and equals ops.fit_epipolar + ops.fit_pose +
    ops.fit_resection on the tracks as recent() emits them; on the structure's own frame it gives exactly (I | 0).  The stream's tracks
    are bit-identical to a twin's that never asks, nothing is re-captured, and the stream's state is not re-allocated."""
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
        p.reconstruct(cam)
    Nu = N + spare
    # synthetic weights track nothing real: the bounds are wide, so that some frames have a fit
    two_view = dict(tol=6.0, min_base=1.0, hypotheses=64, min_points=8, seed=3)
    loc = dict(tol=8.0, hypotheses=33, min_points=6, seed=3, epipolar_tol=6.0, epipolar_hypotheses=64, min_base=1.0)
    lag, checked, fitted, on_anchor = 3, 0, 0, 0
    state, structures = None, []
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
        if k < 2:
            continue
        tr, vi = p.recent(min(done, K))
        full_t, full_v = torch.zeros(done, Nu, 2, device=dev()), torch.zeros(done, Nu, dtype=torch.bool, device=dev())
        full_t[done - tr.shape[1]:], full_v[done - tr.shape[1]:] = tr[g], vi[g]
        # reconstruct on a frame inside the newest step: pose() for the pair, structure_from_pose, a pin
        at = done - 2
        s, rows = recorded(lambda: p.reconstruct(cam, at, lag=lag, max_depth=1e6, group=g, **two_view))
        assert rows.get("fit_epipolar") == 1 and rows.get("fit_pose") == 1 and "fit_resection" not in rows and len(captures) == c1 + (c1 - c0)
        assert isinstance(s, ops.Structure) and s.anchor.frame == at and s.anchor.group == g and s.intrinsics == cam
        assert tuple(s.points.shape) == (gs.N, 3) and tuple(s.valid.shape) == (gs.N,) and s.valid.dtype == torch.int8
        _, depth, label, _ = p.pose(cam, 1, at, lag=lag, group=g, **two_view)
        pts, ok = ops.structure_from_pose(full_t[at], cam, depth[0], label[0], max_depth=1e6)
        assert torch.equal(bits(s.points[:Nu]), bits(pts)) and torch.equal(s.valid[:Nu], ok) and not bool(s.valid[Nu:].any())
        anchor_row = ops.FieldAnchor(full_t[at][None].contiguous(), full_v[at][None].contiguous(), at)
        structures.append((s, anchor_row))
        # localize against every structure so far: three launches, no capture, equal to the three ops calls
        for s_, row_ in structures:
            res, rows = recorded(lambda: p.localize(s_, **loc))
            assert rows == {"fit_epipolar": 1, "fit_pose": 1, "fit_resection": 1} and len(captures) == c1 + (c1 - c0)
            assert [tuple(x.shape) for x in res] == [(STEP, 3, 4), (STEP, Nu), (STEP, Nu), (STEP, 4)]
            mu = s_.valid[:Nu].contiguous()
            e = ops.fit_epipolar(full_t, full_v, mask=mu, anchor=row_, first_row=first, tol=6.0, hypotheses=64, min_base=1.0, min_points=8, seed=3)
            po = ops.fit_pose(full_t, full_v, cam, e[0], e[1], mask=mu, anchor=row_, first_row=first, min_points=8)
            want = ops.fit_resection(full_t, full_v, cam, s_.points[:Nu].contiguous(), mu, po[0], anchor=row_, first_row=first, tol=8.0,
                                     hypotheses=33, min_points=6, seed=3)
            for a_, b_ in zip(res, want):
                assert torch.equal(bits(a_), bits(b_[0, done - STEP:]))
            fitted += int((res[3][:, 2] >= 0).sum())
            checked += 1
            if s_.anchor.frame >= done - STEP and int(s_.valid.sum()) >= 6:  # the structure's own frame is among the rows
                j = s_.anchor.frame - (done - STEP)
                seen = int(((res[1][j] >= 0)).sum())
                if seen >= 6:
                    assert torch.equal(res[0][j], torch.eye(3, 4, device=dev())) and int(res[3][j, 3]) == 32 and int(res[3][j, 2]) == 33 + 2
                    on_anchor += 1
        with pytest.raises(ValueError, match="beyond what has been tracked"):
            p.localize(structures[0][0], 2, first_frame=done - 1)
        with pytest.raises(ValueError, match="must both have been tracked"):
            p.reconstruct(cam, done, lag=lag)
        with pytest.raises(ValueError, match="ops.Structure"):
            p.localize(None)
        with pytest.raises(ValueError, match="intrinsics"):
            p.reconstruct((0.0, 1.0, 2.0, 3.0), lag=lag)
    assert checked == 6 and fitted > 0 and on_anchor > 0  # (not vacuous: some frame had a pose, and a structure's own frame was localised)
    same_tracks = twin.recent(4)
    mine = p.recent(4)
    assert torch.equal(mine[0].view(torch.int32), same_tracks[0].view(torch.int32)) and torch.equal(mine[1], same_tracks[1])
    for x in (p, twin):
        x.finish()
