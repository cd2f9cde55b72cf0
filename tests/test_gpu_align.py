"""ctk_fit_align on the GPU (csrc/align.hip) against the numpy restatement of tests/align_reference.py: every byte of the five poisoned,
fenced outputs, the float32 transforms and errors bit for bit, the inputs unchanged.  The shapes are align_reference.cases(): the
smallest at which the kernel takes each of its paths -- three slots, a fit list of min_points entries and of one less, one less than /
exactly / one more than what a wave (64) and a chunk (256) hold, several chunks, the list cap (bit 3) and the largest N; 1 hypothesis,
one less than / exactly / one more than what a wave and a workgroup make at a time, 1024; G = 1 .. 3 with a no-fit pair between fitted
ones; with and without a mask; NaN, infinite, out-of-range and behind-the-camera points in either set; either `valid` all zero;
collinear and repeated triples; a set on which every sampled triple is skipped; ties between candidates; identical sets (the exact
identity); coplanar sets; entries left out of the rounds.  The last tests hold the host layers to the raw call, and follow a planted
camera path through two reconstructions, their alignment and the merged structure."""
import ctypes as C

import numpy as np
import pytest
import torch

import align_reference as AL
import resection_reference as RR
from ctk_support import STEP, S, dev, recorded, t
from test_gpu_resection import RAW, bits, fenced, small_predictor, GUARD, FENCE

pytestmark = pytest.mark.gpu
NAMES = ("sim", "scale", "label", "error", "stats")


def raw_fit(a, valid_a, b, valid_b, cam, *, mask=None, tol=2.0, depth_tol=0.1, hypotheses=256, min_points=8, seed=0):
    """The C-ABI call itself on poisoned, fenced outputs -> (sim, scale, label, error, stats) as numpy; the fences and the inputs are
    checked here."""
    from cotracker_amd import _lib as L_
    a = np.ascontiguousarray(a, dtype=np.float32)
    G, N, _ = a.shape
    given = (a, np.asarray(valid_a, dtype=np.int8), np.asarray(b, dtype=np.float32), np.asarray(valid_b, dtype=np.int8),
             None if mask is None else np.asarray(mask, dtype=np.uint8))
    keep = [None if x is None else t(np.ascontiguousarray(x)) for x in given]
    before = [None if x is None else x.clone() for x in keep]
    g = L_.Align.Args()
    g.G, g.N, g.min_points, g.hypotheses, g.seed, g.reserved = G, N, min_points, hypotheses, seed, 0
    g.fx, g.fy, g.cx, g.cy = cam
    g.tol, g.depth_tol = tol, depth_tol
    g.a, g.valid_a, g.b, g.valid_b, g.mask = (None if x is None else x.data_ptr() for x in keep)
    outs = [fenced(G * 48), fenced(G * 4), fenced(G * N), fenced(G * N * 4), fenced(G * 16)]
    g.sim, g.scale, g.label, g.error, g.stats = (o[1].data_ptr() for o in outs)
    n = C.c_size_t(99)
    L_.check(L_.load().ctk_fit_align_workspace_bytes(C.byref(g), C.byref(n)), "ctk_fit_align_workspace_bytes")
    assert n.value == 0
    L_.check(L_.load().ctk_fit_align(C.byref(g), None, 0, torch.cuda.current_stream().cuda_stream), "ctk_fit_align")
    torch.cuda.synchronize()
    for whole, _ in outs:  # the bytes next to each output
        assert bool((whole[:GUARD] == FENCE).all()) and bool((whole[-GUARD:] == FENCE).all())
    for x, bf in zip(keep, before):  # the kernel only reads its inputs
        assert x is None or torch.equal(x.view(torch.uint8), bf.view(torch.uint8))
    si, sc, la, er, st = (o[1].cpu().numpy() for o in outs)
    return (si.view(np.float32).reshape(G, 3, 4), sc.view(np.float32).reshape(G), la.view(np.int8).reshape(G, N),
            er.view(np.float32).reshape(G, N), st.view(np.int32).reshape(G, 4))


def same(got, want):
    for g_, w_, name in zip(got, want, NAMES):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        eq = (g_.view(np.int32) if g_.dtype == np.float32 else g_) == (w_.view(np.int32) if w_.dtype == np.float32 else w_)
        assert eq.all(), (name, np.argwhere(~eq)[:5].tolist(), g_[~eq][:5], w_[~eq][:5])


CASES = {name: (args, kw) for name, args, kw in AL.cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_against_the_restatement(name):
    """Every byte of the five poisoned outputs equals the restatement's (no value of which is the poison pattern)."""
    args, kw = CASES[name]
    want = AL.fit_align(*args, **kw)
    same(raw_fit(*args, **kw), want)
    if name == "identical":  # exactly s = 1, R = I, t = 0
        assert np.array_equal(want[0][0], np.eye(3, 4, dtype=np.float32)) and want[1][0] == 1.0 and want[4][0, 3] == 32


def test_the_ops_layer():
    """ops.fit_align: one launch that equals the raw call, `out`, one pair without its axis, a mask, and the refusals; apply,
    compose and merge on the device."""
    from cotracker_amd import ops
    N = 150
    prs = [AL.pair(31, N), AL.pair(32, N, share=0.4)]
    a, b = AL.stack(prs)
    va, vb = np.ones((2, N), dtype=np.int8), np.ones((2, N), dtype=np.int8)
    va[0, 3:9], vb[1, 20:40] = 0, 0
    fit = dict(tol=2.0, depth_tol=0.1, hypotheses=64, min_points=10, seed=4)
    want = raw_fit(a, va, b, vb, AL.CAM, **fit)
    same(want, AL.fit_align(a, va, b, vb, AL.CAM, **fit))
    assert (want[4][:, 2] >= 0).all()
    ta, tb, tva, tvb = t(a), t(b), t(va), t(vb)
    got, rows = recorded(lambda: ops.fit_align(ta, tva, tb, tvb, AL.CAM, **fit))
    assert rows == {"fit_align": 1}
    same([g_.cpu().numpy() for g_ in got], want)
    assert [tuple(g_.shape) for g_ in got] == [(2, 3, 4), (2,), (2, N), (2, N), (2, 4)]
    out = tuple(torch.empty_like(g_) for g_ in got)
    again = ops.fit_align(ta, tva.bool(), tb, tvb.to(torch.uint8), list(AL.CAM), out=out, **fit)
    assert all(a_ is b_ for a_, b_ in zip(again, out))
    same([g_.cpu().numpy() for g_ in again], want)
    one = ops.fit_align(ta[0], tva[0], tb[0], tvb[0], AL.CAM, **fit)
    same([g_.cpu().numpy() for g_ in one], [w[:1] for w in want])
    mask = (np.arange(2 * N).reshape(2, N) % 3 != 0).astype(np.uint8)
    masked = ops.fit_align(ta, tva, tb, tvb, AL.CAM, mask=t(mask), **fit)
    same([g_.cpu().numpy() for g_ in masked], AL.fit_align(a, va, b, vb, AL.CAM, mask=mask, **fit))
    for bad in (dict(min_points=2), dict(hypotheses=0), dict(hypotheses=1025), dict(tol=0.0), dict(tol=float("nan")), dict(depth_tol=0.0),
                dict(depth_tol=float("inf")), dict(out=out[:3]), dict(mask=t(mask)[:, :5])):
        with pytest.raises(ValueError):
            ops.fit_align(ta, tva, tb, tvb, AL.CAM, **{**fit, **bad})
    for bad_cam in ((0.0, 1.0, 2.0, 3.0), (1.0, float("nan"), 2.0, 3.0), (1.0, 2.0, 3.0), t(np.array(AL.CAM))):
        with pytest.raises(ValueError, match="intrinsics"):
            ops.fit_align(ta, tva, tb, tvb, bad_cam)
    for a_, v_ in ((ta.double(), tva), (ta[:, :5], tva), (ta, tva.float()), (ta, tva[:, :5]), (ta.cpu(), tva)):
        with pytest.raises(ValueError):
            ops.fit_align(a_, v_, tb, tvb, AL.CAM)
    # the elementwise helpers on what the launch returned
    sim, scale, label = got[0], got[1], got[2]
    moved = ops.apply_similarity(sim, ta)
    ref = np.einsum("gij,gnj->gni", want[0][:, :, :3].astype(np.float64), a.astype(np.float64)) + want[0][:, None, :, 3]
    assert np.allclose(moved.cpu().numpy(), ref, rtol=1e-5, atol=1e-5)
    pose = torch.eye(3, 4, device=dev()).expand(2, 3, 4)
    back = ops.compose_similarity(pose, sim, scale)  # a's own camera, seen from b: (R^T | -R^T t)
    Rm = (want[0][:, :, :3] / want[1][:, None, None]).astype(np.float64)
    assert np.allclose(back[..., :3].cpu().numpy(), Rm.transpose(0, 2, 1), atol=1e-5)
    assert np.allclose(back[..., 3].cpu().numpy(), -np.einsum("gji,gj->gi", Rm, want[0][:, :, 3].astype(np.float64)), atol=1e-4)


def planted_two_structures(hosts, N=300):
    """One planted camera path of 24 frames (resection_reference.scene on frame 8: 540 x 960, 20 % movers, 0.1 px noise) and two
    reconstructions of it through the g++ builds of epipolar_math.h and pose_math.h, as reconstruct() makes them: A on frame 8 from the
    pair (2, 8), B on frame 20 from the pair (10, 20); a third of B's points are taken out again, so that the merged structure has
    something to carry -> dict."""
    from test_gpu_structure import host_localize
    sc = RR.scene(33, 1, 24, N, src=8, hw=(540, 960), noise=0.1, p_visible=2.0)
    coords, cam = sc["coords"], sc["cam"]
    ones = np.ones((1, 24, N), dtype=np.uint8)
    out = {}
    for name, at, lag in (("A", 8, 6), ("B", 20, 10)):
        e, p, _ = host_localize(hosts, coords, 24, cam, at, 1, lag, None, None, None, visible=ones, structure=False)
        assert e[3][0, 0, 2] >= 0
        pts, valid = RR.structure_from_pose(coords[0, at], cam, p[1][0, 0], e[1][0, 0])
        centre = [-sc["truth"][0, f, :, :3].T @ sc["truth"][0, f, :, 3] for f in (at - lag, at)]  # of both cameras, in frame 8's coordinates
        out[name] = dict(pts=pts, valid=valid, at=at, base=float(np.linalg.norm(centre[1] - centre[0])))
    out["B"]["full"] = out["B"]["valid"].copy()
    out["B"]["valid"] = out["B"]["valid"].copy()
    out["B"]["valid"][::3] = 0
    return dict(sc=sc, cam=cam, ones=ones, **out)


def check_planted_path(ps, sim, scale, label, merged_valid, origin, poses, frames):
    """What the alignment is worth (numpy): the scale is the ratio of the two baselines; movers are not labelled 1; the taken-out
    points are back; and compose_pose(pose, origin) of poses against the merged structure gives the planted path in A's world within
    the bars tests/test_gpu_structure.py holds its extended chain to (a tenth of the distance from the first structure's frame, 0.2
    degrees)."""
    sc, A, B = ps["sc"], ps["A"], ps["B"]
    mover = sc["mover"][0]
    # X_a = X / base_A and X_b = X / base_B in their own cameras: s = base_A / base_B.  Each baseline is known to the noise of one
    # two-view pose, the bar test_gpu_structure's chain is held to: a tenth.
    assert abs(float(scale) * B["base"] / A["base"] - 1.0) <= 0.1, (float(scale), A["base"] / B["base"])
    both = (A["valid"] == 1) & (B["valid"] == 1)
    assert (label[both & ~mover] == 1).mean() > 0.9 and (label[~both] == -1).all()
    carried = (A["valid"] == 1) & (B["valid"] == 0)
    assert carried.sum() > 0.15 * mover.size and (merged_valid[carried] == 1).mean() > 0.95 and (merged_valid[B["valid"] == 1] == 1).all()
    M, to = origin[:, :3].astype(np.float64), origin[:, 3].astype(np.float64)
    s = float(scale)
    for j, f in enumerate(frames):
        Rt, tt = sc["truth"][0, f, :, :3], sc["truth"][0, f, :, 3] / A["base"]
        Rm, tm = poses[j, :, :3].astype(np.float64), poses[j, :, 3].astype(np.float64)
        Mw, tw = Rm @ M, Rm @ to + tm  # ops.compose_pose; (Mw | tw) / s is the rigid pose in A's world and unit
        Ct, Cm = -Rt.T @ tt, -np.linalg.solve(Mw, tw)
        assert np.linalg.norm(Cm - Ct) <= 0.1 * np.linalg.norm(Ct), (f, Cm, Ct)
        assert np.degrees(2.0 * np.arcsin(min(1.0, np.linalg.norm(Mw / s - Rt) / (2.0 * np.sqrt(2.0))))) <= 0.2


PATH_FRAMES = (21, 22, 23)
PATH_FIT = dict(tol=2.0, hypotheses=256, min_points=16, seed=0)


def test_a_planted_path_through_two_structures(tmp_path_factory):
    """reconstruct at frame 8 and again at frame 20 (planted, through the g++ builds), ops.fit_align, ops.merge_structures, then
    the localize chain (ctk_fit_epipolar, ctk_fit_pose, ctk_fit_resection) and ops.fit_p3p against the merged structure on frames
    21..23: both follow the planted path through `origin`, whose left block carries the scale."""
    from cotracker_amd import ops
    from test_gpu_structure import bind_hosts
    ps = planted_two_structures(bind_hosts(tmp_path_factory))
    cam, coords = ps["cam"], ps["sc"]["coords"]
    tr, vi = t(coords), t(ps["ones"]).bool()
    structs = {}
    for name in ("A", "B"):
        at = ps[name]["at"]
        anchor = ops.FieldAnchor(tr[:, at].contiguous(), vi[:, at].contiguous(), at)
        structs[name] = ops.Structure(t(ps[name]["pts"]), t(ps[name]["valid"]), anchor, cam)
    A, B = structs["A"], structs["B"]
    (sim, scale, label, error, stats), rows = recorded(lambda: ops.fit_align(A.points, A.valid, B.points, B.valid, cam, hypotheses=256, seed=0))
    assert rows == {"fit_align": 1} and int(stats[0, 2]) >= 0 and int(stats[0, 3]) == 0
    same([x.cpu().numpy() for x in (sim, scale, label, error, stats)],
         AL.fit_align(ps["A"]["pts"][None], ps["A"]["valid"][None], ps["B"]["pts"][None], ps["B"]["valid"][None], cam, hypotheses=256, seed=0))
    merged = ops.merge_structures(A, B, sim[0], label[0])
    assert merged.anchor is B.anchor and merged.intrinsics == B.intrinsics
    fr = list(PATH_FRAMES)
    mask = merged.valid[None]
    # localize() as the predictor chains it -- ctk_fit_epipolar with the structure's mask, ctk_fit_pose, ctk_fit_resection -- and
    # resect()'s one launch: both against the merged structure's anchor
    fund, lab, _, _ = ops.fit_epipolar(tr, vi, mask=mask, anchor=merged.anchor, tol=1.0, hypotheses=512, min_base=16.0, min_points=16, seed=0)
    seeds, _, _ = ops.fit_pose(tr, vi, cam, fund, lab, mask=mask, anchor=merged.anchor, min_points=16)
    chain = ops.fit_resection(tr, vi, cam, merged.points[None], mask, seeds, anchor=merged.anchor, **PATH_FIT)
    one = ops.fit_p3p(tr, vi, cam, merged.points[None], mask, anchor=merged.anchor, **PATH_FIT)
    for pose, _, _, st in (chain, one):
        assert (st[0, fr, 2] >= 0).all()
        world = ops.compose_pose(pose[0, fr], merged.origin)
        assert tuple(world.shape) == (3, 3, 4)
        check_planted_path(ps, sim[0].cpu().numpy(), scale[0].cpu().numpy(), label[0].cpu().numpy(), merged.valid.cpu().numpy(),
                           merged.origin.cpu().numpy(), pose[0, fr].cpu().numpy(), fr)
        # ops.camera_centre gives the centres check_planted_path compares, in the first world's unit
        Cm = ops.camera_centre(world).cpu().numpy().astype(np.float64)
        for j, f in enumerate(fr):
            Rt, tt = ps["sc"]["truth"][0, f, :, :3], ps["sc"]["truth"][0, f, :, 3] / ps["A"]["base"]
            assert np.linalg.norm(Cm[j] + Rt.T @ tt) <= 0.1 * np.linalg.norm(Rt.T @ tt)


def test_align_and_georeference_on_a_push_stream(monkeypatch):
    """Ring + graph on, frames pushed as uint8.  align() is ONE launch and equals ops.fit_align on the two structures; georeference()
    with 6 known points returns the planted metric scale by the same launch.  The stream's tracks are bit-identical to a twin's that
    never asks, nothing is re-captured, and the stream's state is not re-allocated.  A v2 predictor raises."""
    from cotracker_amd import ops
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    from cotracker_amd.synthetic import synthetic_video
    K, G, N, spare, g = 16, 2, 24, 2, 1
    T = S + 2 * STEP
    cam = (120.0, 118.0, 70.0, 50.0)
    video = synthetic_video(T, *RAW, seed=11)[0].permute(0, 2, 3, 1).round().to(torch.uint8).contiguous().to(dev())
    gen = torch.Generator().manual_seed(2)
    q = (torch.rand(G, N, 3, generator=gen) * torch.tensor([0.0, RAW[1] - 1.0, RAW[0] - 1.0])).to(dev())
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
        p.align(None, None)
    state, checked = None, 0
    rng = np.random.default_rng(7)
    for k, t0 in enumerate(range(0, T - S + 1, STEP)):
        new = video[:S] if k == 0 else video[t0 + S - STEP:t0 + S]
        c0 = len(captures)
        got = p.push_frames(new, add_support_grid=True)
        c1 = len(captures)
        ref = twin.push_frames(new, add_support_grid=True)
        assert len(captures) - c1 == c1 - c0, (k, c0, c1, len(captures))  # nothing is re-captured: the twin, which never asks, captures as often
        assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(got[1], ref[1]), k
        gs = p.model._gstream
        ptrs = tuple(h_.data_ptr() for h_ in gs.hist) + (gs.queries.data_ptr(),)
        assert state is None or state == ptrs  # the stream's state stays where it is
        state = ptrs
        # two structures over the stream's own slots, planted: b = s R a + t with a fifth of the points moved
        Nm = gs.N
        sc = AL.planted(50 + k, N=Nm, share=0.2)
        va, vb = np.ones(Nm, dtype=np.int8), np.ones(Nm, dtype=np.int8)
        va[1], vb[2] = 0, 0
        A = ops.Structure(t(sc["a"]), t(va), p.pin(gs.committed - 2, g), cam)
        B = ops.Structure(t(sc["b"]), t(vb), p.pin(gs.committed - 1, g), AL.CAM)
        fit = dict(hypotheses=65, min_points=6, seed=3)
        res, rows = recorded(lambda: p.align(A, B, **fit))
        assert rows == {"fit_align": 1} and len(captures) == c1 + (c1 - c0)  # ONE launch, no capture
        assert [tuple(x.shape) for x in res] == [(3, 4), (), (Nm,), (Nm,), (4,)]
        want = ops.fit_align(A.points, A.valid, B.points, B.valid, AL.CAM, **fit)  # b's intrinsics
        for a_, b_ in zip(res, want):
            assert torch.equal(bits(a_), bits(b_[0]))
        assert int(res[4][2]) >= 0 and int(res[2][1]) == -1 and int(res[2][2]) == -1
        merged = ops.merge_structures(A, B, res[0], res[2])
        assert merged.anchor is B.anchor and int(merged.valid[2]) == 1 and int(merged.valid[1]) == int(vb[1])
        # georeference: 6 surveyed points of a structure in metres; float32 coordinates of magnitude 10 over sides of about 1 leave
        # the scale good to some 1e-6: 1e-4 is asked
        s0, R0, t0 = 3.7, AL.rotation([0.2, -1.0, 0.3], 0.1), np.array([0.2, -0.1, 0.4])
        slots = rng.permutation(Nm)[:6]
        known = (s0 * sc["b"][slots].astype(np.float64) @ R0.T + t0).astype(np.float32)
        res, rows = recorded(lambda: p.georeference(B, t(known), slots.tolist(), intrinsics=AL.CAM))
        assert rows == {"fit_align": 1} and len(captures) == c1 + (c1 - c0)
        assert int(res[4][0]) == 5 + int(vb[slots].sum() == 6) and int(res[4][2]) >= 0 and int(res[4][1]) == int(res[4][0])
        assert abs(float(res[1]) / s0 - 1.0) <= 1e-4
        metric = ops.apply_similarity(res[0], B.points[t(slots).long()])
        assert np.allclose(metric.cpu().numpy()[vb[slots] == 1], known[vb[slots] == 1], atol=1e-3)
        with pytest.raises(ValueError, match="ops.Structure"):
            p.align(None, B)
        with pytest.raises(ValueError, match="known"):
            p.georeference(B, t(known)[:5], slots.tolist())
        checked += 1
    assert checked == 3  # (not vacuous)
    same_tracks, mine = twin.recent(4), p.recent(4)
    assert torch.equal(mine[0].view(torch.int32), same_tracks[0].view(torch.int32)) and torch.equal(mine[1], same_tracks[1])
    for x in (p, twin):
        x.finish()
    p2 = CoTrackerOnlinePredictor(checkpoint=None, v2=True, window_len=8)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.align(None, None)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.georeference(None, None, None)
