"""ctk_fit_structure on the GPU (csrc/structure.hip) against the numpy restatement of tests/structure_reference.py: every byte of
poisoned, fenced outputs, the float32 points, errors and origins bit for bit, the inputs unchanged.  The shapes are
structure_reference.cases(): 1, 63, 64, 65 and 300 slots (one workgroup less one slot, one, one and a slot, several); 1, 2, 3, 8 and
256 views; one and two groups; min_views 2, 3 and F; a ring of 8 rows after 14 frames with first rows, bytes and logits; NaN and
outside positions; views without a fit, with a NaN pose and with a zero matrix; every mode of into, carry, refine and origin; a point
behind two cameras, wrong views, parallel rays, a point at a camera centre, a standing camera.  One case chains the four kernels as
extend() does; the last ones hold the host layers to them."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_reference as R
import resection_reference as RR
import structure_reference as SR
from ctk_support import STEP, S, dev, host_library, recorded, t

pytestmark = pytest.mark.gpu

GUARD, POISON, FENCE = 64, 0x5A, 0xA5
NAMES = ("points", "label", "error", "stats", "origin")


def fenced(nbytes):
    """A poisoned output of nbytes between two fences: -> (whole buffer, the output's view)."""
    buf = torch.full((nbytes + 2 * GUARD,), FENCE, dtype=torch.uint8, device=dev())
    buf[GUARD:GUARD + nbytes] = POISON
    return buf, buf[GUARD:GUARD + nbytes]


def raw_fit(coords, cam, pose, *, pose_stats=None, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=None,
            into=-1, source_frame=0, structure=None, valid=None, origin_in=None, tol=2.0, min_views=3, sin2=None, refine=0,
            scale=(1.0, 1.0)):
    """The C-ABI call itself on poisoned, fenced outputs -> (points, label, error, stats, origin) as numpy; the fences and the inputs are
    checked here."""
    from cotracker_amd import _lib as L_
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    F = np.asarray(pose).shape[1] if F is None else F
    given = (visible, vis, conf, first_row, np.asarray(pose, dtype=np.float32), pose_stats,
             None if structure is None else np.asarray(structure, dtype=np.float32), None if valid is None else np.asarray(valid, dtype=np.int8),
             None if origin_in is None else np.asarray(origin_in, dtype=np.float32))
    keep = [t(coords)] + [None if x is None else t(np.ascontiguousarray(x)) for x in given]
    before = [None if x is None else x.clone() for x in keep]
    a = L_.Structure3D.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.F = G, N, N_out, R_, f0, F
    a.into, a.source_frame, a.min_views, a.refine, a.reserved = into, source_frame, min_views, refine, 0
    a.fx, a.fy, a.cx, a.cy = cam
    a.sx, a.sy, a.thresh, a.tol, a.min_sin2 = scale[0], scale[1], thresh, tol, SR.min_sin2(1.0) if sin2 is None else sin2
    (a.hist_coords, a.visible, a.hist_vis, a.hist_conf, a.first_row, a.pose, a.pose_stats, a.structure_in, a.valid_in,
     a.origin_in) = (None if x is None else x.data_ptr() for x in keep)
    outs = [fenced(G * N_out * 12), fenced(G * N_out), fenced(G * N_out * 4), fenced(G * N_out * 16), fenced(G * 48)]
    a.points, a.label, a.error, a.stats, a.origin_out = (o[1].data_ptr() for o in outs)
    n = C.c_size_t(99)
    L_.check(L_.load().ctk_fit_structure_workspace_bytes(C.byref(a), C.byref(n)), "ctk_fit_structure_workspace_bytes")
    assert n.value == 0
    L_.check(L_.load().ctk_fit_structure(C.byref(a), None, 0, torch.cuda.current_stream().cuda_stream), "ctk_fit_structure")
    torch.cuda.synchronize()
    for whole, _ in outs:  # the bytes next to each output
        assert bool((whole[:GUARD] == FENCE).all()) and bool((whole[-GUARD:] == FENCE).all())
    for x, b in zip(keep, before):  # the kernel only reads its inputs
        assert x is None or torch.equal(x.view(torch.uint8), b.view(torch.uint8))
    pt, la, er, st, og = (o[1].cpu().numpy() for o in outs)
    return (pt.view(np.float32).reshape(G, N_out, 3), la.view(np.int8).reshape(G, N_out), er.view(np.float32).reshape(G, N_out),
            st.view(np.int32).reshape(G, N_out, 4), og.view(np.float32).reshape(G, 3, 4))


def same(got, want):
    for g_, w_, name in zip(got, want, NAMES):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        eq = (g_.view(np.int32) if g_.dtype == np.float32 else g_) == (w_.view(np.int32) if w_.dtype == np.float32 else w_)
        assert eq.all(), (name, np.argwhere(~eq)[:5].tolist(), g_[~eq][:5], w_[~eq][:5])


CASES = {name: (args, kw) for name, args, kw in SR.cases()}
WANT = {}


def want(name):
    """The restatement's answer, computed once per case and left unchanged."""
    if name not in WANT:
        WANT[name] = SR.fit_structure(*CASES[name][0], **CASES[name][1])
    return WANT[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_against_the_restatement(name):
    """Every byte of the five poisoned outputs equals the restatement's (no value of which is the poison pattern)."""
    args, kw = CASES[name]
    same(raw_fit(*args, **kw), want(name))


# ---- the four kernels chained on a stream-shaped history --------------------------------------------------------------------------------
G_, T_, N_, RING, AT, F0, F1, KEY = 1, 14, 300, 8, 3, 6, 6, 8  # the first chain: frames 6..11 against frame 3; the keyframe: frame 8


def bind_hosts(tmp_path_factory):
    hosts = {n: host_library(tmp_path_factory, n) for n in ("epipolar", "pose", "resection", "structure")}
    hosts["epipolar"].host_fit_epipolar.restype = C.c_int
    hosts["epipolar"].host_fit_epipolar.argtypes = [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 5 + [C.c_void_p] * 12
    hosts["pose"].host_fit_pose.restype = C.c_int
    hosts["pose"].host_fit_pose.argtypes = [C.c_int] * 10 + [C.c_float] * 7 + [C.c_void_p] * 13
    hosts["resection"].host_fit_resection.restype = C.c_int
    hosts["resection"].host_fit_resection.argtypes = [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 8 + [C.c_void_p] * 14
    hosts["structure"].host_fit_structure.restype = C.c_int
    hosts["structure"].host_fit_structure.argtypes = [C.c_int] * 10 + [C.c_float] * 9 + [C.c_void_p] * 15
    return hosts


def host_localize(hosts, c, rows, cam, f0, F_, lag, anchor, mask, pts, vis=None, conf=None, first=None, visible=None, structure=True):
    """The g++ builds chained as localize() chains the kernels (the helper shapes of tests/test_gpu_resection.py) ->
    (fundamental, label), (seed poses, depths), (pose, label, error, stats) or None."""
    N, G = c.shape[2], c.shape[0]
    ptr = [None if x is None else x.ctypes.data for x in (visible, vis, conf, first, None if anchor is None else anchor[0],
                                                          None if anchor is None else anchor[1], mask)]
    af = 0 if anchor is None else anchor[2]
    e = [np.full((G, F_, 3, 3), np.nan, dtype=np.float32), np.full((G, F_, N), 77, dtype=np.int8), np.full((G, F_, N), np.nan, dtype=np.float32),
         np.full((G, F_, 4), -99, dtype=np.int32)]
    assert hosts["epipolar"].host_fit_epipolar(G, N, N, rows, f0, F_, -1, lag, af, 16, 512, 0, 1.0, 16.0, 1.0, 1.0, 0.6, c.ctypes.data, *ptr,
                                               *(w.ctypes.data for w in e)) == 0
    p = [np.full((G, F_, 3, 4), np.nan, dtype=np.float32), np.full((G, F_, N, 2), 77.0, dtype=np.float32), np.full((G, F_, 4), -99, dtype=np.int32)]
    assert hosts["pose"].host_fit_pose(G, N, N, rows, f0, F_, -1, lag, af, 16, *cam, 1.0, 1.0, 0.6, c.ctypes.data, *ptr, e[0].ctypes.data,
                                       e[1].ctypes.data, *(w.ctypes.data for w in p)) == 0
    if not structure:
        return e, p, None
    r = [np.full((G, F_, 3, 4), np.nan, dtype=np.float32), np.full((G, F_, N), 77, dtype=np.int8), np.full((G, F_, N), 77.0, dtype=np.float32),
         np.full((G, F_, 4), -99, dtype=np.int32)]
    assert hosts["resection"].host_fit_resection(G, N, N, rows, f0, F_, -1, lag, af, 16, 256, 0, *cam, 1.0, 1.0, 0.6, 2.0, c.ctypes.data, *ptr[:6],
                                                 pts.ctypes.data, mask.ctypes.data, p[0].ctypes.data, *(w.ctypes.data for w in r)) == 0
    return e, p, r


def planted_stream(hosts):
    """One planted camera path as a stream holds it: a ring of 8 rows after 14 frames, logits, first rows; a planted reconstruct on the
    pair (0, 3) through the g++ builds, a third of its points taken out again."""
    sc = RR.scene(21, G_, T_, N_, src=AT, hw=(540, 960), noise=0.1, p_visible=2.0)
    coords, cam = sc["coords"], sc["cam"]
    ones = np.ones((G_, T_, N_), dtype=np.uint8)
    e, p, _ = host_localize(hosts, coords, T_, cam, AT, 1, AT, None, None, None, visible=ones, structure=False)
    assert e[3][0, 0, 2] >= 0
    pts, full = RR.structure_from_pose(coords[0, AT], cam, p[1][0, 0], e[1][0, 0])
    valid = full.copy()
    valid[::3] = 0
    pts, valid = np.ascontiguousarray(pts[None]), np.ascontiguousarray(valid[None])
    assert valid.sum() > 0.3 * N_ and (full == 1).sum() - valid.sum() > 0.15 * N_
    ring_c = np.ascontiguousarray(R.fold(coords, RING, T_))
    vis = np.ascontiguousarray(np.where(R.fold(ones, RING, T_) != 0, 5.0, -5.0).astype(np.float32))
    conf = np.full(vis.shape, 6.0, dtype=np.float32)
    first = np.zeros((G_, N_), dtype=np.int32)
    first[0, 5], first[0, 7] = AT + 1, F0 + 2  # released after the structure's frame; arrived mid-window
    return dict(sc=sc, cam=cam, pts=pts, valid=valid, full=full, ring_c=ring_c, vis=vis, conf=conf, first=first, ones=ones)


def host_chain(hosts, ps):
    """The whole of extend() and a later localize() through the g++ builds -> what each kernel must give."""
    sc, cam, ring_c, vis, conf, first = ps["sc"], ps["cam"], ps["ring_c"], ps["vis"], ps["conf"], ps["first"]
    coords = sc["coords"]
    anchor = (np.ascontiguousarray(coords[:, AT]), np.ascontiguousarray(ps["ones"][:, AT]), AT)
    one = host_localize(hosts, ring_c, RING, cam, F0, F1, 0, anchor, ps["valid"], ps["pts"], vis=vis, conf=conf, first=first)
    st = [np.full((G_, N_, 3), np.nan, dtype=np.float32), np.full((G_, N_), 77, dtype=np.int8), np.full((G_, N_), 77.0, dtype=np.float32),
          np.full((G_, N_, 4), -99, dtype=np.int32), np.full((G_, 3, 4), np.nan, dtype=np.float32)]
    assert hosts["structure"].host_fit_structure(G_, N_, N_, RING, F0, F1, KEY - F0, AT, 3, 0, *cam, 1.0, 1.0, 0.6, 2.0, SR.min_sin2(1.0),
                                                 ring_c.ctypes.data, None, vis.ctypes.data, conf.ctypes.data, first.ctypes.data,
                                                 one[2][0].ctypes.data, one[2][3].ctypes.data, ps["pts"].ctypes.data, ps["valid"].ctypes.data, None,
                                                 *(w.ctypes.data for w in st)) == 0
    # the keyframe's anchor as pin() takes it: positions and visibility of frame 8, gated by the first rows
    seen = (ps["ones"][:, KEY] != 0) & (first <= KEY)
    anchor2 = (np.ascontiguousarray(coords[:, KEY]), np.ascontiguousarray(seen.astype(np.uint8)), KEY)
    valid2 = np.ascontiguousarray((st[1] >= 1).astype(np.int8))
    two = host_localize(hosts, ring_c, RING, cam, KEY + 4, T_ - KEY - 4, 0, anchor2, valid2, st[0], vis=vis, conf=conf, first=first)
    return dict(anchor=anchor, one=one, structure=st, anchor2=anchor2, valid2=valid2, two=two)


def check_planted_path(ps, ch):
    """What the chain is worth: the taken-out points are back, the movers are not, and compose(pose, origin) of the second chain gives
    the planted path within the bars tests/test_gpu_resection.py holds the unextended structure to (a tenth of the distance from the
    first structure's frame, 0.2 degrees)."""
    sc, full, valid = ps["sc"], ps["full"], ps["valid"][0]
    pt, la, er, st, org = ch["structure"]
    mover = sc["mover"][0]
    taken = (full == 1) & (valid == 0) & ~mover
    taken[[5, 7]] = False  # (the slots with first rows)
    old = valid == 1
    old[[5, 7]] = False  # (both arrived after the structure's frame: their slots are not carried)
    assert (la[0][old] == 2).all() and (la[0, [5, 7]] != 2).all() and (la[0][taken] == 1).mean() > 0.95 and (la[0][mover] == 1).mean() < 0.1
    assert st[0, 7, 0] == F1 - 2 and (st[0][taken][:, 0] == F1).all()
    po, _, _, st2 = ch["two"][2]
    assert (st2[0, :, 2] >= 0).all() and (st2[0, :, 3] == 0).all()
    Ro, to = org[0, :, :3].astype(np.float64), org[0, :, 3].astype(np.float64)
    base = float(np.linalg.norm(sc["truth"][0, 0, :, 3]))
    for j in range(po.shape[1]):
        f = KEY + 4 + j
        Rt, tt = sc["truth"][0, f, :, :3], sc["truth"][0, f, :, 3] / base
        Rm, tm = po[0, j, :, :3].astype(np.float64), po[0, j, :, 3].astype(np.float64)
        Rw, tw = Rm @ Ro, Rm @ to + tm  # ops.compose_pose
        Ct, Cm = -Rt.T @ tt, -Rw.T @ tw
        assert np.linalg.norm(Cm - Ct) <= 0.1 * np.linalg.norm(Ct), (j, Cm, Ct)
        assert np.degrees(2.0 * np.arcsin(min(1.0, np.linalg.norm(Rw - Rt) / (2.0 * np.sqrt(2.0))))) <= 0.2


def test_the_four_kernels_chained_on_a_stream_shaped_history(tmp_path_factory):
    """ctk_fit_epipolar -> ctk_fit_pose -> ctk_fit_resection -> ctk_fit_structure as extend() chains them, on a ring of 8 rows after 14
    frames with logits and first rows and an anchor on frame 3, which the ring has dropped, and through the g++ builds of the four
    headers: every bit is equal.  Then the second localize chain against the extended structure, re-anchored on frame 8: every bit
    again, and the planted path comes back through the origin."""
    from test_gpu_epipolar import raw_fit as raw_epipolar
    from test_gpu_pose import raw_fit as raw_pose
    from test_gpu_resection import raw_fit as raw_resection
    hosts = bind_hosts(tmp_path_factory)
    ps = planted_stream(hosts)
    ch = host_chain(hosts, ps)
    cam, ring_c = ps["cam"], ps["ring_c"]

    def gpu_localize(anchor, mask, pts, f0, F_):
        src = dict(vis=ps["vis"], conf=ps["conf"], thresh=0.6, first_row=ps["first"], f0=f0, F=F_, anchor=anchor)
        fu, lab, _, _ = raw_epipolar(ring_c, mask=mask, **src)
        seeds = raw_pose(ring_c, cam, fu, lab, mask=mask, min_points=16, **src)[0]
        return fu, lab, seeds, raw_resection(ring_c, cam, pts, mask, seeds, tol=2.0, hypotheses=256, seed=0, min_points=16, **src)

    def bits(x):
        return x.view(np.int32) if x.dtype == np.float32 else x
    fu, lab, seeds, res = gpu_localize(ch["anchor"], ps["valid"], ps["pts"], F0, F1)
    assert np.array_equal(bits(fu), bits(ch["one"][0][0])) and np.array_equal(lab, ch["one"][0][1]) and np.array_equal(bits(seeds), bits(ch["one"][1][0]))
    for g_, w_ in zip(res, ch["one"][2]):
        assert np.array_equal(bits(g_), bits(w_))
    got = raw_fit(ring_c, cam, res[0], pose_stats=res[3], vis=ps["vis"], conf=ps["conf"], thresh=0.6, first_row=ps["first"], f0=F0, F=F1,
                  into=KEY - F0, source_frame=AT, structure=ps["pts"], valid=ps["valid"], min_views=3)
    same(got, ch["structure"])
    fu, lab, seeds, res2 = gpu_localize(ch["anchor2"], np.ascontiguousarray((got[1] >= 1).astype(np.int8)), got[0], KEY + 4, T_ - KEY - 4)
    for g_, w_ in zip(res2, ch["two"][2]):
        assert np.array_equal(bits(g_), bits(w_))
    check_planted_path(ps, ch)


def test_the_ops_layer():
    """ops.fit_structure: one launch, `out`, one group without its axis, and the refusals."""
    from cotracker_amd import ops
    name = "size_300_8_2"
    (coords, cam, pose), kw = CASES[name]
    G, T, N = coords.shape[:3]
    N = kw["N_out"]
    coords, visible = np.ascontiguousarray(coords[:, :, :N]), np.ascontiguousarray(kw["visible"][:, :, :N])
    structure = np.random.default_rng(3).normal(0, 1, (G, N, 3)).astype(np.float32) + np.float32([0, 0, 6])
    valid = (np.arange(N)[None] % 4 == 0).astype(np.int8).repeat(G, 0)
    stats = np.zeros((G, T, 4), dtype=np.int32)
    stats[1, 2, 2] = -1
    origin = pose[:, 3].copy()
    fit = dict(tol=2.0, min_views=3, source_frame=0, into=T - 1)
    want_ = SR.fit_structure(coords, cam, pose, pose_stats=stats, visible=visible, structure=structure, valid=valid, origin_in=origin,
                             sin2=SR.min_sin2(0.5), **fit)
    assert (want_[1] == 1).sum() > 200 and (want_[1] == 2).sum() == G * N // 4
    tr, vi, po, ps_, st, va, og = t(coords), t(visible).bool(), t(pose), t(stats), t(structure), t(valid), t(origin)
    old = dict(pose_stats=ps_, structure=st, valid=va, origin=og, min_parallax=0.5)
    got, rows = recorded(lambda: ops.fit_structure(tr, vi, cam, po, **old, **fit))
    assert rows == {"fit_structure": 1}
    same([g_.cpu().numpy() for g_ in got], want_)
    assert [tuple(g_.shape) for g_ in got] == [(G, N, 3), (G, N), (G, N), (G, N, 4), (G, 3, 4)]
    out = tuple(torch.empty_like(g_) for g_ in got)
    again = ops.fit_structure(tr, vi, cam, po, **{**old, "valid": va.bool()}, out=out, **fit)
    assert all(a_ is b_ for a_, b_ in zip(again, out))
    same([g_.cpu().numpy() for g_ in again], want_)
    one = ops.fit_structure(tr[0], vi[0], list(cam), po[0], pose_stats=ps_[0], structure=st[0], valid=va[0].to(torch.uint8), origin=og[0],
                            min_parallax=0.5, **fit)
    same([g_.cpu().numpy() for g_ in one], [w[:1] for w in want_])
    plain = ops.fit_structure(tr, vi, cam, po)  # no old structure, no into: the defaults
    same([g_.cpu().numpy() for g_ in plain], SR.fit_structure(coords, cam, pose, visible=visible))
    for bad in (dict(min_views=1), dict(min_views=257), dict(tol=0.0), dict(tol=float("nan")), dict(into=T), dict(into=-2), dict(min_parallax=0.0),
                dict(min_parallax=91.0), dict(source_frame=-1), dict(valid=None), dict(structure=None), dict(out=out[:4])):
        with pytest.raises(ValueError):
            ops.fit_structure(tr, vi, cam, po, **{**old, **fit, **bad})
    for bad_cam in ((0.0, 1.0, 2.0, 3.0), (1.0, float("nan"), 2.0, 3.0), (1.0, 2.0, 3.0), t(np.array(cam))):
        with pytest.raises(ValueError, match="intrinsics"):
            ops.fit_structure(tr, vi, bad_cam, po)
    for kw_ in (dict(pose=po.double()), dict(pose=po[:, :3]), dict(pose=po.cpu()), dict(pose_stats=ps_.float()), dict(pose_stats=ps_[:, :3]),
                dict(structure=st[:, :5]), dict(valid=va.float()), dict(origin=og.double()), dict(origin=og[:, :2])):
        args = {**dict(pose=po), **old, **fit, **kw_}
        with pytest.raises(ValueError):
            ops.fit_structure(tr, vi, cam, args.pop("pose"), **args)
    with pytest.raises(ValueError, match="views"):  # more than 256 frames
        ops.fit_structure(torch.zeros(257, 4, 2, device=dev()), torch.ones(257, 4, dtype=torch.bool, device=dev()), cam,
                          torch.zeros(257, 3, 4, device=dev()))


# ---- the predictor --------------------------------------------------------------------------------------------------------------------
def test_extend_on_a_push_stream(monkeypatch):
    """Ring + graph on, frames pushed as uint8, as test_reconstruct_and_localize_on_a_push_stream sets it up.  extend() is localize(),
    ops.fit_structure on the tracks as recent() emits them, and pin(): five launches, bit for bit; extend(poses=...) equals extend()
    with two launches; the stream's tracks are bit-identical to a twin's that never asks, nothing is re-captured, the stream's state is
    not re-allocated; localize() runs against the extended structure and world_pose() composes its origin."""
    from cotracker_amd import ops
    from cotracker_amd.synthetic import synthetic_video
    from test_gpu_resection import RAW, bits, small_predictor
    K, G, N, spare, g = 16, 2, 24, 2, 1
    T = S + 4 * STEP
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
    Nu = N + spare
    # synthetic weights track nothing real: the bounds are wide, so that some frames have a fit and some points are accepted
    two_view = dict(tol=6.0, min_base=1.0, hypotheses=64, min_points=8, seed=3)
    loc = dict(hypotheses=33, min_points=6, seed=3, epipolar_tol=6.0, epipolar_hypotheses=64, min_base=1.0)
    ext = dict(tol=8.0, min_views=2, min_parallax=0.05)
    state, checked, kept, added, dead = None, 0, 0, 0, 0
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
        n = STEP + 1
        # a structure on the first of the n frames (its own frame is localised exactly), a quarter of its points taken out again
        s0 = p.reconstruct(cam, done - n, lag=3, max_depth=1e6, group=g, **two_view)
        drop = s0.valid.clone()
        drop[::4] = 0  # (what extend() may add again)
        s0 = ops.Structure(s0.points, drop, s0.anchor, cam)
        pose, _, _, stats = p.localize(s0, n, tol=8.0, **loc)
        fitted = torch.nonzero(stats[:, 2] >= 0).flatten().tolist()  # (a test may wait: the keyframe is the newest localised frame, if any)
        frame = done - n + fitted[-1] if fitted else done - 2
        s1, rows = recorded(lambda: p.extend(s0, frame, n, **ext, **loc))
        assert rows == {"fit_epipolar": 1, "fit_pose": 1, "fit_resection": 1, "fit_structure": 1} and len(captures) == c1 + (c1 - c0)
        assert isinstance(s1, ops.Structure) and s1.anchor.frame == frame and s1.anchor.group == g and s1.intrinsics == cam
        assert tuple(s1.points.shape) == (gs.N, 3) and tuple(s1.valid.shape) == (gs.N,) and s1.valid.dtype == torch.int8
        assert tuple(s1.origin.shape) == (3, 4) and not bool(s1.valid[Nu:].any())
        # the same through the public pieces: localize() (above), ops.fit_structure on the emitted tracks, pin()
        tr, vi = p.recent(min(done, K))
        full_t, full_v = torch.zeros(done, Nu, 2, device=dev()), torch.zeros(done, Nu, dtype=torch.bool, device=dev())
        full_t[done - tr.shape[1]:], full_v[done - tr.shape[1]:] = tr[g], vi[g]
        f0 = done - n
        want_ = ops.fit_structure(full_t[f0:], full_v[f0:], cam, pose, pose_stats=stats, structure=s0.points[:Nu].contiguous(),
                                  valid=s0.valid[:Nu].contiguous(), source_frame=s0.anchor.frame, into=frame - f0,
                                  first_row=None if first is None else (first - f0).clamp(min=0), **ext)  # (rows count from f0 here; no slot arrived after frame 0)
        assert torch.equal(bits(s1.points[:Nu]), bits(want_[0][0])) and torch.equal(s1.valid[:Nu], (want_[1][0] >= 1).to(torch.int8))
        assert torch.equal(bits(s1.origin), bits(want_[4][0]))
        pin = p.pin(frame, g)
        assert torch.equal(bits(s1.anchor.coords), bits(pin.coords)) and torch.equal(s1.anchor.visible, pin.visible)
        # extend(poses=...) skips localize(): two launches, the same structure
        s2, rows = recorded(lambda: p.extend(s0, frame, n, poses=(pose, stats), **ext))
        assert rows == {"fit_structure": 1}
        assert torch.equal(bits(s2.points), bits(s1.points)) and torch.equal(s2.valid, s1.valid) and torch.equal(bits(s2.origin), bits(s1.origin))
        label = want_[1][0]
        localised = int(stats[frame - f0, 2]) >= 0
        if localised:
            kept += int((label == 2).sum())
            added += int((label == 1).sum())
            assert int((label == 2).sum()) == int(s0.valid[:Nu].sum())  # (no slot of this stream is released: every old point is carried)
        else:  # the keyframe could not be localised: no structure, the caller keeps the old one
            dead += 1
            assert not bool(s1.valid.any()) and torch.equal(bits(s1.origin), bits(torch.eye(3, 4, device=dev())))
        print("extend on frame", frame, "of", done, "localised views", fitted, "labels", {v: int((label == v).sum()) for v in (-1, 0, 1, 2)})
        # localize() runs against the extended structure, and world_pose() composes its origin
        res, rows = recorded(lambda: p.localize(s1, tol=8.0, **loc))
        assert rows == {"fit_epipolar": 1, "fit_pose": 1, "fit_resection": 1} and [tuple(x.shape) for x in res] == [(STEP, 3, 4), (STEP, Nu), (STEP, Nu), (STEP, 4)]
        world = p.world_pose(s1, res[0])
        assert torch.equal(bits(world), bits(ops.compose_pose(res[0], s1.origin))) and tuple(world.shape) == (STEP, 3, 4)
        checked += 1
        with pytest.raises(ValueError, match="must lie inside"):
            p.extend(s0, done - n - 1, n, **ext)
        with pytest.raises(ValueError, match="beyond what has been tracked"):
            p.extend(s0, None, 2, first_frame=done - 1)
        with pytest.raises(ValueError, match="ops.Structure"):
            p.extend(None)
    assert checked == 3 and kept > 0 and added > 0, (checked, kept, added, dead)  # (not vacuous: a keyframe was localised and points came back)
    same_tracks, mine = twin.recent(4), p.recent(4)
    assert torch.equal(mine[0].view(torch.int32), same_tracks[0].view(torch.int32)) and torch.equal(mine[1], same_tracks[1])
    for x in (p, twin):
        x.finish()
