"""The arithmetic of the structure kernel (csrc/structure.hip) pinned WITHOUT a GPU.

co-tracker_amd/csrc/structure_math.h holds the rules of ctk_fit_structure -- the views, the linear midpoint start, the three gated
Gauss-Newton rounds, the parallax test, the carry and the origin -- in host/device inline functions.  This test compiles that header
with g++ (-ffp-contract=off, the flag the device translation unit is built with) behind plain loops (tests/host/structure_host.cpp) and
compares it with the numpy restatement of tests/structure_reference.py: every bit of all five outputs, on the shapes the kernel is held
to by tests/test_gpu_structure.py.  The same file, built as a stand-alone program under AddressSanitizer and UBSan, runs clean.  The
last test measures what the rules are worth on planted camera paths through the g++ builds of all four headers, chained as
CoTrackerOnlinePredictor.extend chains the kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import motion_reference as R
import resection_reference as RR
import structure_reference as SR
from ctk_support import ROOT, host_library

NAMES = ("points", "label", "error", "stats", "origin")


def bind(lib):
    lib.host_structure_view.restype = C.c_int
    lib.host_structure_view.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.host_fit_structure.restype = C.c_int
    lib.host_fit_structure.argtypes = [C.c_int] * 10 + [C.c_float] * 9 + [C.c_void_p] * 15
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return bind(host_library(tmp_path_factory, "structure"))


def run_host(host, coords, cam, pose, pose_stats=None, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0,
             F=None, into=-1, source_frame=0, structure=None, valid=None, origin_in=None, tol=2.0, min_views=3, sin2=None, refine=0,
             scale=(1.0, 1.0)):
    coords = np.ascontiguousarray(coords, dtype=np.float32)
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    F = np.asarray(pose).shape[1] if F is None else F
    sin2 = SR.min_sin2(1.0) if sin2 is None else sin2

    def ptr(a, dt):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=dt)
        return a, a.ctypes.data
    keep = [ptr(visible, np.uint8), ptr(vis, np.float32), ptr(conf, np.float32), ptr(first_row, np.int32), ptr(pose, np.float32),
            ptr(pose_stats, np.int32), ptr(structure, np.float32), ptr(valid, np.int8), ptr(origin_in, np.float32)]
    before = [None if k[0] is None else k[0].copy() for k in keep]
    outs = [np.full((G, N_out, 3), np.nan, dtype=np.float32), np.full((G, N_out), 77, dtype=np.int8),
            np.full((G, N_out), 77.0, dtype=np.float32), np.full((G, N_out, 4), -99, dtype=np.int32), np.full((G, 3, 4), np.nan, dtype=np.float32)]
    rc = host.host_fit_structure(G, N, N_out, R_, f0, F, into, source_frame, min_views, refine, *cam, scale[0], scale[1], thresh, tol, sin2,
                                 coords.ctypes.data, *(k[1] for k in keep), *(o.ctypes.data for o in outs))
    assert rc == 0
    for k, b in zip(keep, before):  # the inputs are only read
        assert b is None or np.array_equal(k[0].view(np.uint8), b.view(np.uint8))
    return tuple(outs)


def same(got, want):
    for g_, w_, name in zip(got, want, NAMES):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        eq = (g_.view(np.int32) if g_.dtype == np.float32 else g_) == (w_.view(np.int32) if w_.dtype == np.float32 else w_)
        assert eq.all(), (name, np.argwhere(~eq)[:5].tolist(), g_[~eq][:5], w_[~eq][:5])


def stated_forms(points, label, error, stats, origin):
    """Nothing but the stated forms: labels -1 / 0 / 1 / 2; points zero where the label is < 1 and finite elsewhere; an error of -1
    exactly where the label is not 1, never a NaN; stats (m, counted, first, bits) in their ranges."""
    assert np.isin(label, (-1, 0, 1, 2)).all() and not np.isnan(error).any() and np.isfinite(points).all()
    assert (points[label < 1] == 0).all() and ((error == -1) == (label != 1)).all() and (error[label == 1] >= 0).all()
    m, counted, first, bits = (stats[..., i] for i in range(4))
    assert (m >= 0).all() and (counted >= 0).all() and (counted <= m).all() and (bits & ~127 == 0).all() and ((first >= 0) == (counted > 0)).all()
    assert (m[label == -1] < 2).all() and (bits[label == 1] & (SR.BIT_NO_START | SR.BIT_NO_PARALLAX | SR.BIT_INTO | SR.BIT_MINORITY) == 0).all()
    dead = bits & SR.BIT_INTO != 0
    assert (dead.all(axis=1) | ~dead.any(axis=1)).all() and (label[dead] < 1).all()  # no structure: every slot of the group says so


def test_views_on_edge_values(host):
    from epipolar_reference import rotation
    rng = np.random.default_rng(0)
    views = [np.eye(3, 4), np.zeros((3, 4)), np.full((3, 4), np.nan), np.full((3, 4), 3e38), np.full((3, 4), 1e-30),
             np.concatenate([np.diag([1.0, -1.0, 1.0]), np.ones((3, 1))], axis=1), np.concatenate([np.eye(3), [[np.inf], [0], [0]]], axis=1),
             np.concatenate([rotation(0.3, -0.2, 1.0) * 1.2, [[0.5], [-2.0], [3.0]]], axis=1), np.ones((3, 4))]
    views += [np.concatenate([rotation(*rng.uniform(-3, 3, 3)) + rng.normal(0, 0.05, (3, 3)), rng.normal(0, 1, (3, 1))], axis=1)
              for _ in range(20)]
    counting = 0
    for m in views:
        for stats_ok in (1, 0):
            m32 = np.ascontiguousarray(m, dtype=np.float32)
            out = np.full(15, 7.0)
            ok = host.host_structure_view(m32.ctypes.data, stats_ok, out.ctypes.data)
            wok, Rw, tw, cw = SR.view(m32, stats_ok)
            assert bool(ok) == wok and np.array_equal(out.view(np.int64), np.array(list(Rw) + list(tw) + list(cw)).view(np.int64))
            counting += wok
    assert 5 <= counting < len(views)


CASES = {name: (args, kw) for name, args, kw in SR.cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_bit_for_bit(host, name):
    args, kw = CASES[name]
    want = SR.fit_structure(*args, **kw)
    same(run_host(host, *args, **kw), want)
    stated_forms(*want)


def test_cases_cover_what_they_name():
    """The cases reach the branches they are there for (on the restatement, which the two builds equal)."""
    out = {name: SR.fit_structure(*args, **kw) for name, (args, kw) in CASES.items()}
    pts, la, er, st, org = out["ring_plain"]
    # the special points: behind two cameras (counted less than observed, the first counted view is the third), one wrong view of 5 tol
    # dropped by the gates, parallel rays without parallax, a point at a camera centre (that view is not counted), a wrong view of
    # 40 tol (the start is not robust: rejected, never accepted wrongly)
    assert la[0, 0] == 1 and st[0, 0, 0] - st[0, 0, 1] == 2 and st[0, 0, 2] >= 2 and st[0, 0, 3] == 0
    assert la[0, 1] == 1 and st[0, 1, 1] == st[0, 1, 0] - 1
    assert la[0, 2] == 0 and st[0, 2, 3] & (SR.BIT_NO_PARALLAX | SR.BIT_NO_START)
    assert st[0, 3, 0] == 8 and st[0, 3, 1] < 8 and la[0, 9] == 0
    assert la[0, 4] == -1 and st[0, 4].tolist() == [0, 0, -1, 8]  # an empty slot
    assert 2 <= st[0, 6, 0] <= 5 and st[1, 8, 0] == 0  # arrived mid-window; arrives after it
    assert (st[1, :, 0] <= 5).all() and st[1, :, 0].max() == 5  # three of the eight views of group 1 do not count
    assert np.array_equal(org, np.broadcast_to(np.eye(3, 4, dtype=np.float32), org.shape))
    pts, la, er, st, org = out["ring_carry"]
    assert (la[0, [1, 2]] == 2).all() and (st[0, [1, 2]] == [0, 0, -1, 0]).all() and la[0, 7] != 2 and la[0, 6] == 1  # released after source_frame: not carried
    assert (la[1, ::3] != 2).all() and (la[0, [12, 15]] == 2).all() and (la == 2).sum() > 40 and (la == 1).sum() > 20 and not np.array_equal(org[0, :, :3], np.eye(3, dtype=np.float32))
    assert la[0, 5] != 2 and la[0, 10] == 2  # a NaN point of the old structure is not carried; one behind the camera is (it is a point)
    plain = out["ring_carry_no_into"]
    assert np.array_equal(plain[4], CASES["ring_carry"][1]["origin_in"]) and np.array_equal(plain[1], la)
    pts, la, er, st, org = out["ring_refine"]
    assert (la == 1).sum() > (out["ring_carry"][1] == 1).sum() + 40 and (la == 2).sum() > 0 and (st[la == 2][:, 0] > 0).any()
    for name in ("ring_into_dead_view", "ring_into_no_fit_view", "ring_stats_null"):
        pts, la, er, st, org = out[name]
        dead = 1 if name != "ring_stats_null" else None  # (without pose_stats the view that had no fit counts)
        if dead is None:
            assert (st[..., 3] & SR.BIT_INTO == 0).all() and (la[1] >= 1).any()
            continue
        assert (st[1, :, 3] == SR.BIT_INTO).all() and (la[1] < 1).all() and (pts[1] == 0).all() and (la[1] == 0).sum() > 50 and (la[1] == -1).any()
        assert (st[0, :, 3] & SR.BIT_INTO == 0).all() and (la[0] >= 1).any()
        want = np.eye(3, 4, dtype=np.float32) if "origin_in" not in CASES[name][1] else CASES[name][1]["origin_in"][1]
        assert np.array_equal(org[1], want)  # a copy of origin_in
    assert (out["ring_stats_null"][3][..., 3] & 7 == 7).any()  # min_views = F: a slot with fewer observations falls back every round
    assert (out["size_1_1_1"][1] == -1).all() and (out["size_1_1_1"][3][..., 3] == SR.BIT_NO_START).all()  # one view: nothing to triangulate
    assert (out["size_9_256_2"][1] == 1).all() and (out["size_9_256_2"][3][..., 1] == 256).all()
    assert (out["size_65_256_1"][1] == 1).sum() > 50 and (out["size_300_8_2"][1] == 1).sum() > 300 and (out["size_64_3_2"][1] == 1).sum() > 20
    assert (out["standing"][1] == 0).all() and (out["standing"][3][..., 3] & SR.BIT_NO_PARALLAX != 0).all()  # a standing camera: every label 0
    assert (out["ring_logits"][1] >= 1).sum() > 100


def test_stand_alone_program_under_sanitizers(tmp_path):
    """tests/host/structure_host.cpp as a program with its own main, built with -fsanitize=address,undefined: it runs the same function
    over spoiled inputs in every mode, with 1 to 256 views and 1 to 300 slots, and must exit clean."""
    exe = str(tmp_path / "structure_host_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DSTRUCTURE_HOST_MAIN", "-o", exe, os.path.join(ROOT, "tests", "host", "structure_host.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert run.returncode == 0, run.stderr[-2000:]
    assert "slots accepted" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


# ---- what the rules are worth: planted camera paths through the g++ builds ---------------------------------------------------------------
KINDS = ("sideways", "forward", "few")
CAM = (1000.0, 1000.0, 960.0, 540.0)
T, KEY, MIN_VIEWS, MIN_PARALLAX, TOL = 12, 8, 3, 1.0, 2.0
# measured below, worst of the 60 scenes (the docstring of test_planted_paths has them).  The distance is gated at four times the largest
# value seen; a path ratio at 1 + four times its largest excess over 1 (the factor covers other seeds)
REL_DISTANCE, PATH_POSITION, PATH_ROTATION = 5.9e-8, 1.0043, 1.0273


def orthogonal(Rm):
    U, _, Vt = np.linalg.svd(Rm)
    return U @ Vt


def reference_points(Rs, ts, q, obs, steps=25):
    """The float64 reference: per point the linear midpoint of its rays, then plain Gauss-Newton on the reprojection error over ALL
    its observations, run to convergence (the step is below 1e-12 long before).  Rs [F,3,3], ts [F,3], q [F,n,2] pixels, obs bool
    [F,n] -> X float64 [n,3]."""
    F, n = obs.shape
    y = np.stack([(q[..., 0] - CAM[2]) / CAM[0], (q[..., 1] - CAM[3]) / CAM[1], np.ones((F, n))], axis=-1)
    d = np.einsum("fji,fnj->fni", Rs, y)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    P = (np.eye(3) - d[..., :, None] * d[..., None, :]) * obs[..., None, None]
    c = -np.einsum("fji,fj->fi", Rs, ts)
    X = np.linalg.solve(P.sum(axis=0) + 1e-300 * np.eye(3), np.einsum("fnij,fj->ni", P, c)[..., None])[..., 0]
    for _ in range(steps):
        Xc = np.einsum("fij,nj->fni", Rs, X) + ts[:, None]
        with np.errstate(all="ignore"):
            iz = 1.0 / Xc[..., 2]
        u, v = Xc[..., 0] * iz, Xc[..., 1] * iz
        r = np.stack([CAM[0] * u + CAM[2] - q[..., 0], CAM[1] * v + CAM[3] - q[..., 1]], axis=-1) * obs[..., None]
        g = np.stack([np.stack([CAM[0] * iz, 0 * iz, -CAM[0] * iz * u], axis=-1), np.stack([0 * iz, CAM[1] * iz, -CAM[1] * iz * v], axis=-1)], axis=-2)
        J = np.einsum("fnkj,fji->fnki", g, Rs) * obs[..., None, None]
        H, b = np.einsum("fnki,fnkj->nij", J, J) + 1e-300 * np.eye(3), np.einsum("fnki,fnk->ni", J, r)
        lost = ~(np.isfinite(H).all(axis=(1, 2)) & np.isfinite(b).all(axis=1))  # (a mover's point may run away: it stays where it is)
        with np.errstate(all="ignore"):
            lost |= ~(np.abs(np.linalg.det(np.where(lost[:, None, None], np.eye(3), H))) > 0.0)
        H[lost], b[lost] = np.eye(3), 0.0
        X = X - np.linalg.solve(H, b[..., None])[..., 0]
    return X


def reference_accepts(Rs, ts, q, obs, X):
    """The float64 reference's verdict under its converged point: at least MIN_VIEWS views within TOL, and the arm of the first of them
    at MIN_PARALLAX degrees or more against another's (the angle itself, by arctan2)."""
    Xc = np.einsum("fij,nj->fni", Rs, X) + ts[:, None]
    with np.errstate(all="ignore"):
        e = (CAM[0] * Xc[..., 0] / Xc[..., 2] + CAM[2] - q[..., 0]) ** 2 + (CAM[1] * Xc[..., 1] / Xc[..., 2] + CAM[3] - q[..., 1]) ** 2
    cnt = obs & (Xc[..., 2] > 0) & (e <= TOL * TOL)
    c = -np.einsum("fji,fj->fi", Rs, ts)
    w = X[None] - c[:, None]
    first = np.argmax(cnt, axis=0)
    wa = w[first, np.arange(X.shape[0])]
    ang = np.degrees(np.arctan2(np.linalg.norm(np.cross(wa[None], w), axis=-1), (wa[None] * w).sum(axis=-1)))
    return (cnt.sum(axis=0) >= MIN_VIEWS) & ((ang >= MIN_PARALLAX) & cnt).any(axis=0)


@pytest.mark.parametrize("kind", KINDS)
def test_planted_paths(host, tmp_path_factory, kind):
    """The 12-frame planted paths of tests/test_resection_host.py (1080p, focal length 1000 px, depths 3..12 m, 0.1 px noise, 25 %
    movers; sideways, forward, 90 points), 20 seeds each.  A planted reconstruct on the pair, then 30 % of the static structure points
    are taken out of `valid`; the poses of the 12 frames come from the chain of the g++ builds as localize() runs it against what is
    left; then the g++ build of structure_math.h as extend() runs it: all 12 frames are views, into = frame 8, the reduced structure
    is carried, min_views 3, min_parallax 1 degree, tol 2.  The restatement equals the build bit for bit here too.  The float64
    reference is reference_points over all observations of a slot under the same poses, with reference_accepts as its verdict.

    Conditions, per scene: every taken-out static point that the float64 reference accepts comes back with label 1 -- the cap on what
    may stay out is the reference's own share, and that was measured first: it accepts every taken-out point on sideways and few and
    leaves out on forward the points near the axis whose parallax stays below one degree, which the rules leave out as well; every
    point that stayed in the structure is carried (label 2); the accepted static points lie within 4 x REL_DISTANCE of the
    reference's in relative distance (the float32 rounding of the output: 2^-24 = 6.0e-8); of the planted movers the rules accept no
    more than the reference plus one point (this is what the majority rule of the header is for: without it 84 of the 2000 movers of
    sideways came back against the reference's 59, up to 8 more in one scene; a mover that drifts along the camera's own flow is
    a static point at another depth to both).  After the extend onto frame 8 a second chain of the g++ builds localises the frames
    9..11 against the new structure and its anchor on frame 8, and compose(pose, origin) gives the planted path: the RMS camera
    position and rotation errors are within 1.10 x the float64 reference pose's of test_resection_host.py for the UNEXTENDED
    structure on the same frames (that test's bar) times 1 + 4 x (PATH_POSITION - 1) and 1 + 4 x (PATH_ROTATION - 1): the new
    structure's poses carry the error of the keyframe's own pose, one link of the chain, on top of their own.

    Measured, worst of 20 seeds (taken-out static points the reference accepts / the rules return; largest relative distance to the
    reference; movers accepted by the rules / by the reference, of all; the extended path against the reference pose of the
    unextended structure, RMS ratio: position, rotation):
      sideways  1800 / 1800   5.8e-08   36 / 59 of 2000   1.0024  1.0273
      forward   1748 / 1748   5.6e-08    0 /  2 of 2000   1.0042  0.9835
      few        400 /  400   5.4e-08    2 /  6 of  440   1.0025  1.0273"""
    from test_epipolar_host import run_host as run_epipolar
    from test_pose_host import run_host as run_pose
    from test_resection_host import centre, reference_pose, rotation_angle, run_host as run_resection
    epi_host = host_library(tmp_path_factory, "epipolar")
    epi_host.host_fit_epipolar.restype = C.c_int
    epi_host.host_fit_epipolar.argtypes = [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 5 + [C.c_void_p] * 12
    pose_host = host_library(tmp_path_factory, "pose")
    pose_host.host_fit_pose.restype = C.c_int
    pose_host.host_fit_pose.argtypes = [C.c_int] * 10 + [C.c_float] * 7 + [C.c_void_p] * 13
    res_host = host_library(tmp_path_factory, "resection")
    res_host.host_fit_resection.restype = C.c_int
    res_host.host_fit_resection.argtypes = [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 8 + [C.c_void_p] * 14
    two_view = dict(K=512, tol=1.0, min_points=16, min_base=16.0, seed=0)

    def localize(coords, visible, pts, valid, row, f0, F):
        src = dict(visible=visible, f0=f0, F=F, anchor=(coords[:, row].copy(), visible[:, row].copy(), row))
        fu, lab, _, _ = run_epipolar(epi_host, coords, mask=valid[None], **two_view, **src)
        seeds, _, _ = run_pose(pose_host, coords, CAM, fu, lab, mask=valid[None], min_points=16, **src)
        return run_resection(res_host, coords, CAM, pts[None], valid[None], seeds, tol=2.0, hypotheses=256, seed=0, min_points=16, **src)
    tot = dict(ref=0, back=0, movers=0, mov_rules=0, mov_ref=0)
    worst_rel = worst_pos = worst_rot = 0.0
    for seed in range(20):
        sc = RR.planted_path(seed, kind, T)
        coords, mover = sc["coords"], sc["mover"]
        N = coords.shape[2]
        visible = np.ones((1, T + 2, N), dtype=np.uint8)
        fu, lab, _, est = run_epipolar(epi_host, coords, visible=visible, f0=1, F=1, lag=1, **two_view)
        _, de, _ = run_pose(pose_host, coords, CAM, fu, lab, visible=visible, f0=1, F=1, lag=1, min_points=16)
        pts, full = RR.structure_from_pose(coords[0, 1], CAM, de[0, 0], lab[0, 0])
        rng = np.random.default_rng(1000 + seed)
        static = np.nonzero((full == 1) & ~mover)[0]
        out = rng.permutation(static)[:int(round(0.3 * static.size))]
        valid = full.copy()
        valid[out] = 0
        po, la, _, st = localize(coords, visible, pts, valid, 1, 2, T)
        assert (st[0, :, 2] >= 0).all()
        kw = dict(pose_stats=st, visible=visible, f0=2, F=T, into=KEY, source_frame=1, structure=pts[None], valid=valid[None], tol=TOL,
                  min_views=MIN_VIEWS, sin2=SR.min_sin2(MIN_PARALLAX))
        got = run_host(host, coords, CAM, po, **kw)
        same(got, SR.fit_structure(coords, CAM, po, **kw))
        npts, nlab, nerr, nst, norg = got
        # the float64 reference under the same poses
        ok, q16 = R.quant(coords[0, 2:], 1.0)
        assert ok.all()
        q = q16 / 16.0
        Rs = np.stack([orthogonal(po[0, j, :, :3].astype(np.float64)) for j in range(T)])
        ts = po[0, :, :, 3].astype(np.float64)
        obs = np.ones((T, N), dtype=bool)
        Xr = reference_points(Rs, ts, q, obs)
        acc = reference_accepts(Rs, ts, q, obs, Xr)
        taken = np.zeros(N, dtype=bool)
        taken[out] = True
        ref_n, back_n = int((taken & acc).sum()), int((taken & acc & (nlab[0] == 1)).sum())
        assert back_n == ref_n, (seed, ref_n, back_n)  # the cap is the reference's own share: what it accepts comes back
        assert (nlab[0][valid == 1] == 2).all()  # what stayed in the structure is carried
        both = acc & (nlab[0] == 1) & ~mover  # (a mover that both keep is kept on different views: no one point to compare)
        Xk = Xr @ Rs[KEY].T + ts[KEY]
        rel = np.linalg.norm(npts[0][both].astype(np.float64) - Xk[both], axis=1) / np.linalg.norm(Xk[both], axis=1)
        assert rel.max() <= 4 * REL_DISTANCE, (seed, rel.max())
        worst_rel = max(worst_rel, float(rel.max()))
        mr, mf = int((mover & (nlab[0] == 1)).sum()), int((mover & acc).sum())
        assert mr <= mf + 1, (seed, mr, mf)
        for k_, v_ in (("ref", ref_n), ("back", back_n), ("movers", int(mover.sum())), ("mov_rules", mr), ("mov_ref", mf)):
            tot[k_] += v_
        # the second chain: frames 9..11 against the extended structure, re-anchored on frame 8
        nvalid = (nlab[0] >= 1).astype(np.int8)
        rows = list(range(2 + KEY + 1, T + 2))
        po2, _, _, st2 = localize(coords, visible, npts[0], nvalid, 2 + KEY, rows[0], len(rows))
        assert (st2[0, :, 2] >= 0).all() and (st2[0, :, 3] == 0).all()
        Ro, to = norg[0, :, :3].astype(np.float64), norg[0, :, 3].astype(np.float64)
        pos, pos_f, rot, rot_f = [], [], [], []
        for i, row in enumerate(rows):
            j = row - 2
            Rt, tt = sc["truth"][j, :, :3], sc["truth"][j, :, 3]
            Rm, tm = po2[0, i, :, :3].astype(np.float64), po2[0, i, :, 3].astype(np.float64)
            Rw, tw = Rm @ Ro, Rm @ to + tm  # ops.compose_pose
            kept = la[0, j] == 1
            Rf, tf = reference_pose(Rt.copy(), tt.copy(), pts.astype(np.float64)[kept], q[j][kept])
            pos.append(np.linalg.norm(centre(Rw, tw) - centre(Rt, tt))), pos_f.append(np.linalg.norm(centre(Rf, tf) - centre(Rt, tt)))
            rot.append(rotation_angle(Rw, Rt)), rot_f.append(rotation_angle(Rf, Rt))

        def rms(a):
            return float(np.sqrt((np.asarray(a) ** 2).mean()))
        assert rms(pos) <= 1.10 * (1 + 4 * (PATH_POSITION - 1)) * rms(pos_f) and rms(rot) <= 1.10 * (1 + 4 * (PATH_ROTATION - 1)) * rms(rot_f), \
            (seed, rms(pos), rms(pos_f), rms(rot), rms(rot_f))
        worst_pos, worst_rot = max(worst_pos, rms(pos) / rms(pos_f)), max(worst_rot, rms(rot) / rms(rot_f))
    print(kind, "taken-out static points the reference accepts / the rules return:", tot["ref"], "/", tot["back"], "; largest relative distance:",
          worst_rel, "; movers accepted by the rules / the reference, of all:", tot["mov_rules"], "/", tot["mov_ref"], "of", tot["movers"],
          "; extended path / reference pose of the unextended structure, RMS ratio: position", worst_pos, "rotation", worst_rot)
