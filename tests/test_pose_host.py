"""The arithmetic of the pose kernel (csrc/pose.hip) pinned WITHOUT a GPU.

co-tracker_amd/csrc/pose_math.h holds the rules of ctk_fit_pose -- the rays, E = K^T F K, the closed-form decomposition with its
reciprocal root of products and differences, the polar steps, the least-squares depths, the cheirality vote, the two fixed-point
Gauss-Newton rounds through ctk_plane_solve -- in host/device inline functions.  This test compiles that header with g++
(-ffp-contract=off, the flag the device translation unit is built with) behind plain loops (tests/host/pose_host.cpp) and compares it
with the numpy restatement of tests/pose_reference.py: every bit of all three outputs.  The last test measures what the rules are worth
on planted scenes through the g++ builds of both headers; the kernel is held to the same restatement by tests/test_gpu_pose.py."""
import ctypes as C
import math

import numpy as np
import pytest

import epipolar_reference as ER
import motion_reference as R
import objects_reference as O
import pose_reference as PZ
from ctk_support import host_library

NAMES = ("pose", "depth", "stats")
NAN_BITS = 0x7FC00000


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = host_library(tmp_path_factory, "pose")
    lib.host_pose_rsqrt.restype = C.c_double
    lib.host_pose_rsqrt.argtypes = [C.c_double]
    lib.host_pose_polar.restype = C.c_double
    lib.host_pose_polar.argtypes = [C.c_void_p]
    lib.host_pose_decompose.restype = C.c_int
    lib.host_pose_decompose.argtypes = [C.c_void_p] * 5
    lib.host_fit_pose.restype = C.c_int
    lib.host_fit_pose.argtypes = [C.c_int] * 10 + [C.c_float] * 7 + [C.c_void_p] * 13
    return lib


@pytest.fixture(scope="module")
def epi_host(tmp_path_factory):
    lib = host_library(tmp_path_factory, "epipolar")
    lib.host_fit_epipolar.restype = C.c_int
    lib.host_fit_epipolar.argtypes = [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 5 + [C.c_void_p] * 12
    return lib


def run_host(host, coords, cam, fundamental, label, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1,
             to=None, lag=None, anchor=None, mask=None, min_points=8, scale=(1.0, 1.0)):
    coords = np.ascontiguousarray(coords, dtype=np.float32)
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out

    def ptr(a, dt):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=dt)
        return a, a.ctypes.data
    keep = [ptr(visible, np.uint8), ptr(vis, np.float32), ptr(conf, np.float32), ptr(first_row, np.int32),
            ptr(None if anchor is None else anchor[0], np.float32), ptr(None if anchor is None else anchor[1], np.uint8), ptr(mask, np.int8),
            ptr(fundamental, np.float32), ptr(label, np.int8)]
    before = [None if k[0] is None else k[0].copy() for k in keep]
    pose = np.full((G, F, 3, 4), np.nan, dtype=np.float32)
    depth = np.full((G, F, N_out, 2), 77.0, dtype=np.float32)
    stats = np.full((G, F, 4), -99, dtype=np.int32)
    rc = host.host_fit_pose(G, N, N_out, R_, f0, F, -1 if to is None else to, 0 if lag is None else lag, 0 if anchor is None else anchor[2],
                            min_points, *cam, scale[0], scale[1], thresh, coords.ctypes.data, *(k[1] for k in keep), pose.ctypes.data,
                            depth.ctypes.data, stats.ctypes.data)
    assert rc == 0
    for k, b in zip(keep, before):  # the inputs are only read
        assert b is None or np.array_equal(k[0].view(np.uint8), b.view(np.uint8))
    return pose, depth, stats


def same(got, want):
    for g_, w_, name in zip(got, want, NAMES):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        eq = (g_.view(np.int32) if g_.dtype == np.float32 else g_) == (w_.view(np.int32) if w_.dtype == np.float32 else w_)
        assert eq.all(), (name, np.argwhere(~eq)[:5].tolist(), g_[~eq][:5], w_[~eq][:5])


def both(host, coords, cam, fundamental, label, **kw):
    got, want = run_host(host, coords, cam, fundamental, label, **kw), PZ.fit_pose(coords, cam, fundamental, label, **kw)
    same(got, want)
    return want


def stated_forms(pose, depth, stats):
    """Nothing but the stated forms: a fitted row has a finite pose and depths that are finite, +inf or the quiet NaN; a no-fit row is
    (I | 0) with NaN depths and stats (M, 0, -1, 0)."""
    bits = depth.view(np.uint32)
    assert (np.isfinite(depth) | (depth == np.inf) | (bits == NAN_BITS)).all()
    assert (np.isinf(depth[..., 0]) == np.isinf(depth[..., 1])).all() and (np.isnan(depth[..., 0]) == np.isnan(depth[..., 1])).all()
    eye = np.eye(3, 4, dtype=np.float32)
    for g in range(pose.shape[0]):
        for f in range(pose.shape[1]):
            if stats[g, f, 2] < 0:
                assert np.array_equal(pose[g, f], eye) and stats[g, f, 1] == 0 and stats[g, f, 3] == 0 and np.isnan(depth[g, f]).all()
            else:
                assert np.isfinite(pose[g, f]).all() and 0 <= stats[g, f, 2] <= 3 and 0 <= stats[g, f, 1] <= stats[g, f, 0]
                assert 0 <= stats[g, f, 3] <= 7 and abs(float(np.linalg.norm(pose[g, f, :, 3].astype(np.float64))) - 1.0) < 1e-6


def test_rsqrt_and_polar_on_edge_values(host):
    values = [1.0, 2.0, 0.5, 4.0, 0.25, 3.0, 1.0 / 3.0, 1.9999999999999998, 0.5000000000000001, 5e-324, 2.2250738585072014e-308,
              1.7976931348623157e308, 1e-300, 1e300, 7.0, 1e-9, 123456.789]
    rng = np.random.default_rng(0)
    values += list(np.exp(rng.uniform(-700, 700, 200)))
    worst = 0.0
    for a in values:
        got, want = host.host_pose_rsqrt(a), PZ.rsqrt(a)
        assert np.float64(got).view(np.int64) == np.float64(want).view(np.int64), a
        true = 1.0 / np.sqrt(np.longdouble(a))
        worst = max(worst, abs(float((np.longdouble(got) - true) / true)))
    assert worst <= 4e-16, worst
    for a in (1.0, 4.0, 0.25, 2.0 ** -1074, 2.0 ** 1022):  # even powers of two come out exactly
        assert host.host_pose_rsqrt(a) == 2.0 ** (-(math.frexp(a)[1] - 1) // 2)
    mats = [np.eye(3), np.diag([1.0, -1.0, 1.0]), np.zeros((3, 3)), np.full((3, 3), np.nan), np.full((3, 3), 1e200), np.ones((3, 3)),
            ER.rotation(0.3, -0.2, 1.0), ER.rotation(0.3, -0.2, 1.0) * 1.2, ER.rotation(3.0, 0.1, 0.0) + 0.05, np.diag([1.7, 0.1, 1.0])]
    mats += [ER.rotation(*rng.uniform(-3, 3, 3)) + rng.normal(0, 0.1, (3, 3)) for _ in range(20)]
    for m in mats:
        buf = np.ascontiguousarray(m, dtype=np.float64).reshape(9).copy()
        det = host.host_pose_polar(buf.ctypes.data)
        want, wdet = PZ.polar([float(v) for v in np.asarray(m, dtype=np.float64).reshape(9)])
        assert np.array_equal(buf.view(np.int64), np.array(want).view(np.int64))
        assert np.float64(det).view(np.int64) == np.float64(wdet).view(np.int64)
    good, gdet = PZ.polar([float(v) for v in (ER.rotation(0.3, -0.2, 1.0) * 1.01).reshape(9)])  # four steps: 1e-2 -> 1.5e-4 -> 3e-8 -> 1e-15
    assert abs(gdet - 1.0) < 1e-12 and np.abs(np.array(good).reshape(3, 3) - ER.rotation(0.3, -0.2, 1.0)).max() < 1e-12


def test_decomposition_against_the_restatement(host):
    """E and the four candidates, bit for bit: planted matrices, matrices of noise (not essential at all), rank-one and zero ones."""
    rng = np.random.default_rng(1)
    cam = (900.0, 950.0, 640.5, 360.25)
    mats = [ER.planted(s, k)["F_true"].astype(np.float32) for s in range(3) for k in ("sideways", "forward")]
    mats += [rng.normal(0, 1, (3, 3)).astype(np.float32) for _ in range(20)]
    mats += [np.outer([1, 2, 3], [3, 2, 1]).astype(np.float32), np.zeros((3, 3), dtype=np.float32), np.eye(3, dtype=np.float32),
             np.full((3, 3), np.inf, dtype=np.float32), np.array([[0, 0, 0], [0, 0, 0], [0, 0, np.nan]], dtype=np.float32),
             np.array([[0, 0, 0], [0, 0, 0], [0, 0, 1e-38]], dtype=np.float32), np.full((3, 3), 3e38, dtype=np.float32)]
    seen = set()
    camf = np.array(cam, dtype=np.float32)
    for m in mats:
        m = np.ascontiguousarray(m)
        E, cand, ok = np.full(9, 7.0), np.full(48, 7.0), np.full(4, 7, dtype=np.int32)
        rc = host.host_pose_decompose(m.ctypes.data, camf.ctypes.data, E.ctypes.data, cand.ctypes.data, ok.ctypes.data)
        wE = PZ.essential(m, PZ.camera(cam))
        seen.add(rc)
        assert (rc == 0) == (wE is None)
        if wE is None:
            continue
        assert np.array_equal(E.view(np.int64), np.array(wE).view(np.int64)) and np.abs(E).max() == 1.0
        wc = PZ.decompose(wE)
        assert (rc == 1) == (wc is None)
        if wc is not None:
            for k, (Rm, t, valid) in enumerate(wc):
                assert np.array_equal(cand[k * 12:k * 12 + 12].view(np.int64), np.array(list(Rm) + list(t)).view(np.int64)), k
                assert bool(ok[k]) == valid
    assert {0, 2} <= seen


def epipolar_inputs(coords, **kw):
    fu, lab, _, _ = ER.fit_epipolar(coords, **kw)
    return fu, lab


SOURCE = ("visible", "vis", "conf", "thresh", "first_row", "N_out", "f0", "F", "to", "lag", "anchor", "scale")


def chain(host, coords, cam, fit, mask=None, pose_mask="same", min_points=8, **source):
    """fit_epipolar (numpy) and then the pose on its matrix and labels, through both builds."""
    fu, lab = epipolar_inputs(coords, mask=mask, **fit, **source)
    return both(host, coords, cam, fu, lab, mask=mask if isinstance(pose_mask, str) else pose_mask, min_points=min_points, **source), lab


def test_scenes_three_forms(host):
    """The three source forms, a ring, first rows, positions that are not valid, masks, and the logits form; F and the labels are
    epipolar_reference's."""
    G, T, N, N_out = 2, 8, 123, 120
    coords, visible, mover = ER.history(3, G, T, N)
    cam = (0.9 * 480, 0.9 * 480, 240.0, 135.0)
    first = O.spoil(coords, N_out)
    mask = (~mover).astype(np.int8)
    mask[0, :6] = (-1, 20, 0, -128, 127, 0)
    fit = dict(K=128, seed=11, min_base=8.0, tol=1.0, min_points=12)
    src = dict(visible=visible, first_row=first, N_out=N_out)
    (po, de, st), lab = chain(host, coords, cam, fit, f0=0, F=5, lag=3, **src)
    stated_forms(po, de, st)
    assert (st[:, :3, 2] == -1).all() and (st[:, :3, 0] == 0).all() and np.isnan(de[:, :3]).all()  # no source frame yet
    assert (st[:, 3:, 2] >= 0).all() and (st[:, 3:, 0] > 40).all() and (st[:, 3:, 1] >= 0.9 * st[:, 3:, 0]).all()
    assert (np.isnan(de[:, 3:, :, 0]) == (lab[:, 3:] < 0)).all()  # every correspondence has depths, a label of 0 included
    assert (lab[:, 3:] == 0).any() and np.isnan(de[0, :, 4]).all()
    chain(host, coords, cam, fit, mask=mask, f0=3, F=3, lag=3, **src)
    chain(host, coords, cam, fit, mask=None, pose_mask=mask, f0=3, F=3, lag=3, **src)  # a mask for the pose alone
    chain(host, coords, cam, fit, f0=1, F=7, to=2, **src)
    anchor = (coords[:, 1].copy(), visible[:, 1].copy(), 1)
    first[1, 7] = 2  # released and reassigned after the anchor was taken: drops out
    want, _ = chain(host, coords, cam, fit, mask=mask, f0=3, F=5, anchor=anchor, **src)
    assert np.isnan(want[1][1, :, 7]).all()
    ring, _ = chain(host, R.fold(coords, 6, 8), cam, fit, mask=mask, f0=3, F=5, anchor=anchor, **{**src, "visible": R.fold(visible, 6, 8)})
    same(ring, want)
    rng = np.random.default_rng(5)
    vis_l = np.where(visible != 0, 4.0, -4.0).astype(np.float32) + rng.uniform(-1, 1, visible.shape).astype(np.float32)
    src.pop("visible")
    po, de, st = chain(host, coords, (1.37 * cam[0], 0.81 * cam[1], 1.37 * cam[2], 0.81 * cam[3]), fit, vis=vis_l,
                       conf=np.full(visible.shape, 5.0, dtype=np.float32), thresh=0.6, f0=2, F=3, lag=2, scale=(1.37, 0.81), **src)[0]
    assert (st[..., 2] >= 0).all()


@pytest.mark.parametrize("M", (8, 9, 64))
def test_a_fit_list_of_exactly_min_points_and_of_one_less(host, M):
    coords, visible, _ = ER.history(M, 1, 2, M + 3, movers=0.0)
    cam = (0.9 * 480, 0.9 * 480, 240.0, 135.0)
    visible[:] = 1
    visible[0, 1, M:] = 0  # three slots are not on both frames
    src = dict(visible=visible, f0=1, lag=1)
    fu, lab = epipolar_inputs(coords, K=64, min_base=2.0, min_points=8, seed=M, **src)
    assert (lab[0, 0, :M] == 1).sum() >= 8
    lab[0, 0, :M] = 1  # the labels are an input: M entries exactly
    po, de, st = both(host, coords, cam, fu, lab, min_points=M, **src)
    stated_forms(po, de, st)
    assert st[0, 0, 0] == M and st[0, 0, 2] >= 0 and np.isnan(de[0, 0, M:]).all() and not np.isnan(de[0, 0, :M]).any()
    lab[0, 0, 2] = 0  # one less: no fit, and the correspondences are still there
    po, de, st = both(host, coords, cam, fu, lab, min_points=M, **src)
    assert st[0, 0].tolist() == [M - 1, 0, -1, 0] and (de.view(np.uint32) == NAN_BITS).all() and np.array_equal(po[0, 0], np.eye(3, 4))
    lab[0, 0, 2] = 1
    mask = np.ones((1, M + 3), dtype=np.int8)
    mask[0, 5] = 0  # the mask takes one away as well
    po, de, st = both(host, coords, cam, fu, lab, mask=mask, min_points=M, **src)
    assert st[0, 0].tolist() == [M - 1, 0, -1, 0]
    if M > 8:
        po, de, st = both(host, coords, cam, fu, lab, mask=mask, min_points=M - 1, **src)
        assert st[0, 0, 0] == M - 1 and st[0, 0, 2] >= 0 and not np.isnan(de[0, 0, 5]).any()  # off the fit list, with depths


def test_matrices_that_are_no_fit(host):
    coords, visible, _ = ER.history(2, 1, 3, 40, movers=0.0)
    cam = (0.9 * 480, 0.9 * 480, 240.0, 135.0)
    visible[:] = 1
    src = dict(visible=visible, f0=1, F=2, lag=1)
    fu, lab = epipolar_inputs(coords, K=64, min_base=2.0, min_points=8, seed=1, **src)
    assert (fu != 0).any(axis=(2, 3)).all()
    fu[0, 0] = 0.0  # epipolar's no-fit row next to a fitted one
    po, de, st = both(host, coords, cam, fu, lab, **src)
    stated_forms(po, de, st)
    assert st[0, 0, 2] == -1 and st[0, 0, 0] > 8 and st[0, 1, 2] >= 0
    for bad in (np.nan, np.inf, -np.inf):
        fu[0, 0] = 1.0
        fu[0, 0, 1, 2] = bad
        po, de, st = both(host, coords, cam, fu, lab, **src)
        assert st[0, 0].tolist()[1:] == [0, -1, 0] and st[0, 1, 2] >= 0
    fu[0, 0] = np.eye(3)  # not a fundamental matrix at all: whatever comes out, both make the same
    stated_forms(*both(host, coords, cam, fu, lab, **src))
    fu[0, 0] = 0.0
    fu[0, 0, 2, 2] = 1.0  # E E^T has one entry: TT has no positive diagonal beyond rounding
    stated_forms(*both(host, coords, cam, fu, lab, **src))


def test_degenerate_scenes(host):
    """A static camera (P == Q) and all points on one line: whatever the decomposition makes of them, the g++ build and the restatement
    make the same, and nothing but the stated forms appears."""
    coords, visible, _ = ER.history(2, 1, 2, 80, movers=0.0)
    cam = (0.9 * 480, 0.9 * 480, 240.0, 135.0)
    visible[:] = 1
    coords[0, 1] = coords[0, 0]
    line = coords.copy()
    line[0, :, :, 1] = line[0, :, :, 0] * 0.5 + 3.0
    line[0, 1, :, 0] += 2.0
    src = dict(visible=visible, f0=1, lag=1)
    for c in (coords, line):
        for K in (1, 64):
            fu, lab = epipolar_inputs(c, K=K, min_base=2.0, min_points=8, seed=5, **src)
            for labels in (lab, np.ones_like(lab)):
                stated_forms(*both(host, c, cam, fu, labels, **src))
        for fu in (np.eye(3, dtype=np.float32)[None, None], np.array([[[[0, -1, 3], [1, 0, -2], [-3, 2, 0]]]], dtype=np.float32)):
            stated_forms(*both(host, c, cam, fu, np.ones((1, 1, 80), dtype=np.int8), **src))


def test_an_entry_that_the_cap_leaves_out(host):
    """A camera that moves straight ahead, K made of powers of two so that E = [t]x comes out of F exactly, t = (0, 0, 1), R = I; one
    entry sits on the principal point on both frames: its ray goes through the epipole, e = t x (R x) = 0 and g = 0 exactly.  It is left
    out of round 1 (stats[3] bit 2)."""
    f, cx, cy = 1024.0, 960.0, 540.0
    rng = np.random.default_rng(3)
    N = 60
    P = np.stack([rng.uniform(100, 1820, N), rng.uniform(60, 1020, N)], axis=1)
    Z = rng.uniform(3.0, 12.0, N)
    Q = np.array([cx, cy]) + (P - np.array([cx, cy])) * (Z / (Z - 0.3))[:, None]
    P[0] = Q[0] = (cx, cy)
    coords = np.stack([P, Q])[None].astype(np.float32)
    Ki = np.array([[1 / f, 0, -cx / f], [0, 1 / f, -cy / f], [0, 0, 1]])
    fu = (Ki.T @ np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 0]]) @ Ki).astype(np.float32)[None, None]
    E = PZ.essential(fu, PZ.camera((f, f, cx, cy)))
    assert [abs(v) for v in E] == [0, 1, 0, 1, 0, 0, 0, 0, 0]
    lab = np.ones((1, 1, N), dtype=np.int8)
    po, de, st = both(host, coords, (f, f, cx, cy), fu, lab, visible=np.ones((1, 2, N), dtype=np.uint8), f0=1, lag=1)
    stated_forms(po, de, st)
    assert st[0, 0, 0] == N and st[0, 0, 2] >= 0 and st[0, 0, 3] & 4 and st[0, 0, 1] >= N - 2
    assert np.abs(po[0, 0, :, :3] - np.eye(3)).max() < 1e-3 and po[0, 0, 2, 3] < -0.999  # the points come closer: X_f = X_s - d z
    x = PZ.rays(PZ.camera((f, f, cx, cy)), R.quant(coords[0, 0], 1.0)[1][:1])
    v, g, take = PZ.entries([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], [0.0, 0.0, 1.0], x, x)
    assert g[0] == 0.0 and not take[0]
    # wide rays (a focal length of 20 px on a 1080p picture) make v_i v_i exceed 16 g on many entries: the cap itself
    sc = ER.planted(0, "sideways")
    coords = np.stack([sc["P"], sc["Q"]])[None].astype(np.float32)
    visible = np.ones((1, 2, coords.shape[2]), dtype=np.uint8)
    fu, lab = epipolar_inputs(coords, visible=visible, f0=1, lag=1, K=64)
    po, de, st = both(host, coords, (20.0, 20.0, 960.0, 540.0), fu, lab, visible=visible, f0=1, lag=1)
    stated_forms(po, de, st)
    assert st[0, 0, 2] >= 0 and st[0, 0, 3] & 4


# ---- what the rules are worth: planted scenes through the g++ builds --------------------------------------------------------------------
KINDS = ("sideways", "forward", "few")
CAM = (1000.0, 1000.0, 960.0, 540.0)
# the largest distance, over 20 seeds, of the rules' result from the float64 reference below: rotation and translation direction in
# degrees, the depths of the static inliers relative; measured through the g++ builds
MEASURED_ROTATION = {"sideways": 4.83e-6, "forward": 1.77e-6, "few": 2.69e-5}
MEASURED_DIRECTION = {"sideways": 7.58e-5, "forward": 5.65e-6, "few": 3.07e-4}
MEASURED_DEPTH = {"sideways": 6.24e-6, "forward": 9.98e-6, "few": 3.30e-5}


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def angle_between(a, b):
    """Degrees, without an arccos near 1."""
    return float(np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b)), np.dot(a, b))))


def rotation_angle(Ra, Rb):
    """Degrees between two rotations, from the chord: exact to rounding for small angles."""
    return float(np.degrees(2.0 * np.arcsin(min(1.0, np.linalg.norm(Ra - Rb) / (2.0 * np.sqrt(2.0))))))


def triangulate(Rm, t, x, y):
    """float64 least squares of z_s R x + t = z_f y per correspondence; x, y [n,3]."""
    a = x @ Rm.T
    out = np.zeros((len(x), 2))
    for i in range(len(x)):
        out[i] = np.linalg.lstsq(np.stack([a[i], -y[i]], axis=1), -t, rcond=None)[0]
    return out


def svd_candidates(E):
    U, _, Vt = np.linalg.svd(E)
    U, Vt = U * np.sign(np.linalg.det(U)), Vt * np.sign(np.linalg.det(Vt))
    W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    return [(U @ W_ @ Vt, s * U[:, 2]) for W_ in (W, W.T) for s in (1.0, -1.0)]


def reference_pose(E, x, y, steps=10):
    """The float64 reference: an SVD decomposition of the same E, the candidate with most points in front, plain Gauss-Newton steps on
    the Sampson error over the same fit list (the same linearisation as the rules: r / sqrt(g) with g held), an exact rotation update."""
    best = None
    for Rm, t in svd_candidates(E):
        z = triangulate(Rm, t, x, y)
        n = int(((z[:, 0] > 0) & (z[:, 1] > 0)).sum())
        if best is None or n > best[0]:
            best = (n, Rm, t)
    _, Rm, t = best
    for _ in range(steps):
        p = x @ Rm.T
        c, e = np.cross(y, t), np.cross(t, p)
        b = c @ Rm
        g = e[:, 0] ** 2 + e[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2
        r = (y * e).sum(axis=1)
        J = np.concatenate([np.cross(p, c), np.cross(p, y)], axis=1) / np.sqrt(g)[:, None]
        A = np.concatenate([J, np.sqrt(len(x)) * np.concatenate([np.zeros(3), t])[None]], axis=0)
        d = np.linalg.lstsq(A, np.concatenate([-r / np.sqrt(g), [0.0]]), rcond=None)[0]
        U, _, Vt = np.linalg.svd((np.eye(3) + skew(d[:3])) @ Rm)
        Rm = U @ Vt
        t = (t + d[3:]) / np.linalg.norm(t + d[3:])
    return Rm, t


def planted_truth(sc):
    """R, the unit t and the static points' depths (in baselines) that the scene was planted with, from its F_true and clean points."""
    Kc = np.array([[CAM[0], 0, CAM[2]], [0, CAM[1], CAM[3]], [0, 0, 1]])
    E = Kc.T @ sc["F_true"] @ Kc
    Ki = np.linalg.inv(Kc)
    static = ~sc["mover"]
    x = np.concatenate([sc["P_clean"][static], np.ones((static.sum(), 1))], axis=1) @ Ki.T
    y = np.concatenate([sc["Q_clean"][static], np.ones((static.sum(), 1))], axis=1) @ Ki.T
    best = None
    for Rm, t in svd_candidates(E):
        z = triangulate(Rm, t, x[:20], y[:20])
        n = int(((z[:, 0] > 0) & (z[:, 1] > 0)).sum())
        if best is None or n > best[0]:
            best = (n, Rm, t)
    assert best[0] == 20 and rotation_angle(best[1], np.eye(3)) < 3.0
    return best[1], best[2], triangulate(best[1], best[2], x, y)


@pytest.mark.parametrize("kind", KINDS)
def test_planted_scenes(host, epi_host, kind):
    """1080p, focal length 1000 px, depths 3..12 m, 0.1 px noise, 25 % movers in three groups, 20 seeds; F and the labels come from
    the g++ build of epipolar_math.h with its defaults (512 hypotheses, tol 1), min_points 16.  On every scene: every static inlier has
    both depths > 0, no entry is left out by the cap, stats[3] == 0.  The rules' rotation, direction and static-inlier depths stay within
    MEASURED_* plus half of it of the float64 reference (reference_pose, then a least-squares triangulation), and their errors against
    the planted truth do not exceed the reference's own by more than that margin.

    Measured, worst of 20 seeds, rules / reference against the truth (rotation deg, direction deg, median depth error):
      sideways  0.012913 / 0.012912   0.60211 / 0.60204   0.61354 % / 0.61353 %
      forward   0.009382 / 0.009382   0.17774 / 0.17774   0.44777 % / 0.44777 %
      few       0.033410 / 0.033431   0.49498 / 0.49474   1.62951 % / 1.63066 %
    The errors against the truth are those of the fundamental matrix (a robust fit over noisy points, some of them movers that happen to
    obey it), not of the rules: the reference inherits them to the fourth digit."""
    from test_epipolar_host import run_host as run_epipolar
    cam = PZ.camera(CAM)
    rot, dirn, dep, truth_rules, truth_ref = [], [], [], [], []
    for seed in range(20):
        sc = ER.planted(seed, kind)
        coords = np.stack([sc["P"], sc["Q"]])[None].astype(np.float32)
        N = coords.shape[2]
        visible = np.ones((1, 2, N), dtype=np.uint8)
        fu, lab, _, est = run_epipolar(epi_host, coords, visible=visible, f0=1, lag=1, K=512, tol=1.0, min_points=16, min_base=16.0, seed=0)
        assert est[0, 0, 2] >= 0
        po, de, st = run_host(host, coords, CAM, fu, lab, visible=visible, f0=1, lag=1, min_points=16)
        fit = lab[0, 0] == 1
        static_in = fit & ~sc["mover"]
        assert st[0, 0, 0] == fit.sum() and st[0, 0, 2] >= 0
        assert st[0, 0, 3] == 0, (seed, st[0, 0])  # no round fell back, and the cap left no entry out
        assert (de[0, 0][static_in] > 0).all(), seed  # every static inlier lies in front of both cameras
        ok, pos = R.quant(coords[0], 1.0)
        assert ok.all()
        x, y = np.stack(PZ.rays(cam, pos[0]), axis=1), np.stack(PZ.rays(cam, pos[1]), axis=1)
        E = np.array(PZ.essential(fu[0, 0], cam)).reshape(3, 3)
        Rr, tr = reference_pose(E, x[fit], y[fit])
        zr = triangulate(Rr, tr, x[static_in], y[static_in])
        Rm, t = po[0, 0, :, :3].astype(np.float64), po[0, 0, :, 3].astype(np.float64)
        rot.append(rotation_angle(Rm, Rr))
        dirn.append(angle_between(t, tr))
        dep.append(float(np.abs(de[0, 0][static_in].astype(np.float64) / zr - 1.0).max()))
        Rt, tt, zt = planted_truth(sc)
        zt = zt[fit[~sc["mover"]]]
        truth_rules.append((rotation_angle(Rm, Rt), angle_between(t, tt), float(np.median(np.abs(de[0, 0][static_in] / zt - 1.0)))))
        truth_ref.append((rotation_angle(Rr, Rt), angle_between(tr, tt), float(np.median(np.abs(zr / zt - 1.0)))))
    tru, trf = np.array(truth_rules).max(axis=0), np.array(truth_ref).max(axis=0)
    print(kind, "against the reference: rotation", max(rot), "deg, direction", max(dirn), "deg, depth", max(dep), "relative")
    print(kind, "against the truth, rules:", tru.tolist(), "reference:", trf.tolist())
    margins = [1.5 * MEASURED_ROTATION[kind], 1.5 * MEASURED_DIRECTION[kind], 1.5 * MEASURED_DEPTH[kind]]
    assert max(rot) <= margins[0] and max(dirn) <= margins[1] and max(dep) <= margins[2]
    for i in range(3):
        assert (np.array(truth_rules)[:, i] <= np.array(truth_ref)[:, i] + margins[i]).all(), i
