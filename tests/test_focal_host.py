"""The arithmetic of the focal kernels (csrc/focal.hip) pinned WITHOUT a GPU.

co-tracker_amd/csrc/focal_math.h holds the rules of ctk_fit_focal -- the camera of a candidate, which frames take part, the score of an
entry under ctk_fit_pose's final pose, the integer costs and totals, the choice with its contrast rule and the refinement -- in
host/device inline functions.  This test compiles that header with g++ (-ffp-contract=off, the flag the device translation unit is
built with) behind plain loops (tests/host/focal_host.cpp) and compares it with the numpy restatement of tests/focal_reference.py:
every bit of the four arrays the entry point writes (the fifth value ops.fit_focal returns, the candidates, is an input here and is
checked unchanged).  The last test measures what the rules are worth on planted scenes through the g++ builds of the epipolar and the
focal headers; the kernels are held to the same restatement by tests/test_gpu_focal.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import epipolar_reference as ER
import focal_reference as FR
import motion_reference as R
import objects_reference as O
from ctk_support import host_library

NAMES = ("focal", "curve", "cost", "stats")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = host_library(tmp_path_factory, "focal")
    lib.host_fit_focal.restype = C.c_int
    lib.host_fit_focal.argtypes = [C.c_int] * 12 + [C.c_float] * 7 + [C.c_void_p] * 16
    return lib


@pytest.fixture(scope="module")
def epi_host(tmp_path_factory):
    lib = host_library(tmp_path_factory, "epipolar")
    lib.host_fit_epipolar.restype = C.c_int
    lib.host_fit_epipolar.argtypes = [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 5 + [C.c_void_p] * 12
    return lib


def run_host(host, coords, fundamental, label, focals, principal, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None,
             f0=0, F=1, to=None, lag=None, anchor=None, mask=None, min_points=16, scale=(1.0, 1.0), tol=1.0, contrast=1.5, min_frames=1,
             curve_in=None):
    coords = np.ascontiguousarray(coords, dtype=np.float32)
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    focals = np.ascontiguousarray(focals, dtype=np.float32)
    K = focals.shape[0]

    def ptr(a, dt):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=dt)
        return a, a.ctypes.data
    keep = [ptr(visible, np.uint8), ptr(vis, np.float32), ptr(conf, np.float32), ptr(first_row, np.int32),
            ptr(None if anchor is None else anchor[0], np.float32), ptr(None if anchor is None else anchor[1], np.uint8), ptr(mask, np.int8),
            ptr(fundamental, np.float32), ptr(label, np.int8), ptr(focals, np.float32), ptr(curve_in, np.int64)]
    before = [None if k[0] is None else k[0].copy() for k in keep]
    focal = np.full(G, np.nan, dtype=np.float32)
    curve = np.full((G, K + 2), -77, dtype=np.int64)
    cost = np.full((G, F, K), -77, dtype=np.int64)
    stats = np.full((G, 4), -99, dtype=np.int32)
    rc = host.host_fit_focal(G, N, N_out, R_, f0, F, -1 if to is None else to, 0 if lag is None else lag, 0 if anchor is None else anchor[2],
                             min_points, K, min_frames, principal[0], principal[1], scale[0], scale[1], thresh, tol, contrast,
                             coords.ctypes.data, *(k[1] for k in keep), focal.ctypes.data, curve.ctypes.data, cost.ctypes.data,
                             stats.ctypes.data)
    assert rc == 0
    for k, b in zip(keep, before):  # the inputs are only read
        assert b is None or np.array_equal(k[0].view(np.uint8), b.view(np.uint8))
    return focal, curve, cost, stats


def same(got, want):
    for g_, w_, name in zip(got, want, NAMES):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        eq = (g_.view(np.int32) if g_.dtype == np.float32 else g_) == (w_.view(np.int32) if w_.dtype == np.float32 else w_)
        assert eq.all(), (name, np.argwhere(~eq)[:5].tolist(), g_[~eq][:5], w_[~eq][:5])


def both(host, coords, fundamental, label, focals, principal, **kw):
    got = run_host(host, coords, fundamental, label, focals, principal, **kw)
    want = FR.fit_focal(coords, fundamental, label, focals, principal, **kw)
    same(got, want)
    return want


def stated_forms(focal, curve, cost, stats, focals, F):
    """Nothing but the stated forms: costs within [0, M 2^32], a fit lies between its neighbours, no fit is 0.0 and -1."""
    K = len(focals)
    assert (cost >= 0).all() and (curve >= 0).all()
    for g in range(len(focal)):
        assert 0 <= stats[g, 3] <= 7
        if stats[g, 1] < 0:
            assert focal[g].view(np.int32) == 0
        else:
            i = stats[g, 1]
            lo, hi = focals[max(i - 1, 0)], focals[min(i + 1, K - 1)]
            assert min(lo, focals[i]) <= focal[g] <= max(hi, focals[i]) and curve[g, i] == curve[g, :K].min()
            assert bool(stats[g, 3] & FR.BIT_END) == (i == 0 or i == K - 1)


def turning_history(seed, G, T, N, **kw):
    """epipolar_reference.history turns by up to 0.003 rad a frame; read at a lag of 3 or more, and with the matrices of the numpy
    restatement, that is enough of a turn for costs that differ from candidate to candidate."""
    return ER.history(seed, G, T, N, **kw)


def epipolar_inputs(coords, **kw):
    fu, lab, _, _ = ER.fit_epipolar(coords, **kw)
    return fu, lab


EPI = dict(K=128, seed=11, min_base=8.0, tol=1.0, min_points=12)
CENTRE = (240.0, 135.0)


def test_scenes_three_forms(host):
    """The three source forms across a ring, first rows, positions that are not valid, masks, and the logits form."""
    G, T, N, N_out = 2, 8, 123, 120
    coords, visible, mover = turning_history(3, G, T, N)
    focals = FR.candidates(480, K=7)
    first = O.spoil(coords, N_out)
    mask = (~mover).astype(np.int8)
    mask[0, :6] = (-1, 20, 0, -128, 127, 0)
    src = dict(visible=visible, first_row=first, N_out=N_out)
    fu, lab = epipolar_inputs(coords, f0=0, F=5, lag=3, **EPI, **src)
    fo, cu, co, st = both(host, coords, fu, lab, focals, CENTRE, f0=0, F=5, lag=3, min_points=12, **src)
    stated_forms(fo, cu, co, st, focals, 5)
    assert (co[:, :3] == 0).all() and (st[:, 0] == 2).all() and (co[:, 3:] > 0).all()  # no source frame yet: the frame adds nothing
    assert (cu[:, 7] == 2).all() and (cu[:, 8] == (lab[:, 3:] == 1).sum(axis=(1, 2))).all()
    fu, lab = epipolar_inputs(coords, mask=mask, f0=3, F=3, lag=3, **EPI, **src)
    both(host, coords, fu, lab, focals, CENTRE, mask=mask, f0=3, F=3, lag=3, min_points=12, **src)
    both(host, coords, fu, lab, focals, CENTRE, f0=3, F=3, lag=3, min_points=12, **src)  # the labels of a masked fit, no mask here
    fu, lab = epipolar_inputs(coords, f0=1, F=7, to=2, **EPI, **src)
    both(host, coords, fu, lab, focals, CENTRE, f0=1, F=7, to=2, min_points=12, **src)
    anchor = (coords[:, 1].copy(), visible[:, 1].copy(), 1)
    first[1, 7] = 2  # released and reassigned after the anchor was taken: drops out
    fu, lab = epipolar_inputs(coords, mask=mask, f0=3, F=5, anchor=anchor, **EPI, **src)
    want = both(host, coords, fu, lab, focals, CENTRE, mask=mask, f0=3, F=5, anchor=anchor, min_points=12, **src)
    ring = both(host, R.fold(coords, 6, 8), fu, lab, focals, CENTRE, mask=mask, f0=3, F=5, anchor=anchor, min_points=12,
                **{**src, "visible": R.fold(visible, 6, 8)})
    same(ring, want)
    rng = np.random.default_rng(5)
    vis_l = np.where(visible != 0, 4.0, -4.0).astype(np.float32) + rng.uniform(-1, 1, visible.shape).astype(np.float32)
    src.pop("visible")
    logit = dict(vis=vis_l, conf=np.full(visible.shape, 5.0, dtype=np.float32), thresh=0.6, f0=3, F=3, lag=3, scale=(1.37, 1.37), **src)
    fu, lab = epipolar_inputs(coords, **EPI, **logit)
    fo, cu, co, st = both(host, coords, fu, lab, FR.candidates(480 * 1.37, K=5), (1.37 * 240.0, 1.37 * 135.0), min_points=12, **logit)
    assert (st[:, 0] == 3).all()


@pytest.mark.parametrize("M", (8, 9, 64))
def test_a_fit_list_of_exactly_min_points_and_of_one_less(host, M):
    coords, visible, _ = turning_history(M, 1, 4, M + 3, movers=0.0)
    visible[:] = 1
    visible[0, 3, M:] = 0  # three slots are not on both frames
    src = dict(visible=visible, f0=3, lag=3)
    fu, lab = epipolar_inputs(coords, K=64, min_base=2.0, min_points=8, seed=M, **src)
    assert (fu != 0).any()
    lab[0, 0, :M] = 1  # the labels are an input: M entries exactly
    focals = FR.candidates(480, K=4)
    fo, cu, co, st = both(host, coords, fu, lab, focals, CENTRE, min_points=M, contrast=1.0, **src)
    assert st[0].tolist()[:3] == [1, int(np.argmin(cu[0, :4])), M] and cu[0, 4:].tolist() == [1, M] and fo[0] > 0
    lab[0, 0, 2] = 0  # one less: the frame does not take part
    fo, cu, co, st = both(host, coords, fu, lab, focals, CENTRE, min_points=M, contrast=1.0, **src)
    assert st[0].tolist() == [0, -1, 0, 0] and (co == 0).all() and (cu == 0).all() and fo[0].view(np.int32) == 0
    lab[0, 0, 2] = 1
    mask = np.ones((1, M + 3), dtype=np.int8)
    mask[0, 5] = 0  # the mask takes one away as well
    fo, cu, co, st = both(host, coords, fu, lab, focals, CENTRE, mask=mask, min_points=M, contrast=1.0, **src)
    assert st[0].tolist() == [0, -1, 0, 0]


def fitted(seed=2, T=6, N=60, F=3, lag=3):
    coords, visible, _ = turning_history(seed, 1, T, N, movers=0.0)
    visible[:] = 1
    src = dict(visible=visible, f0=lag, F=F, lag=lag)
    fu, lab = epipolar_inputs(coords, K=64, min_base=2.0, min_points=8, seed=1, **src)
    assert (fu != 0).any(axis=(2, 3)).all()
    return coords, fu, lab, src


def test_matrices_that_are_no_fit_next_to_fitted_ones(host):
    coords, fu, lab, src = fitted()
    focals = FR.candidates(480, K=6)
    full = both(host, coords, fu, lab, focals, CENTRE, **src)
    assert full[3][0, 0] == 3
    for bad in (0.0, np.nan, np.inf, -np.inf):
        m = fu.copy()
        m[0, 1] = 0.0 if bad == 0.0 else 1.0
        if bad != 0.0:
            m[0, 1, 1, 2] = bad
        fo, cu, co, st = both(host, coords, m, lab, focals, CENTRE, **src)
        assert st[0, 0] == 2 and (co[0, 1] == 0).all() and np.array_equal(co[0, 0], full[2][0, 0]) and np.array_equal(co[0, 2], full[2][0, 2])
    m = fu.copy()
    m[0, 0] = np.eye(3)  # not a fundamental matrix at all: whatever comes out, both make the same
    m[0, 2] = 0.0
    m[0, 2, 2, 2] = 1.0  # E E^T has one entry: the decomposition fails under every candidate, the frame still takes part
    fo, cu, co, st = both(host, coords, m, lab, focals, CENTRE, **src)
    M2 = int((lab[0, 2] == 1).sum())
    assert st[0, 0] == 3 and (co[0, 2] == M2 * FR.ONE).all()
    zeros = np.zeros_like(lab)  # labels all 0: nothing takes part
    fo, cu, co, st = both(host, coords, fu, zeros, focals, CENTRE, **src)
    assert st[0].tolist() == [0, -1, 0, 0] and (co == 0).all()


@pytest.mark.parametrize("K", (1, 2, 3, 64, 256))
def test_candidate_counts(host, K):
    coords, fu, lab, src = fitted(F=2)
    focals = FR.candidates(480, K=K)
    fo, cu, co, st = both(host, coords, fu, lab, focals, CENTRE, contrast=1.0, **src)
    stated_forms(fo, cu, co, st, focals, 2)
    assert st[0, 1] >= 0 and cu.shape == (1, K + 2)
    if K == 1:
        assert fo[0] == focals[0] and st[0, 3] == FR.BIT_END


def test_the_minimum_at_either_end_and_ties(host):
    coords, fu, lab, src = fitted()
    wide = both(host, coords, fu, lab, FR.candidates(480, K=32), CENTRE, contrast=1.0, **src)
    i = int(wide[3][0, 1])
    assert 0 < i < 31 and wide[3][0, 3] == 0
    best = float(wide[0][0])
    above = np.linspace(best * 1.5, best * 3.0, 5).astype(np.float32)
    fo, cu, co, st = both(host, coords, fu, lab, above, CENTRE, contrast=1.0, **src)
    assert st[0, 1] == 0 and st[0, 3] == FR.BIT_END and fo[0] == above[0]
    below = np.linspace(best * 0.3, best * 0.7, 5).astype(np.float32)
    fo, cu, co, st = both(host, coords, fu, lab, below, CENTRE, contrast=1.0, **src)
    assert st[0, 1] == 4 and st[0, 3] == FR.BIT_END and fo[0] == below[4]
    f = FR.candidates(480, K=32)[i]
    tied = np.array([f * 0.5, f, f, f, f * 2.0], dtype=np.float32)  # equal candidates have equal totals: the lowest index wins
    fo, cu, co, st = both(host, coords, fu, lab, tied, CENTRE, contrast=1.0, **src)
    assert cu[0, 1] == cu[0, 2] == cu[0, 3] and st[0, 1] == 1 and fo[0] <= f  # d = 0: the parabola leans towards the lower side
    flat = np.array([f, f, f], dtype=np.float32)
    fo, cu, co, st = both(host, coords, fu, lab, flat, CENTRE, contrast=1.0, **src)
    assert st[0, 1] == 0 and fo[0] == f
    fo, cu, co, st = both(host, coords, fu, lab, flat, CENTRE, contrast=1.5, **src)
    assert st[0].tolist()[1:] == [-1, cu[0, 4], FR.BIT_FLAT] and fo[0].view(np.int32) == 0


@pytest.mark.parametrize("bad", (0.0, -300.0, np.nan, np.inf))
def test_a_candidate_that_does_not_stand(host, bad):
    coords, fu, lab, src = fitted()
    good = FR.candidates(480, K=9)
    want = both(host, coords, fu, lab, good, CENTRE, contrast=1.0, **src)
    i = int(want[3][0, 1])
    for at in (0, i, i + 1, 8):
        focals = good.copy()
        focals[at] = bad
        fo, cu, co, st = both(host, coords, fu, lab, focals, CENTRE, contrast=1.0, **src)
        M = (lab[0] == 1).sum(axis=1)
        assert st[0, 3] & FR.BIT_CANDIDATE and (co[0, :, at] == M * FR.ONE).all() and np.isfinite(fo[0])
        keep = [k for k in range(9) if k != at]
        assert np.array_equal(co[0][:, keep], want[2][0][:, keep])
    none = np.full(3, bad, dtype=np.float32)  # no candidate stands: no frame takes part
    fo, cu, co, st = both(host, coords, fu, lab, none, CENTRE, contrast=1.0, **src)
    assert st[0].tolist() == [0, -1, 0, FR.BIT_CANDIDATE] and (co == 0).all()


def test_two_calls_accumulated_equal_one_call(host):
    coords, visible, _ = turning_history(7, 2, 9, 70)
    focals = FR.candidates(480, K=12)
    src = dict(visible=visible, lag=3)
    fu, lab = epipolar_inputs(coords, f0=3, F=6, **EPI, **src)
    one = both(host, coords, fu, lab, focals, CENTRE, f0=3, F=6, min_points=12, **src)
    a = both(host, coords, fu[:, :2], lab[:, :2], focals, CENTRE, f0=3, F=2, min_points=12, **src)
    b = both(host, coords, fu[:, 2:], lab[:, 2:], focals, CENTRE, f0=5, F=4, min_points=12, curve_in=a[1], **src)
    assert np.array_equal(b[1], one[1]) and np.array_equal(b[0].view(np.int32), one[0].view(np.int32)) and np.array_equal(b[3], one[3])
    assert np.array_equal(np.concatenate([a[2], b[2]], axis=1), one[2])
    # min_frames above what took part, and exactly what took part
    n = int(one[3][0, 0])
    fo, cu, co, st = both(host, coords, fu, lab, focals, CENTRE, f0=3, F=6, min_points=12, min_frames=n + 1, contrast=1.0, **src)
    assert (st[:, 1] == -1).all() and (st[:, 3] == 0).all() and (fo.view(np.int32) == 0).all() and np.array_equal(cu, one[1])
    fo, cu, co, st = both(host, coords, fu, lab, focals, CENTRE, f0=3, F=6, min_points=12, min_frames=n, contrast=1.0, **src)
    assert (st[:, 1] >= 0).all()
    # the frames of an earlier call count towards min_frames
    fo, cu, co, st = both(host, coords, fu[:, 2:], lab[:, 2:], focals, CENTRE, f0=5, F=4, min_points=12, min_frames=n, contrast=1.0,
                          curve_in=a[1], **src)
    assert (st[:, 1] >= 0).all() and (st[:, 0] == n).all()


def test_a_contrast_the_curve_just_meets_and_just_misses(host):
    coords, fu, lab, src = fitted()
    focals = FR.candidates(480, K=16)
    fo, cu, co, st = both(host, coords, fu, lab, focals, CENTRE, contrast=1.0, **src)
    mx, mn = int(cu[0, :16].max()), int(cu[0, :16].min())
    c = np.float32(mx / mn)
    while float(c) * float(mn) > float(mx):  # the largest float32 contrast the curve meets
        c = np.nextafter(c, np.float32(0))
    while float(np.nextafter(c, np.float32(np.inf))) * float(mn) <= float(mx):
        c = np.nextafter(c, np.float32(np.inf))
    assert c > 1.0
    fo, cu, co, st = both(host, coords, fu, lab, focals, CENTRE, contrast=float(c), **src)
    assert st[0, 1] >= 0 and not st[0, 3] & FR.BIT_FLAT and fo[0] > 0
    fo, cu, co, st = both(host, coords, fu, lab, focals, CENTRE, contrast=float(np.nextafter(c, np.float32(np.inf))), **src)
    assert st[0, 1] == -1 and st[0, 3] == FR.BIT_FLAT and fo[0].view(np.int32) == 0


def test_refused_numbers(host):
    coords, fu, lab, src = fitted()
    focals = FR.candidates(480, K=4)

    def rc(**kw):
        a = dict(min_points=16, K=4, min_frames=1, contrast=1.5)
        a.update(kw)
        out = [np.zeros(1, dtype=np.float32), np.zeros(a["K"] + 2 if 0 < a["K"] < 300 else 2, dtype=np.int64),
               np.zeros(3 * max(a["K"], 1), dtype=np.int64), np.zeros(4, dtype=np.int32)]
        vis = np.ascontiguousarray(src["visible"])
        return host.host_fit_focal(1, 60, 60, 6, 3, 3, -1, 3, 0, a["min_points"], a["K"], a["min_frames"], 240.0, 135.0, 1.0, 1.0, 0.0, 1.0,
                                   a["contrast"], coords.ctypes.data, vis.ctypes.data, None, None, None, None, None, None, fu.ctypes.data,
                                   lab.ctypes.data, np.resize(focals, max(a["K"], 1)).astype(np.float32).ctypes.data, None,
                                   *(o.ctypes.data for o in out))
    assert rc() == 0
    for kw in (dict(min_points=7), dict(min_points=8193), dict(K=0), dict(K=257), dict(min_frames=0), dict(contrast=0.99),
               dict(contrast=float("nan"))):
        assert rc(**kw) == -2, kw


# ---- what the rules are worth: planted scenes through the g++ builds --------------------------------------------------------------------
FOCALS = (700.0, 1000.0, 1600.0)
MOTIONS = ("sideways", "forward")
TURNS = {"wide": 0.06, "narrow": 0.02, "none": 0.0}
PAIRS, SEEDS, WIDTH, PRINCIPAL = 4, 20, 1920, (960.0, 540.0)
SCENES_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "profiles", "focal_scenes.json")


def planted_pairs(seed, motion, focal, turn):
    """Four pairs of one camera as a four-frame history at lag 1 over two rows each: group p holds pair p."""
    scs = [FR.planted(seed * PAIRS + p, motion, focal, turn) for p in range(PAIRS)]
    coords = np.stack([np.stack([sc["P"], sc["Q"]]) for sc in scs]).astype(np.float32)
    return scs, coords


def sampson_cost(f, cx, cy, Fm, x_pix, y_pix, T, reference_pose):
    """The float64 reference's cost of one pair under focal length f: SVD decomposition, ten Gauss-Newton steps, the truncated squared
    Sampson distance in pixels summed over the fit list, in units of T."""
    Kc = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])
    E = Kc.T @ Fm @ Kc
    E = E / np.abs(E).max()
    Ki = np.linalg.inv(Kc)
    x, y = x_pix @ Ki.T, y_pix @ Ki.T
    Rm, t = reference_pose(E, x, y)
    p = x @ Rm.T
    c, e = np.cross(y, t), np.cross(t, p)
    b = c @ Rm
    g = e[:, 0] ** 2 + e[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2
    r = (y * e).sum(axis=1)
    return float(np.minimum((r * r / g) * (f * f) / T, 1.0).sum())


def golden(fun, lo, hi, iters=40):
    """A continuous 1-D minimisation by golden section over [lo, hi]."""
    gr = (np.sqrt(5.0) - 1.0) / 2.0
    a, b = lo, hi
    c, d = b - gr * (b - a), a + gr * (b - a)
    fc, fd = fun(c), fun(d)
    for _ in range(iters):
        if fc < fd:
            b, d, fd = d, c, fc
            c = b - gr * (b - a)
            fc = fun(c)
        else:
            a, c, fc = c, d, fd
            d = a + gr * (b - a)
            fd = fun(d)
    return 0.5 * (a + b)


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def reference_pose(E, x, y, steps=10):
    """The float64 reference (as tests/test_pose_host.py::reference_pose, with the triangulation of the vote in closed form): an SVD
    decomposition of E, the candidate with most points in front, plain Gauss-Newton steps on the Sampson error over the same fit list
    (r / sqrt(g) with g held), an exact rotation update."""
    U, _, Vt = np.linalg.svd(E)
    U, Vt = U * np.sign(np.linalg.det(U)), Vt * np.sign(np.linalg.det(Vt))
    W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    best = None
    for Rm, t in [(U @ W_ @ Vt, s * U[:, 2]) for W_ in (W, W.T) for s in (1.0, -1.0)]:
        a = x @ Rm.T
        aa, yy, ay, at, yt = (a * a).sum(1), (y * y).sum(1), (a * y).sum(1), a @ t, y @ t
        den = aa * yy - ay * ay
        n = int((((ay * yt - at * yy) / den > 0) & ((aa * yt - ay * at) / den > 0)).sum())
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


def measure(host, epi_host, motion, focal, turn, seeds=SEEDS, reference=True):
    """One scene kind over `seeds` seeds: four pairs of a 1080p camera, 400 points 3..12 m deep, 0.1 px noise, 25 % movers; F and the
    labels from the g++ build of epipolar_math.h with its defaults (512 hypotheses, tol 1, min_points 16); 64 candidates geometric over
    0.25..4 picture widths, the four pairs accumulated through curve_in -> per seed the contrast (largest total over smallest), the
    rules' focal length and, with `reference`, the float64 reference's."""
    from test_epipolar_host import run_host as run_epipolar
    focals = FR.candidates(WIDTH, K=64)
    out = dict(contrast=[], rules=[], reference=[], index=[])
    for seed in range(seeds):
        _, coords = planted_pairs(seed, motion, focal, TURNS[turn])
        curve, pairs = None, []
        for p in range(PAIRS):
            c = coords[p][None]
            visible = np.ones((1, 2, c.shape[2]), dtype=np.uint8)
            fu, lab, _, est = run_epipolar(epi_host, c, visible=visible, f0=1, lag=1, K=512, tol=1.0, min_points=16, min_base=16.0, seed=0)
            assert est[0, 0, 2] >= 0
            fo, curve, co, st = run_host(host, c, fu, lab, focals, PRINCIPAL, visible=visible, f0=1, lag=1, contrast=1.0, curve_in=curve)
            ok, pos = R.quant(c[0], 1.0)
            fit = lab[0, 0] == 1
            assert ok.all() and st[0, 0] == p + 1 and curve[0, 65] - (0 if p == 0 else entries) == fit.sum()
            entries = int(curve[0, 65])
            pairs.append((fu[0, 0].astype(np.float64),) + tuple(
                np.concatenate([q[fit].astype(np.float64) / 16.0, np.ones((int(fit.sum()), 1))], axis=1) for q in (pos[0], pos[1])))
        out["contrast"].append(float(curve[0, :64].max()) / float(curve[0, :64].min()))
        out["rules"].append(float(fo[0]))
        out["index"].append(int(st[0, 1]))
        out["curve"] = curve
        if reference:
            def fun(f):
                return sum(sampson_cost(f, PRINCIPAL[0], PRINCIPAL[1], Fm, xp, yp, 1.0, reference_pose) for Fm, xp, yp in pairs)
            j = 2 * int(np.argmin([fun(float(f)) for f in focals[::2]]))
            out["reference"].append(golden(fun, float(focals[max(j - 2, 0)]), float(focals[min(j + 2, 63)]), iters=20))
    return out


# the largest relative distance, over 20 seeds, of the rules' focal length from the float64 reference's (reference_pose, sampson_cost,
# golden): measured through the g++ builds; it is the grid's own error (64 candidates, a parabola through three costs)
MEASURED_DISTANCE = {
    "wide-sideways-700": 1.05e-3, "wide-sideways-1000": 1.71e-3, "wide-sideways-1600": 1.66e-3,
    "wide-forward-700": 2.34e-3, "wide-forward-1000": 2.17e-3, "wide-forward-1600": 2.05e-3,
    "narrow-sideways-700": 1.63e-3, "narrow-sideways-1000": 1.79e-3, "narrow-sideways-1600": 1.67e-3,
    "narrow-forward-700": 3.92e-3, "narrow-forward-1000": 2.00e-3, "narrow-forward-1600": 4.70e-3,
}
# contrast over 20 seeds, smallest .. largest: every scene with a turn against every scene without one
MEASURED_CONTRAST_TURN = (1.5028, 91.74)
MEASURED_CONTRAST_NO_TURN = (1.00008, 1.2611)
DEFAULT_CONTRAST = 1.5


@pytest.mark.parametrize("focal", FOCALS)
@pytest.mark.parametrize("motion", MOTIONS)
def test_planted_scenes_without_a_turn_are_refused(host, epi_host, motion, focal):
    """A camera that only translates: F does not depend on the focal length, the curve is flat, and the default contrast refuses every
    one of the 20 seeds.  Measured: contrast 1.00008 .. 1.2611 over the six kinds (the largest on sideways, 700 px)."""
    m = measure(host, epi_host, motion, focal, "none", reference=False)
    print("none", motion, focal, "contrast", min(m["contrast"]), "..", max(m["contrast"]))
    assert max(m["contrast"]) < DEFAULT_CONTRAST
    assert MEASURED_CONTRAST_NO_TURN[0] * (1 - 1e-4) <= min(m["contrast"]) and max(m["contrast"]) <= MEASURED_CONTRAST_NO_TURN[1] * (1 + 1e-4)
    fo, _, _, st = _choice_of(m["curve"], DEFAULT_CONTRAST)
    assert st[1] == -1 and st[3] & FR.BIT_FLAT and fo.view(np.int32) == 0  # (the last seed, through the rule itself)


def _choice_of(curve, contrast):
    focals = FR.candidates(WIDTH, K=64)
    fo, i, bits = FR.choose([int(v) for v in curve[0, :64]], focals, int(curve[0, 64]), 1, contrast)
    return fo, None, None, (int(curve[0, 64]), i, int(curve[0, 65]), bits)


@pytest.mark.parametrize("focal", FOCALS)
@pytest.mark.parametrize("motion", MOTIONS)
@pytest.mark.parametrize("turn", ("wide", "narrow"))
def test_planted_scenes_with_a_turn(host, epi_host, turn, motion, focal):
    """A camera that turns by up to 0.06 (wide) or 0.02 (narrow) rad about every axis between the frames of a pair: the default
    contrast accepts every one of the 20 seeds, the minimum lies inside the range, the rules' focal length stays within 1.5 x
    MEASURED_DISTANCE of the float64 reference's, and its error against the planted focal length exceeds the reference's own by no more
    than that.  Measured over the twelve kinds: contrast 1.5028 (narrow, forward, 700 px: just above the default of 1.5; the next
    smallest kind has 3.20) .. 91.74; the error against the truth is at most 0.38 % (wide, sideways), 2.1 % (wide, forward), 1.0 %
    (narrow, sideways), 4.6 % (narrow, forward), and the reference's own is within 0.4 % of it everywhere: it is the error of the
    fundamental matrices, not of the rules (profiles/focal_scenes.json has every kind)."""
    kind = f"{turn}-{motion}-{int(focal)}"
    m = measure(host, epi_host, motion, focal, turn)
    ru, re = np.array(m["rules"]), np.array(m["reference"])
    dist = np.abs(ru / re - 1.0)
    print(kind, "contrast", min(m["contrast"]), "..", max(m["contrast"]), "distance", dist.max(), "against the truth: rules",
          np.abs(ru / focal - 1.0).max(), "reference", np.abs(re / focal - 1.0).max())
    assert min(m["contrast"]) >= DEFAULT_CONTRAST and all(0 < i < 63 for i in m["index"])
    margin = 1.5 * MEASURED_DISTANCE[kind]
    assert dist.max() <= margin
    assert (np.abs(ru / focal - 1.0) <= np.abs(re / focal - 1.0) + margin).all()


def test_the_recorded_ranges_are_the_measured_ones():
    rows = json.load(open(SCENES_JSON))["kinds"]
    assert set(rows) == {f"{t}-{m}-{int(f)}" for t in TURNS for m in MOTIONS for f in FOCALS}
    for kind, d in MEASURED_DISTANCE.items():
        assert abs(rows[kind]["distance_from_reference"] / d - 1.0) < 0.02, kind
    turning = [rows[k]["contrast"] for k in rows if not k.startswith("none")]
    still = [rows[k]["contrast"] for k in rows if k.startswith("none")]
    assert max(c[1] for c in still) < DEFAULT_CONTRAST <= min(c[0] for c in turning)


if __name__ == "__main__":  # python tests/test_focal_host.py: measures every kind again and rewrites profiles/focal_scenes.json (no GPU)
    import tempfile

    class _Tmp:
        @staticmethod
        def mktemp(name):
            return tempfile.mkdtemp(prefix=name)
    libs = {}
    for name_, fn, types in (("focal", "host_fit_focal", [C.c_int] * 12 + [C.c_float] * 7 + [C.c_void_p] * 16),
                             ("epipolar", "host_fit_epipolar", [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 5 + [C.c_void_p] * 12)):
        libs[name_] = host_library(_Tmp, name_)
        getattr(libs[name_], fn).restype, getattr(libs[name_], fn).argtypes = C.c_int, types
    rows = {}
    for turn_ in TURNS:
        for motion_ in MOTIONS:
            for focal_ in FOCALS:
                m_ = measure(libs["focal"], libs["epipolar"], motion_, focal_, turn_, reference=turn_ != "none")
                row = dict(contrast=[min(m_["contrast"]), max(m_["contrast"])])
                if turn_ != "none":
                    ru_, re_ = np.array(m_["rules"]), np.array(m_["reference"])
                    er_, ee_ = np.abs(ru_ / focal_ - 1.0), np.abs(re_ / focal_ - 1.0)
                    row.update(distance_from_reference=float(np.abs(ru_ / re_ - 1.0).max()), rules_error_against_truth=float(er_.max()),
                               reference_error_against_truth=float(ee_.max()), worst_excess_over_reference=float((er_ - ee_).max()))
                rows[f"{turn_}-{motion_}-{int(focal_)}"] = row
                print(f"{turn_}-{motion_}-{int(focal_)}", row, flush=True)
    doc = json.load(open(SCENES_JSON))
    turning = [r["contrast"] for k_, r in rows.items() if not k_.startswith("none")]
    still = [r["contrast"] for k_, r in rows.items() if k_.startswith("none")]
    doc.update(kinds=rows, contrast_with_a_turn=[min(c[0] for c in turning), max(c[1] for c in turning)],
               contrast_without_a_turn=[min(c[0] for c in still), max(c[1] for c in still)])
    json.dump(doc, open(SCENES_JSON, "w"), indent=1)
