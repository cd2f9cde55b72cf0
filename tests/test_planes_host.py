"""The arithmetic of the planes kernels (csrc/planes.hip, csrc/warp_planes.hip) pinned WITHOUT a GPU.

co-tracker_amd/csrc/plane_math.h holds the rules of ctk_fit_planes and ctk_warp_planes -- the four-point sample, the integer admissibility,
the hypothesis matrix, the inlier test, the fixed-point refit and its L D L^T solve, the move to pixels, the projective coordinate -- in
host/device inline functions.  This test compiles that header with g++ (-ffp-contract=off, the flag the device translation units are
built with) behind plain loops (tests/host/planes_host.cpp) and compares it with the numpy restatement of tests/planes_reference.py:
every output exactly, the float32 matrices bit for bit.  The last tests measure what the rules are worth on planted scenes, on the g++
build of the header and the restatement alike; the kernel is held to the same restatement by tests/test_gpu_planes.py."""
import ctypes as C

import numpy as np
import pytest

import motion_reference as R
import objects_reference as O
import planes_reference as PR
from ctk_support import host_library

NAMES = ("homography", "label", "stats", "box")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = host_library(tmp_path_factory, "planes")
    lib.host_plane_sample.restype = None
    lib.host_plane_sample.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.host_plane_hyp.restype = C.c_int
    lib.host_plane_hyp.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    lib.host_fit_planes.restype = C.c_int
    lib.host_fit_planes.argtypes = [C.c_int] * 13 + [C.c_uint32] + [C.c_float] * 5 + [C.c_void_p] * 12
    lib.host_warp_coords.restype = None
    lib.host_warp_coords.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.host_warp_planes.restype = None
    lib.host_warp_planes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    return lib


def run_host(host, coords, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1, to=None, lag=None,
             anchor=None, labels=None, L=1, inverse=0, min_points=8, tol=2.0, K=128, min_base=16.0, seed=0, scale=(1.0, 1.0)):
    coords = np.ascontiguousarray(coords, dtype=np.float32)
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out

    def ptr(a, dt):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=dt)
        return a, a.ctypes.data
    keep = [ptr(visible, np.uint8), ptr(vis, np.float32), ptr(conf, np.float32), ptr(first_row, np.int32),
            ptr(None if anchor is None else anchor[0], np.float32), ptr(None if anchor is None else anchor[1], np.uint8), ptr(labels, np.int8)]
    hom = np.full((G, F, L, 3, 3), np.nan, dtype=np.float32)
    label = np.full((G, F, N_out), 77, dtype=np.int8)
    stats = np.full((G, F, L, 4), -99, dtype=np.int32)
    box = np.full((G, F, L, 4), -99, dtype=np.int32)
    rc = host.host_fit_planes(G, N, N_out, R_, f0, F, -1 if to is None else to, 0 if lag is None else lag, 0 if anchor is None else anchor[2],
                              L, min_points, inverse, K, seed, tol, min_base, scale[0], scale[1], thresh, coords.ctypes.data,
                              *(k[1] for k in keep), hom.ctypes.data, label.ctypes.data, stats.ctypes.data, box.ctypes.data)
    assert rc == 0
    return hom, label, stats, box


def same(got, want):
    for g_, w_, name in zip(got, want, NAMES):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        eq = (g_.view(np.int32) if g_.dtype == np.float32 else g_) == (w_.view(np.int32) if w_.dtype == np.float32 else w_)
        assert eq.all(), (name, np.argwhere(~eq)[:5].tolist(), g_[~eq][:5], w_[~eq][:5])


def both(host, coords, **kw):
    got, want = run_host(host, coords, **kw), PR.fit_planes(coords, **kw)
    same(got, want)
    return want


def test_the_sample_and_the_hypothesis(host):
    for seed, f, M in ((0, 0, 4), (7, 3, 5), (0xdeadbeef, 2 ** 30 - 1, 64), (5, 9, 8192)):
        for k in (0, 1, 2, 127, 4095):
            i = (C.c_int * 4)()
            host.host_plane_sample(seed, f, k, M, i)
            assert list(i) == PR.sample(seed, f, k, M) and len(set(i)) == 4 and 0 <= min(i) and max(i) < M
    assert {tuple(sorted(PR.sample(1, 0, k, 4))) for k in range(50)} == {(0, 1, 2, 3)}
    assert len({tuple(PR.sample(1, 0, k, 4)) for k in range(400)}) == 24  # every order of four
    rng = np.random.default_rng(0)
    seen = set()
    for trial in range(300):
        P = rng.integers(-2 ** 17, 2 ** 17 + 1, (4, 2)) if trial % 3 else rng.integers(-40, 41, (4, 2))
        Q = P + rng.integers(-300, 301, (4, 2)) if trial % 2 else rng.integers(-2 ** 17, 2 ** 17 + 1, (4, 2))
        if trial == 0:  # the corners of the position range
            P = np.array([[-2 ** 17, -2 ** 17], [2 ** 17, -2 ** 17], [2 ** 17, 2 ** 17], [-2 ** 17, 2 ** 17]])
            Q = -P
        pt = np.ascontiguousarray(np.concatenate([P, Q], axis=1), dtype=np.int32)
        h = np.full(9, 7.0)
        b2 = (0, 16, 256 * 256)[trial % 3]
        ok = host.host_plane_hyp(pt.ctypes.data, b2, h.ctypes.data)
        want_ok, want = PR.hypothesis(P.tolist(), Q.tolist(), b2)
        assert bool(ok) == want_ok
        seen.add(want_ok)
        if want_ok:
            assert np.array_equal(h.view(np.int64), want.view(np.int64)) and h[8] == 1.0
            got = PR.apply(h, (P - P[0]).astype(np.float64))  # the four points are mapped onto their partners
            assert np.abs(got - (Q - Q[0])).max() <= 1e-6 * max(1.0, float(np.abs(Q - Q[0]).max()))
    assert seen == {True, False}


@pytest.mark.parametrize("inverse", (0, 1))
@pytest.mark.parametrize("L,K", ((1, 1), (1, 128), (3, 3), (3, 300), (16, 128)))
def test_scenes_three_forms(host, L, K, inverse):
    """L = 1, 3, 16, K = 1, 3, 128, 300, both values of inverse, the three source forms, a ring, first rows, positions that are not
    valid, labels outside 0..L-1, no labels, and the logits form."""
    G, T, N, N_out = 2, 8, 123, 120
    coords, visible, who = PR.planes_scene(3 + L + K, G, T, N, planes=min(L, 3))
    first = O.spoil(coords, N_out)
    labels = who.astype(np.int8)
    labels[0, :6] = (-1, 20, 16, -128, 127, L)  # no round's
    kw = dict(visible=visible, first_row=first, N_out=N_out, labels=labels, L=L, inverse=inverse, min_points=5, K=K, seed=11 * L,
              min_base=8.0, tol=2.0)
    m, lab, st, bx = both(host, coords, f0=0, F=5, lag=3, **kw)
    assert (st[:, :3, :, 0] == 0).all() and (lab[:, :3] == -1).all() and (st[:, 3:, 0, 0] > 10).all()
    assert (lab[0, :, 4] == -1).all() and (lab[0, 3:, :6][lab[0, 3:, :6] >= 0] == PR.NONE).all()
    if K >= 128:
        assert (st[:, 3:, :min(L, 3), 1] >= 5).all() and (st[..., 3] == 0).all() and (bx[:, 3:, 0, 2] >= bx[:, 3:, 0, 0]).all()
    both(host, coords, f0=1, F=7, to=2, **kw)
    anchor = (coords[:, 1].copy(), visible[:, 1].copy(), 1)
    first[1, 7] = 2  # released and reassigned after the anchor was taken: drops out
    want = both(host, coords, f0=3, F=5, anchor=anchor, **kw)
    assert (want[1][1, :, 7] == -1).all()
    ring = both(host, R.fold(coords, 6, 8), f0=3, F=5, anchor=anchor, **{**kw, "visible": R.fold(visible, 6, 8)})
    same(ring, want)
    if L == 1:  # no labels: one list of every correspondence
        m, lab, st, bx = both(host, coords, f0=2, F=3, lag=2, **{**kw, "labels": None})
        assert (st[:, :, 0, 0] == (lab >= 0).sum(axis=-1)).all()
    rng = np.random.default_rng(L)
    vis_l = np.where(visible != 0, 4.0, -4.0).astype(np.float32) + rng.uniform(-1, 1, visible.shape).astype(np.float32)
    kw.pop("visible")
    both(host, coords, vis=vis_l, conf=np.full(visible.shape, 5.0, dtype=np.float32), thresh=0.6, f0=2, F=3, lag=2, scale=(1.37, 0.81), **kw)


def test_inverse_swaps_the_roles(host):
    """inverse = 1 on (P, Q) is inverse = 0 on (Q, P): the matrix, the stats and the labels; the box stays on frame f."""
    coords, visible, who = PR.planes_scene(5, 1, 2, 90, planes=1)
    visible[:] = 1
    kw = dict(visible=visible, f0=1, F=1, lag=1, K=64, seed=3, min_base=8.0)
    fwd = both(host, coords, inverse=0, **kw)
    inv = both(host, coords, inverse=1, **kw)
    swapped = both(host, coords[:, ::-1].copy(), inverse=0, **kw)
    assert np.array_equal(inv[0].view(np.int32), swapped[0].view(np.int32)) and np.array_equal(inv[2], swapped[2])
    assert np.array_equal(inv[1], swapped[1]) and inv[2][0, 0, 0, 1] >= 40
    took = inv[1][0, 0] == 0
    q = R.quant(coords[0, 1], 1.0)[1], R.quant(coords[0, 1, :, 1], 1.0)[1]
    assert inv[3][0, 0, 0].tolist() == [q[0][took, 0].min(), q[1][took].min(), q[0][took, 0].max(), q[1][took].max()]
    # the two matrices are each other's inverse to within the noise of the scene
    corners = np.array([[0.0, 0.0], [480.0, 0.0], [480.0, 270.0], [0.0, 270.0]])
    assert np.abs(PR.apply(inv[0][0, 0, 0], PR.apply(fwd[0][0, 0, 0], corners)) - corners).max() < 0.5


@pytest.mark.parametrize("M", (0, 1, 2, 3, 4, 5, 63, 64, 65, 300))
def test_list_lengths(host, M):
    N = max(M, 1) + 2
    coords, visible, _ = PR.planes_scene(M, 1, 2, N, planes=1)
    visible[:] = 0
    visible[:, :, :M] = 1
    for K in (1, 3, 128):
        m, lab, st, bx = both(host, coords, visible=visible, f0=1, F=1, lag=1, K=K, seed=M, min_points=min(max(M, 1), 4), min_base=2.0)
        assert st[0, 0, 0, 0] == M and (lab[0, 0, M:] == -1).all()
        if M < 4:
            assert st[0, 0, 0].tolist() == [M, 0, -1, 0] and np.array_equal(m[0, 0, 0], np.eye(3, dtype=np.float32))


def degenerate(P, Q):
    """Lists given as pixel positions -> coords [1,2,M,2], all visible."""
    coords = np.stack([np.asarray(P, dtype=np.float32), np.asarray(Q, dtype=np.float32)])[None]
    return coords, np.ones(coords.shape[:3], dtype=np.uint8)


def test_lists_that_fit_nothing(host):
    kw = dict(f0=1, F=1, lag=1, K=128, seed=2, min_points=4)
    # exactly collinear points: nothing admissible, even with min_base = 0
    x = np.arange(40, dtype=np.float32) * 7.0
    line = np.stack([x, 2.0 * x + 3.0], axis=1)
    for mb in (0.0, 16.0):
        coords, visible = degenerate(line, line + 5.0)
        m, lab, st, bx = both(host, coords, visible=visible, min_base=mb, **kw)
        assert st[0, 0, 0].tolist() == [40, 0, -1, 0] and np.array_equal(m[0, 0, 0], np.eye(3, dtype=np.float32))
        assert bx[0, 0, 0].tolist() == [0, 0, -1, -1] and (lab == PR.NONE).all()
    # a destination that is the mirror image of the source: every sample quad changes its orientation and is refused
    rng = np.random.default_rng(1)
    P = rng.uniform(0, 400, (50, 2))
    coords, visible = degenerate(P, P * np.array([-1.0, 1.0]) + np.array([500.0, 0.0]))
    m, lab, st, bx = both(host, coords, visible=visible, min_base=4.0, **kw)
    assert st[0, 0, 0].tolist() == [50, 0, -1, 0]
    # the same list unmirrored fits; duplicate points: samples that hold a pair of them are refused, the others fit
    coords, visible = degenerate(np.repeat(P, 2, axis=0), np.repeat(P, 2, axis=0) * 1.01 + 3.0)
    m, lab, st, bx = both(host, coords, visible=visible, min_base=4.0, **kw)
    assert st[0, 0, 0, :2].tolist() == [100, 100] and st[0, 0, 0, 3] == 0
    # too few inliers for min_points
    m, lab, st, bx = both(host, coords, visible=visible, min_base=4.0, **{**kw, "min_points": 101})
    assert st[0, 0, 0].tolist() == [100, 0, -1, 0]


def test_four_correspondences_and_a_fall_back(host):
    """A list of exactly four correspondences makes the system exactly determined: the refit solves it (it does NOT fall back: the
    normal matrix of four points in general position is positive definite), and returns the four-point matrix to rounding.  A
    fall-back needs a normal matrix that is singular to working precision: a sliver, four points within 1/16 pixel of a line that is
    8000 pixels long, which min_base = 0 admits."""
    P = np.array([[100.0, 100.0], [500.0, 120.0], [480.0, 400.0], [90.0, 380.0]])
    Q = np.array([[130.0, 90.0], [520.0, 140.0], [470.0, 420.0], [100.0, 390.0]])
    coords, visible = degenerate(P, Q)
    m, lab, st, bx = both(host, coords, visible=visible, f0=1, F=1, lag=1, K=8, seed=1, min_points=4, min_base=16.0)
    assert st[0, 0, 0].tolist()[:2] == [4, 4] and st[0, 0, 0, 3] == 0
    assert np.abs(PR.apply(m[0, 0, 0], P) - Q).max() < 1e-3
    fell = 0
    for P, Q in SLIVERS:
        coords, visible = degenerate(P, Q)
        m, lab, st, bx = both(host, coords, visible=visible, f0=1, F=1, lag=1, K=8, seed=1, min_points=4, min_base=0.0)
        assert st[0, 0, 0, :2].tolist() == [4, 4]
        fell += int(st[0, 0, 0, 3])
        if st[0, 0, 0, 3]:
            assert np.isfinite(m).all()
    assert fell >= 1


def sliver(seed):
    rng = np.random.default_rng(seed)
    x = np.array([-4000.0, -1500.0, 1000.0, 4000.0])
    y = np.array([0.0, 1.0, -1.0, 1.0]) / 16.0
    P = np.stack([x, y], axis=1)
    Q = np.stack([x + rng.integers(-3, 4, 4), y * rng.integers(1, 3, 4)], axis=1)
    return P, Q


SLIVERS = [sliver(s) for s in range(6)]


def test_positions_at_the_corners_of_the_range(host):
    """8192 points on a lattice that spans the whole position range: the refit sums of n = 8192 points at the largest reach."""
    N = 8192
    g = np.stack(np.meshgrid(np.linspace(-8192, 8192, 128), np.linspace(-8192, 8192, 64)), axis=-1).reshape(N, 2).astype(np.float32)
    coords = np.stack([g, -g])[None]
    m, lab, st, bx = both(host, coords, visible=np.ones((1, 2, N), dtype=np.uint8), min_points=8192, K=8, seed=3, f0=1, F=1, lag=1, tol=256.0,
                          min_base=64.0)
    assert st[0, 0, 0].tolist()[:2] == [N, N] and bx[0, 0, 0].tolist() == [-2 ** 17, -2 ** 17, 2 ** 17, 2 ** 17] and st[0, 0, 0, 3] == 0


# ---- the warp -------------------------------------------------------------------------------------------------------------------------
HORIZON = [[1.0, 0.2, -3.0], [0.1, 0.9, 2.0], [0.0, -0.05, 1.0]]  # Z = 0 on y = 20: a horizon across a 40-row picture
MATRICES = {
    "identity": np.eye(3),
    "horizon": np.array(HORIZON),
    "zero": np.zeros((3, 3)),
    "nan": np.array([[1.0, 0.0, 0.0], [0.0, np.nan, 0.0], [0.0, 0.0, 1.0]]),
    "inf": np.array([[1.0, 0.0, np.inf], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]),
    "far": np.array([[40000.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]),  # |sx| beyond 2^20 from x = 27 on
    "perspective": np.array([[0.9, 0.05, 1.3], [-0.04, 1.1, 0.7], [0.002, 0.001, 1.0]]),
    "negative": -np.eye(3),
    "halves": np.array([[1.0, 0.0, 0.5 / 256], [0.0, 1.0, 1.5 / 256], [0.0, 0.0, 1.0]]),  # ties of llrint
}


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_warp_coordinate_rule(host, name):
    H, W = 40, 50
    m = np.ascontiguousarray(MATRICES[name], dtype=np.float32)
    inside, X, Y = np.zeros((H, W), dtype=np.uint8), np.full((H, W), 9, dtype=np.int64), np.full((H, W), 9, dtype=np.int64)
    host.host_warp_coords(m.ctypes.data, H, W, inside.ctypes.data, X.ctypes.data, Y.ctypes.data)
    w_in, wX, wY = PR.coordinates(m, H, W)
    assert np.array_equal(inside != 0, w_in) and np.array_equal(X, wX) and np.array_equal(Y, wY)
    want = {"identity": H * W, "zero": 0, "nan": 0, "inf": 0, "negative": 0, "far": 27 * H, "halves": H * W}.get(name)
    assert want is None or int(w_in.sum()) == want
    if name == "horizon":
        assert w_in[:20].all() and not w_in[20:].any()
    if name == "halves":
        assert (wX[0, :4] & 255).tolist() == [0, 0, 0, 0] and (wY[:4, 0] & 255).tolist() == [2, 2, 2, 2]  # half to even
    # the whole picture rule on top of it, the three borders
    src = PR.WR.texture(3, 23, 31)
    fill = np.array([7, 200, 90, 0], dtype=np.uint8)
    for border in (PR.FILL, PR.EDGE, PR.KEEP):
        dst = PR.WR.texture(4, H, W)
        want_pic = PR.warp_planes(src[None], m[None], dst[None], border=border, fill=fill[:3])[0]
        got = dst.copy()
        host.host_warp_planes(src.ctypes.data, 23, 31, 3, m.ctypes.data, border, fill.ctypes.data, got.ctypes.data, H, W)
        assert np.array_equal(got, want_pic), (name, border)
        if border == PR.KEEP and name in ("zero", "nan", "inf", "negative"):
            assert np.array_equal(got, dst)
    if name == "identity":
        same_size = PR.warp_planes(src[None], m[None], np.zeros_like(src)[None])[0]
        assert np.array_equal(same_size, src)


# ---- what the rules are worth, on the restatement -------------------------------------------------------------------------------------
SEEDS = range(20)
SCENES = {"large": dict(quad=(400, 600), N=1024), "small": dict(quad=(120, 160), N=64)}
CORNER_CAP = 2 * 0.0099  # px against the float64 DLT over the same inliers: twice the worst value measured (docstring below)
TRUTH_CAP = 2 * 0.23     # px against the planted matrix


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("size", sorted(SCENES))
def test_planted_scenes(host, size, seed):
    """Planted scenes (planes_reference.planted): a quad of 600 x 400 px with 1024 points, or of 160 x 120 px with 64, on a 1920 x
    1080 frame; its corners displaced by up to 12 % of the size plus a shift of up to 100 px; 0.1 px Gaussian noise; 40 % of the
    points replaced by uniform outliers; tol 2, K 128, min_base 16.  On every scene there is a fit that keeps no planted outlier and
    drops no planted inlier, and the quad's corners under the refit lie within CORNER_CAP of their place under a float64
    Hartley-normalised SVD-DLT over the same inliers.  The fit is the g++ build's of plane_math.h (`both`: equal to the restatement on
    every output), so the bars apply to the shipped rules.

    Measured with these rules over the 20 seeds: against the DLT 0.0017 px at worst (large) and 0.0098 px (small, 38 inliers: the two
    algebraic costs weigh the noise differently); against the planted matrix 0.14 px (large) and 0.23 px (small, 64 points); the
    condition number of the normal matrix was at most 3.2e3.  The bars are twice the worst values."""
    coords, out, truth, corners = PR.planted(seed, **SCENES[size])
    N = out.size
    details = {}
    T, b2 = R.tol_steps(2.0), R.base2(16.0)
    _, P = R.quant(coords[0, 0], 1.0)
    _, Q = R.quant(coords[0, 1], 1.0)
    # the g++ build of plane_math.h fits the scene (and equals the restatement on every output): the figures below are the header's
    hom, lab, stats, _ = both(host, coords, visible=np.ones((1, 2, N), dtype=np.uint8), f0=1, F=1, lag=1, K=128, seed=seed)
    m9, inl, st = hom[0, 0, 0].reshape(9), lab[0, 0] == 0, tuple(int(v) for v in stats[0, 0, 0])
    r9, r_inl, r_st = PR.fit_list(P, Q, 1, T, b2, 128, seed, 8, details)  # (once more, for the normal matrix alone)
    assert np.array_equal(r9.view(np.int32), m9.view(np.int32)) and np.array_equal(r_inl, inl) and tuple(r_st) == st
    kept = int((inl & out).sum())
    dropped = int((~inl & ~out).sum())
    ref = PR.dlt(P[inl] / 16.0, Q[inl] / 16.0)
    got = PR.apply(m9, corners)
    against_dlt = float(np.abs(got - PR.apply(ref, corners)).max())
    against_truth = float(np.abs(got - PR.apply(truth, corners)).max())
    cond = float(np.linalg.cond(details["N"]))
    print(f"planted {size} seed={seed}: inliers {st[1]} of {N}, outliers kept {kept}, inliers dropped {dropped}, corners against the DLT "
          f"{against_dlt:.5f} px, against the truth {against_truth:.4f} px, cond {cond:.3g}, fell back {st[3]}")
    assert st[2] >= 0 and st[3] == 0
    assert kept == 0
    assert dropped == 0
    assert against_dlt <= CORNER_CAP
    assert against_truth <= TRUTH_CAP
