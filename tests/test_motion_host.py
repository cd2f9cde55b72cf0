"""The arithmetic of the motion kernel (csrc/motion.hip) pinned WITHOUT a GPU.

co-tracker_amd/csrc/motion_math.h holds the quantisation of a position, the seeded samples, the integer scoring and the refit in
host/device inline functions.  This test compiles that header with g++ (-ffp-contract=off, the flag the device translation unit is
built with) behind plain loops (tests/host/motion_host.cpp) and compares it with the numpy restatement of tests/motion_reference.py:
every output exactly, the float32 matrix bit for bit.  The last test measures what the rules are worth on planted motions; it covers
the restatement, not the kernel."""
import ctypes as C

import numpy as np
import pytest

import motion_reference as R
from ctk_support import host_library


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = host_library(tmp_path_factory, "motion")
    lib.host_motion_quant.restype = C.c_int
    lib.host_motion_quant.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_int)]
    lib.host_motion_tol.restype = C.c_int
    lib.host_motion_tol.argtypes = [C.c_float]
    lib.host_motion_base2.restype = C.c_int64
    lib.host_motion_base2.argtypes = [C.c_float]
    lib.host_motion_mix.restype = C.c_uint32
    lib.host_motion_mix.argtypes = [C.c_uint32]
    lib.host_motion_sample.restype = None
    lib.host_motion_sample.argtypes = [C.c_uint32] + [C.c_int] * 4 + [C.POINTER(C.c_int)] * 2
    lib.host_fit_motion.restype = C.c_int
    lib.host_fit_motion.argtypes = [C.c_int] * 9 + [C.c_uint32] + [C.c_float] * 5 + [C.c_void_p] * 8
    return lib


def run_host(host, coords, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1, lag=1, model=1, tol=2.0,
             K=128, min_base=16.0, seed=0, scale=(1.0, 1.0)):
    coords = np.ascontiguousarray(coords, dtype=np.float32)
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out

    def ptr(a, dt):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=dt)
        return a, a.ctypes.data
    keep = [ptr(visible, np.uint8), ptr(vis, np.float32), ptr(conf, np.float32), ptr(first_row, np.int32)]
    motion = np.full((G, F, 2, 3), np.nan, dtype=np.float32)
    inlier = np.full((G, F, N_out), 77, dtype=np.int8)
    stats = np.full((G, F, 4), -99, dtype=np.int32)
    rc = host.host_fit_motion(G, N, N_out, R_, f0, F, lag, model, K, seed, tol, min_base, scale[0], scale[1], thresh, coords.ctypes.data,
                              *(k[1] for k in keep), motion.ctypes.data, inlier.ctypes.data, stats.ctypes.data)
    assert rc == 0
    return motion, inlier, stats


def same(got, want):
    for g_, w_, name in zip(got, want, ("motion", "inlier", "stats")):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        assert np.array_equal(g_.view(np.int32) if g_.dtype == np.float32 else g_, w_.view(np.int32) if w_.dtype == np.float32 else w_), name


def both(host, coords, **kw):
    got, want = run_host(host, coords, **kw), R.fit_motion(coords, **kw)
    same(got, want)
    return want


def test_positions_and_parameters(host):
    f32 = np.float32
    beyond = np.nextafter(f32(8192), f32(np.inf))
    xs = [0.0, 0.5 / 16, -0.5 / 16, 1.5 / 16, -1.5 / 16, 2.5 / 16, 100.03, -77.77, 8192.0, -8192.0, beyond, -beyond, 1e30, np.nan, np.inf, -np.inf]
    for s in (1.0, 1.37, 0.5):
        for x in xs:
            p = C.c_int(-12345)
            ok = host.host_motion_quant(float(f32(x)), float(f32(s)), C.byref(p))
            rok, rp = R.quant(f32(x), s)
            assert bool(ok) == bool(rok), (x, s)
            if ok:
                assert p.value == int(rp) and abs(p.value) <= 2 ** 17, (x, s)
            else:
                assert p.value == -12345
    p = C.c_int(0)
    assert host.host_motion_quant(0.5 / 16, 1.0, C.byref(p)) and p.value == 0       # half to even
    assert host.host_motion_quant(1.5 / 16, 1.0, C.byref(p)) and p.value == 2
    assert host.host_motion_quant(-8192.0, 1.0, C.byref(p)) and p.value == -2 ** 17
    assert not host.host_motion_quant(float(beyond), 1.0, C.byref(p)) and not host.host_motion_quant(float("nan"), 1.0, C.byref(p))
    for tol in (2.0, 1 / 16, 1 / 32, 0.03, 0.0, -1.0, 256.0, 256.03, 256.04, 1e30, float("nan"), float("inf"), 0.72):
        assert host.host_motion_tol(tol) == R.tol_steps(tol), tol
    assert R.tol_steps(2.0) == 32 and R.tol_steps(256.0) == 4096 and R.tol_steps(256.04) == 0 and R.tol_steps(float("nan")) == 0
    assert R.tol_steps(1 / 32) == 0  # (0.5 rounds to even: 0)
    for mb in (0.0, 16.0, 0.03, 8192.0, float(beyond), -0.001, float("nan"), float("inf"), 77.7):
        assert host.host_motion_base2(mb) == R.base2(mb), mb
    assert R.base2(16.0) == 256 ** 2 and R.base2(8192.0) == 2 ** 34 and R.base2(-1.0) == -1
    for x in (0, 1, 2, 0xdeadbeef, 0xffffffff, 12345678):
        assert host.host_motion_mix(x) == R.mix(x)
    i, j = C.c_int(), C.c_int()
    for seed, f, k, M in ((0, 0, 0, 2), (7, 3, 5, 2), (0xffffffff, 2 ** 30 - 1, 4095, 8192), (123, 99, 17, 3), (5, 1000, 299, 1088)):
        for model in (0, 1):
            host.host_motion_sample(seed, f, k, M, model, C.byref(i), C.byref(j))
            assert (i.value, j.value) == R.sample(seed, f, k, M, model)
            assert 0 <= i.value < M and 0 <= j.value < M and (model == 0 or i.value != j.value)


@pytest.mark.parametrize("model", (0, 1))
@pytest.mark.parametrize("lag", (1, 3))
@pytest.mark.parametrize("K", (1, 64, 300))
def test_scenes(host, model, lag, K):
    """Moving camera, points of their own, invisible frames, first rows, positions that are not valid."""
    coords, visible, _ = R.scene(3 + K, G=2, T=8, N=41)
    coords[0, 2, 5] = np.nan
    coords[0, 3, 6, 1] = np.inf
    coords[1, 4, 7, 0] = 9000.0
    coords[1, 5, 8] = (8192.0, -8192.0)
    first = np.zeros((2, 41), dtype=np.int32)
    first[0, :4] = (3, 5, R.INT32_MAX, 7)
    first[1, 40] = R.INT32_MAX
    kw = dict(model=model, lag=lag, K=K, seed=11 * K, tol=2.0, min_base=8.0)
    m, inl, st = both(host, coords, visible=visible, first_row=first, f0=0, F=8 - lag if lag > 1 else 7, N_out=39, **kw)
    assert (st[:, :lag, 0] == 0).all() and (inl[:, :lag] == -1).all()  # f - lag < 0: no correspondences, the identity
    assert np.array_equal(m[:, 0], np.broadcast_to(np.array([[1, 0, 0], [0, 1, 0]], dtype=np.float32), (2, 2, 3)))
    assert (inl[0, :, 2] == -1).all() and (st[:, lag:, 0] > 2).all() and (st[:, :, 3] == 0).all()
    # the logits form, away from the threshold
    rng = np.random.default_rng(K)
    vis_l = np.where(visible != 0, 4.0, -4.0).astype(np.float32) + rng.uniform(-1, 1, visible.shape).astype(np.float32)
    conf_l = np.full(visible.shape, 5.0, dtype=np.float32)
    vis_l[0, 1, 0] = np.nan
    got = both(host, coords, vis=vis_l, conf=conf_l, thresh=0.6, f0=lag, F=3, scale=(1.37, 0.81), **kw)
    assert (got[2][..., 0] > 2).all()


def test_split_invariance_and_ring(host):
    coords, visible, _ = R.scene(9, G=1, T=12, N=30)
    kw = dict(visible=visible, model=1, K=64, seed=5, lag=2)
    whole = both(host, coords, f0=2, F=9, **kw)
    a, b = both(host, coords, f0=2, F=4, **kw), both(host, coords, f0=6, F=5, **kw)
    same(tuple(np.concatenate([x, y], axis=1) for x, y in zip(a, b)), whole)
    # a ring of 6 rows after 10 frames holds frames 4 .. 9, frame 6 in row 0: frames 6 and 7 read their sources across the wrap
    ring = both(host, R.fold(coords, 6, 10), visible=R.fold(visible, 6, 10), model=1, K=64, seed=5, lag=2, f0=6, F=4)
    same(ring, tuple(x[:, 4:8] for x in whole))


@pytest.mark.parametrize("model", (0, 1))
def test_few_points_close_pairs_and_ties(host, model):
    N = 6
    coords = np.zeros((1, 5, N, 2), dtype=np.float32)
    coords[0, :, :, 0] = np.arange(N) * 20.0 + np.arange(5)[:, None] * 3.0  # everything shifts by 3 px a frame
    coords[0, :, :, 1] = (np.arange(N) % 2) * 30.0 + np.arange(5)[:, None] * 1.0
    visible = np.zeros((1, 5, N), dtype=np.uint8)
    visible[0, :2, :] = 1         # frame 1: M = 6
    visible[0, 2, :2] = 1         # frame 2: M = 2
    visible[0, 3, :1] = 1         # frame 3: M = 1
    m, inl, st = both(host, coords, visible=visible, model=model, K=64, seed=1, f0=0, F=5, min_base=16.0)  # frame 4: M = 0
    assert st[0, :, 0].tolist() == [0, 6, 2, 1, 0]
    # every hypothesis of frame 1 has all 6 inliers: the lowest k wins
    assert st[0, 1].tolist() == [6, 6, 0, 0] and st[0, 2].tolist() == [2, 2, 0, 0]
    assert st[0, 3].tolist() == ([1, 1, 0, 0] if model == 0 else [1, 0, -1, 0]) and inl[0, 3, 0] == (1 if model == 0 else 0)
    assert np.array_equal(m[0, 1], np.array([[1, 0, 3], [0, 1, 1]], dtype=np.float32))
    # all pairs closer than min_base: a similarity has no admissible hypothesis, a translation does not care
    m, inl, st = both(host, coords, visible=visible, model=model, K=64, seed=1, f0=1, F=1, min_base=200.0)
    assert st[0, 0].tolist() == ([6, 6, 0, 0] if model == 0 else [6, 0, -1, 0])
    assert model == 0 or (np.array_equal(m[0, 0], np.array([[1, 0, 0], [0, 1, 0]], dtype=np.float32)) and (inl[0, 0] == 0).all())
    # ties where the lowest k is NOT admissible: min_base = 50 admits only some pairs; the winner is the first admissible k
    if model == 1:
        m, inl, st = both(host, coords, visible=visible, model=1, K=64, seed=1, f0=1, F=1, min_base=50.0)
        P = R.quant(coords[0, 0, :, 0], 1.0)[1], R.quant(coords[0, 0, :, 1], 1.0)[1]
        adm = [k for k in range(64) for i, j in [R.sample(1, 1, k, 6, 1)]
               if (int(P[0][j] - P[0][i]) ** 2 + int(P[1][j] - P[1][i]) ** 2) >= R.base2(50.0)]
        assert 0 < len(adm) < 64 and adm[0] > 0 and st[0, 0].tolist() == [6, 6, adm[0], 0]
    # coincident sources with min_base = 0: D = 0 is not admissible
    same_spot = np.zeros((1, 2, 3, 2), dtype=np.float32)
    same_spot[0, 1] = 5.0
    m, inl, st = both(host, same_spot, visible=np.ones((1, 2, 3), dtype=np.uint8), model=model, K=8, f0=1, F=1, min_base=0.0)
    assert st[0, 0].tolist() == ([3, 3, 0, 0] if model == 0 else [3, 0, -1, 0])


@pytest.mark.parametrize("model", (0, 1))
def test_corners_reach_the_stated_bounds(host, model):
    """8192 points on the four corners (+-8192, +-8192), turned by half a turn: D = |A| = 2^37, T D = 2^49 at tol = 256, and the refit
    sums of n = 8192 points; the restatement's Python integers assert every stated bound on the way."""
    N = 8192
    c = np.array([[-8192, -8192], [8192, -8192], [8192, 8192], [-8192, 8192]], dtype=np.float32)
    coords = np.zeros((1, 2, N, 2), dtype=np.float32)
    coords[0, 0] = c[np.arange(N) % 4]
    coords[0, 1] = -coords[0, 0]
    visible = np.ones((1, 2, N), dtype=np.uint8)
    m, inl, st = both(host, coords, visible=visible, model=model, K=8, seed=3, f0=1, F=1, tol=256.0, min_base=8192.0)
    if model == 1:
        assert st[0, 0, :2].tolist() == [N, N] and np.array_equal(m[0, 0], np.array([[-1, 0, 0], [0, -1, 0]], dtype=np.float32))
    else:
        assert st[0, 0, 0] == N and st[0, 0, 1] == N // 4
    # one corner only moved: a quarter turn about the centre, the products at their bounds with both signs
    coords[0, 1, :, 0], coords[0, 1, :, 1] = -coords[0, 0, :, 1], coords[0, 0, :, 0]
    m, inl, st = both(host, coords, visible=visible, model=model, K=8, seed=4, f0=1, F=1, tol=256.0, min_base=16.0)
    if model == 1:
        assert st[0, 0, :2].tolist() == [N, N] and np.array_equal(m[0, 0], np.array([[0, -1, 0], [1, 0, 0]], dtype=np.float32))


def least_squares(src, dst):
    """The float64 least-squares similarity src -> dst: [2,3]."""
    x, y = src[:, 0], src[:, 1]
    one, zero = np.ones_like(x), np.zeros_like(x)
    A = np.concatenate([np.stack([x, -y, one, zero], 1), np.stack([y, x, zero, one], 1)])
    a, b, tx, ty = np.linalg.lstsq(A, np.concatenate([dst[:, 0], dst[:, 1]]), rcond=None)[0]
    return np.array([[a, -b, tx], [b, a, ty]])


CORNER_BAR = 2 * 0.0335  # twice the largest corner difference measured over the cases below (see the docstring)
ACCURACY = [(n, hw, frac, noise, seed) for n, hw in ((64, (64, 96)), (300, (384, 512))) for frac in (0.0, 0.4) for noise in (0.0, 0.25)
            for seed in range(5)]


def planted(n, hw, frac, noise, seed):
    rng = np.random.default_rng(1000 + seed)
    H, W = hw
    src = rng.uniform([0, 0], [W - 1, H - 1], size=(n, 2))
    A = R.similarity(rng.uniform(-0.05, 0.05), rng.uniform(0.95, 1.05), rng.uniform(-8, 8, 2), (W / 2, H / 2))
    dst = src @ A[:, :2].T + A[:, 2]
    out = np.zeros(n, dtype=bool)
    out[rng.permutation(n)[:int(round(frac * n))]] = True
    ang, far = rng.uniform(0, 2 * np.pi, n), rng.uniform(5, 40, n)
    dst = dst + out[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1) * far[:, None]
    src = src + ~out[:, None] * rng.normal(0, 1, (n, 2)) * noise
    dst = dst + ~out[:, None] * rng.normal(0, 1, (n, 2)) * noise
    return np.stack([src, dst])[None].astype(np.float32), out


def corner_difference(m, coords, out, hw):
    H, W = hw
    ls = least_squares(coords[0, 0][~out].astype(np.float64), coords[0, 1][~out].astype(np.float64))
    corners = np.array([[0, 0, 1], [W - 1, 0, 1], [0, H - 1, 1], [W - 1, H - 1, 1]], dtype=np.float64)
    return float(np.abs(corners @ m.astype(np.float64).T - corners @ ls.T).max())


@pytest.mark.parametrize("n,hw,frac,noise,seed", ACCURACY)
def test_accuracy_of_the_rules(n, hw, frac, noise, seed):
    """What the rules are worth, on the restatement (the kernel is pinned to it elsewhere): a planted similarity (rotation within
    +-0.05 rad, scale 0.95 .. 1.05, shift within +-8 px), 0 % or 40 % of the points displaced by 5 .. 40 px, Gaussian noise of 0 or
    0.25 px on the rest, tol = 2, 256 hypotheses.  Every planted outlier is reported 0, every planted inlier 1, and the matrix moves
    the four picture corners to within CORNER_BAR of a float64 least-squares fit over the planted inliers.  Measured over these 40
    cases: the largest corner difference is 0.0335 px (64 points, 40 % outliers, no noise: 38 inliers quantised to 1/16 px); next 0.0207 px
    (64 points, 40 %, noise), 0.0121 px at 300 points.  The bar is twice the largest."""
    coords, out = planted(n, hw, frac, noise, seed)
    m, inl, st = R.fit_motion(coords, visible=np.ones((1, 2, n), dtype=np.uint8), model=1, K=256, seed=seed, f0=1, F=1, tol=2.0, min_base=16.0)
    assert np.array_equal(inl[0, 0], (~out).astype(np.int8))
    diff = corner_difference(m[0, 0], coords, out, hw)
    print(f"corner difference n={n} frac={frac} noise={noise} seed={seed}: {diff:.5f} px")
    assert diff <= CORNER_BAR
