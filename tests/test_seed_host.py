"""The arithmetic of the seed-point kernel (csrc/seed.hip) pinned WITHOUT a GPU.

co-tracker_amd/csrc/seed_math.h holds every step of the score, the cell rule, the candidate rectangle and the selection key in
host/device inline functions.  This test compiles that header with g++ (-ffp-contract=off, the flag the device translation unit is
built with) behind a plain loop (tests/host/seed_host.cpp) and compares it with the numpy restatement of tests/seed_reference.py:
integers on both sides, every comparison exact."""
import ctypes as C

import numpy as np
import pytest

import seed_reference as R
from ctk_support import host_library


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = host_library(tmp_path_factory, "seed")
    lib.host_seed_ceil_sqrt.restype = C.c_longlong
    lib.host_seed_ceil_sqrt.argtypes = [C.c_longlong]
    lib.host_seed_cell_axis.restype = C.c_int
    lib.host_seed_cell_axis.argtypes = [C.c_float, C.c_float, C.c_float, C.c_int]
    lib.host_seed_points.restype = C.c_int
    lib.host_seed_points.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_float] * 4 + [C.c_int] * 2 + [C.c_float] * 2 + [C.c_void_p] * 2

    def run(frame, grid, bounds=None, radius=3, margin=None, inset=0, min_score=1):
        """-> (seeds [gh*gw,3] int32, scores [h,w] int32)"""
        frame = np.ascontiguousarray(frame, dtype=np.float32)
        h, w = frame.shape[1:]
        gh, gw = grid
        x_lo, x_hi, y_lo, y_hi = bounds if bounds is not None else (0.0, w - 1.0, 0.0, h - 1.0)
        seeds, scores = np.empty((gh * gw, 3), dtype=np.int32), np.empty((h, w), dtype=np.int32)
        lib.host_seed_points(frame.ctypes.data, h, w, radius, radius + 1 if margin is None else margin, inset, min_score, x_lo, x_hi, y_lo,
                             y_hi, gh, gw, R.cell_scale(gw, x_lo, x_hi), R.cell_scale(gh, y_lo, y_hi), scores.ctypes.data, seeds.ctypes.data)
        return seeds, scores

    run.lib = lib
    return run


def frame_of(kind, h, w, seed):
    rng = np.random.RandomState(seed)
    # smooth blobs plus noise: a score map with structure, not white noise alone
    yy, xx = np.mgrid[:h, :w]
    base = 128 + 80 * np.sin(xx / 5.0 + rng.rand(3, 1, 1) * 6) * np.cos(yy / 7.0 + rng.rand(3, 1, 1) * 6)
    f = base + rng.randint(-30, 31, (3, h, w))
    if kind == "uint8":
        return np.clip(np.rint(f), 0, 255).astype(np.float32)
    if kind == "fractional":
        return np.clip(f + rng.rand(3, h, w), 0, 255).astype(np.float32)
    assert kind == "wild"  # values below 0 and above 255, halves (rint's ties), NaNs
    f = (f * 2.5 - 150).astype(np.float32)
    f[rng.rand(3, h, w) < 0.05] = np.float32("nan")
    f[rng.rand(3, h, w) < 0.05] = np.float32(100.5)
    f[rng.rand(3, h, w) < 0.05] = np.float32(101.5)
    return f


SIZES = [(37, 53, (3, 5)), (64, 96, (4, 6)), (96, 128, (5, 7))]


@pytest.mark.parametrize("radius", [1, 3, 7])
@pytest.mark.parametrize("kind", ["uint8", "fractional", "wild"])
@pytest.mark.parametrize("h,w,grid", SIZES)
def test_scores_and_seeds_equal_the_reference(host, h, w, grid, kind, radius):
    f = frame_of(kind, h, w, seed=h + radius)
    if kind == "wild":
        assert np.isnan(f).any() and (f < 0).any() and (f > 255).any()
    want_scores = R.score_map(f, radius)
    seeds, scores = host(f, grid, radius=radius)
    assert np.array_equal(scores, want_scores)
    assert np.array_equal(seeds, R.seed_points(f, grid, radius=radius, scores=want_scores))
    if radius < 7:
        assert (seeds[:, 2] > 0).all()  # every cell of these textured frames has a seed
    # widened bounds, an inset, another margin and a threshold that drops some cells
    kw = dict(bounds=(-2.5, w + 1.5, -3.0, h + 2.0), radius=radius, margin=2, inset=1, min_score=int(np.median(want_scores)))
    assert np.array_equal(host(f, grid, **kw)[0], R.seed_points(f, grid, scores=want_scores, **kw))


@pytest.mark.parametrize("h,w,grid", SIZES)
def test_one_pixel_per_cell_checks_every_pixel(host, h, w, grid):
    f = frame_of("fractional", h, w, seed=3)
    want = R.score_map(f, 3)
    seeds, _ = host(f, (h, w), margin=0, inset=0, min_score=0)
    ref = R.seed_points(f, (h, w), margin=0, inset=0, min_score=0, scores=want)
    assert np.array_equal(seeds, ref)
    got = seeds[seeds[:, 2] >= 0]
    assert len(got) >= h * w - (h + w) and np.array_equal(got[:, 2], want[got[:, 1], got[:, 0]])  # (the last row / column share a cell)


def test_constant_frame(host):
    f = np.full((3, 37, 53), 77.0, dtype=np.float32)
    seeds, scores = host(f, (3, 5))
    assert not scores.any() and (seeds == -1).all()
    seeds, _ = host(f, (3, 5), min_score=0, inset=1)
    ref = R.seed_points(f, (3, 5), min_score=0, inset=1)
    assert np.array_equal(seeds, ref) and (seeds[:, 2] == 0).all()
    # the tie-break pixel: the lowest py, then the lowest px of the candidates -- cell 0 starts at the margin plus nothing, cell 6 at
    # its own first pixel plus the inset
    assert seeds[0].tolist() == [4, 4, 0]
    cx, cy = R.cell_axis(53, 0, 52, R.cell_scale(5, 0, 52), 5), R.cell_axis(37, 0, 36, R.cell_scale(3, 0, 36), 3)
    assert seeds[6].tolist() == [int(np.flatnonzero(cx == 1)[0]) + 1, int(np.flatnonzero(cy == 1)[0]) + 1, 0]


def test_flat_frame_with_a_patch(host):
    f = R.flat_with_patches(64, 96, [(20, 40)], seed=4)
    seeds, _ = host(f, (4, 6))
    assert np.array_equal(seeds, R.seed_points(f, (4, 6)))
    hit = seeds[:, 2] >= 0
    assert 1 <= hit.sum() <= 4 and (seeds[hit, 2] > 100000).all()
    assert ((seeds[hit, 0] >= 40 - 4) & (seeds[hit, 0] < 56 + 4) & (seeds[hit, 1] >= 20 - 4) & (seeds[hit, 1] < 36 + 4)).all()


def test_insets_and_margins_that_empty_a_cell(host):
    f = frame_of("uint8", 37, 53, seed=8)
    for kw in (dict(inset=6), dict(inset=7), dict(margin=18), dict(margin=19), dict(margin=40), dict(inset=2 ** 31 - 1), dict(margin=2 ** 31 - 1)):
        seeds, _ = host(f, (3, 5), **kw)
        assert np.array_equal(seeds, R.seed_points(f, (3, 5), **kw)), kw
    assert (host(f, (3, 5), inset=7)[0] == -1).all() and (host(f, (3, 5), inset=4)[0][:, 2] > 0).any()


def test_ceil_sqrt(host):
    ks = list(range(0, 70)) + [2 ** e + o for e in range(6, 26) for o in (-1, 0, 1)] + [2 ** 25 - 3, 33554431, 33554432, 94906265, 94906266]
    rng = np.random.RandomState(0)
    ks += rng.randint(1, 2 ** 25, 400).tolist()
    for k in ks:
        for d in (k * k - 1, k * k, k * k + 1):
            if 0 <= d <= 2 ** 50 + 2 ** 27:
                got = host.lib.host_seed_ceil_sqrt(d)
                assert got == R.ceil_sqrt(d) and got * got >= d and (got == 0 or (got - 1) ** 2 < d), d
    assert host.lib.host_seed_ceil_sqrt(2 ** 50) == 2 ** 25 and host.lib.host_seed_ceil_sqrt(2 ** 50 + 1) == 2 ** 25 + 1


def test_cell_axis_is_the_rule_of_the_health_kernel(host):
    """clamp((int)floorf((x - lo) * inv), 0, g - 1) in float32, on positions inside and outside the bounds."""
    rng = np.random.RandomState(1)
    for lo, hi, g in ((0.0, 95.0, 6), (-2.5, 97.5, 12), (0.0, 63.0, 64), (0.0, 511.0, 80)):
        inv = R.cell_scale(g, lo, hi)
        xs = np.concatenate([np.arange(int(hi) + 1), rng.uniform(lo - 3, hi + 3, 200)]).astype(np.float32)
        want = np.clip(np.floor((xs - np.float32(lo)) * inv), 0, g - 1).astype(np.int64)
        got = [host.lib.host_seed_cell_axis(float(x), lo, float(inv), g) for x in xs]
        assert got == want.tolist()
