"""The arithmetic of the objects kernel (csrc/objects.hip) pinned WITHOUT a GPU.

co-tracker_amd/csrc/objects_math.h holds what ctk_fit_objects adds to the rules of ctk_fit_motion -- the seed of a round, the source
frame, the round of a label, acceptance, the box -- in host/device inline functions.  This test compiles that header with g++
(-ffp-contract=off, the flag the device translation unit is built with) behind plain loops (tests/host/objects_host.cpp) and compares it
with the numpy restatement of tests/objects_reference.py: every output exactly, the float32 matrices bit for bit.  The last tests
measure what the rules are worth on planted scenes; they cover the restatement, not the kernel."""
import ctypes as C

import numpy as np
import pytest

import motion_reference as R
import objects_reference as O
from ctk_support import host_library

NAMES = ("motion", "label", "stats", "box")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = host_library(tmp_path_factory, "objects")
    lib.host_objects_seed.restype = C.c_uint32
    lib.host_objects_seed.argtypes = [C.c_uint32, C.c_int]
    lib.host_objects_source.restype = C.c_int
    lib.host_objects_source.argtypes = [C.c_int] * 5
    lib.host_objects_round.restype = C.c_int
    lib.host_objects_round.argtypes = [C.c_int] * 2
    lib.host_fit_objects.restype = C.c_int
    lib.host_fit_objects.argtypes = [C.c_int] * 13 + [C.c_uint32] + [C.c_float] * 5 + [C.c_void_p] * 12
    return lib


def run_host(host, coords, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1, to=None, lag=None,
             anchor=None, labels=None, L=4, min_points=8, model=1, tol=2.0, K=128, min_base=16.0, seed=0, scale=(1.0, 1.0)):
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
    motion = np.full((G, F, L, 2, 3), np.nan, dtype=np.float32)
    label = np.full((G, F, N_out), 77, dtype=np.int8)
    stats = np.full((G, F, L, 4), -99, dtype=np.int32)
    box = np.full((G, F, L, 4), -99, dtype=np.int32)
    rc = host.host_fit_objects(G, N, N_out, R_, f0, F, -1 if to is None else to, 0 if lag is None else lag, 0 if anchor is None else anchor[2],
                               L, min_points, model, K, seed, tol, min_base, scale[0], scale[1], thresh, coords.ctypes.data,
                               *(k[1] for k in keep), motion.ctypes.data, label.ctypes.data, stats.ctypes.data, box.ctypes.data)
    assert rc == 0
    return motion, label, stats, box


def same(got, want):
    for g_, w_, name in zip(got, want, NAMES):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        assert np.array_equal(g_.view(np.int32) if g_.dtype == np.float32 else g_, w_.view(np.int32) if w_.dtype == np.float32 else w_), name


def both(host, coords, **kw):
    got, want = run_host(host, coords, **kw), O.fit_objects(coords, **kw)
    same(got, want)
    return want


def test_the_small_rules(host):
    assert host.host_objects_seed(1234, 0) == 1234 and R.mix(0) == 0  # round 0 samples with the seed itself
    for seed in (0, 7, 0xffffffff, 0xdeadbeef):
        for r in range(16):
            assert host.host_objects_seed(seed, r) == O.seed_of(seed, r)
    assert len({O.seed_of(5, r) for r in range(16)}) == 16
    assert host.host_objects_source(9, -1, 3, 0, 0) == 6 and host.host_objects_source(2, -1, 3, 0, 0) == -1
    assert host.host_objects_source(9, 4, 0, 0, 0) == 4 and host.host_objects_source(9, -1, 0, 1, 77) == 77
    assert [host.host_objects_round(v, 3) for v in (-128, -1, 0, 2, 3, 20, 127)] == [-1, -1, 0, 2, -1, -1, -1]


@pytest.mark.parametrize("model", (0, 1))
@pytest.mark.parametrize("L", (1, 3, 16))
@pytest.mark.parametrize("mode", ("split", "labels"))
def test_scenes_three_forms(host, model, L, mode):
    """Both modes, L = 1, 3, 16, both models, the three source forms, first rows, positions that are not valid, labels outside
    0..L-1, and the logits form."""
    G, T, N, N_out = 2, 8, 83, 80
    coords, visible, who = O.objects_scene(3 + L, G, T, N)
    first = O.spoil(coords, N_out)
    labels = None
    if mode == "labels":
        labels = who.astype(np.int8)
        labels[0, :6] = (-1, 20, 16, -128, 127, L)  # no round's
    kw = dict(visible=visible, first_row=first, N_out=N_out, labels=labels, L=L, min_points=4, model=model, K=64, seed=11 * L, min_base=8.0,
              tol=1.5 if model == 0 else 2.0)
    m, lab, st, bx = both(host, coords, f0=0, F=5, lag=3, **kw)
    assert (st[:, :3, :, 0] == 0).all() and (lab[:, :3] == -1).all() and (st[:, 3:, 0, 0] > 10).all()
    assert (lab[0, :, 4] == -1).all() and (st[..., 3] == 0).all()
    if mode == "labels":
        assert (lab[0, 3:, :6][lab[0, 3:, :6] >= 0] == O.NONE).all()
        assert L == 1 or ((st[:, 3:, 1, 1] >= 4).all() and (bx[:, 3:, 1, 2] >= bx[:, 3:, 1, 0]).all())
    elif L >= 3:
        assert (st[:, 3:, 1, 1] >= 4).all() and (lab == 1).any() and (L == 16 or (lab == O.NONE).any())  # (16 rounds may take them all)
    both(host, coords, f0=1, F=7, to=2, **kw)
    anchor = (coords[:, 1].copy(), visible[:, 1].copy(), 1)
    first[1, 7] = 2  # released and reassigned after the anchor was taken: drops out
    want = both(host, coords, f0=3, F=5, anchor=anchor, **kw)
    assert (want[1][1, :, 7] == -1).all()
    # a ring: 6 rows after 8 frames hold frames 2 .. 7; the anchor (frame 1) has left it
    ring = both(host, R.fold(coords, 6, 8), f0=3, F=5, anchor=anchor, **{**kw, "visible": R.fold(visible, 6, 8)})
    same(ring, want)
    # the logits form, away from the threshold
    rng = np.random.default_rng(L)
    vis_l = np.where(visible != 0, 4.0, -4.0).astype(np.float32) + rng.uniform(-1, 1, visible.shape).astype(np.float32)
    kw.pop("visible")
    both(host, coords, vis=vis_l, conf=np.full(visible.shape, 5.0, dtype=np.float32), thresh=0.6, f0=2, F=3, lag=2, scale=(1.37, 0.81), **kw)


@pytest.mark.parametrize("model", (0, 1))
@pytest.mark.parametrize("lag,K", ((1, 1), (3, 64), (1, 300)))
def test_round_0_is_fit_motion(host, model, lag, K):
    """Split mode, the lag form, min_points = 1: round 0's matrix and stats and (label == 0) are ctk_fit_motion's."""
    coords, visible, _ = R.scene(3 + K, G=2, T=8, N=41)
    first = O.spoil(coords, 39)
    kw = dict(visible=visible, first_row=first, N_out=39, f0=0, F=8 - lag, lag=lag, model=model, K=K, seed=11 * K, min_base=8.0)
    m, lab, st, bx = both(host, coords, L=3, min_points=1, **kw)
    mm, inl, ms = R.fit_motion(coords, **kw)
    assert np.array_equal(m[:, :, 0].view(np.int32), mm.view(np.int32)) and np.array_equal(st[:, :, 0], ms)
    assert np.array_equal(lab == 0, inl == 1) and np.array_equal(lab == -1, inl == -1)


@pytest.mark.parametrize("model", (0, 1))
def test_few_points_and_rounds_that_stop(host, model):
    N = 12
    coords = np.zeros((1, 6, N, 2), dtype=np.float32)
    coords[0, :, :, 0] = np.arange(N) * 20.0 + np.arange(6)[:, None] * 3.0  # everything shifts by (3, 1) px a frame ...
    coords[0, :, :, 1] = (np.arange(N) % 2) * 30.0 + np.arange(6)[:, None] * 1.0
    coords[0, :, 8:, 1] += np.arange(6)[:, None] * 40.0                      # ... but the last four, which also sink by 40
    visible = np.zeros((1, 6, N), dtype=np.uint8)
    visible[0, :2, :] = 1   # frame 1: M = 12
    visible[0, 2, :2] = 1   # frame 2: M = 2
    visible[0, 3, :1] = 1   # frame 3: M = 1;  frame 4: M = 0
    kw = dict(visible=visible, model=model, K=64, seed=1, f0=0, F=5, lag=1, min_base=16.0)
    m, lab, st, bx = both(host, coords, L=4, min_points=3, **kw)
    # frame 1: 8 points, then 4, then nothing is left: round 2 has M_r = 0 and ends the rounds
    assert st[0, 1, :, :2].tolist() == [[12, 8], [4, 4], [0, 0], [0, 0]] and st[0, 1, :, 2].min() == -1 and (st[0, 1, :2, 2] >= 0).all()
    assert lab[0, 1].tolist() == [0] * 8 + [1] * 4 and bx[0, 1, 2].tolist() == [0, 0, -1, -1]
    assert bx[0, 1, 1].tolist() == [(8 * 20 + 3) * 16, (0 + 41) * 16, (11 * 20 + 3) * 16, (30 + 41) * 16]
    assert np.array_equal(m[0, 1, 1], np.array([[1, 0, 3], [0, 1, 41]], dtype=np.float32))
    # frame 2: M = 2 < min_points: round 0 fits nothing, takes nothing, and every round reports M_r = 2
    assert st[0, 2].tolist() == [[2, 0, -1, 0]] * 4 and lab[0, 2, :3].tolist() == [O.NONE, O.NONE, -1]
    assert np.array_equal(m[0, 2], np.broadcast_to(np.array([[1, 0, 0], [0, 1, 0]], dtype=np.float32), (4, 2, 3)))
    assert st[0, 3, :, 0].tolist() == [1] * 4 and st[0, 4, :, 0].tolist() == [0] * 4 and (lab[0, 4] == -1).all()
    # min_points = 5: the second group is too small; the split stops at round 1 and its four points stay untaken
    m, lab, st, bx = both(host, coords, L=3, min_points=5, **kw)
    assert st[0, 1, :, :2].tolist() == [[12, 8], [4, 0], [4, 0]] and st[0, 1, 1:, 2].tolist() == [-1, -1] and lab[0, 1].tolist() == [0] * 8 + [O.NONE] * 4
    # min_points = 1: M_r = 1 is a fit for a translation and none for a similarity
    m, lab, st, bx = both(host, coords, L=2, min_points=1, **kw)
    assert st[0, 3].tolist() == ([[1, 1, 0, 0], [0, 0, -1, 0]] if model == 0 else [[1, 0, -1, 0], [1, 0, -1, 0]])  # (M = 1: every k ties, the lowest wins)
    # labels mode: the rounds are independent -- an empty label, a label with one point, a label too small, a label that fits
    labels = np.array([[2] * 8 + [3, 3, 3, 1]], dtype=np.int8)
    m, lab, st, bx = both(host, coords, L=4, min_points=2, labels=labels, **kw)
    assert st[0, 1, :, 0].tolist() == [0, 1, 8, 3] and st[0, 1, :, 1].tolist() == [0, 0, 8, 3]
    assert lab[0, 1].tolist() == [2] * 8 + [3, 3, 3, O.NONE]
    # every pair closer than min_base: a similarity has no admissible hypothesis
    m, lab, st, bx = both(host, coords, L=2, min_points=1, **{**kw, "min_base": 400.0})
    assert st[0, 1, 0, :2].tolist() == ([12, 8] if model == 0 else [12, 0]) and (model == 0 or st[0, 1, 0, 2] == -1)


def test_corners_reach_the_stated_bounds(host):
    """8192 points on the four corners of the position range: the box at its bounds, the refit sums of n = 8192 points."""
    N = 8192
    c = np.array([[-8192, -8192], [8192, -8192], [8192, 8192], [-8192, 8192]], dtype=np.float32)
    coords = np.zeros((1, 2, N, 2), dtype=np.float32)
    coords[0, 0] = c[np.arange(N) % 4]
    coords[0, 1] = -coords[0, 0]
    m, lab, st, bx = both(host, coords, visible=np.ones((1, 2, N), dtype=np.uint8), L=2, min_points=8192, model=1, K=8, seed=3, f0=1, F=1,
                          lag=1, tol=256.0, min_base=8192.0)
    assert st[0, 0].tolist() == [[N, N, 0, 0], [0, 0, -1, 0]] and bx[0, 0, 0].tolist() == [-2 ** 17, -2 ** 17, 2 ** 17, 2 ** 17]


# ---- what the rules are worth, on the restatement -------------------------------------------------------------------------------------
FIT = dict(tol=2.0, min_base=16.0, min_points=8, K=128, L=4, f0=1, F=1, lag=1)
SEEDS = range(20)
CORNER_CAP = 0.05       # px: the float64 fit's own distance plus margin for the 1/16 px grid
LOSE_CAP, KEEP_CAP = 0.01, 0.10


def least_squares(src, dst):
    """The float64 least-squares similarity src -> dst: [2,3]."""
    x, y = src[:, 0], src[:, 1]
    one, zero = np.ones_like(x), np.zeros_like(x)
    A = np.concatenate([np.stack([x, -y, one, zero], 1), np.stack([y, x, zero, one], 1)])
    a, b, tx, ty = np.linalg.lstsq(A, np.concatenate([dst[:, 0], dst[:, 1]]), rcond=None)[0]
    return np.array([[a, -b, tx], [b, a, ty]])


@pytest.mark.parametrize("seed", SEEDS)
def test_split_recovers_the_planted_objects(seed):
    """Planted scenes (objects_reference.planted): a camera and three objects of 50 / 25 / 15 / 10 % of 1024 points at 480 x 270, each
    under its own similarity, 0.1 px of noise.  Split mode recovers every planted label -- the round order is the size order -- and
    each object's matrix moves the corners of its 80 x 80 box to within CORNER_CAP of a float64 least-squares fit on its true
    members."""
    coords, who, _ = O.planted(seed)
    m, lab, st, bx = O.fit_objects(coords, visible=np.ones((1, 2, who.size), dtype=np.uint8), seed=seed, **FIT)
    wrong = int((lab[0, 0] != who).sum())
    worst = 0.0
    for k in (1, 2, 3):
        ls = least_squares(coords[0, 0][who == k].astype(np.float64), coords[0, 1][who == k].astype(np.float64))
        cx, cy = O.CENTRES[k - 1]
        h = O.OBJECT_SIDE / 2
        corners = np.array([[cx - h, cy - h, 1], [cx + h, cy - h, 1], [cx - h, cy + h, 1], [cx + h, cy + h, 1]], dtype=np.float64)
        worst = max(worst, float(np.abs(corners @ m[0, 0, k].astype(np.float64).T - corners @ ls.T).max()))
    print(f"split seed={seed}: wrong labels {wrong}, worst corner difference {worst:.4f} px, inliers {st[0, 0, :, 1].tolist()}")
    assert wrong == 0
    assert worst <= CORNER_CAP


@pytest.mark.parametrize("seed", SEEDS)
def test_labels_mode_sheds_wrong_labels(seed):
    """The same scenes in labels mode, 15 % of the labels replaced by another object's: a correctly labelled point keeps its label
    (LOSE_CAP), a mislabelled one loses it unless its two motions agree within tol where it lies (KEEP_CAP)."""
    coords, who, _ = O.planted(seed)
    rng = np.random.default_rng(5000 + seed)
    given = who.copy()
    bad = rng.random(who.size) < 0.15
    given[bad] = (who[bad] + rng.integers(1, 4, int(bad.sum()))) % 4
    m, lab, st, bx = O.fit_objects(coords, visible=np.ones((1, 2, who.size), dtype=np.uint8), labels=given[None].astype(np.int8), seed=seed,
                                   **FIT)
    lost = float((lab[0, 0][~bad] != who[~bad]).mean())
    kept = float((lab[0, 0][bad] == given[bad]).mean())
    print(f"labels seed={seed}: correctly labelled points that lose their label {lost:.4f}, mislabelled that keep theirs {kept:.4f}")
    assert set(np.unique(lab[0, 0][bad])) <= {0, 1, 2, 3, O.NONE}
    assert lost <= LOSE_CAP
    assert kept <= KEEP_CAP
