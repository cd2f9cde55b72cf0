"""The arithmetic of the epipolar kernel (csrc/epipolar.hip) pinned WITHOUT a GPU.

co-tracker_amd/csrc/epipolar_math.h holds the rules of ctk_fit_epipolar -- the eight-point sample, the integer admissibility, the pivoted
elimination of the 7 x 8 system, the division-free Sampson test, the two fixed-point refits through ctk_plane_solve, the move to pixels --
in host/device inline functions.  This test compiles that header with g++ (-ffp-contract=off, the flag the device translation unit is
built with) behind plain loops (tests/host/epipolar_host.cpp) and compares it with the numpy restatement of tests/epipolar_reference.py:
every bit of all four outputs.  The last tests measure what the rules are worth on planted scenes through the g++ build; the kernel is
held to the same restatement by tests/test_gpu_epipolar.py."""
import ctypes as C

import numpy as np
import pytest

import epipolar_reference as ER
import motion_reference as R
import objects_reference as O
from ctk_support import host_library

NAMES = ("fundamental", "label", "error", "stats")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = host_library(tmp_path_factory, "epipolar")
    lib.host_epi_sample.restype = None
    lib.host_epi_sample.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.host_epi_hyp.restype = C.c_int
    lib.host_epi_hyp.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.host_fit_epipolar.restype = C.c_int
    lib.host_fit_epipolar.argtypes = [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 5 + [C.c_void_p] * 12
    return lib


def run_host(host, coords, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1, to=None, lag=None,
             anchor=None, mask=None, min_points=16, tol=1.0, K=512, min_base=16.0, seed=0, scale=(1.0, 1.0)):
    coords = np.ascontiguousarray(coords, dtype=np.float32)
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out

    def ptr(a, dt):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=dt)
        return a, a.ctypes.data
    keep = [ptr(visible, np.uint8), ptr(vis, np.float32), ptr(conf, np.float32), ptr(first_row, np.int32),
            ptr(None if anchor is None else anchor[0], np.float32), ptr(None if anchor is None else anchor[1], np.uint8), ptr(mask, np.int8)]
    fund = np.full((G, F, 3, 3), np.nan, dtype=np.float32)
    label = np.full((G, F, N_out), 77, dtype=np.int8)
    error = np.full((G, F, N_out), np.nan, dtype=np.float32)
    stats = np.full((G, F, 4), -99, dtype=np.int32)
    rc = host.host_fit_epipolar(G, N, N_out, R_, f0, F, -1 if to is None else to, 0 if lag is None else lag, 0 if anchor is None else anchor[2],
                                min_points, K, seed, tol, min_base, scale[0], scale[1], thresh, coords.ctypes.data, *(k[1] for k in keep),
                                fund.ctypes.data, label.ctypes.data, error.ctypes.data, stats.ctypes.data)
    assert rc == 0
    return fund, label, error, stats


def same(got, want):
    for g_, w_, name in zip(got, want, NAMES):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        eq = (g_.view(np.int32) if g_.dtype == np.float32 else g_) == (w_.view(np.int32) if w_.dtype == np.float32 else w_)
        assert eq.all(), (name, np.argwhere(~eq)[:5].tolist(), g_[~eq][:5], w_[~eq][:5])


def both(host, coords, **kw):
    got, want = run_host(host, coords, **kw), ER.fit_epipolar(coords, **kw)
    same(got, want)
    return want


def test_the_sample_and_the_hypothesis(host):
    for seed, f, M in ((0, 0, 8), (7, 3, 9), (0xdeadbeef, 2 ** 30 - 1, 64), (5, 9, 8192)):
        for k in (0, 1, 2, 127, 4095):
            i = (C.c_int * 8)()
            host.host_epi_sample(seed, f, k, M, i)
            assert list(i) == ER.sample(seed, f, k, M) and len(set(i)) == 8 and 0 <= min(i) and max(i) < M
    assert {tuple(sorted(ER.sample(1, 0, k, 8))) for k in range(50)} == {tuple(range(8))}
    assert len({ER.sample(1, 0, k, 8)[0] for k in range(200)}) == 8  # every point is the anchor of some sample
    rng = np.random.default_rng(0)
    seen = set()
    for trial in range(200):
        P = rng.integers(-2 ** 17, 2 ** 17 + 1, (8, 2)) if trial % 3 else rng.integers(-40, 41, (8, 2))
        Q = P + rng.integers(-300, 301, (8, 2)) if trial % 2 else rng.integers(-2 ** 17, 2 ** 17 + 1, (8, 2))
        if trial == 0:  # the corners of the position range, and the anchor in the middle
            P = np.array([[0, 0], [-2 ** 17, -2 ** 17], [2 ** 17, -2 ** 17], [2 ** 17, 2 ** 17], [-2 ** 17, 2 ** 17], [2 ** 17, 5], [7, 2 ** 17],
                          [-3, -2 ** 17]])
            Q = -P[::-1] // 3
            Q[0] = 0
        if trial == 5:  # Q == P: every skew matrix fits; whatever the elimination makes of it, both make the same
            Q = P.copy()
        if trial == 7:  # all on one line
            P = np.stack([np.arange(8) * 100, np.arange(8) * 50], axis=1)
            Q = P + 3
        pt = np.ascontiguousarray(np.concatenate([P, Q], axis=1), dtype=np.int32)
        f9, ej = np.full(9, 7.0), np.zeros(2, dtype=np.int32)
        b2 = (0, 16, 256 * 256)[trial % 3]
        ok = host.host_epi_hyp(pt.ctypes.data, b2, f9.ctypes.data, ej.ctypes.data)
        want = ER.hypothesis(P.tolist(), Q.tolist(), b2)
        assert bool(ok) == (want is not None), trial
        seen.add(bool(ok))
        if want is not None:
            fm, e, js = want
            assert np.array_equal(f9.view(np.int64), np.array(fm).view(np.int64)) and (int(ej[0]), int(ej[1])) == (e, js)
            assert f9[js] == 1.0 and f9[8] == 0.0 and np.abs(f9).max() == 1.0
            if trial % 2 == 0 and trial > 7:  # eight points in general position: all obey the matrix
                r, g = ER.residual(fm, e, P[0], Q[0], P, Q)
                assert (g > 0).all() and (np.abs(r) / np.sqrt(g) * 2.0 ** e <= 1e-6 * 2.0 ** e).all()
    assert seen == {True, False}


@pytest.mark.parametrize("K", (1, 256, 300))
def test_scenes_three_forms(host, K):
    """K = 1, 256, 300, the three source forms, a ring, first rows, positions that are not valid, masks, and the logits form."""
    G, T, N, N_out = 2, 8, 123, 120
    coords, visible, mover = ER.history(3 + K, G, T, N)
    first = O.spoil(coords, N_out)
    mask = (~mover).astype(np.int8)
    mask[0, :6] = (-1, 20, 0, -128, 127, 0)
    kw = dict(visible=visible, first_row=first, N_out=N_out, K=K, seed=11 + K, min_base=8.0, tol=1.0, min_points=12)
    fu, lab, er, st = both(host, coords, f0=0, F=5, lag=3, **kw)
    assert (st[:, :3, 0] == 0).all() and (lab[:, :3] == -1).all() and (er[:, :3] == -1).all() and (st[:, 3:, 0] > 60).all()
    assert (lab[0, :, 4] == -1).all() and (fu[:, :3] == 0).all()
    if K >= 256:
        assert (st[:, 3:, 1] >= 12).all() and (st[:, 3:, 2] >= 0).all() and (st[..., 3] == 0).all()
        assert ((lab[:, 3:] == 1).sum(axis=-1) > 50).all() and np.isfinite(er[lab >= 0]).all() and (er[lab >= 0] >= 0).all()
    both(host, coords, f0=3, F=3, lag=3, mask=mask, **kw)
    both(host, coords, f0=1, F=7, to=2, **kw)
    anchor = (coords[:, 1].copy(), visible[:, 1].copy(), 1)
    first[1, 7] = 2  # released and reassigned after the anchor was taken: drops out
    want = both(host, coords, f0=3, F=5, anchor=anchor, mask=mask, **kw)
    assert (want[1][1, :, 7] == -1).all()
    ring = both(host, R.fold(coords, 6, 8), f0=3, F=5, anchor=anchor, mask=mask, **{**kw, "visible": R.fold(visible, 6, 8)})
    same(ring, want)
    rng = np.random.default_rng(K)
    vis_l = np.where(visible != 0, 4.0, -4.0).astype(np.float32) + rng.uniform(-1, 1, visible.shape).astype(np.float32)
    kw.pop("visible")
    both(host, coords, vis=vis_l, conf=np.full(visible.shape, 5.0, dtype=np.float32), thresh=0.6, f0=2, F=3, lag=2, scale=(1.37, 0.81), **kw)


@pytest.mark.parametrize("M", (7, 8, 9, 64, 257))
def test_list_lengths_masks_and_ties(host, M):
    """M = 7 (no fit), 8, 9, 64, 257 correspondences, without a mask and with one that leaves M - 1 or 7; with M = 8 every sample holds
    the same eight points: many hypotheses tie and the lowest k wins."""
    coords, visible, _ = ER.history(M, 1, 2, M + 3, movers=0.0 if M < 64 else 0.25)
    visible[:] = 1
    visible[0, 1, M:] = 0  # three slots are not on both frames
    kw = dict(visible=visible, f0=1, lag=1, min_base=2.0, min_points=8, seed=M)
    for K in (1, 64):
        fu, lab, er, st = both(host, coords, K=K, **kw)
        assert st[0, 0, 0] == M and (lab[0, 0, M:] == -1).all() and (lab[0, 0, :M] >= 0).all()
        if M < 8:
            assert st[0, 0].tolist() == [7, 0, -1, 0] and (fu == 0).all() and (lab[0, 0, :M] == 0).all() and (er == -1).all()
        elif K == 64:
            assert st[0, 0, 2] >= 0 and st[0, 0, 1] >= 8
    mask = np.ones((1, M + 3), dtype=np.int8)
    mask[0, 2] = 0
    fu, lab, er, st = both(host, coords, K=64, mask=mask, **kw)
    assert st[0, 0, 0] == M - 1
    if M == 8:  # the mask leaves 7: no fit, and the correspondences are still there
        assert st[0, 0].tolist() == [7, 0, -1, 0] and (lab[0, 0, :M] == 0).all() and (er[0, 0, :M] == -1).all()
    elif M > 8:
        assert lab[0, 0, 2] >= 0 and er[0, 0, 2] >= 0  # classified, with an error, though it was not fitted on
    mask[0, 7:] = 0
    mask[0, 2] = 1
    fu, lab, er, st = both(host, coords, K=64, mask=mask, **kw)
    assert st[0, 0].tolist() == [7, 0, -1, 0]
    if M == 8:
        T, b2 = R.tol_steps(1.0), R.base2(2.0)
        ok, pos = R.quant(coords[0], 1.0)
        assert ok.all()
        P, Q = pos[0, :8], pos[1, :8]
        counts = []
        for k in range(64):
            i = ER.sample(M, 1, k, 8)
            h = ER.hypothesis([P[t].tolist() for t in i], [Q[t].tolist() for t in i], b2)
            counts.append(-1 if h is None else int(ER.test(*ER.residual(h[0], h[1], P[i[0]], Q[i[0]], P, Q), h[1], T).sum()))
        fu, lab, er, st = both(host, coords, K=64, **kw)
        assert counts.count(max(counts)) > 1 and st[0, 0, 2] == counts.index(max(counts))


def test_degenerate_scenes(host):
    """A static camera (P == Q: every skew matrix fits) and all points on one line: whatever the elimination makes of them, the g++
    build and the restatement make the same, and nothing but a label, a finite or infinite error >= 0, or the no-fit row comes out."""
    coords, visible, _ = ER.history(2, 1, 2, 80, movers=0.0)
    visible[:] = 1
    coords[0, 1] = coords[0, 0]
    line = coords.copy()
    line[0, :, :, 1] = line[0, :, :, 0] * 0.5 + 3.0
    line[0, 1, :, 0] += 2.0
    for c in (coords, line):
        for K in (1, 64):
            fu, lab, er, st = both(host, c, visible=visible, f0=1, lag=1, K=K, min_base=2.0, min_points=8, seed=5)
            assert set(np.unique(lab)) <= {0, 1} and not np.isnan(er).any() and not np.isnan(fu).any()
            assert (er >= 0).all() or st[0, 0, 2] == -1
            assert st[0, 0, 3] == 3  # both normal matrices are singular: both refits fall back to the hypothesis' own matrix


def test_error_where_the_gradient_vanishes(host):
    host.host_epi_error.restype = C.c_float
    host.host_epi_error.argtypes = [C.c_double, C.c_double, C.c_int]
    for r, g, e in ((0.0, 0.0, 5), (1.0, 0.0, 5), (1.0, -1.0, 5), (1.0, float("nan"), 5), (0.25, 0.5, 12), (3e-9, 7e-3, 1), (0.0, 2.0, 19)):
        got, want = np.float32(host.host_epi_error(r, g, e)), ER.error(np.float64(r), np.float64(g), e)
        assert got.view(np.int32) == want.view(np.int32) and (g > 0 or got == np.inf)


# ---- what the rules are worth: planted scenes through the g++ build -------------------------------------------------------------------
KINDS = ("sideways", "forward", "few")
# the largest ratio, over 20 seeds, of the RMS Sampson distance of the static points under the fitted matrix to that under a float64
# Hartley-normalised eight-point SVD fit over the same inliers; measured through the g++ build
MEASURED_RATIO = {"sideways": 1.0669, "forward": 1.0082, "few": 1.0097}


def planted_run(host, kind, seed):
    sc = ER.planted(seed, kind)
    coords = np.stack([sc["P"], sc["Q"]])[None].astype(np.float32)
    visible = np.ones((1, 2, coords.shape[2]), dtype=np.uint8)
    return sc, coords, visible, run_host(host, coords, visible=visible, f0=1, lag=1, K=512, tol=1.0, min_points=16, min_base=16.0, seed=0)


@pytest.mark.parametrize("kind", KINDS)
def test_planted_scenes(host, kind):
    """1080p, focal length 1000 px, depths 3..12 m, 0.1 px noise, 25 % movers in three groups, 512 hypotheses, tol 1, 20 seeds:
    (a) no scene drops more than 1 % of its static points; (b) no kept mover's noise-free displacement lies further than 8 px from its
    planted epipolar line; (c) the RMS Sampson distance of the static points stays within MEASURED_RATIO plus half its excess over 1 of
    the float64 Hartley fit over the same inliers."""
    drops, lines, ratios, errs = [], [], [], []
    for seed in range(20):
        sc, coords, visible, (fu, lab, er, st) = planted_run(host, kind, seed)
        static, lab = ~sc["mover"], lab[0, 0]
        assert st[0, 0, 2] >= 0 and st[0, 0, 3] == 0 and st[0, 0, 0] == len(lab) and st[0, 0, 1] == (lab == 1).sum()
        drops.append(float((lab[static] == 0).mean()))
        kept = sc["mover"] & (lab == 1)
        lines.append(float(ER.line_distance(sc["F_true"], sc["P_clean"][kept], sc["Q_clean"][kept]).max()) if kept.any() else 0.0)
        P, Q = coords[0, 0].astype(np.float64), coords[0, 1].astype(np.float64)
        rms = np.sqrt((ER.sampson(fu[0, 0], P[static], Q[static]) ** 2).mean())
        ref = np.sqrt((ER.sampson(ER.hartley(P[lab == 1], Q[lab == 1]), P[static], Q[static]) ** 2).mean())
        ratios.append(float(rms / ref))
        # the error output is the squared Sampson distance of the QUANTISED positions (1/16 pixel) under the double matrix; under the
        # float32 matrix the residual (Q, 1)^T F (P, 1) moves by at most 2^-24 sum |F_ij| |Q_i| |P_j|, and the distance by that over the
        # gradient's length (the gradient itself moves by parts in 10^7): held to twice that
        Pq, Qq = R.quant(coords[0, 0], 1.0)[1] / 16.0, R.quant(coords[0, 1], 1.0)[1] / 16.0
        Ph, Qh = np.concatenate([Pq, np.ones((len(Pq), 1))], axis=1), np.concatenate([Qq, np.ones((len(Qq), 1))], axis=1)
        Fm = fu[0, 0].astype(np.float64)
        a, b = Ph @ Fm.T, Qh @ Fm
        grad = np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2)
        slack = 2.0 ** -24 * ((np.abs(Qh) @ np.abs(Fm)) * np.abs(Ph)).sum(axis=1) / grad
        d = ER.sampson(Fm, Pq, Qq)
        off = np.abs(np.sqrt(er[0, 0].astype(np.float64)) - d)
        assert (off <= 2.0 * slack + 1e-6 * d).all(), float((off / slack).max())
        errs.append(float(off[d <= 4.0].max()))
    print(kind, "dropped", max(drops), "kept mover from its line", max(lines), "px; ratio", max(ratios), "error output against the float32 matrix", max(errs), "px")
    assert max(drops) <= 0.01
    assert max(lines) <= 8.0
    assert max(ratios) <= MEASURED_RATIO[kind] + 0.5 * (MEASURED_RATIO[kind] - 1.0)


MEASURED_F32 = 4.6e-4  # px: the largest change of a Sampson distance when the pixel matrix is rounded to float32, over the scenes below


def test_float32_matrix_keeps_the_distances():
    """The float32 pixel-unit matrix reproduces the double one's Sampson distances of the points within 4 px of the matrix: measured
    (MEASURED_F32), and held to 1e-3 px at 1080p.  The rounding is amplified where the gradient is short, next to an epipole inside the
    picture: over all 20 forward scenes of test_planted_scenes one such point moves by 1.16e-3 px."""
    worst = 0.0
    for kind in KINDS:
        for seed in (0, 1):
            sc = ER.planted(seed, kind)
            coords = np.stack([sc["P"], sc["Q"]]).astype(np.float32)
            ok, pos = R.quant(coords, 1.0)
            assert ok.all()
            details = {}
            m32 = ER.fit_list(pos[0], pos[1], np.ones(len(pos[0]), dtype=bool), 1, R.tol_steps(1.0), R.base2(16.0), 512, 0, 16, details)[0]
            P, Q = coords[0].astype(np.float64), coords[1].astype(np.float64)
            d64, d32 = ER.sampson(details["px64"], P, Q), ER.sampson(m32, P, Q)
            near = d64 <= 4.0  # the points a caller could call static; a mover's distance changes in proportion to itself
            worst = max(worst, float(np.abs(d64 - d32)[near].max()))
    print("float32 against double, Sampson distance:", worst, "px")
    assert worst <= 1.05 * MEASURED_F32 <= 1e-3
