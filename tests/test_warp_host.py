"""The rules of ctk_warp_frames and ctk_smooth_path without a GPU: co-tracker_amd/csrc/warp_math.h built with g++ (tests/host/
warp_host.cpp) against the numpy restatement of tests/warp_reference.py on every byte and every float bit, the consequences the rules
promise (the identity copies, an integer shift is a shifted copy), the accuracy of the Q24 / 1/256-pixel arithmetic against an
unrounded float64 evaluation, the path rule's properties, and a planted lock-on through tests/motion_reference.py."""
import ctypes as C

import numpy as np
import pytest

import motion_reference as MR
import warp_reference as R
from ctk_support import host_library


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return host_library(tmp_path_factory, "warp")


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_warp(host, src, matrices, border, fill, layout):
    src, matrices = np.ascontiguousarray(src), np.ascontiguousarray(matrices, dtype=np.float32)
    F = src.shape[0]
    H, W = src.shape[1:3] if layout == R.HWC else src.shape[2:4]
    row = W * 3 if layout == R.HWC else W
    dst = np.full_like(src, 0x5A)
    fill = np.array(list(fill) + [0], dtype=np.uint8)
    host.host_warp_frames(F, H, W, layout, border, ptr(fill), C.c_int64(3 * H * W), C.c_int64(row), C.c_int64(3 * H * W), C.c_int64(row),
                          ptr(matrices), ptr(src), ptr(dst))
    return dst


def host_path(host, motion, state, alpha, post):
    motion = np.ascontiguousarray(motion, dtype=np.float32)
    G, F = motion.shape[:2]
    st = np.tile(R.IDENTITY.astype(np.float64), (G, 1)) if state is None else np.array(state, dtype=np.float64).reshape(G, 6)
    post = None if post is None else np.ascontiguousarray(post, dtype=np.float32)
    warp = np.full((G, F, 2, 3), np.nan, dtype=np.float32)
    host.host_smooth_path(G, F, C.c_float(alpha), ptr(motion), ptr(post), ptr(st), ptr(warp))
    return warp, st


def random_matrices(rng, n, hw):
    H, W = hw
    return np.stack([R.similarity(rng.uniform(-0.3, 0.3), rng.uniform(0.7, 1.4), rng.uniform(-40, 40, 2), ((W - 1) / 2, (H - 1) / 2))
                     for _ in range(n)])


def same_f32(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def same_f64(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


@pytest.mark.parametrize("layout", (R.HWC, R.CHW))
@pytest.mark.parametrize("border", (R.FILL, R.EDGE))
def test_host_build_equals_the_restatement_on_every_byte(host, layout, border):
    rng = np.random.default_rng(3 + layout * 2 + border)
    H, W, F = 37, 53, 6
    src = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    if layout == R.CHW:
        src = np.ascontiguousarray(src.transpose(0, 3, 1, 2))
    m = random_matrices(rng, F, (H, W))
    fill = (7, 200, 90)
    got, want = host_warp(host, src, m, border, fill, layout), R.warp_frames(src, m, border, fill, layout)
    assert np.array_equal(got, want)
    assert (want != R.warp_frames(src, m, 1 - border, fill, layout)).any()  # the two borders differ on these matrices
    c = np.zeros(6, dtype=np.int64)
    for row in m:
        host.host_warp_fix(ptr(np.ascontiguousarray(row)), ptr(c))
        assert np.array_equal(c, R.fix(row)) and host.host_warp_valid(ptr(np.ascontiguousarray(row))) == 1


def test_identity_integer_shift_and_invalid_matrices(host):
    rng = np.random.default_rng(5)
    H, W = 21, 30
    pic = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    ident = R.IDENTITY.reshape(1, 2, 3)
    for warp in (lambda m, b, f: R.warp_frames(pic, m, b, f), lambda m, b, f: host_warp(host, pic, m, b, f, R.HWC)):
        for border in (R.FILL, R.EDGE):
            assert np.array_equal(warp(ident, border, (9, 9, 9)), pic)
        # an integer translation: out(x, y) = src(x + 4, y - 3), the fill where that lies outside
        m = np.array([[[1, 0, 4], [0, 1, -3]]], dtype=np.float32)
        out = warp(m, R.FILL, (1, 2, 3))
        assert np.array_equal(out[0, 3:, :W - 4], pic[0, :H - 3, 4:])
        assert (out[0, :3] == (1, 2, 3)).all() and (out[0, :, W - 4:] == (1, 2, 3)).all()
        edge = warp(m, R.EDGE, (1, 2, 3))
        assert np.array_equal(edge[0, 3:, :W - 4], pic[0, :H - 3, 4:]) and np.array_equal(edge[0, 0, :W - 4], pic[0, 0, 4:])
        assert np.array_equal(edge[0, 5, W - 4:], np.repeat(pic[0, 2, W - 1:], 4, axis=0))
        # not valid: a copy
        for k, v in ((0, np.nan), (5, np.inf), (2, -np.inf), (1, 9.0), (3, -8.5), (2, 40000.0), (5, -32769.0)):
            bad = np.array([1, 0, 2.5, 0, 1, -1.25], dtype=np.float32)
            bad[k] = v
            assert not R.valid(bad) and host.host_warp_valid(ptr(bad)) == 0
            assert np.array_equal(warp(bad.reshape(1, 2, 3), R.FILL, (9, 9, 9)), pic), (k, v)
        # the bounds themselves are valid
        edge_ok = np.array([8, -8, 32768, -8, 8, -32768], dtype=np.float32)
        assert R.valid(edge_ok) and host.host_warp_valid(ptr(edge_ok)) == 1
        assert (warp(edge_ok.reshape(1, 2, 3), R.FILL, (9, 9, 9)) == 9).all()


def bilinear64(src, m, border, fill):
    """The unrounded evaluation: float64 coordinates of the float32 matrix, float64 weights, no rounding of the result."""
    H, W, _ = src.shape
    m = np.asarray(m, dtype=np.float32).astype(np.float64)
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    sx, sy = m[0, 0] * x + m[0, 1] * y + m[0, 2], m[1, 0] * x + m[1, 1] * y + m[1, 2]
    ix, iy = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    fx, fy = (sx - ix)[..., None], (sy - iy)[..., None]

    def tap(tx, ty):
        cx, cy = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
        v = src[cy, cx].astype(np.float64)
        return np.where(((cx == tx) & (cy == ty))[..., None], v, np.asarray(fill, dtype=np.float64)) if border == R.FILL else v
    return ((1 - fx) * (1 - fy) * tap(ix, iy) + fx * (1 - fy) * tap(ix + 1, iy) + (1 - fx) * fy * tap(ix, iy + 1) +
            fx * fy * tap(ix + 1, iy + 1))


def test_accuracy_against_an_unrounded_float64_evaluation(host):
    """The coordinate is rounded to 1/256 px (off by at most 1/512 per axis) and each Q24 coefficient is off by at most 2^-25, which
    moves a coordinate by at most (H + W + 1) 2^-25 per axis; a bilinear surface of 8-bit values has a slope of at most 255 per pixel
    along each axis, and the result is rounded to an integer: the bar is 255 (2/512 + 2 (H + W + 1) 2^-25) + 0.5 grey levels.
    Measured at 270 x 480 over these 40 random similarities: 1.24 against the bar of 1.51."""
    rng = np.random.default_rng(11)
    H, W = 270, 480
    bar = 255.0 * (2.0 / 512.0 + 2.0 * (H + W + 1) * 2.0 ** -25) + 0.5
    pic = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    worst = 0.0
    for k, m in enumerate(random_matrices(rng, 40, (H, W))):
        border = k % 2
        got = host_warp(host, pic[None], m[None], border, (30, 60, 90), R.HWC)[0].astype(np.float64)  # the header's own arithmetic
        worst = max(worst, float(np.abs(got - bilinear64(pic, m, border, (30, 60, 90))).max()))
    print(f"worst error {worst:.4f} grey levels, bar {bar:.4f}")
    assert worst <= bar


def test_path_rule(host):
    rng = np.random.default_rng(2)
    G, F = 3, 9
    motion = np.stack([[R.similarity(rng.uniform(-0.05, 0.05), rng.uniform(0.95, 1.05), rng.uniform(-6, 6, 2), (48, 32)) for _ in range(F)]
                       for _ in range(G)])
    post = R.zoom_matrix(64, 96, 1.1)
    for alpha in (0.0, 0.1, 0.37, 1.0):
        for po in (None, post):
            (w_h, s_h), (w_r, s_r) = host_path(host, motion, None, alpha, po), R.smooth_path(motion, None, alpha, po)
            assert same_f32(w_h, w_r) and same_f64(s_h, s_r), (alpha, po is None)
            # a range cut into two calls with the state carried over: the bits of one call
            for path in (lambda *a: host_path(host, *a), R.smooth_path):
                w0, s0 = path(motion[:, :4], None, alpha, po)
                w1, s1 = path(motion[:, 4:], s0, alpha, po)
                assert same_f32(np.concatenate([w0, w1], axis=1), w_r) and same_f64(s1, s_r)
    # alpha = 1: nothing is corrected, exactly (k = 0 leaves zeros of either sign: the values are compared, and the Q24 coefficients)
    w, s = R.smooth_path(motion, None, 1.0)
    assert np.array_equal(w, np.broadcast_to(R.IDENTITY.reshape(2, 3), w.shape)) and np.array_equal(s, np.tile(R.IDENTITY, (G, 1)))
    assert all(np.array_equal(R.fix(m), R.fix(R.IDENTITY)) for m in w.reshape(-1, 6))
    # alpha = 0 with constant integer translations accumulates exactly
    step = np.array([[1, 0, 3], [0, 1, -2]], dtype=np.float32)
    w, s = R.smooth_path(np.broadcast_to(step, (1, 12, 2, 3)), None, 0.0)
    for f in range(12):
        assert np.array_equal(w[0, f], np.array([[1, 0, 3 * (f + 1)], [0, 1, -2 * (f + 1)]], dtype=np.float32))
    # a steady pan of 3 px a frame at alpha = 0.1 settles at a lag of (1 - alpha) v / alpha = 27 px
    pan = np.broadcast_to(np.array([[1, 0, 3], [0, 1, 0]], dtype=np.float32), (1, 400, 2, 3))
    w, s = R.smooth_path(pan, None, 0.1)
    assert abs(float(w[0, -1, 0, 2]) - 27.0) < 1e-3 and w[0, -1, 0, 0] == 1 and w[0, -1, 1, 2] == 0
    assert float(w[0, 5, 0, 2]) < 27.0  # (it gets there from below)
    # a NaN (or infinite) motion counts as the identity: the state stays finite
    bad = motion.copy()
    bad[0, 2, 0, 1], bad[1, 5, 1, 2], bad[2, 0] = np.nan, np.inf, np.nan
    (w_h, s_h), (w_r, s_r) = host_path(host, bad, None, 0.2, post), R.smooth_path(bad, None, 0.2, post)
    assert same_f32(w_h, w_r) and same_f64(s_h, s_r) and np.isfinite(w_r).all() and np.isfinite(s_r).all()
    good = motion.copy()
    good[0, 2], good[1, 5], good[2, 0] = R.IDENTITY.reshape(2, 3), R.IDENTITY.reshape(2, 3), R.IDENTITY.reshape(2, 3)
    assert same_f32(R.smooth_path(good, None, 0.2, post)[0], w_r)


@pytest.mark.parametrize("model", (MR.TRANSLATION, MR.SIMILARITY))
def test_planted_lock_on(host, model):
    """A picture moved by integer offsets, exact tracks, alpha = 0: the fitted motions are exact integer translations (the refit's
    sums make a = 1 and b = 0 exactly), the path accumulates them exactly, and every stabilised picture is frame 0 bit for bit
    wherever its taps lie inside."""
    frames, tracks, off = R.planted(seed=4)
    T, N = tracks.shape[:2]
    motion, inl, st = MR.fit_motion(tracks[None], visible=np.ones((1, T, N), dtype=np.uint8), f0=0, F=T, lag=1, model=model, K=128,
                                    min_base=8.0)
    assert np.array_equal(motion[0, 0], R.IDENTITY.reshape(2, 3))
    for f in range(1, T):
        d = off[f - 1] - off[f]
        assert np.array_equal(motion[0, f], np.array([[1, 0, d[0]], [0, 1, d[1]]], dtype=np.float32)), f
    warp, _ = R.smooth_path(motion, None, 0.0)
    for f in range(T):
        d = off[0] - off[f]
        assert np.array_equal(warp[0, f], np.array([[1, 0, d[0]], [0, 1, d[1]]], dtype=np.float32))
    for out in (R.warp_frames(frames, warp[0], R.FILL, (255, 0, 255)), host_warp(host, frames, warp[0], R.FILL, (255, 0, 255), R.HWC)):
        seen = 0
        for f in range(T):
            inside = R.taps_inside(warp[0, f], *frames.shape[1:3])
            assert np.array_equal(out[f][inside], frames[0][inside]), f
            seen += int(inside.sum())
        assert seen > T * frames.shape[1] * frames.shape[2] // 2 and (off[1:] != off[0]).any()
