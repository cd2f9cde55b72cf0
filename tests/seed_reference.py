"""The rules of ctk_seed_points (include/ctk.h, "seed points"; co-tracker_amd/csrc/seed_math.h) restated in numpy: the reference of
tests/test_seed_host.py, tests/test_stream_seed_cabi.py and tests/test_gpu_stream_seed.py (`import seed_reference`; a plain module).
Integer arithmetic throughout, math.isqrt for the root, the cell of every pixel computed pixel by pixel in float32 -- no search, no
tiles: nothing here is shaped like the kernel.  Every comparison against it is exact."""
import math

import numpy as np


def f32(v):
    return np.float32(v)


def cell_scale(n, lo, hi):
    """float32(n) / (float32(hi) - float32(lo)): inv_cw / inv_ch as the host rounds them once."""
    return f32(f32(n) / f32(f32(hi) - f32(lo)))


def luminance(frame):
    """frame [3,h,w] float32 -> int64 [h,w] in 0..255."""
    q = np.asarray(frame, dtype=np.float32)
    q = np.where(np.isnan(q), np.float32(0), q)
    q = np.rint(np.clip(q, np.float32(0), np.float32(255))).astype(np.int64)  # (rint: half to even)
    return (77 * q[0] + 150 * q[1] + 29 * q[2] + 128) >> 8


def gradients(lum):
    p = np.pad(lum, 1, mode="edge")
    return p[1:-1, 2:] - p[1:-1, :-2], p[2:, 1:-1] - p[:-2, 1:-1]


def box(v, r):
    """Sums over the (2r+1)^2 window, pixels outside the image contributing nothing (int64)."""
    h, w = v.shape
    s = np.zeros((h + 1, w + 1), dtype=np.int64)
    s[1:, 1:] = v.cumsum(0).cumsum(1)
    y0, y1 = np.clip(np.arange(h) - r, 0, h), np.clip(np.arange(h) + r + 1, 0, h)
    x0, x1 = np.clip(np.arange(w) - r, 0, w), np.clip(np.arange(w) + r + 1, 0, w)
    return s[y1][:, x1] - s[y0][:, x1] - s[y1][:, x0] + s[y0][:, x0]


def ceil_sqrt(d):
    """The smallest integer t with t * t >= d (python integers: exact)."""
    d = int(d)
    return 0 if d <= 0 else math.isqrt(d - 1) + 1


def score_map(frame, radius=3):
    """-> int64 [h,w]: a + c - ceil_sqrt((a - c)^2 + 4 b^2) of every pixel."""
    gx, gy = gradients(luminance(frame))
    a, b, c = box(gx * gx, radius), box(gx * gy, radius), box(gy * gy, radius)
    d = (a - c) ** 2 + 4 * b * b
    root = np.array([ceil_sqrt(v) for v in d.reshape(-1).tolist()], dtype=np.int64).reshape(d.shape)
    out = a + c - root
    assert int(out.min()) >= 0 and int(out.max()) < 2 ** 31 and int(d.max()) < 2 ** 50
    return out


def cell_axis(n, lo, hi, inv, g):
    """-> int64 [n]: the cell of every pixel 0..n-1 along one axis, -1 outside the inclusive float32 bounds."""
    x = np.arange(n).astype(np.float32)
    t = np.floor((x - f32(lo)) * f32(inv))  # two float32 operations
    c = np.clip(t, 0, g - 1).astype(np.int64)
    return np.where((x >= f32(lo)) & (x <= f32(hi)), c, -1)


def seed_points(frame, grid, bounds=None, radius=3, margin=None, inset=0, min_score=1, scores=None):
    """-> int32 [gh*gw,3]: (px, py, score) per cell, (-1, -1, -1) without a candidate or below min_score.  scores: a score_map
    computed before (the same frame and radius)."""
    h, w = np.asarray(frame).shape[1:]
    gh, gw = grid
    x_lo, x_hi, y_lo, y_hi = bounds if bounds is not None else (0.0, w - 1.0, 0.0, h - 1.0)
    margin = radius + 1 if margin is None else margin
    sc = score_map(frame, radius) if scores is None else scores
    cx, cy = cell_axis(w, x_lo, x_hi, cell_scale(gw, x_lo, x_hi), gw), cell_axis(h, y_lo, y_hi, cell_scale(gh, y_lo, y_hi), gh)
    out = np.full((gh * gw, 3), -1, dtype=np.int32)

    def runs(c, g, n):
        """per cell: the candidate pixels along one axis"""
        res = []
        for k in range(g):
            px = np.flatnonzero(c == k)
            if len(px):
                assert np.array_equal(px, np.arange(px[0], px[-1] + 1))  # a run
                px = px[(px >= px[0] + inset) & (px <= px[-1] - inset) & (px >= margin) & (px <= n - 1 - margin)]
            res.append(px)
        return res

    xs, ys = runs(cx, gw, w), runs(cy, gh, h)
    for j in range(gh):
        for i in range(gw):
            if len(xs[i]) == 0 or len(ys[j]) == 0:
                continue
            sub = sc[ys[j][0]:ys[j][-1] + 1, xs[i][0]:xs[i][-1] + 1]
            k = int(np.argmax(sub))  # the first maximum in row-major order: the lowest py, then the lowest px
            py, px = divmod(k, sub.shape[1])
            if int(sub[py, px]) >= min_score:
                out[j * gw + i] = (xs[i][0] + px, ys[j][0] + py, int(sub[py, px]))
    return out


def flat_with_patches(h, w, patches, seed=0, size=16, level=128.0):
    """A constant frame [3,h,w] float32 with size x size random-dot patches (0 / 255 per pixel, all channels alike) whose top-left
    corners are `patches` = [(y, x), ...]."""
    rng = np.random.RandomState(seed)
    f = np.full((3, h, w), level, dtype=np.float32)
    for y, x in patches:
        f[:, y:y + size, x:x + size] = (rng.randint(0, 2, (size, size)) * 255).astype(np.float32)[None]
    return f
