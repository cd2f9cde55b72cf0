"""The rules of ctk_track_field and ctk_warp_field (include/ctk.h, "track field"; co-tracker_amd/csrc/field_math.h) restated in numpy,
int64 throughout: what the kernels (tests/test_gpu_field.py) and the g++ build of the header (tests/test_field_host.py) are compared
with, exactly.  Positions are quantised with float32 operations (motion_reference.quant), the tent is the literal floor division by
rad (the header shifts and divides by the radius: the same quotient), the sums are int64 matrix products whose stated bounds are
asserted, the one division per node component is float64 with numpy's round-half-to-even."""
import numpy as np

import motion_reference as MR

INT32_MAX = 2 ** 31 - 1
FILL, EDGE = 0, 1
HWC, CHW = 0, 1
NO_LEVEL = 255


def grid(n, cs):
    return ((n - 1) >> cs) + 2


def tent(P, n_nodes, cs, radius):
    """int64 [M, n_nodes]: max(0, 1024 - (|P - N| * 1024) // rad) of every pair on every node of one axis."""
    N = (np.arange(n_nodes, dtype=np.int64) << cs) * 16
    rad = radius * (1 << cs) * 16
    return np.maximum(0, 1024 - (np.abs(P[:, None] - N[None, :]) * 1024) // rad)


def pairs(coords, f, ft, g, visible, vis, conf, thresh, first_row, N_out, sx, sy, anchor):
    """The correspondences of frame f of group g against frame ft -> (P int64 [M,2], d int64 [M,2])."""
    R = coords.shape[1]
    if ft < 0:
        return np.zeros((0, 2), dtype=np.int64), np.zeros((0, 2), dtype=np.int64)
    rp = f % R
    okx, Px = MR.quant(coords[g, rp, :N_out, 0], sx)
    oky, Py = MR.quant(coords[g, rp, :N_out, 1], sy)
    if anchor is not None:
        qc, qv = anchor[0][g, :N_out], np.asarray(anchor[1])[g, :N_out] != 0
    else:
        rq = ft % R
        qc = coords[g, rq, :N_out]
        qv = visible[g, rq, :N_out] != 0 if visible is not None else MR.visible_from_logits(vis[g, rq, :N_out], conf[g, rq, :N_out], thresh)
    pv = visible[g, rp, :N_out] != 0 if visible is not None else MR.visible_from_logits(vis[g, rp, :N_out], conf[g, rp, :N_out], thresh)
    okqx, Qx = MR.quant(qc[:, 0], sx)
    okqy, Qy = MR.quant(qc[:, 1], sy)
    ok = okx & oky & okqx & okqy & pv & qv
    if first_row is not None:
        first = np.asarray(first_row)[g, :N_out].astype(np.int64)
        ok &= (f >= first) & (ft >= first)
    P, Q = np.stack([Px, Py], axis=1)[ok], np.stack([Qx, Qy], axis=1)[ok]
    d = Q - P
    assert np.abs(P).max(initial=0) <= 2 ** 17 and np.abs(d).max(initial=0) <= 2 ** 18
    return P, d


def node_sums(P, d, gh, gw, cs, radius):
    """int64 [gh,gw,3] = (Wn, Sx, Sy)."""
    wx, wy = tent(P[:, 0], gw, cs, radius), tent(P[:, 1], gh, cs, radius)
    assert wx.max(initial=0) <= 1024 and wy.max(initial=0) <= 1024
    out = np.stack([wy.T @ wx, wy.T @ (wx * d[:, :1]), wy.T @ (wx * d[:, 1:])], axis=-1)
    assert out.dtype == np.int64 and out[..., 0].max(initial=0) <= 2 ** 33 and np.abs(out[..., 1:]).max(initial=0) <= 2 ** 51
    return out


def pyramid(level0):
    levels = [level0]
    while levels[-1].shape[:2] != (1, 1):
        a = levels[-1]
        h, w = a.shape[:2]
        p = np.zeros((2 * ((h + 1) >> 1), 2 * ((w + 1) >> 1), 3), dtype=np.int64)
        p[:h, :w] = a
        levels.append(p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2])
    return levels


def resolve(levels):
    """-> (field int32 [gh,gw,2], level uint8 [gh,gw])."""
    gh, gw = levels[0].shape[:2]
    j, i = np.arange(gh)[:, None], np.arange(gw)[None, :]
    field, level = np.zeros((gh, gw, 2), dtype=np.int32), np.full((gh, gw), NO_LEVEL, dtype=np.uint8)
    for l in range(len(levels) - 1, -1, -1):  # from the top down: the lowest level with support is written last
        e = levels[l][j >> l, i >> l]
        has = e[..., 0] >= 1
        wn = np.where(has, e[..., 0], 1).astype(np.float64)
        assert np.abs(e[..., 1:]).max(initial=0) * 16 <= 2 ** 55
        v = np.rint((e[..., 1:] * 16).astype(np.float64) / wn[..., None]).astype(np.int32)
        field[has], level[has] = v[has], l
    return field, level


def track_field(coords, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1, size=(1, 1), cs=4, radius=2,
                to=-1, lag=0, anchor=None, sx=1.0, sy=1.0):
    """coords float32 [G,R,N,2] (row of frame f: f % R); visible uint8 [G,R,N] or vis / conf logits; anchor = (coords [G,N,2], visible
    [G,N], frame) -> (field int32 [G,F,gh,gw,2], level uint8 [G,F,gh,gw], stats int32 [G,F,4])."""
    coords = np.asarray(coords, dtype=np.float32)
    G, R, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    assert (to >= 0) + (lag != 0) + (anchor is not None) == 1
    gh, gw = grid(size[0], cs), grid(size[1], cs)
    field, level = np.zeros((G, F, gh, gw, 2), dtype=np.int32), np.zeros((G, F, gh, gw), dtype=np.uint8)
    stats = np.zeros((G, F, 4), dtype=np.int32)
    for g in range(G):
        for k in range(F):
            f = f0 + k
            ft = anchor[2] if anchor is not None else (to if to >= 0 else f - lag)
            P, d = pairs(coords, f, ft, g, visible, vis, conf, thresh, first_row, N_out, sx, sy, anchor)
            levels = pyramid(node_sums(P, d, gh, gw, cs, radius))
            field[g, k], level[g, k] = resolve(levels)
            used = level[g, k].max()
            stats[g, k] = (len(P), int((level[g, k] == 0).sum()), int(used), 0)
    return field, level, stats


def positions(field, H, W, cs):
    """One picture's field int32 [gh,gw,2] -> (dx, dy) int64 [H,W]: the displacement of every pixel in 1/256 pixel."""
    c = 1 << cs
    f = np.asarray(field).astype(np.int64)
    assert f.shape == (grid(H, cs), grid(W, cs), 2)
    x, y = np.arange(W, dtype=np.int64)[None, :], np.arange(H, dtype=np.int64)[:, None]
    i, ax, j, ay = x >> cs, x & (c - 1), y >> cs, y & (c - 1)
    out = []
    for k in range(2):
        D = (c - ax) * (c - ay) * f[j, i, k] + ax * (c - ay) * f[j, i + 1, k] + (c - ax) * ay * f[j + 1, i, k] + ax * ay * f[j + 1, i + 1, k]
        out.append((D + ((c * c) >> 1)) >> (2 * cs))
    return out


def warp_picture(src, field, cs, border, fill):
    """src uint8 [H,W,C] -> [H,W,C] resampled through field [gh,gw,2]."""
    H, W, C = src.shape
    dx, dy = positions(field, H, W, cs)
    X, Y = np.arange(W, dtype=np.int64)[None, :] * 256 + dx, np.arange(H, dtype=np.int64)[:, None] * 256 + dy
    ix, iy = X >> 8, Y >> 8
    fx, fy = (X & 255).astype(np.int32)[..., None], (Y & 255).astype(np.int32)[..., None]
    fv = np.asarray(fill, dtype=np.int32).reshape(-1)[:C]

    def tap(tx, ty):
        cx, cy = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)  # (nothing outside the picture is read)
        v = src[cy, cx].astype(np.int32)
        if border == FILL:
            v = np.where(((cx == tx) & (cy == ty))[..., None], v, fv)
        return v
    p00, p01, p10, p11 = tap(ix, iy), tap(ix + 1, iy), tap(ix, iy + 1), tap(ix + 1, iy + 1)
    gx, gy = 256 - fx, 256 - fy
    out = (gx * gy * p00 + fx * gy * p01 + gx * fy * p10 + fx * fy * p11 + 32768) >> 16
    assert out.dtype == np.int32 and out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def warp_field(src, field, cs, border=FILL, fill=(0, 0, 0), layout=HWC):
    """src uint8 [F,H,W,3] (HWC), [F,3,H,W] (CHW) or [F,H,W] (one channel; also one picture for all with F = 1 and several fields),
    field int32 [F,gh,gw,2] -> the pictures in the layout of src."""
    src, field = np.asarray(src), np.asarray(field)
    assert src.dtype == np.uint8 and src.ndim in (3, 4)
    F = field.shape[0]
    x = src[..., None] if src.ndim == 3 else (src if layout == HWC else src.transpose(0, 2, 3, 1))
    out = np.stack([warp_picture(x[j if x.shape[0] > 1 else 0], field[j], cs, border, fill) for j in range(F)])
    if src.ndim == 3:
        return np.ascontiguousarray(out[..., 0])
    return np.ascontiguousarray(out if layout == HWC else out.transpose(0, 3, 1, 2))


def flow(field, H, W, cs):
    """field int32 [F,gh,gw,2] -> float32 [F,H,W,2]: (float)disp / 256.0f."""
    out = np.zeros((len(field), H, W, 2), dtype=np.float32)
    for j, f in enumerate(field):
        dx, dy = positions(f, H, W, cs)
        out[j, ..., 0], out[j, ..., 1] = dx.astype(np.float32) / np.float32(256.0), dy.astype(np.float32) / np.float32(256.0)
    return out


def similarity_scene(seed=0, hw=(270, 480), n=24, theta=np.deg2rad(1.7), s=1.02, shift=(3.25, -2.5), jitter=0.35):
    """The planted similarity of the accuracy test: a jittered n x n grid of points on an H x W picture (frame 0) and where a
    similarity about the picture centre takes them (frame 1) -> (coords float32 [1,2,N,2], the float64 map x -> position on frame 1)."""
    rng = np.random.default_rng(seed)
    H, W = hw
    gy, gx = np.meshgrid((np.arange(n) + 0.5) * H / n, (np.arange(n) + 0.5) * W / n, indexing="ij")
    p = np.stack([gx.ravel(), gy.ravel()], axis=1) + rng.uniform(-jitter, jitter, (n * n, 2)) * np.array([W / n, H / n])
    centre = np.array([(W - 1) / 2, (H - 1) / 2])
    A = s * np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])

    def move(x):
        return (np.asarray(x, dtype=np.float64) - centre) @ A.T + centre + np.asarray(shift)
    return np.stack([p, move(p)]).astype(np.float32)[None], move
