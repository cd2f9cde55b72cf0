"""The rules of ctk_warp_frames and ctk_smooth_path (include/ctk.h, "warp frames"; co-tracker_amd/csrc/warp_math.h) restated in numpy:
int64 coordinates, int32 blends and one float64 operation per step -- the kernels, the g++ build of the header and this file agree on
every byte and on every float32 / float64 bit.  Also the planted sequence the lock-on tests share."""
import numpy as np

FILL, EDGE = 0, 1
HWC, CHW = 0, 1
IDENTITY = np.array([1, 0, 0, 0, 1, 0], dtype=np.float32)


def valid(m):
    m = np.asarray(m, dtype=np.float32).reshape(6)
    with np.errstate(invalid="ignore"):
        return bool((np.abs(m[[0, 1, 3, 4]]) <= np.float32(8)).all() and (np.abs(m[[2, 5]]) <= np.float32(32768)).all())


def fix(m):
    """float32 matrix -> the six Q24 coefficients, int64; the identity's when the matrix is not valid."""
    m = np.asarray(m, dtype=np.float32).reshape(6)
    if not valid(m):
        m = IDENTITY
    return np.rint(m.astype(np.float64) * 16777216.0).astype(np.int64)


def warp_picture(src, m, border, fill):
    """src uint8 [H,W,3] -> [H,W,3]."""
    H, W, _ = src.shape
    c = fix(m)
    x, y = np.arange(W, dtype=np.int64)[None, :], np.arange(H, dtype=np.int64)[:, None]
    X, Y = c[0] * x + c[1] * y + c[2] + 32768, c[3] * x + c[4] * y + c[5] + 32768
    ix, iy = X >> 24, Y >> 24
    fx, fy = ((X >> 16) & 255).astype(np.int32)[..., None], ((Y >> 16) & 255).astype(np.int32)[..., None]
    fv = np.asarray(fill, dtype=np.int32).reshape(-1)[:3]

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


def warp_frames(src, matrices, border=FILL, fill=(0, 0, 0), layout=HWC):
    """src uint8 [F,H,W,3] (HWC) or [F,3,H,W] (CHW), matrices float32 [F,2,3] -> the warped pictures in the layout of src."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 4
    matrices = np.asarray(matrices, dtype=np.float32).reshape(src.shape[0], 6)
    hwc = src if layout == HWC else src.transpose(0, 2, 3, 1)
    out = np.stack([warp_picture(hwc[j], matrices[j], border, fill) for j in range(src.shape[0])])
    return np.ascontiguousarray(out if layout == HWC else out.transpose(0, 3, 1, 2))


def taps_inside(m, H, W):
    """bool [H,W]: the four taps of the output pixel lie inside the picture."""
    c = fix(m)
    x, y = np.arange(W, dtype=np.int64)[None, :], np.arange(H, dtype=np.int64)[:, None]
    ix, iy = (c[0] * x + c[1] * y + c[2] + 32768) >> 24, (c[3] * x + c[4] * y + c[5] + 32768) >> 24
    return (ix >= 0) & (ix + 1 <= W - 1) & (iy >= 0) & (iy + 1 <= H - 1)


def compose(A, B):
    """A o B on float64 [...,6] rows, one rounded operation per step."""
    P = np.empty(np.broadcast(A, B).shape, dtype=np.float64)
    for r in (0, 3):
        a0, a1, a2 = A[..., r], A[..., r + 1], A[..., r + 2]
        P[..., r] = a0 * B[..., 0] + a1 * B[..., 3]
        P[..., r + 1] = a0 * B[..., 1] + a1 * B[..., 4]
        P[..., r + 2] = (a0 * B[..., 2] + a1 * B[..., 5]) + a2
    return P


def smooth_path(motion, state=None, alpha=0.1, post=None):
    """motion float32 [G,F,2,3]; state float64 [G,6] (None: the identity) -> (warp float32 [G,F,2,3], the state after the F frames)."""
    motion = np.asarray(motion, dtype=np.float32)
    G, F = motion.shape[:2]
    W = np.tile(IDENTITY.astype(np.float64), (G, 1)) if state is None else np.array(state, dtype=np.float64).reshape(G, 6)
    a = np.float64(np.float32(alpha))
    k = np.float64(1.0) - a
    B = None if post is None else np.asarray(post, dtype=np.float32).reshape(6).astype(np.float64)
    out = np.empty((G, F, 6), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(F):
            m = motion[:, f].reshape(G, 6)
            M = np.where(np.isfinite(m).all(axis=1)[:, None], m, IDENTITY).astype(np.float64)
            W = k * compose(M, W)
            W[:, 0] += a
            W[:, 4] += a
            out[:, f] = (W if B is None else compose(W, B)).astype(np.float32)
    return out.reshape(G, F, 2, 3), W


def zoom_matrix(H, W, zoom):
    """float32 [2,3]: a scale by 1 / zoom about the picture centre."""
    s = np.float32(1.0) / np.float32(zoom)
    cx, cy = np.float32((W - 1) / 2), np.float32((H - 1) / 2)
    return np.array([[s, 0, cx - s * cx], [0, s, cy - s * cy]], dtype=np.float32)


def similarity(theta, s, t, centre):
    """-> float32 [2,3]: x -> s Rot(theta) (x - centre) + centre + t."""
    c, n = s * np.cos(theta), s * np.sin(theta)
    lin = np.array([[c, -n], [n, c]])
    return np.concatenate([lin, (np.asarray(centre) - lin @ np.asarray(centre) + np.asarray(t))[:, None]], axis=1).astype(np.float32)


def texture(seed, H, W):
    """A textured uint8 picture [H,W,3]: smooth waves plus noise, so that every shift shows."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = 96 + 60 * np.sin(x / 3.1) * np.cos(y / 4.3) + 40 * np.sin((x + 2 * y) / 7.7)
    return np.clip(base[..., None] + rng.integers(-40, 41, (H, W, 3)), 0, 255).astype(np.uint8)


def planted(seed=0, T=7, hw=(48, 64), N=40, max_step=3):
    """A textured picture moved by integer offsets from frame to frame, with exact tracks: -> (frames uint8 [T,H,W,3]: frame f shows
    the picture `big` from offset off[f]; tracks float32 [T,N,2], every point visible and inside on every frame; off int [T,2] as
    (x, y)).  A scene point at p on frame 0 is at p - (off[f] - off[0]) on frame f: the motion of frame f - 1 to f is the integer
    translation off[f - 1] - off[f]."""
    rng = np.random.default_rng(seed)
    H, W = hw
    pad = max_step * T
    big = texture(seed, H + 2 * pad, W + 2 * pad)
    off = np.concatenate([[[0, 0]], np.cumsum(rng.integers(-max_step, max_step + 1, (T - 1, 2)), axis=0)]) + pad
    frames = np.stack([big[oy:oy + H, ox:ox + W] for ox, oy in off])
    p0 = rng.uniform([pad, pad], [W - 1 - pad, H - 1 - pad], size=(N, 2)).round()
    tracks = (p0[None] - (off - off[0])[:, None, :]).astype(np.float32)
    return frames, tracks, off
