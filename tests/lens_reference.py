"""The rules of ctk_lens_frames and ctk_lens_points (include/ctk.h, "lens"; co-tracker_amd/csrc/lens_math.h) restated in numpy, step for
step from the header: one float64 operation per assignment in the header's order, integer taps and int32 blends -- the kernels, the g++
build of the header and this file agree on every byte and on every float32 bit.  Also the lenses the tests share."""
import numpy as np

TO_IDEAL, TO_SENSOR = 0, 1
FILL, EDGE = 0, 1
HWC, CHW = 0, 1
ROUNDS = 8
REACH = 32768.0
NAN_BITS = 0x7FC00000

# (k1, k2, p1, p2, k3), focal length: from a mild barrel to a strong pincushion; ACTION is the ordinary action-camera lens
LENSES = {
    "mild": ((-0.1, 0.02, 5e-4, -5e-4, 0.0), 1400.0),
    "mixed": ((0.12, -0.25, 1e-3, 1e-3, 0.1), 1500.0),
    "action900": ((-0.28, 0.09, 1e-3, -8e-4, -0.013), 900.0),
    "action": ((-0.28, 0.09, 1e-3, -8e-4, -0.013), 1000.0),
    "pincushion": ((0.2, 0.05, 0.0, 0.0, 0.0), 1000.0),
}
FOLDING = ((-0.35, 0.15, 0.0, 0.0, -0.03), 800.0)  # det < 0 in the corners of a 1080p field: no inverse there
ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)


def lens13(k, f, centre=(959.5, 539.5), ideal=None):
    """-> float64 [13]: sensor (f, f, cx, cy), ideal (default: the sensor's), k."""
    sensor = (float(f), float(f), float(centre[0]), float(centre[1]))
    return np.array(sensor + tuple(sensor if ideal is None else ideal) + tuple(k), dtype=np.float64)


def valid(lens):
    lens = np.asarray(lens, dtype=np.float64).reshape(13)
    with np.errstate(invalid="ignore"):
        ok = all(1.0 <= lens[i] <= 1e6 for i in (0, 1, 4, 5)) and all(abs(lens[i]) <= REACH for i in (2, 3, 6, 7))
        return bool(ok and (np.abs(lens[8:]) <= 64.0).all())


def _f64(*a):
    return [np.asarray(v, dtype=np.float64) for v in a]


def forward(k, x, y):
    """-> (xd, yd, (a, b, d, det)): forward and its jacobian, float64 arrays."""
    with np.errstate(all="ignore"):  # (what is no position stays none: NaN and infinity go through)
        return _forward(k, *_f64(x, y))


def _forward(k, x, y):
    k1, k2, p1, p2, k3 = (np.float64(v) for v in k)
    two, three, six, one = np.float64(2.0), np.float64(3.0), np.float64(6.0), np.float64(1.0)
    xx, yy = x * x, y * y
    r2 = xx + yy
    xy = x * y
    txy = two * xy
    t = r2 * k3
    t = k2 + t
    t = r2 * t
    t = k1 + t
    t = r2 * t
    rad = one + t
    txx, tyy = two * xx, two * yy
    x1, x2 = x * rad, p1 * txy
    x3 = r2 + txx
    x3 = p2 * x3
    xd = (x1 + x2) + x3
    y1, y3 = y * rad, p2 * txy
    y2 = r2 + tyy
    y2 = p1 * y2
    yd = (y1 + y2) + y3
    u = k3 * r2
    u = three * u
    v = two * k2
    u = v + u
    u = r2 * u
    dr = k1 + u
    tp1, tp2, sp1, sp2 = two * p1, two * p2, six * p1, six * p2
    a = ((rad + txx * dr) + tp1 * y) + sp2 * x
    b = ((txy * dr) + tp1 * x) + tp2 * y
    d = ((rad + tyy * dr) + sp1 * y) + tp2 * x
    det = a * d - b * b
    return xd, yd, (a, b, d, det)


def jacobian(k, x, y):
    return forward(k, x, y)[2]


def inverse(k, fx, fy, tol, xd, yd, rounds=ROUNDS):
    """Newton from (xd, yd), always `rounds` rounds -> (x, y, accepted)."""
    xd, yd = _f64(xd, yd)
    tol2 = np.float64(np.float32(tol)) * np.float64(np.float32(tol))
    fx, fy = np.float64(fx), np.float64(fy)
    x, y = xd.copy(), yd.copy()
    with np.errstate(all="ignore"):
        for _ in range(rounds):
            fxd, fyd, (a, b, d, det) = forward(k, x, y)
            ex, ey = xd - fxd, yd - fyd
            idet = np.float64(1.0) / det
            sx, sy = d * ex - b * ey, a * ey - b * ex
            x, y = x + sx * idet, y + sy * idet
        fxd, fyd, (a, b, d, det) = forward(k, x, y)
        ex, ey = xd - fxd, yd - fyd
        rx, ry = fx * ex, fy * ey
        e = rx * rx + ry * ry
        return x, y, (det > 0.0) & (e <= tol2)


def lens_map(lens, direction, tol, px, py):
    """The map of the POINT rule `direction` on float64 pixel positions -> (qx, qy, ok)."""
    lens = np.asarray(lens, dtype=np.float64).reshape(13)
    cin, cout = (lens[0:4], lens[4:8]) if direction == TO_IDEAL else (lens[4:8], lens[0:4])
    k = lens[8:]
    px, py = _f64(px, py)
    ifx, ify = np.float64(1.0) / cin[0], np.float64(1.0) / cin[1]
    with np.errstate(all="ignore"):
        xn, yn = (px - cin[2]) * ifx, (py - cin[3]) * ify
        if direction == TO_IDEAL:
            x, y, ok = inverse(k, cin[0], cin[1], tol, xn, yn)
        else:
            x, y, (_, _, _, det) = forward(k, xn, yn)
            ok = det > 0.0
        return cout[0] * x + cout[2], cout[1] * y + cout[3], ok


def within(px, py):
    with np.errstate(invalid="ignore"):
        return (np.abs(px) <= REACH) & (np.abs(py) <= REACH)


def lens_points(src, lens, direction=TO_IDEAL, tol=0.01):
    """src float32 [...,2] -> (dst float32 [...,2] with NaN = 0x7FC00000 where the label is not 1, label int8 [...])."""
    src = np.asarray(src, dtype=np.float32)
    px, py = src[..., 0].astype(np.float64), src[..., 1].astype(np.float64)
    inb = within(px, py)
    qx, qy, ok = lens_map(lens, direction, tol, np.where(inb, px, 0.0), np.where(inb, py, 0.0))
    label = np.where(inb, np.where(ok, 1, 0), -1).astype(np.int8)
    with np.errstate(all="ignore"):
        out = np.stack([qx, qy], axis=-1).astype(np.float32)
    bits = out.view(np.uint32).copy()
    bits[label != 1] = NAN_BITS
    return bits.view(np.float32), label


def source_positions(lens, direction, tol, Ho, Wo):
    """The picture rule's coordinate for every output pixel -> (inside bool [Ho,Wo], qx, qy float64 [Ho,Wo])."""
    x, y = np.meshgrid(np.arange(Wo, dtype=np.float64), np.arange(Ho, dtype=np.float64))
    qx, qy, ok = lens_map(lens, TO_SENSOR if direction == TO_IDEAL else TO_IDEAL, tol, x, y)
    return ok & within(qx, qy), qx, qy


def lens_frames(src, lens, direction=TO_IDEAL, size=None, border=FILL, fill=(0, 0, 0), tol=0.01, layout=HWC):
    """src uint8 [F,H,W,3] (HWC) or [F,3,H,W] (CHW) -> the resampled pictures [F,Ho,Wo,3] / [F,3,Ho,Wo]; size = (Ho, Wo)."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 4
    hwc = src if layout == HWC else src.transpose(0, 2, 3, 1)
    _, H, W, _ = hwc.shape
    Ho, Wo = (H, W) if size is None else size
    inside, qx, qy = source_positions(lens, direction, tol, Ho, Wo)
    with np.errstate(all="ignore"):
        X = np.rint(np.where(inside, qx, 0.0) * 256.0).astype(np.int64)
        Y = np.rint(np.where(inside, qy, 0.0) * 256.0).astype(np.int64)
    ix, iy = X >> 8, Y >> 8
    fx, fy = (X & 255).astype(np.int32)[None, ..., None], (Y & 255).astype(np.int32)[None, ..., None]
    fv = np.asarray(fill, dtype=np.int32).reshape(-1)[:3]

    def tap(tx, ty):
        cx, cy = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)  # (nothing outside the picture is read)
        v = hwc[:, cy, cx].astype(np.int32)
        if border == FILL:
            v = np.where(((cx == tx) & (cy == ty))[None, ..., None], v, fv)
        return v
    p00, p01, p10, p11 = tap(ix, iy), tap(ix + 1, iy), tap(ix, iy + 1), tap(ix + 1, iy + 1)
    gx, gy = 256 - fx, 256 - fy
    out = (gx * gy * p00 + fx * gy * p01 + gx * fy * p10 + fx * fy * p11 + 32768) >> 16
    assert out.dtype == np.int32 and out.min() >= 0 and out.max() <= 255
    out = np.where(inside[None, ..., None], out, fv).astype(np.uint8)
    return np.ascontiguousarray(out if layout == HWC else out.transpose(0, 3, 1, 2))


def exact_frames(src_hwc, lens, direction, Ho, Wo, border, fill, tol=0.01):
    """The unrounded float64 bilinear value at the exact (float64) source position, for the accuracy bound -> (value float64
    [F,Ho,Wo,3], inside bool [Ho,Wo])."""
    src_hwc = np.asarray(src_hwc)
    _, H, W, _ = src_hwc.shape
    inside, qx, qy = source_positions(lens, direction, tol, Ho, Wo)
    qx, qy = np.where(inside, qx, 0.0), np.where(inside, qy, 0.0)
    ix, iy = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
    wx, wy = (qx - ix)[None, ..., None], (qy - iy)[None, ..., None]
    fv = np.asarray(fill, dtype=np.float64).reshape(-1)[:3]

    def tap(tx, ty):
        cx, cy = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
        v = src_hwc[:, cy, cx].astype(np.float64)
        if border == FILL:
            v = np.where(((cx == tx) & (cy == ty))[None, ..., None], v, fv)
        return v
    out = (1 - wx) * (1 - wy) * tap(ix, iy) + wx * (1 - wy) * tap(ix + 1, iy) + (1 - wx) * wy * tap(ix, iy + 1) + wx * wy * tap(ix + 1, iy + 1)
    return np.where(inside[None, ..., None], out, fv), inside


def distort_pixels(P, k, cam):
    """float64 pixels of the pinhole camera cam = (fx, fy, cx, cy) -> the pixels the same camera with the lens k sees (plain float64,
    for planting scenes)."""
    P = np.asarray(P, dtype=np.float64)
    xd, yd, _ = forward(k, (P[:, 0] - cam[2]) / cam[0], (P[:, 1] - cam[3]) / cam[1])
    return np.stack([cam[0] * xd + cam[2], cam[1] * yd + cam[3]], axis=1)
