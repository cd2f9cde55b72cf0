"""The drawing rules of ctk_draw_tracks (include/ctk.h, "draw tracks"; co-tracker_amd/csrc/draw_math.h) restated in numpy: plain loops
over the primitives in the stated order, each applied to the WHOLE picture -- no tiles, no bounding boxes, no lists.  Integers past the
quantisation of a position, int64 throughout: tests/test_draw_host.py holds a g++ build of the header against these functions and
tests/test_gpu_draw.py the kernels, both with array_equal."""
import numpy as np

INT32_MAX = 2 ** 31 - 1


def quant(x, s):
    """One component of a position -> (valid, pixel): one float32 multiplication, valid iff -65536 <= v <= 65536, rint (half to even)."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.float32(x) * np.float32(s)
    if not (v >= np.float32(-65536.0) and v <= np.float32(65536.0)):
        return False, 0
    return True, int(np.rint(v))


def visible_from_logits(vis, conf, thresh):
    """emit's expression in float32: sigmoid(vis) * sigmoid(conf) > thresh, sigmoid(x) = 1 / (1 + exp(-x)); a NaN is not visible."""
    vis, conf = np.asarray(vis, dtype=np.float32), np.asarray(conf, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s = lambda x: np.float32(1.0) / (np.float32(1.0) + np.exp(-x, dtype=np.float32))  # noqa: E731
        return (s(vis) * s(conf)) > np.float32(thresh)


def mark_mask(dx, dy, r, visible):
    """dx, dy: integer arrays of pixel offsets from the mark's centre -> covered."""
    d2 = dx.astype(np.int64) ** 2 + dy.astype(np.int64) ** 2
    disc = d2 <= r * r + r
    return disc if visible else disc & (d2 > (r - 1) * (r - 1) + (r - 1))


def segment_mask(px, py, dx, dy, hw):
    """px, py: integer arrays of pixel offsets from A; (dx, dy) = B - A -> covered."""
    px, py = px.astype(np.int64), py.astype(np.int64)
    dx, dy = int(dx), int(dy)
    w2, dd = hw * hw + hw, dx * dx + dy * dy
    t = px * dx + py * dy
    cross = px * dy - py * dx
    return np.where(t <= 0, px * px + py * py <= w2, np.where(t >= dd, (px - dx) ** 2 + (py - dy) ** 2 <= w2, cross * cross <= w2 * dd))


def blend(v, c, a):
    return (v.astype(np.int64) * (255 - a) + int(c) * a + 127) // 255


def default_alpha(trail):
    """alpha[0] = 255, alpha[k] = 255 * (L + 1 - k)^2 // (L + 1)^2: the quadratic fade."""
    a = np.zeros(65, dtype=np.uint8)
    a[0] = 255
    for k in range(1, trail + 1):
        a[k] = 255 * (trail + 1 - k) ** 2 // (trail + 1) ** 2
    return a


def draw(frames, tracks, visible, colors, f0=0, trail=0, alpha=None, radius=4, half_width=1, max_jump=256, sx=1.0, sy=1.0,
         first_row=None, N_out=None):
    """frames uint8 [F,H,W,3]; tracks float32 [G,R,N,2], visible [G,R,N] (the row of frame f is f % R); colors uint8 [G,N,3];
    first_row [G,N] or None -> the pictures, a new array."""
    out = np.array(frames, dtype=np.uint8, copy=True)
    F, H, W, _ = out.shape
    tracks, visible = np.asarray(tracks, dtype=np.float32), np.asarray(visible)
    G, R, N, _ = tracks.shape
    N_out = N if N_out is None else N_out
    alpha = default_alpha(trail) if alpha is None else np.asarray(alpha)
    yy, xx = np.mgrid[:H, :W]

    def point(g, n, f):
        """-> (shown, visible, qx, qy)"""
        if f < 0 or (first_row is not None and f < int(first_row[g, n])):
            return False, False, 0, 0
        okx, qx = quant(tracks[g, f % R, n, 0], sx)
        oky, qy = quant(tracks[g, f % R, n, 1], sy)
        if not (okx and oky):
            return False, False, 0, 0
        return True, bool(visible[g, f % R, n]), qx, qy

    def apply(pic, mask, g, n, k):
        a = int(alpha[k])
        for c in range(3):
            ch = pic[:, :, c]
            ch[mask] = blend(ch[mask], colors[g, n, c], a)

    for j in range(F):
        f, pic = f0 + j, out[j]
        for k in range(trail, 0, -1):
            for g in range(G):
                for n in range(N_out):
                    sa, va, ax, ay = point(g, n, f - k)
                    sb, vb, bx, by = point(g, n, f - k + 1)
                    if not (sa and va and sb and vb) or abs(bx - ax) > max_jump or abs(by - ay) > max_jump:
                        continue
                    apply(pic, segment_mask(xx - ax, yy - ay, bx - ax, by - ay, half_width), g, n, k)
        for g in range(G):
            for n in range(N_out):
                shown, vis, qx, qy = point(g, n, f)
                if shown:
                    apply(pic, mark_mask(xx - qx, yy - qy, radius, vis), g, n, 0)
    return out
