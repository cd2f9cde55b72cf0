"""The stream-state kernels (include/ctk.h, "stream state step" through "health") restated in numpy: no torch, no library.

Every function works on numpy arrays laid out as the header lays out the device buffers, takes a `ring` switch, and returns NEW
arrays for everything the call may write (the inputs are left alone): a caller that compares every buffer bit for bit takes the
returned arrays for the written buffers and its own inputs for the rest.  What a function does not write keeps the bytes it was given
-- arrays are copied, never recomputed, so NaN payloads and random bytes pass through.

Float steps are single float32 numpy operations in the order the header states them: queries * float32(1 / stride), * float32(1 /
2^l), history * float32(1 / stride) on begin, * stride on commit, * (sx, sy) on emit.  The trilinear patch is the restatement
oracle/cotracker_oracle.py already has (get_track_feat; tests/test_gpu_corr_matrix.py checks ops.sample_support against it bit for
bit).  The visibility product sigmoid(vis) * sigmoid(conf) is formed in float64 and handed back beside the decision: the device forms
it with expf and three float32 roundings, which move it by parts in 10^7, so a test states how far its inputs lie from the threshold
(tests/test_stream_reference_host.py) instead of widening a comparison.

Query frames: qframe() truncates toward zero as torch's .long(); a frame that is NaN or outside [-2^31, 2^31) matches no window
(NO_FRAME, beyond every ind + S)."""
import numpy as np

from oracle import cotracker_oracle as O

f32 = np.float32
LEVELS, TAPS, CH = 4, 49, 128
EMPTY_FRAME = f32(2 ** 30)  # CTK_STREAM_EMPTY_FRAME
NO_FRAME = 1 << 62          # what a NaN / out-of-range query frame reads as
BIG = 2 ** 31 - 1           # INT32_MAX: the first_row of an empty slot
_FAR = f32(1e4)             # a level coordinate whose every lattice tap is clamped to the border it lies beyond


def qframe(q0):
    """float32 query frames -> int64 frame numbers: truncation toward zero; NaN or outside [-2^31, 2^31) -> NO_FRAME."""
    q0 = np.asarray(q0, f32)
    with np.errstate(invalid="ignore"):
        ok = (q0 >= f32(-2.0 ** 31)) & (q0 < f32(2.0 ** 31))
    out = np.full(q0.shape, NO_FRAME, np.int64)
    out[ok] = np.trunc(q0[ok]).astype(np.int64)
    return out


def row_of(frame, R, ring):
    """The history row of a frame: f % R in a ring of R rows, f in a linear history."""
    return frame % R if ring else frame


def inv_stride(stride):
    return f32(1.0 / stride)


# ---- begin ------------------------------------------------------------------------------------------------------------------------
def begin(ring, G, N, S, step, ind, R, stride, queries, hc, hv, hf):
    """-> (coords [G,S,N,2], vis [G,S,N], conf [G,S,N], point_mask [G*N] uint8): every element of the four is written."""
    inv = inv_stride(stride)
    q = np.asarray(queries, f32).reshape(G, N, 3)
    qf = qframe(q[..., 0])
    overlap = S - step
    with np.errstate(all="ignore"):
        fresh = (q[..., 1:3] * inv).astype(f32)
    coords = np.repeat(fresh[:, None], S, axis=1)
    vis, conf = np.zeros((G, S, N), f32), np.zeros((G, S, N), f32)
    if ind > 0:
        carry = qf < ind + overlap
        for t in range(S):
            r = row_of(ind + min(t, overlap - 1), R, ring)
            with np.errstate(all="ignore"):
                c = (hc[:, r] * inv).astype(f32)
            coords[:, t][carry] = c[carry]
            vis[:, t][carry] = hv[:, r][carry]
            conf[:, t][carry] = hf[:, r][carry]
    return coords, vis, conf, (qf < ind + S).astype(np.uint8).reshape(G * N)


# ---- support ----------------------------------------------------------------------------------------------------------------------
def level_xy(xy, stride, l):
    """(x, y) pixels -> level-l feature units, two float32 multiplications.  A NaN or infinite coordinate is then put where the
    sampler's clamp puts it (ctk_tap: fmaxf drops a NaN, so NaN and -inf end on the low border, +inf on the high one): far outside
    on that side, finite, so that the shared patch restatement can take it."""
    with np.errstate(all="ignore"):
        c = (np.asarray(xy, f32) * inv_stride(stride)).astype(f32)
        c = (c * f32(1.0 / 2 ** l)).astype(f32)
    c = np.where(np.isnan(c) | np.isneginf(c), -_FAR, c)
    return np.where(np.isposinf(c), _FAR, c).astype(f32)


def patch(fmap, z, xy):
    """fmap [S,H,W,128] (the layout of the device pyramid), z [n] integer frame rows, xy [n,2] level units -> [n,49,128]."""
    nchw = np.ascontiguousarray(np.asarray(fmap, f32).transpose(0, 3, 1, 2))[None]
    out = O.get_track_feat(nchw, np.asarray(z, f32)[None], np.asarray(xy, f32)[None])  # [1,49,n,128]
    return np.ascontiguousarray(out[0].transpose(1, 0, 2))


def support(ring, G, N, S, step, ind, stride, queries, fmaps, acc):
    """-> acc' (a list of [G*N,49,128] per level).  Only the rows of points with left <= qframe < right change.  (The ring form
    touches no history: the switch is taken for symmetry.)"""
    q = np.asarray(queries, f32).reshape(G * N, 3)
    qf = qframe(q[:, 0])
    left, right = (0 if ind == 0 else ind + step), ind + S
    hit = np.nonzero((qf >= left) & (qf < right))[0]
    out = [a.copy() for a in acc]
    if len(hit):
        for l in range(LEVELS):
            s = patch(fmaps[l], qf[hit] - ind, level_xy(q[hit, 1:3], stride, l))
            out[l][hit] = (out[l][hit] + s).astype(f32)
    return out


# ---- commit -----------------------------------------------------------------------------------------------------------------------
def commit(ring, G, N, S, ind, T_valid, R, stride, coords, vis, conf, hc, hv, hf, flag=None):
    """-> (hist_coords, hist_vis, hist_conf, flag'): rows of frames ind .. ind + T_valid - 1; flag' = flag | 1 when a committed value
    is not finite (None stays None)."""
    hc, hv, hf = hc.copy(), hv.copy(), hf.copy()
    bad = False
    for t in range(T_valid):
        r = row_of(ind + t, R, ring)
        with np.errstate(all="ignore"):
            hc[:, r] = (coords[:, t] * f32(stride)).astype(f32)
        hv[:, r], hf[:, r] = vis[:, t], conf[:, t]
        bad = bad or not (np.isfinite(hc[:, r]).all() and np.isfinite(hv[:, r]).all() and np.isfinite(hf[:, r]).all())
    return hc, hv, hf, (None if flag is None else int(flag) | int(bad))


# ---- assign and resident assign -----------------------------------------------------------------------------------------------------
def assign(ring, G, N, R, rows, slots, newq, queries, acc, hc, hv, hf):
    """-> (queries, acc, hist_coords, hist_vis, hist_conf).  ring: all R rows of a listed slot are cleared, `rows` is not read."""
    return _assign(ring, G, N, R, rows, slots, newq, queries, acc, hc, hv, hf, None)


def assign_resident(ring, G, N, S, step, ind, R, rows, stride, fmaps, slots, newq, queries, acc, hc, hv, hf):
    """`ind`: the first frame of the NEXT call's window; fmaps: the resident pyramid, frames [ind - step, ind - step + S)."""
    return _assign(ring, G, N, R, rows, slots, newq, queries, acc, hc, hv, hf, (S, step, ind, stride, fmaps))


def _assign(ring, G, N, R, rows, slots, newq, queries, acc, hc, hv, hf, res):
    queries = np.array(queries, f32).reshape(G * N, 3)
    acc = [a.copy() for a in acc]
    hc, hv, hf = hc.copy(), hv.copy(), hf.copy()
    newq = np.asarray(newq, f32).reshape(-1, 3)
    nrows = R if ring else rows
    for m, s in enumerate(int(s) for s in slots):
        if s < 0 or s >= G * N:
            continue  # a listed index outside the range writes nothing
        g, n = divmod(s, N)
        queries[s] = newq[m]
        hc[g, :nrows, n], hv[g, :nrows, n], hf[g, :nrows, n] = 0.0, 0.0, 0.0
        for l in range(LEVELS):
            acc[l][s] = 0.0
        if res is None:
            continue
        S, step, ind, stride, fmaps = res
        qf = int(qframe(newq[m, 0]))
        if not (ind - step <= qf < ind + (S - step)):
            continue  # not in the resident pyramid: exactly the plain assign
        for l in range(LEVELS):
            s_ = patch(fmaps[l], [qf - (ind - step)], level_xy(newq[m:m + 1, 1:3], stride, l))[0]
            acc[l][s] = (f32(0.0) + s_).astype(f32)
        for f in range(ind, ind + (S - step)):  # the rows the next begin carries over: (x, y) and zero logits
            r = row_of(f, R, ring)
            hc[g, r, n], hv[g, r, n], hf[g, r, n] = newq[m, 1:3], 0.0, 0.0
    return queries.reshape(-1), acc, hc, hv, hf


# ---- emit and health ----------------------------------------------------------------------------------------------------------------
def visible_product(v, c):
    """sigmoid(v) * sigmoid(c) in float64 from the float32 logits (NaN where a logit is NaN)."""
    with np.errstate(all="ignore"):
        sv = 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))
        sc = 1.0 / (1.0 + np.exp(-np.asarray(c, np.float64)))
        return sv * sc


def visible(v, c, thresh):
    """-> (decision, the float64 product beside it).  A NaN product is not visible."""
    p = visible_product(v, c)
    with np.errstate(invalid="ignore"):
        return p > np.float64(f32(thresh)), p


def emit(ring, G, N, N_out, R, f0, f1, sx, sy, thresh, hc, hv, hf, first_row=None):
    """-> (tracks [G,F,N_out,2], vis_logit, conf_logit [G,F,N_out], visible uint8 [G,F,N_out], product float64 [G,F,N_out])."""
    rows = np.array([row_of(f, R, ring) for f in range(f0, f1)])
    with np.errstate(all="ignore"):
        tracks = (hc[:, rows, :N_out] * np.array([sx, sy], f32)).astype(f32)
    v, c = hv[:, rows, :N_out].copy(), hf[:, rows, :N_out].copy()
    on, p = visible(v, c, thresh)
    if first_row is not None:
        on = on & (np.arange(f0, f1)[None, :, None] >= np.asarray(first_row).reshape(G, N)[:, None, :N_out])
    return tracks, v, c, on.astype(np.uint8), p


def health(ring, G, N, N_out, R, f1, look, ind_next, thresh, bounds, grid, queries, hc, hv, hf, first_row):
    """-> (lost [G,N_out] int32, cell [G,N_out] int32, cover [G,gh*gw] int32, product float64 [G,look,N_out] of frames
    [f1 - look, f1)).  inv_cw = float32(gw) / (x_hi - x_lo), inv_ch likewise, as the header asks of the caller."""
    gh, gw = grid
    x_lo, x_hi, y_lo, y_hi = (f32(b) for b in bounds)
    inv_cw, inv_ch = f32(f32(gw) / f32(x_hi - x_lo)), f32(f32(gh) / f32(y_hi - y_lo))
    q = np.asarray(queries, f32).reshape(G, N, 3)
    fr = np.asarray(first_row).reshape(G, N)
    qf = qframe(q[..., 0])
    rows = np.array([row_of(f, R, ring) for f in range(f1 - look, f1)])
    alive, p = visible(hv[:, rows, :N_out], hf[:, rows, :N_out], thresh)
    h = hc[:, rows, :N_out]
    x, y = h[..., 0], h[..., 1]

    def inside(x, y):
        with np.errstate(invalid="ignore"):
            return (x >= x_lo) & (x <= x_hi) & (y >= y_lo) & (y <= y_hi)

    def cell_of(x, y):
        cx = min(max(int(np.floor(f32(f32(x - x_lo) * inv_cw))), 0), gw - 1)
        cy = min(max(int(np.floor(f32(f32(y - y_lo) * inv_ch))), 0), gh - 1)
        return cy * gw + cx

    alive = alive & inside(x, y)
    lost = np.full((G, N_out), -1, np.int32)
    cell = np.full((G, N_out), -1, np.int32)
    for g in range(G):
        for n in range(N_out):
            if fr[g, n] == BIG or q[g, n, 0] == EMPTY_FRAME:
                continue  # an empty slot
            lost[g, n] = 0
            start = max(int(fr[g, n]), int(qf[g, n]))
            if fr[g, n] >= ind_next or start >= f1:  # pending: judged at its query position
                if inside(q[g, n, 1], q[g, n, 2]):
                    cell[g, n] = cell_of(q[g, n, 1], q[g, n, 2])
                continue
            for f in range(f1 - 1, max(f1 - look, start) - 1, -1):
                k = f - (f1 - look)
                if alive[g, k, n]:
                    if f == f1 - 1:
                        cell[g, n] = cell_of(x[g, k, n], y[g, k, n])
                    break
                lost[g, n] += 1
    cover = np.stack([np.bincount(c[c >= 0], minlength=gh * gw) for c in cell]).astype(np.int32)
    return lost, cell, cover, p
