"""The rules of ctk_fit_planes and ctk_warp_planes (include/ctk.h, "fit planes / warp planes"; co-tracker_amd/csrc/plane_math.h) restated in
numpy and Python numbers: what the kernels (tests/test_gpu_planes.py) and the g++ build of the header (tests/test_planes_host.py) are
compared with, exactly.  Positions, mix, the pair rule, the seed of a round and the labels are motion_reference's and
objects_reference's; the taps and the blend are warp_reference's.  Admissibility is Python integers; everything in double is one
float64 operation per step in the header's order (Python floats and numpy float64 round every operation on its own)."""
import math

import numpy as np

import motion_reference as R
import objects_reference as O
import warp_reference as WR

NONE = O.NONE
IDENTITY = np.eye(3, dtype=np.float32).reshape(9)
NO_BOX = O.NO_BOX
FILL, EDGE, KEEP = 0, 1, 2
HWC, CHW = 0, 1
FIX, UNFIX = 2.0 ** 44, 2.0 ** -44
REACH = 1048576.0


# ---- fit ------------------------------------------------------------------------------------------------------------------------------
def sample(seed, f, k, M):
    base = (f * 0x9e3779b9 + 4 * k) & 0xffffffff
    taken = []
    for t in range(4):
        v = R.mix(seed ^ R.mix((base + t) & 0xffffffff)) % (M - t)
        for e in sorted(taken):
            v += 1 if v >= e else 0
        taken.append(v)
    return taken


def cross(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def dets(p):
    return [cross(p[1], p[2], p[3]), cross(p[0], p[2], p[3]), cross(p[0], p[1], p[3]), cross(p[0], p[1], p[2])]


def basis(p, d):
    l = [float(d[1]), float(-d[2]), float(d[3])]
    B = [[0.0] * 3 for _ in range(3)]
    for c in range(3):
        B[0][c] = l[c] * float(p[c + 1][0])
        B[1][c] = l[c] * float(p[c + 1][1])
        B[2][c] = l[c] * 1.0
    return B


def div(a, b):
    """IEEE division of two floats, the cases Python raises on included."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def hypothesis(P4, Q4, b2):
    """P4, Q4: four sample points as Python integer pairs -> (admissible, h: nine floats, centred, 1/16 pixel)."""
    p = [(P4[t][0] - P4[0][0], P4[t][1] - P4[0][1]) for t in range(4)]
    q = [(Q4[t][0] - Q4[0][0], Q4[t][1] - Q4[0][1]) for t in range(4)]
    d, e = dets(p), dets(q)
    for v in d + e:
        assert abs(v) <= 2 ** 37
    if not all(abs(a) >= b2 and abs(a) >= 1 and abs(b) >= b2 and abs(b) >= 1 and (a > 0) == (b > 0) for a, b in zip(d, e)):
        return False, None
    BP, BQ = basis(p, d), basis(q, e)
    with np.errstate(all="ignore"):
        BP, BQ = np.array(BP, dtype=np.float64), np.array(BQ, dtype=np.float64)
        A = np.zeros((3, 3), dtype=np.float64)
        for i in range(3):
            for j in range(3):
                j1, j2, i1, i2 = (j + 1) % 3, (j + 2) % 3, (i + 1) % 3, (i + 2) % 3
                t1, t2 = BP[j1, i1] * BP[j2, i2], BP[j1, i2] * BP[j2, i1]
                A[i, j] = t1 - t2
        H = np.zeros((3, 3), dtype=np.float64)
        for i in range(3):
            for j in range(3):
                t0, t1, t2 = BQ[i, 0] * A[0, j], BQ[i, 1] * A[1, j], BQ[i, 2] * A[2, j]
                H[i, j] = (t0 + t1) + t2
        h = (H / H[2, 2]).reshape(9)
    return bool(np.isfinite(h).all()), h


def inliers(h, P0, Q0, P, Q, T):
    """h float64 [9]; P0, Q0 the anchor pair; P, Q int64 [M,2] -> bool [M]."""
    u, w = (P - P0).astype(np.float64), (Q - Q0).astype(np.float64)
    with np.errstate(all="ignore"):
        X = (h[0] * u[:, 0] + h[1] * u[:, 1]) + h[2]
        Y = (h[3] * u[:, 0] + h[4] * u[:, 1]) + h[5]
        Z = (h[6] * u[:, 0] + h[7] * u[:, 1]) + h[8]
        TZ = float(T) * Z
        rx, ry = X - w[:, 0] * Z, Y - w[:, 1] * Z
        return (Z > 0) & (np.abs(rx) <= TZ) & (np.abs(ry) <= TZ)


SUMS = 23


def terms(u, w, e):
    """u, w int64 [n,2] of the inliers -> the 23 sums as Python integers."""
    sc = 2.0 ** -e
    x, y, U, V = u[:, 0] * sc, u[:, 1] * sc, w[:, 0] * sc, w[:, 1] * sc
    xx, xy, yy = x * x, x * y, y * y
    Rr = U * U + V * V
    cols = [np.ones_like(x), x, y, xx, xy, yy, U, V, x * U, y * U, x * V, y * V, xx * U, xy * U, yy * U, xx * V, xy * V, yy * V,
            xx * Rr, xy * Rr, yy * Rr, x * Rr, y * Rr]
    out = []
    for c in cols:
        assert float(np.abs(c).max()) <= 2.0
        out.append(int(np.rint(c * FIX).astype(np.int64).sum()))
        assert abs(out[-1]) < 2 ** 59
    return out


def system(s):
    S = [float(v) * UNFIX for v in s]
    (n, x, y, xx, xy, yy, U, V, xU, yU, xV, yV, xxU, xyU, yyU, xxV, xyV, yyV, xxR, xyR, yyR, xR, yR) = S
    N = [[0.0] * 8 for _ in range(8)]
    for o in (0, 3):
        N[o][o], N[o][o + 1], N[o][o + 2] = xx, xy, x
        N[o + 1][o + 1], N[o + 1][o + 2] = yy, y
        N[o + 2][o + 2] = n
    N[0][6], N[0][7], N[1][6], N[1][7], N[2][6], N[2][7] = -xxU, -xyU, -xyU, -yyU, -xU, -yU
    N[3][6], N[3][7], N[4][6], N[4][7], N[5][6], N[5][7] = -xxV, -xyV, -xyV, -yyV, -xV, -yV
    N[6][6], N[6][7], N[7][7] = xxR, xyR, yyR
    for i in range(8):
        for j in range(i):
            N[i][j] = N[j][i]
    return N, [xU, yU, U, xV, yV, V, -xR, -yR]


def solve(N, b):
    """N h = b by N = L D L^T in the header's loop order -> the eight values, or None (the fall-back)."""
    L = [[0.0] * 8 for _ in range(8)]
    D, v, z, h = [0.0] * 8, [0.0] * 8, [0.0] * 8, [0.0] * 8
    for j in range(8):
        for k in range(j):
            v[k] = L[j][k] * D[k]
        d = N[j][j]
        for k in range(j):
            d = d - L[j][k] * v[k]
        if not (d > 0.0) or not math.isfinite(d):
            return None
        D[j] = d
        for i in range(j + 1, 8):
            s = N[i][j]
            for k in range(j):
                s = s - L[i][k] * v[k]
            L[i][j] = div(s, d)
    for i in range(8):
        s = b[i]
        for k in range(i):
            s = s - L[i][k] * z[k]
        z[i] = s
    for i in range(7, -1, -1):
        s = div(z[i], D[i])
        for k in range(i + 1, 8):
            s = s - L[k][i] * h[k]
        h[i] = s
    return h if all(math.isfinite(x) for x in h) else None


def pixels(hc, e, P0, Q0):
    """A centred matrix (nine floats) whose coordinates are 2^e / 16 pixel -> float32 [9] in pixels."""
    sig, isig = 2.0 ** (4 - e), 2.0 ** (e - 4)
    cx, cy, kx, ky = P0[0] / 16.0, P0[1] / 16.0, Q0[0] / 16.0, Q0[1] / 16.0
    with np.errstate(all="ignore"):
        hc = np.asarray(hc, dtype=np.float64)
        G = np.array([[hc[0], hc[1], hc[2] * isig], [hc[3], hc[4], hc[5] * isig], [hc[6] * sig, hc[7] * sig, hc[8]]])
        M = G.copy()
        for r in range(3):
            M[r, 2] = G[r, 2] - (G[r, 0] * cx + G[r, 1] * cy)
        out = M.copy()
        out[0] = M[0] + kx * M[2]
        out[1] = M[1] + ky * M[2]
        return out.reshape(9).astype(np.float32)


def fit_list(P, Q, f, T, b2, K, seed, min_points, details=None):
    """One round over P, Q int64 [M,2] -> (matrix float32 [9], inlier bool [M], (M, inliers, best k, fell back) or (M, 0, -1, 0))."""
    M = P.shape[0]
    none = (IDENTITY.copy(), np.zeros(M, dtype=bool), (M, 0, -1, 0))
    if M < 4:
        return none
    assert int(np.abs(P).max()) <= 2 ** 17 and int(np.abs(Q).max()) <= 2 ** 17
    Pl, Ql = P.tolist(), Q.tolist()
    best, kept = -1, None
    for k in range(K):
        i = sample(seed, f, k, M)
        assert len(set(i)) == 4 and 0 <= min(i) and max(i) < M
        ok, h = hypothesis([Pl[t] for t in i], [Ql[t] for t in i], b2)
        if not ok:
            continue
        inl = inliers(h, P[i[0]], Q[i[0]], P, Q, T)
        key = (int(inl.sum()) << 32) | (K - 1 - k)
        if key > best:
            best, kept = key, (k, h, i[0], inl)
    if best < 0 or (best >> 32) < min_points:
        return none
    k, h, i0, inl = kept
    u, w = (P - P[i0])[inl], (Q - Q[i0])[inl]
    e = max(int(max(np.abs(u).max(), np.abs(w).max())).bit_length(), 1)
    N, b = system(terms(u, w, e))
    sol = solve(N, b)
    if details is not None:
        details.update(N=np.array(N), e=e, i0=i0)
    if sol is None:
        return pixels(h, 0, Pl[i0], Ql[i0]), inl, (M, int(inl.sum()), k, 1)
    return pixels(sol + [1.0], e, Pl[i0], Ql[i0]), inl, (M, int(inl.sum()), k, 0)


def fit_planes(coords, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1, to=None, lag=None,
               anchor=None, labels=None, L=1, inverse=0, min_points=8, tol=2.0, K=128, min_base=16.0, seed=0, scale=(1.0, 1.0)):
    """coords float32 [G,R,N,2]; visible [G,R,N] (or the logits vis, conf and thresh); first_row int [G,N] or None; exactly one of
    to (a frame), lag (>= 1) and anchor = (coords float32 [G,N,2], visible [G,N], frame); labels int8 [G,N] or None (then L = 1) ->
    (homography float32 [G,F,L,3,3], label int8 [G,F,N_out], stats int32 [G,F,L,4], box int32 [G,F,L,4])."""
    coords = np.asarray(coords, dtype=np.float32)
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    assert (to is not None) + (lag is not None) + (anchor is not None) == 1 and (lag is None or lag >= 1) and (to is None or to >= 0)
    assert 1 <= L <= 16 and 1 <= min_points <= 8192 and inverse in (0, 1) and (labels is not None or L == 1)
    T, b2 = R.tol_steps(tol), R.base2(min_base)
    assert T > 0 and b2 >= 0

    def positions(c):
        okx, px = R.quant(c[..., 0], scale[0])
        oky, py = R.quant(c[..., 1], scale[1])
        return okx & oky, np.stack([px, py], axis=-1)
    ok, pos = positions(coords)
    seen = np.asarray(visible) != 0 if visible is not None else R.visible_from_logits(vis, conf, thresh)
    good = ok & seen
    if anchor is not None:
        a_ok, a_pos = positions(np.asarray(anchor[0], dtype=np.float32))
        a_good = a_ok & (np.asarray(anchor[1]) != 0)
    homography = np.tile(IDENTITY, (G, F, L, 1))
    label = np.full((G, F, N_out), -1, dtype=np.int8)
    stats, box = np.zeros((G, F, L, 4), dtype=np.int32), np.zeros((G, F, L, 4), dtype=np.int32)
    for g in range(G):
        first = np.zeros(N, dtype=np.int64) if first_row is None else np.asarray(first_row[g], dtype=np.int64)
        for jf in range(F):
            f = f0 + jf
            fs = anchor[2] if anchor is not None else (to if to is not None else f - lag)
            corr = np.zeros(N_out, dtype=bool)
            src = pos[g, 0]
            if fs >= 0:
                src, src_good = (a_pos[g], a_good[g]) if anchor is not None else (pos[g, fs % R_], good[g, fs % R_])
                corr = src_good[:N_out] & good[g, f % R_, :N_out] & (fs >= first[:N_out]) & (f >= first[:N_out])
            idx = np.nonzero(corr)[0]
            here = pos[g, f % R_][idx]
            P, Q = (here, src[idx]) if inverse else (src[idx], here)
            lab = np.zeros(len(idx), dtype=np.int64) if labels is None else np.asarray(labels[g], dtype=np.int64)[idx]
            label[g, jf, idx] = NONE
            for r in range(L):
                sub = np.nonzero(lab == r)[0]
                m9, inl, st = fit_list(P[sub], Q[sub], f, T, b2, K, O.seed_of(seed, r), min_points)
                homography[g, jf, r], stats[g, jf, r], box[g, jf, r] = m9, st, NO_BOX
                if st[2] >= 0:
                    took = sub[inl]
                    label[g, jf, idx[took]] = r
                    box[g, jf, r] = (here[took, 0].min(), here[took, 1].min(), here[took, 0].max(), here[took, 1].max())
    return homography.reshape(G, F, L, 3, 3), label, stats, box


# ---- warp -----------------------------------------------------------------------------------------------------------------------------
def coordinates(m, H, W):
    """float32 matrix [3,3] over an H x W output -> (inside bool [H,W], X, Y int64 [H,W] in 1/256 pixel; 0 where outside)."""
    m32 = np.asarray(m, dtype=np.float32).reshape(9)
    md = m32.astype(np.float64)
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        Xh = (md[0] * x + md[1] * y) + md[2]
        Yh = (md[3] * x + md[4] * y) + md[5]
        Zh = (md[6] * x + md[7] * y) + md[8]
        r = 1.0 / Zh
        sx, sy = Xh * r, Yh * r
        inside = (Zh > 0) & (np.abs(sx) <= REACH) & (np.abs(sy) <= REACH) & bool(np.isfinite(m32).all())
        X = np.rint(np.where(inside, sx, 0.0) * 256.0).astype(np.int64)
        Y = np.rint(np.where(inside, sy, 0.0) * 256.0).astype(np.int64)
    return np.broadcast_to(inside, (H, W)).copy(), X, Y


def warp_picture(src, m, dst, border, fill):
    """src uint8 [Hs,Ws,C], dst uint8 [H,W,C] (what is there before) -> [H,W,C]."""
    Hs, Ws, C = src.shape
    H, W, _ = dst.shape
    inside, X, Y = coordinates(m, H, W)
    ix, iy = X >> 8, Y >> 8
    fx, fy = (X & 255).astype(np.int32)[..., None], (Y & 255).astype(np.int32)[..., None]
    fv = np.asarray(fill, dtype=np.int32).reshape(-1)[:C]
    whole = np.ones((H, W), dtype=bool)

    def tap(tx, ty):
        cx, cy = np.clip(tx, 0, Ws - 1), np.clip(ty, 0, Hs - 1)  # (nothing outside the source is read)
        v = src[cy, cx].astype(np.int32)
        within = (cx == tx) & (cy == ty)
        whole[...] &= within
        if border == FILL:
            v = np.where(within[..., None], v, fv)
        return v
    p00, p01, p10, p11 = tap(ix, iy), tap(ix + 1, iy), tap(ix, iy + 1), tap(ix + 1, iy + 1)
    out = WR_blend(fx, fy, p00, p01, p10, p11)
    if border == KEEP:
        return np.where((inside & whole)[..., None], out, dst)
    return np.where(inside[..., None], out, fv.astype(np.uint8))


def WR_blend(fx, fy, p00, p01, p10, p11):
    gx, gy = 256 - fx, 256 - fy
    out = (gx * gy * p00 + fx * gy * p01 + gx * fy * p10 + fx * fy * p11 + 32768) >> 16
    assert out.dtype == np.int32 and out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def warp_planes(src, matrices, dst, border=FILL, fill=(0, 0, 0), layout=HWC):
    """src uint8 [F or 1,Hs,Ws,C] (HWC), [F or 1,C,Hs,Ws] (CHW) or [F or 1,Hs,Ws]; dst likewise with its own H x W: what is there
    before the call; matrices float32 [F,3,3] -> dst after the call."""
    src, dst = np.asarray(src), np.asarray(dst)
    mask = src.ndim == 3
    if mask:
        src, dst = src[..., None], dst[..., None]
    elif layout == CHW:
        src, dst = src.transpose(0, 2, 3, 1), dst.transpose(0, 2, 3, 1)
    Fn = dst.shape[0]
    matrices = np.asarray(matrices, dtype=np.float32).reshape(Fn, 9)
    out = np.stack([warp_picture(src[j if src.shape[0] > 1 else 0], matrices[j], dst[j], border, fill) for j in range(Fn)])
    if mask:
        return np.ascontiguousarray(out[..., 0])
    return np.ascontiguousarray(out if layout == HWC else out.transpose(0, 3, 1, 2))


# ---- host-side helpers and scenes -----------------------------------------------------------------------------------------------------
def quad_matrix(corners, size):
    """float64 [3,3]: pixel (x, y) of an h x w picture -> the quad `corners` [4,2] = the images of (0, 0), (w - 1, 0), (w - 1, h - 1),
    (0, h - 1); h22 = 1."""
    h, w = size
    src = np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], dtype=np.float64)
    dst = np.asarray(corners, dtype=np.float64).reshape(4, 2)
    A, b = [], []
    for (x, y), (X, Y) in zip(src, dst):
        A += [[x, y, 1, 0, 0, 0, -x * X, -y * X], [0, 0, 0, x, y, 1, -x * Y, -y * Y]]
        b += [X, Y]
    return np.append(np.linalg.solve(np.array(A), np.array(b)), 1.0).reshape(3, 3)


def apply(Hm, pts):
    """A 3 x 3 matrix on points [n,2] -> [n,2], float64."""
    pts = np.asarray(pts, dtype=np.float64)
    v = np.concatenate([pts, np.ones((len(pts), 1))], axis=1) @ np.asarray(Hm, dtype=np.float64).reshape(3, 3).T
    return v[:, :2] / v[:, 2:3]


def dlt(src, dst):
    """The float64 Hartley-normalised SVD-DLT homography src -> dst ([n,2] each)."""
    def norm(p):
        c = p.mean(axis=0)
        s = np.sqrt(2.0) / np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
        return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1]])
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    Ts, Td = norm(src), norm(dst)
    a, b = apply(Ts, src), apply(Td, dst)
    rows = []
    for (x, y), (X, Y) in zip(a, b):
        rows += [[-x, -y, -1, 0, 0, 0, x * X, y * X, X], [0, 0, 0, -x, -y, -1, x * Y, y * Y, Y]]
    Hn = np.linalg.svd(np.array(rows))[2][-1].reshape(3, 3)
    Hm = np.linalg.inv(Td) @ Hn @ Ts
    return Hm / Hm[2, 2]


PICTURE = (1080, 1920)


def planted(seed, quad=(400, 600), N=1024, noise=0.1, outliers=0.4, shear=0.12, shift=100.0):
    """A planar quad of quad = (h, w) pixels somewhere on a 1920 x 1080 frame with N points on it; on the next frame its corners are
    displaced by up to `shear` of the size plus a common shift of up to `shift` pixels; Gaussian noise on both frames; a fraction of the
    points is replaced by outliers uniform over the frame -> (coords float32 [1,2,N,2], planted outlier bool [N], the planted
    float64 matrix, the quad's corners on frame 0 [4,2])."""
    rng = np.random.default_rng(seed)
    H, W = PICTURE
    h, w = quad
    x0, y0 = rng.uniform(150, W - 150 - w), rng.uniform(150, H - 150 - h)
    corners = np.array([[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h]])
    moved = corners + rng.uniform(-shear, shear, (4, 2)) * np.array([w, h]) + rng.uniform(-shift, shift, 2)
    to_quad = quad_matrix(corners, (h + 1, w + 1))  # the unit picture has its corners on the quad's
    truth = quad_matrix(moved, (h + 1, w + 1)) @ np.linalg.inv(to_quad)
    src = rng.uniform([x0, y0], [x0 + w, y0 + h], size=(N, 2))
    dst = apply(truth, src)
    src = src + rng.normal(0, 1, src.shape) * noise
    dst = dst + rng.normal(0, 1, dst.shape) * noise
    out = rng.random(N) < outliers
    dst[out] = rng.uniform([0, 0], [W - 1, H - 1], size=(int(out.sum()), 2))
    return np.stack([src, dst])[None].astype(np.float32), out, truth / truth[2, 2], corners


def planes_scene(seed, G, T, N, planes=3, hw=(270, 480)):
    """`planes` planar regions that each move under their own slowly changing homography over T frames, a share of the points moving on
    their own -> (coords float32 [G,T,N,2], visible uint8 [G,T,N], who int [G,N]: the region of a point)."""
    rng = np.random.default_rng(seed)
    H, W = hw
    who = rng.integers(0, planes, (G, N))
    coords = np.empty((G, T, N, 2), dtype=np.float32)
    base = rng.uniform([20, 20], [W - 20, H - 20], size=(G, N, 2))
    wild = rng.random((G, N)) < 0.2
    for g in range(G):
        for k in range(planes):
            mine = who[g] == k
            corners = np.array([[0.0, 0.0], [W, 0.0], [W, H], [0.0, H]])
            cur = corners.copy()
            for r in range(T):
                Hm = quad_matrix(cur, (H + 1, W + 1)) @ np.linalg.inv(quad_matrix(corners, (H + 1, W + 1)))
                coords[g, r, mine] = apply(Hm, base[g, mine])
                cur = cur + rng.uniform(-4, 4, (4, 2)) + rng.uniform(-3, 3, 2) * (k + 1)
    coords += (wild[:, None, :, None] * rng.uniform(-30, 30, (G, T, N, 2))).astype(np.float32)
    coords += rng.normal(0, 0.05, coords.shape).astype(np.float32)
    visible = (rng.random((G, T, N)) < 0.93).astype(np.uint8)
    return coords, visible, who
