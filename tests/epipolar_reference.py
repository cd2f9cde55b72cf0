"""The rules of ctk_fit_epipolar (include/ctk.h, "fit epipolar"; co-tracker_amd/csrc/epipolar_math.h) restated in numpy and Python
numbers: what the kernel (tests/test_gpu_epipolar.py) and the g++ build of the header (tests/test_epipolar_host.py) are compared with,
exactly.  Positions, mix, the pair rule, T and base2 are motion_reference's; the L D L^T solve and the IEEE division are
planes_reference's.  Admissibility is Python integers; everything in double is one float64 operation per step in the header's order
(Python floats and numpy float64 round every operation on its own)."""
import math

import numpy as np

import motion_reference as R
import planes_reference as PR

FIX, UNFIX = PR.FIX, PR.UNFIX
div = PR.div


def sample(seed, f, k, M):
    base = (f * 0x9e3779b9 + 8 * k) & 0xffffffff
    taken = []
    for t in range(8):
        v = R.mix(seed ^ R.mix((base + t) & 0xffffffff)) % (M - t)
        for e in sorted(taken):
            v += 1 if v >= e else 0
        taken.append(v)
    return taken


def bits(mx):
    return max(int(mx).bit_length(), 1)


def largest(f):
    j, m = 0, abs(f[0])
    for i in range(1, len(f)):
        if abs(f[i]) > m:
            j, m = i, abs(f[i])
    return j


def hypothesis(P8, Q8, b2):
    """P8, Q8: eight sample points as Python integer pairs -> None, or (f: nine floats, e, j*): centred on the first pair."""
    p = [(P8[t][0] - P8[0][0], P8[t][1] - P8[0][1]) for t in range(1, 8)]
    q = [(Q8[t][0] - Q8[0][0], Q8[t][1] - Q8[0][1]) for t in range(1, 8)]
    for a in p + q:
        d = a[0] * a[0] + a[1] * a[1]
        if d < b2 or d < 1:
            return None
    e = bits(max(abs(c) for a in p + q for c in a))
    sc = 2.0 ** -e
    A = []
    for (px, py), (qx, qy) in zip(p, q):
        x, y, X, Y = float(px) * sc, float(py) * sc, float(qx) * sc, float(qy) * sc
        A.append([X * x, X * y, X, Y * x, Y * y, Y, x, y])
    perm = list(range(8))
    for s in range(7):
        best, pr, pc = -1.0, s, s
        for r in range(s, 7):
            for c in range(s, 8):
                a = abs(A[r][c])
                if a > best:
                    best, pr, pc = a, r, c
        A[s], A[pr] = A[pr], A[s]
        for r in range(7):
            A[r][s], A[r][pc] = A[r][pc], A[r][s]
        perm[s], perm[pc] = perm[pc], perm[s]
        piv = A[s][s]
        if piv == 0.0 or not math.isfinite(piv):
            return None
        for r in range(s + 1, 7):
            m = div(A[r][s], piv)
            for c in range(s + 1, 8):
                A[r][c] = A[r][c] - m * A[s][c]
    z = [0.0] * 8
    z[7] = 1.0
    for s in range(6, -1, -1):
        acc = A[s][7]
        for c in range(s + 1, 7):
            acc = acc + A[s][c] * z[c]
        z[s] = div(-acc, A[s][s])
    f = [0.0] * 8
    for c in range(8):
        f[perm[c]] = z[c]
    js = largest(f)
    den = f[js]
    f = [div(v, den) for v in f]
    if not all(math.isfinite(v) for v in f):
        return None
    return f + [0.0], e, js


def residual(f, e, P0, Q0, P, Q):
    """A matrix (nine floats) of scale e centred on (P0, Q0); P, Q int64 [M,2] -> (r, g) float64 [M]."""
    sc = 2.0 ** -e
    u, w = (P - P0).astype(np.float64) * sc, (Q - Q0).astype(np.float64) * sc
    ux, uy, wx, wy = u[:, 0], u[:, 1], w[:, 0], w[:, 1]
    with np.errstate(all="ignore"):
        a0 = (f[0] * ux + f[1] * uy) + f[2]
        a1 = (f[3] * ux + f[4] * uy) + f[5]
        a2 = (f[6] * ux + f[7] * uy) + f[8]
        b0 = (f[0] * wx + f[3] * wy) + f[6]
        b1 = (f[1] * wx + f[4] * wy) + f[7]
        r = (wx * a0 + wy * a1) + a2
        g = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1
    return r, g


def test(r, g, e, T):
    Ts = float(T) * 2.0 ** -e
    with np.errstate(all="ignore"):
        return (g > 0) & (r * r <= (Ts * Ts) * g)


def error(r, g, e):
    with np.errstate(all="ignore"):
        v = ((r * r) / g) * 2.0 ** (2 * e - 8)
        return np.where(g > 0, v, np.inf).astype(np.float32)


def sum_index(i, j):
    return i * 9 - i * (i - 1) // 2 + (j - i)


def terms(u, w, e):
    """u, w int64 [n,2] of the inliers -> the 45 sums as Python integers."""
    sc = 2.0 ** -e
    x, y, X, Y = u[:, 0] * sc, u[:, 1] * sc, w[:, 0] * sc, w[:, 1] * sc
    a = [X * x, X * y, X, Y * x, Y * y, Y, x, y, np.ones_like(x)]
    out = []
    for i in range(9):
        for j in range(i, 9):
            t = a[i] * a[j]
            assert t.size == 0 or float(np.abs(t).max()) <= 1.0
            out.append(int(np.rint(t * FIX).astype(np.int64).sum()))
            assert abs(out[-1]) < 2 ** 58
    return out


def refit(s, jstar):
    """The 45 sums and j* -> the nine entries, or None (the solve failed)."""
    S = [float(v) * UNFIX for v in s]
    keep = [i for i in range(9) if i != jstar]
    N = [[S[sum_index(min(i, j), max(i, j))] for j in keep] for i in keep]
    b = [-S[sum_index(min(i, jstar), max(i, jstar))] for i in keep]
    h = PR.solve(N, b)
    if h is None:
        return None
    f = list(h)
    f.insert(jstar, 1.0)
    return f


def rescale(f, e_from, e_to):
    s = 2.0 ** (e_to - e_from)
    ss = s * s
    return [f[0] * ss, f[1] * ss, f[2] * s, f[3] * ss, f[4] * ss, f[5] * s, f[6] * s, f[7] * s, f[8]]


def pixels(f, e, P0, Q0):
    """A centred matrix (nine floats) of scale e -> (float64 [9] in pixels, before the cast; float32 [9])."""
    s = 2.0 ** (4 - e)
    cx, cy, kx, ky = P0[0] / 16.0, P0[1] / 16.0, Q0[0] / 16.0, Q0[1] / 16.0
    G = [0.0] * 9
    for r in range(3):
        G[r * 3], G[r * 3 + 1] = f[r * 3] * s, f[r * 3 + 1] * s
        G[r * 3 + 2] = f[r * 3 + 2] - (G[r * 3] * cx + G[r * 3 + 1] * cy)
    out = [0.0] * 9
    for c in range(3):
        out[c], out[3 + c] = s * G[c], s * G[3 + c]
        out[6 + c] = G[6 + c] - (out[c] * kx + out[3 + c] * ky)
    return np.array(out, dtype=np.float64), np.array(out, dtype=np.float64).astype(np.float32)


def fit_list(P, Q, fit, f, T, b2, K, seed, min_points, details=None):
    """P, Q int64 [A,2]: every correspondence; fit bool [A]: the fit list -> (matrix float32 [9], label int8 [A], error float32 [A],
    (M, inliers, best k, fall-back bits) or (M, 0, -1, 0))."""
    Pf, Qf = P[fit], Q[fit]
    M = Pf.shape[0]
    none = (np.zeros(9, dtype=np.float32), np.zeros(P.shape[0], dtype=np.int8), np.full(P.shape[0], -1.0, dtype=np.float32), (M, 0, -1, 0))
    if M < 8:
        return none
    assert int(np.abs(P).max()) <= 2 ** 17 and int(np.abs(Q).max()) <= 2 ** 17
    Pl, Ql = Pf.tolist(), Qf.tolist()
    best, kept = -1, None
    for k in range(K):
        i = sample(seed, f, k, M)
        assert len(set(i)) == 8 and 0 <= min(i) and max(i) < M
        h = hypothesis([Pl[t] for t in i], [Ql[t] for t in i], b2)
        if h is None:
            continue
        fm, e, js = h
        inl = test(*residual(fm, e, Pf[i[0]], Qf[i[0]], Pf, Qf), e, T)
        key = (int(inl.sum()) << 32) | (K - 1 - k)
        if key > best:
            best, kept = key, (k, fm, e, js, i[0])
    if best < 0 or (best >> 32) < min_points:
        return none
    k, fm, e, js, i0 = kept
    P0, Q0 = Pf[i0], Qf[i0]
    fell = 0
    for rnd in range(2):
        inl = test(*residual(fm, e, P0, Q0, Pf, Qf), e, T)
        u, w = (Pf - P0)[inl], (Qf - Q0)[inl]
        e2 = bits(max(np.abs(u).max(), np.abs(w).max())) if inl.any() else 1
        jstar = js if rnd == 0 else largest(fm)
        new = refit(terms(u, w, e2), jstar)
        if new is not None:
            fm, e = new, e2
        else:
            fell |= 1 << rnd
            if rnd == 0:
                fm, e = rescale(fm, e, e2), e2
    count = int(test(*residual(fm, e, P0, Q0, Pf, Qf), e, T).sum())
    r, g = residual(fm, e, P0, Q0, P, Q)
    m64, m32 = pixels(fm, e, Pl[i0], Ql[i0])
    if details is not None:
        details.update(f=fm, e=e, i0=i0, px64=m64)
    return m32, test(r, g, e, T).astype(np.int8), error(r, g, e), (M, count, k, fell)


def fit_epipolar(coords, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1, to=None, lag=None,
                 anchor=None, mask=None, min_points=16, tol=1.0, K=512, min_base=16.0, seed=0, scale=(1.0, 1.0)):
    """coords float32 [G,R,N,2]; visible [G,R,N] (or the logits vis, conf and thresh); first_row int [G,N] or None; exactly one of
    to (a frame), lag (>= 1) and anchor = (coords float32 [G,N,2], visible [G,N], frame); mask int8 [G,N] or None ->
    (fundamental float32 [G,F,3,3], label int8 [G,F,N_out], error float32 [G,F,N_out], stats int32 [G,F,4])."""
    coords = np.asarray(coords, dtype=np.float32)
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    assert (to is not None) + (lag is not None) + (anchor is not None) == 1 and (lag is None or lag >= 1) and (to is None or to >= 0)
    assert 8 <= min_points <= 8192
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
    fundamental = np.zeros((G, F, 9), dtype=np.float32)
    label = np.full((G, F, N_out), -1, dtype=np.int8)
    err = np.full((G, F, N_out), -1.0, dtype=np.float32)
    stats = np.zeros((G, F, 4), dtype=np.int32)
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
            fit = np.ones(len(idx), dtype=bool) if mask is None else np.asarray(mask[g])[idx] != 0
            m9, lab, er, st = fit_list(src[idx], pos[g, f % R_][idx], fit, f, T, b2, K, seed, min_points)
            fundamental[g, jf], stats[g, jf] = m9, st
            label[g, jf, idx], err[g, jf, idx] = lab, er
    return fundamental.reshape(G, F, 3, 3), label, err, stats


# ---- planted scenes ---------------------------------------------------------------------------------------------------------------------
def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def planted(seed, kind, N=None):
    """A 1080p camera of focal length 1000 px that moves through a static scene 3..12 m deep, `kind` = "sideways", "forward" or
    "few" (90 points, sideways); 25 % of the points move on their own in three groups; 0.1 px noise ->
    dict(P, Q float64 [N,2] noisy pixels, Q_clean, mover bool [N], F_true [3,3] with (Q,1)^T F (P,1) = 0)."""
    rng = np.random.default_rng(seed)
    N = (90 if kind == "few" else 400) if N is None else N
    Wd, Hd, fl = 1920.0, 1080.0, 1000.0
    Kc = np.array([[fl, 0, Wd / 2], [0, fl, Hd / 2], [0, 0, 1]])
    P = np.stack([rng.uniform(40, Wd - 40, N), rng.uniform(40, Hd - 40, N)], axis=1)
    depth = rng.uniform(3.0, 12.0, N)
    X = (np.linalg.inv(Kc) @ np.concatenate([P, np.ones((N, 1))], axis=1).T).T * depth[:, None]
    t = np.array([0.0, 0.02, 0.35]) if kind == "forward" else np.array([0.30, 0.03, 0.02])
    Rm = rotation(*(rng.uniform(-0.02, 0.02, 3)))
    X2 = (Rm @ X.T).T + t
    Q = (Kc @ X2.T).T
    Q = Q[:, :2] / Q[:, 2:3]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ft = np.linalg.inv(Kc).T @ tx @ Rm @ np.linalg.inv(Kc)
    mover = np.zeros(N, dtype=bool)
    order = rng.permutation(N)
    n_mov = N // 4
    Qc = Q.copy()
    for grp in range(3):
        ids = order[grp * n_mov // 3:(grp + 1) * n_mov // 3]
        mover[ids] = True
        ang = rng.uniform(0, 2 * np.pi)
        Qc[ids] += rng.uniform(25.0, 60.0) * np.array([np.cos(ang), np.sin(ang)])
    noise = rng.normal(0.0, 0.1, (2, N, 2))
    return dict(P=P + noise[0], Q=Qc + noise[1], Q_clean=Qc, P_clean=P, mover=mover, F_true=Ft)


def line_distance(Fm, P, Q):
    """The distance in pixels of Q from the epipolar line F (P, 1)."""
    l = (np.asarray(Fm, dtype=np.float64).reshape(3, 3) @ np.concatenate([P, np.ones((len(P), 1))], axis=1).T).T
    return np.abs((l[:, :2] * Q).sum(axis=1) + l[:, 2]) / np.hypot(l[:, 0], l[:, 1])


def sampson(Fm, P, Q):
    """The Sampson distance in pixels, float64."""
    Fm = np.asarray(Fm, dtype=np.float64).reshape(3, 3)
    Ph, Qh = np.concatenate([P, np.ones((len(P), 1))], axis=1), np.concatenate([Q, np.ones((len(Q), 1))], axis=1)
    a, b = (Fm @ Ph.T).T, (Fm.T @ Qh.T).T
    r = (Qh * a).sum(axis=1)
    return np.abs(r) / np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2)


def hartley(P, Q):
    """The float64 Hartley-normalised eight-point fit by SVD, without the rank-2 step (the device has none either)."""
    def norm(X):
        c = X.mean(axis=0)
        s = np.sqrt(2.0) / np.sqrt(((X - c) ** 2).sum(axis=1)).mean()
        return (X - c) * s, np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1]])
    p, Tp = norm(P)
    q, Tq = norm(Q)
    A = np.stack([q[:, 0] * p[:, 0], q[:, 0] * p[:, 1], q[:, 0], q[:, 1] * p[:, 0], q[:, 1] * p[:, 1], q[:, 1], p[:, 0], p[:, 1],
                  np.ones(len(p))], axis=1)
    Fm = np.linalg.svd(A)[2][-1].reshape(3, 3)
    return Tq.T @ Fm @ Tp


def history(seed, G, T, N, hw=(270, 480), movers=0.25, noise=0.05, p_visible=0.92):
    """A stream-shaped history: a camera of focal length 0.9 W that translates and turns a little from frame to frame through G static
    scenes 3..12 m deep; a fraction `movers` of the points moves on its own in three groups ->
    (coords float32 [G,T,N,2], visible uint8 [G,T,N], mover bool [G,N])."""
    rng = np.random.default_rng(seed)
    Hd, Wd = hw
    fl = 0.9 * Wd
    Kc = np.array([[fl, 0, Wd / 2], [0, fl, Hd / 2], [0, 0, 1]])
    coords = np.zeros((G, T, N, 2), dtype=np.float32)
    mover = np.zeros((G, N), dtype=bool)
    for g in range(G):
        P = np.stack([rng.uniform(8, Wd - 8, N), rng.uniform(8, Hd - 8, N)], axis=1)
        X = (np.linalg.inv(Kc) @ np.concatenate([P, np.ones((N, 1))], axis=1).T).T * rng.uniform(3.0, 12.0, N)[:, None]
        step = np.array([0.05, 0.004, 0.01]) * (1.0 + 0.3 * g)
        turn = rng.uniform(-0.003, 0.003, 3)
        order = rng.permutation(N)
        n_mov = int(N * movers)
        drift = np.zeros((N, 2))
        for grp in range(3):
            ids = order[grp * n_mov // 3:(grp + 1) * n_mov // 3]
            mover[g, ids] = True
            ang = rng.uniform(0, 2 * np.pi)
            drift[ids] = rng.uniform(3.0, 6.0) * np.array([np.cos(ang), np.sin(ang)])
        for t in range(T):
            Xt = (rotation(*(turn * t)) @ X.T).T + step * t
            Q = (Kc @ Xt.T).T
            coords[g, t] = Q[:, :2] / Q[:, 2:3] + drift * t + rng.normal(0.0, noise, (N, 2))
    visible = (rng.uniform(size=(G, T, N)) < p_visible).astype(np.uint8)
    return coords, visible, mover
