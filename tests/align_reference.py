"""The rules of ctk_fit_align (include/ctk.h, "fit align"; co-tracker_amd/csrc/align_math.h) restated in numpy and Python numbers: what
the kernel (tests/test_gpu_align.py) and the g++ build of the header (tests/test_align_host.py) are compared with, exactly.  The sample,
the L D L^T solve and the IEEE division are planes_reference's; dot / cross / polar / rsqrt / valid are pose_reference's; the cofactors
are p3p_reference's.  A candidate is what one lane does in the kernel: Python floats here, one IEEE operation per step in the header's
order; what every entry does is numpy over the entries.  Below the rules: the cases of the GPU test, the planted scenes and the float64
reference (Umeyama by SVD, then converged Gauss-Newton) the scenes are judged against."""
import math

import numpy as np

import p3p_reference as P3
import planes_reference as PR
import pose_reference as PO

div = PR.div
FIX, UNFIX = PR.FIX, PR.UNFIX
LIST_MAX, MIN_POINTS, HYPOTHESES_MAX, ROUNDS, SOLVE_MIN = 4096, 3, 1024, 3, 3
REACH = 1048576.0
BIT_ROUND, BIT_LEFT, BIT_CAP, BIT_IDENTICAL = 2, 4, 8, 32
NO_REACH = -100000
EYE = (1.0, [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0])
GATES = (4.0, 2.0, 1.0)


def correspondences(a, valid_a, b, valid_b):
    """a, b float32 [N,3] -> bool [N]."""
    with np.errstate(all="ignore"):
        ok = (np.asarray(valid_a) != 0) & (np.asarray(valid_b) != 0)
        ok = ok & (np.abs(a) <= np.float32(REACH)).all(axis=1) & (np.abs(b) <= np.float32(REACH)).all(axis=1)
        return ok & (b[:, 2] > 0)


def sample(seed, k, M):
    return [0, 1, 2] if M < 4 else PR.sample(seed, 0, k, M)[:3]


def sides(P):
    e01, e02, e12 = ([P[1][i] - P[0][i] for i in range(3)], [P[2][i] - P[0][i] for i in range(3)], [P[2][i] - P[1][i] for i in range(3)])
    return (PO.dot(e01, e01) + PO.dot(e02, e02)) + PO.dot(e12, e12), e01, e02


def frame(e1, e2):
    e3 = PO.cross(e1, e2)
    return [e1[0], e2[0], e3[0], e1[1], e2[1], e3[1], e1[2], e2[2], e3[2]]


def candidate(X, Y):
    """Three entries: X, Y three lists of three floats -> (s, R nine floats, t three floats), or None."""
    da, a1, a2 = sides(X)
    db, b1, b2 = sides(Y)
    if not (da > 0.0) or not PO.finite(da) or not (db > 0.0) or not PO.finite(db):
        return None
    s2 = div(db, da)
    if not (s2 > 0.0) or not PO.finite(s2):
        return None
    s = s2 * PO.rsqrt(s2)
    a1, a2 = [s * v for v in a1], [s * v for v in a2]
    A, B = frame(a1, a2), frame(b1, b2)
    C, detA = P3.cofactors(A)
    _, detB = P3.cofactors(B)
    if not (detA > 0.0) or not (detB > 0.0):
        return None
    inv = div(1.0, detA)
    Rm, det = PO.polar([PO.dot(B[i * 3:i * 3 + 3], C[j * 3:j * 3 + 3]) * inv for i in range(3) for j in range(3)])
    t = [Y[0][i] - s * PO.dot(Rm[i * 3:i * 3 + 3], X[0]) for i in range(3)]
    return (s, Rm, t) if PO.valid(Rm, t, det) and s <= PO.FLT_MAX else None


def apply(c, X):
    """X: three arrays -> Z = s R X + t, three arrays."""
    s, Rm, t = c
    with np.errstate(all="ignore"):
        return [s * PO.dot(Rm[i * 3:i * 3 + 3], X) + t[i] for i in range(3)]


def pixels(cam, Z, Y):
    fx, fy = cam[0], cam[1]
    with np.errstate(all="ignore"):
        nx, ny = fx * (Z[0] * Y[2] - Y[0] * Z[2]), fy * (Z[1] * Y[2] - Y[1] * Z[2])
        w = Z[2] * Y[2]
        return nx * nx + ny * ny, w * w


def within(cam, Z, Y, t2, dtol):
    with np.errstate(all="ignore"):
        num, den = pixels(cam, Z, Y)
        return (Z[2] > 0.0) & (num <= t2 * den) & (np.abs(Z[2] - Y[2]) <= dtol * Y[2])


def error(cam, Z, Y):
    with np.errstate(all="ignore"):
        num, den = pixels(cam, Z, Y)
        e = num / den
        return np.where((Z[2] > 0.0) & ~np.isnan(e), e, np.inf).astype(np.float32)


def tol2(tol, g=1.0):
    t = g * float(np.float32(tol))
    return t * t


def weights(cam, tol, depth_tol):
    """-> (q_x, q_y, q_z): the rows' weights with the 1/16 of the fixed-point scaling."""
    return 0.0625, 0.0625 * div(cam[1], cam[0]), 0.0625 * div(float(np.float32(tol)), cam[0] * float(np.float32(depth_tol)))


def entries(q, Z, Y, e):
    """The entries within the round's gates (arrays) -> (three rows of eight arrays, takes part bool [n])."""
    with np.errstate(all="ignore"):
        ia, ib = 1.0 / Z[2], 1.0 / Y[2]
        ha, hb = np.ldexp(ia, e), np.ldexp(ib, e)
        u, t, ub, tb = Z[0] * ia, Z[1] * ia, Y[0] * ib, Y[1] * ib
        uu, ut, tt = u * u, u * t, t * t
        cu, ct, hu, ht = 1.0 + uu, 1.0 + tt, u * ha, t * ha
        zero = np.zeros_like(ia)
        qx, qy, qz = q
        rows = [[-(ut * qx), cu * qx, -(t * qx), ha * qx, zero, -(hu * qx), zero, (u - ub) * qx],
                [-(ct * qy), ut * qy, u * qy, zero, ha * qy, -(ht * qy), zero, (t - tb) * qy],
                [(Z[1] * ib) * qz, -((Z[0] * ib) * qz), zero, zero, zero, hb * qz, (Z[2] * ib) * qz, ((Z[2] - Y[2]) * ib) * qz]]
        take = np.ones(ia.shape, dtype=bool)
        for row in rows:
            for v in row:
                take = take & (v * v <= 16.0)
    return rows, take


PAIRS = [(i, j) for i in range(7) for j in range(i, 7)] + [(i, 7) for i in range(8)]


def sums(rows, take):
    """-> the 36 sums as Python integers, in the header's order."""
    out = [0] * len(PAIRS)
    for v in rows:
        v = [a[take] for a in v]
        for n, (i, j) in enumerate(PAIRS):
            w = v[i] * v[j]
            assert w.size == 0 or float(np.abs(w).max()) <= 16.0
            out[n] += int(np.rint(w * FIX).astype(np.int64).sum())
    assert all(abs(v) < 2 ** 62 for v in out)
    return out


def sum_index(i, j):
    return i * 7 - i * (i - 1) // 2 + (j - i)


def update(c, s, n, e):
    """One round from its sums -> (s, R, t), or None."""
    if n < SOLVE_MIN:
        return None
    sc, Rm, t = c
    N = [[0.0] * 8 for _ in range(8)]
    for i in range(7):
        for j in range(7):
            N[i][j] = float(s[sum_index(min(i, j), max(i, j))]) * UNFIX
    N[7][7] = 1.0
    b = [-(float(s[28 + i]) * UNFIX) for i in range(7)] + [0.0]
    h = PR.solve(N, b)
    if h is None:
        return None
    W = PO.skew_times(h[:3], Rm)
    R2, det = PO.polar([Rm[i] + W[i] for i in range(9)])
    wt = PO.cross(h[:3], t)
    t2 = [((t[i] + wt[i]) + h[6] * t[i]) + math.ldexp(h[3 + i], e) for i in range(3)]
    s2 = sc * (1.0 + h[6])
    return (s2, R2, t2) if PO.valid(R2, t2, det) and s2 > 0.0 and s2 <= PO.FLT_MAX else None


def fit_pair(a, valid_a, b, valid_b, cam, mask=None, tol=2.0, depth_tol=0.1, hypotheses=256, min_points=8, seed=0, details=None):
    """a, b float32 [N,3] -> (sim float32 [12], scale float32, label int8 [N], error float32 [N], (M, labelled 1, k, bits))."""
    N = a.shape[0]
    corr = correspondences(a, valid_a, b, valid_b)
    listed = corr if mask is None else corr & (np.asarray(mask) != 0)
    L = int(listed.sum())
    M = min(L, LIST_MAX)
    identical = bool(corr.any()) and bool((a[corr] == b[corr]).all())
    bits = (BIT_CAP if L > LIST_MAX else 0) | (BIT_IDENTICAL if identical else 0)
    label = np.where(corr, 0, -1).astype(np.int8)
    err = np.full(N, -1.0, dtype=np.float32)
    none = (np.zeros(12, dtype=np.float32), np.float32(0.0), label, err)
    if M < MIN_POINTS:
        return none + ((M, 0, -1, bits),)
    idx = np.nonzero(listed)[0][:M]
    X = [a[idx, i].astype(np.float64) for i in range(3)]
    Y = [b[idx, i].astype(np.float64) for i in range(3)]
    t2, dt = tol2(tol), float(np.float32(depth_tol))
    K = hypotheses
    cands = []
    for k in range(K):
        if identical:
            cands.append(None)
            continue
        tri = sample(seed, k, M)
        cands.append(candidate([[float(X[0][i]), float(X[1][i]), float(X[2][i])] for i in tri],
                               [[float(Y[0][i]), float(Y[1][i]), float(Y[2][i])] for i in tri]))
    cands.append(EYE)
    best, bk, counts = -1, -1, []
    for k, c in enumerate(cands):
        if c is None:
            counts.append(-1)
            continue
        counts.append(int(within(cam, apply(c, X), Y, t2, dt).sum()))
        if counts[-1] > best:
            best, bk = counts[-1], k
    if details is not None:
        details.update(counts=counts, made=sum(c is not None for c in cands[:K]))
    if best < min_points:
        return none + ((M, 0, -1, bits),)
    cur, q = cands[bk], weights(cam, tol, depth_tol)
    for rnd in range(ROUNDS):
        Z = apply(cur, X)
        inl = within(cam, Z, Y, tol2(tol, GATES[rnd]), GATES[rnd] * dt)
        Zi, Yi = [v[inl] for v in Z], [v[inl] for v in Y]
        e = int(np.frexp(Yi[2])[1].max()) if inl.any() else NO_REACH
        rows, take = entries(q, Zi, Yi, e)
        if not take.all():
            bits |= BIT_LEFT
        new = update(cur, sums(rows, take), int(take.sum()), e)
        if new is None:
            bits |= BIT_ROUND
        else:
            cur = new
    Xa = [a[:, i].astype(np.float64) for i in range(3)]
    Ya = [b[:, i].astype(np.float64) for i in range(3)]
    Z = apply(cur, Xa)
    label = np.where(corr, within(cam, Z, Ya, t2, dt).astype(np.int8), -1).astype(np.int8)
    err = np.where(corr, error(cam, Z, Ya), np.float32(-1.0)).astype(np.float32)
    s, Rm, t = cur
    with np.errstate(all="ignore"):
        sim = np.array([s * Rm[0], s * Rm[1], s * Rm[2], t[0], s * Rm[3], s * Rm[4], s * Rm[5], t[1], s * Rm[6], s * Rm[7], s * Rm[8], t[2]],
                       dtype=np.float64).astype(np.float32)
        scale = np.float32(s)
    if details is not None:
        details.update(s=s, R=np.array(Rm).reshape(3, 3), t=np.array(t))
    return sim, scale, label, err, (M, int((label == 1).sum()), bk, bits)


def fit_align(a, valid_a, b, valid_b, intrinsics, mask=None, **kw):
    """a, b float32 [G,N,3]; valid int8 [G,N]; mask uint8 [G,N] or None -> (sim float32 [G,3,4], scale float32 [G], label int8 [G,N],
    error float32 [G,N], stats int32 [G,4])."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    G, N, _ = a.shape
    assert MIN_POINTS <= kw.get("min_points", 8) <= 8192 and 1 <= kw.get("hypotheses", 256) <= HYPOTHESES_MAX
    cam = PO.camera(intrinsics)
    sim, scale = np.zeros((G, 12), dtype=np.float32), np.zeros(G, dtype=np.float32)
    label, err, stats = np.zeros((G, N), dtype=np.int8), np.zeros((G, N), dtype=np.float32), np.zeros((G, 4), dtype=np.int32)
    details = kw.pop("details", None)
    for g in range(G):
        d = None if details is None else details.setdefault(g, {})
        sim[g], scale[g], label[g], err[g], stats[g] = fit_pair(a[g], valid_a[g], b[g], valid_b[g], cam,
                                                                mask=None if mask is None else mask[g], details=d, **kw)
    return sim.reshape(G, 3, 4), scale, label, err, stats


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
CAM = (1000.0, 1000.0, 960.0, 540.0)


def rotation(axis, angle):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)


def planted(seed, N=400, share=0.3, plane=False, depth_noise=0.005, ray_noise=0.1, moved_px=(12.0, 80.0)):
    """The 1080p scenes of tests/test_resection_host.py with a second structure: focal length 1000 px, N points 3..12 deep in b's camera
    (plane: on a slanted plane); a = the points of b taken back through a random similarity (scale 0.2..5, up to 30 degrees, shift up
    to 3 units), so that b = s R a + t; both sets get 0.5 % depth noise along and 0.1 px across the rays of b's camera (a's is
    applied in b's frame before the similarity takes the points back); a `share` of the points moves by 12..80 px (and up to 30 % in depth)
    between the two -> dict(a, b float32 [N,3], moved bool [N], s, R, t)."""
    rng = np.random.default_rng(seed)
    Wd, Hd, fl = 1920.0, 1080.0, 1000.0
    P = np.stack([rng.uniform(40, Wd - 40, N), rng.uniform(40, Hd - 40, N)], axis=1)
    rx, ry = (P[:, 0] - Wd / 2) / fl, (P[:, 1] - Hd / 2) / fl
    z = 6.0 / (1.0 + 0.45 * rx - 0.25 * ry) if plane else rng.uniform(3.0, 12.0, N)
    Yt = np.stack([rx * z, ry * z, z], axis=1)

    def noisy(Pt):
        zz = Pt[:, 2] * (1.0 + rng.normal(0.0, depth_noise, N))
        uv = Pt[:, :2] / Pt[:, 2:3] + rng.normal(0.0, ray_noise / fl, (N, 2))
        return np.concatenate([uv * zz[:, None], zz[:, None]], axis=1)
    s = float(np.exp(rng.uniform(np.log(0.2), np.log(5.0))))
    Rm = rotation(rng.normal(size=3), rng.uniform(0.0, np.radians(30.0)))
    t = rng.uniform(-1.0, 1.0, 3)
    t = t / np.linalg.norm(t) * rng.uniform(0.0, 3.0)
    moved = np.zeros(N, dtype=bool)
    moved[rng.permutation(N)[:int(round(N * share))]] = True
    Ya = Yt.copy()  # what a saw: the moved points sat elsewhere
    ang, far = rng.uniform(0, 2 * np.pi, N), rng.uniform(moved_px[0], moved_px[1], N)
    za = Ya[:, 2] * np.where(moved, 1.0 + rng.uniform(-0.3, 0.3, N), 1.0)
    uva = Ya[:, :2] / Ya[:, 2:3] + np.where(moved[:, None], np.stack([far * np.cos(ang), far * np.sin(ang)], axis=1) / fl, 0.0)
    Ya = np.concatenate([uva * za[:, None], za[:, None]], axis=1)
    a = (noisy(Ya) - t) @ Rm / s  # R^T (Y - t) / s
    b = noisy(Yt)
    return dict(a=a.astype(np.float32), b=b.astype(np.float32), moved=moved, s=s, R=Rm, t=t)


def umeyama(X, Y):
    """float64 [n,3] each -> (s, R, t) of the least-squares similarity Y ~ s R X + t (Umeyama 1991, by SVD)."""
    mx, my = X.mean(axis=0), Y.mean(axis=0)
    Xc, Yc = X - mx, Y - my
    U, D, Vt = np.linalg.svd(Yc.T @ Xc / X.shape[0])
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    Rm = U @ S @ Vt
    s = float(np.trace(np.diag(D) @ S) / (Xc ** 2).sum() * X.shape[0])
    return s, Rm, my - s * Rm @ mx


def reference(a, b, cam, start, tol=2.0, depth_tol=0.1, iters=50, textbook=False):
    """The float64 reference of a scene: the inliers (tol, depth_tol) under `start` = (s, R, t); Umeyama over them; then Gauss-Newton on
    the rules' residual over the SAME inliers until the step is below 1e-13 -> ((s, R, t), inliers bool [N]).  textbook: the residual
    is (Z - Y) / Y_z, three numbers weighted alike -- what the rules do NOT use (test_align_host.test_the_textbook_residual)."""
    X, Y = a.astype(np.float64), b.astype(np.float64)

    def inliers(c):
        Z = c[0] * X @ c[1].T + c[2]
        with np.errstate(all="ignore"):
            px = lambda P: np.stack([cam[0] * P[:, 0] / P[:, 2], cam[1] * P[:, 1] / P[:, 2]], axis=1)
            e = ((px(Z) - px(Y)) ** 2).sum(axis=1)
            return (Z[:, 2] > 0) & (e <= tol * tol) & (np.abs(Z[:, 2] - Y[:, 2]) <= depth_tol * Y[:, 2])
    inl = inliers(start)
    Xi, Yi = X[inl], Y[inl]

    def moved(c, h):
        dR = rotation(h[:3], np.linalg.norm(h[:3])) if np.linalg.norm(h[:3]) > 0 else np.eye(3)
        return c[0] * (1.0 + h[6]), dR @ c[1], (1.0 + h[6]) * (dR @ c[2]) + h[3:6]

    def residual(c):
        """The rules' residual (align_math.h, refit): the two pixel differences over tol and the relative depth difference over
        depth_tol, [n * 3]."""
        Z = c[0] * Xi @ c[1].T + c[2]
        if textbook:
            return ((Z - Yi) / Yi[:, 2:3]).reshape(-1)
        return np.stack([cam[0] * (Z[:, 0] / Z[:, 2] - Yi[:, 0] / Yi[:, 2]) / tol, cam[1] * (Z[:, 1] / Z[:, 2] - Yi[:, 1] / Yi[:, 2]) / tol,
                         (Z[:, 2] - Yi[:, 2]) / Yi[:, 2] / depth_tol], axis=1).reshape(-1)
    cur = umeyama(Xi, Yi)
    for _ in range(iters):
        r = residual(cur)
        J = np.zeros((r.size, 7))
        for i in range(7):  # central differences about the current transform: independent of the rules' algebra
            h = np.zeros(7)
            h[i] = 1e-6
            J[:, i] = (residual(moved(cur, h)) - residual(moved(cur, -h))) / 2e-6
        h = np.linalg.lstsq(J, -r, rcond=None)[0]
        cur = moved(cur, h)
        if np.abs(h).max() < 1e-13:
            break
    return cur, inl


def distance(c, truth):
    """-> (relative scale error, rotation angle in degrees, translation distance in units)."""
    s, Rm, t = c
    D = np.asarray(Rm) @ np.asarray(truth[1]).T
    sinv = np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) / 2.0  # (an arccos alone loses small angles)
    return abs(s / truth[0] - 1.0), float(np.degrees(np.arctan2(sinv, (np.trace(D) - 1.0) / 2.0))), float(np.linalg.norm(np.asarray(t) - truth[2]))


def from_sim(sim, scale):
    """The outputs of one pair -> (s, R, t) in float64."""
    sim = np.asarray(sim, dtype=np.float64).reshape(3, 4)
    s = float(scale)
    return s, sim[:, :3] / s, sim[:, 3]


# ---- the cases of the GPU test ------------------------------------------------------------------------------------------------------------
def pair(seed, N, share=0.2, plane=False, **kw):
    sc = planted(seed, N=N, share=share, plane=plane, **kw)
    return sc["a"], sc["b"]


def stack(pairs):
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def cases():
    """The shapes at which the kernel can go wrong -> (name, (a, valid_a, b, valid_b, cam), kwargs) of fit_align."""
    ones = lambda G, N: np.ones((G, N), dtype=np.int8)
    # sizes: N = 3, min_points - 1, min_points, round the wave and the chunk, 600, the cap and one beyond (bit 3), the largest
    for N, K, mp in ((3, 5, 3), (7, 16, 8), (8, 16, 8), (63, 63, 8), (64, 64, 8), (65, 65, 8), (255, 1, 8), (256, 256, 8), (257, 257, 8),
                     (600, 1024, 8), (4096, 24, 8), (4097, 24, 8), (8192, 16, 8)):
        a, b = stack([pair(N, N, share=0.2) if N > 8 else pair(N, N, share=0.0, depth_noise=0.0, ray_noise=0.0)])
        yield "size_%d" % N, (a, ones(1, N), b, ones(1, N), CAM), dict(hypotheses=K, min_points=mp, seed=N)
    # G = 3 with a no-fit pair between fitted ones (its b is unrelated to its a); a mask; spoiled inputs in either set
    N = 300
    prs = [pair(1, N), (pair(2, N)[0], pair(3, N)[1]), pair(4, N, share=0.5)]
    a, b = stack(prs)
    a, b = a.copy(), b.copy()
    va, vb = ones(3, N), ones(3, N)
    a[0, 5, 1], a[0, 6, 0], a[0, 7, 2], a[0, 8, 0] = np.nan, np.inf, -np.inf, 2.0 ** 20 * 1.0001
    b[0, 9, 0], b[0, 10, 2], b[0, 11, 2], b[0, 12, 1], b[0, 13, 2] = np.nan, -b[0, 10, 2], 0.0, 2.0 ** 21, np.inf
    a[2, 20] = 2.0 ** 20  # the limit itself is taken
    va[0, 30:34], vb[2, 40:45] = 0, 0
    rng = np.random.default_rng(9)
    mask = (rng.uniform(size=(3, N)) < 0.7).astype(np.uint8)
    yield "batch_spoiled", (a, va, b, vb, CAM), dict(hypotheses=200, min_points=8, seed=3)
    yield "batch_spoiled_mask", (a, va, b, vb, CAM), dict(mask=mask, hypotheses=65, min_points=8, seed=4)
    yield "batch_2", (a[:2], va[:2], b[:2], vb[:2], CAM), dict(hypotheses=64, min_points=8, seed=5, tol=1.0, depth_tol=0.05)
    yield "valid_a_zero", (a, np.zeros_like(va), b, vb, CAM), dict(hypotheses=7, min_points=3, seed=5)
    yield "valid_b_zero", (a, va, b, np.zeros_like(vb), CAM), dict(hypotheses=7, min_points=3, seed=5)
    # collinear and repeated triples in either set among good points
    a, b = stack([pair(10, 40, share=0.0)])
    a, b = a.copy(), b.copy()
    line = np.arange(8, dtype=np.float32)[:, None] * np.array([0.25, 0.5, 0.125], dtype=np.float32)
    a[0, :8] = a[0, 0] + line
    b[0, 8:16] = b[0, 8]
    yield "degenerate_triples", (a, ones(1, 40), b, ones(1, 40), CAM), dict(hypotheses=128, min_points=6, seed=2)
    # every sampled triple is skipped: a on one line; candidate K alone is scored and wins under wide tolerances, loses under the defaults
    al = a.copy()
    al[0] = a[0, 0] + np.arange(40, dtype=np.float32)[:, None] * np.array([0.25, 0.5, 0.125], dtype=np.float32)
    for tol, dt in ((2.0, 0.1), (1.0e6, 1.0e3)):
        yield "all_skipped_%d" % tol, (al, ones(1, 40), b, ones(1, 40), CAM), dict(hypotheses=70, min_points=6, seed=1, tol=tol, depth_tol=dt)
    # ties: six clean points, more hypotheses than triples
    a, b = stack([pair(6, 6, share=0.0, depth_noise=0.0, ray_noise=0.0)])
    yield "ties", (a, ones(1, 6), b, ones(1, 6), CAM), dict(hypotheses=256, min_points=6, seed=3)
    # identical sets: the exact identity; coplanar sets
    a, _ = stack([pair(12, 200)])
    yield "identical", (a, ones(1, 200), a.copy(), ones(1, 200), CAM), dict(hypotheses=64, min_points=8, seed=6)
    a, b = stack([pair(13, 300, plane=True), pair(14, 300, share=0.4, plane=True)])
    yield "coplanar", (a, ones(2, 300), b, ones(2, 300), CAM), dict(hypotheses=128, min_points=8, seed=7)
    # a unit so small that near points exceed the reach cap (bit 2), and a camera that is not square
    sc = planted(15, N=120, share=0.1)
    a, b = sc["a"][None].copy(), sc["b"][None].copy()
    b[0, :6] *= np.float32(1.0 / 256.0)  # six points 256 times nearer than the rest, the same in both sets
    a[0, :6] = ((b[0, :6].astype(np.float64) - sc["t"]) @ sc["R"] / sc["s"]).astype(np.float32)
    yield "left_out", (a, ones(1, 120), b, ones(1, 120), (900.0, 1100.0, 955.5, 541.25)), dict(hypotheses=96, min_points=8, seed=8,
                                                                                            tol=3.0, depth_tol=0.2)
