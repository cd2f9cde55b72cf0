"""The rules of ctk_fit_resection (include/ctk.h, "fit resection"; co-tracker_amd/csrc/resection_math.h) restated in numpy and Python
numbers: what the kernel (tests/test_gpu_resection.py) and the g++ build of the header (tests/test_resection_host.py) are compared
with, exactly.  Positions and the pair rule are motion_reference's, the L D L^T solve and the IEEE division are planes_reference's,
dot / cross / polar / valid / sums are pose_reference's.  Everything in double is one float64 operation per step in the header's
order; what one thread does in the kernel is Python floats here, what every entry does is numpy over the entries."""
import numpy as np

import motion_reference as R
import planes_reference as PR
import pose_reference as PO

UNFIX = PR.UNFIX
div = PR.div
LIST_MAX, MIN_POINTS, HYPOTHESES_MAX, ROUNDS, SOLVE_MIN = 4096, 6, 1024, 3, 6
EYE = ([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0])
EYE32 = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float32)
ROUND_BITS = (1, 2, 16)


def seed_pose(m12):
    """Twelve float32 (R | t) -> (R0: nine floats, t0: three floats)."""
    m = np.asarray(m12, dtype=np.float32).reshape(12)
    if not np.isfinite(m).all():
        return EYE
    Rm = [float(m[r * 4 + c]) for r in range(3) for c in range(3)]
    t = [float(m[3]), float(m[7]), float(m[11])]
    Rm, det = PO.polar(Rm)
    return (Rm, t) if PO.valid(Rm, t, det) else EYE


def tol2(tol):
    t = float(np.float32(tol))
    return t * t


def c2(cam):
    fx, fy = cam[0], cam[1]
    return 256.0 * (fx * fx + fy * fy)


def apply(Rm, t, X):
    """X: three arrays -> X' = R X + t, three arrays."""
    return [PO.dot(Rm[i * 3:i * 3 + 3], X) + t[i] for i in range(3)]


def shift(a, s, t0):
    return [a[i] + s * t0[i] for i in range(3)]


def error(cam, Xc, Q):
    """-> (e float64 [n], +inf behind the camera; u, v, dx, dy, iz)."""
    fx, fy, cx, cy = cam
    with np.errstate(all="ignore"):
        front = Xc[2] > 0.0
        iz = 1.0 / Xc[2]
        u, v = Xc[0] * iz, Xc[1] * iz
        dx = (fx * u + cx) - Q[:, 0].astype(np.float64) / 16.0
        dy = (fy * v + cy) - Q[:, 1].astype(np.float64) / 16.0
        e = dx * dx + dy * dy
        e = np.where(front & ~np.isnan(e), e, np.inf)
    return e, (u, v, dx, dy, iz)


def scale(cam, a, q, t0):
    """One entry (a: three floats, q: two integers) -> s (a float, inf where there is none)."""
    y = [float(v[0]) for v in PO.rays(cam, np.array([q], dtype=np.int64))]
    yy, tt, yt, ya, ta = PO.dot(y, y), PO.dot(t0, t0), PO.dot(y, t0), PO.dot(y, a), PO.dot(t0, a)
    den = yy * tt - yt * yt
    if not (den > 0.0):
        return float("inf")
    return div(yt * ya - yy * ta, den)


def entries(cam, cc, Xc, uvd):
    """The entries within tol (arrays) -> (vx, vy: seven arrays each, takes part bool [n])."""
    fx, fy = cam[0], cam[1]
    u, v, dx, dy, iz = uvd
    with np.errstate(all="ignore"):
        ax, ay = fx * iz, fy * iz
        bx, by = ax * u, ay * v
        zero = np.zeros_like(iz)
        gx, gy = [ax, zero, -bx], [zero, ay, -by]
        vx = PO.cross(Xc, gx) + gx + [dx]
        vy = PO.cross(Xc, gy) + gy + [dy]
        cap = 16.0 * cc
        take = np.ones(iz.shape, dtype=bool)
        for a in vx + vy:
            take = take & (a * a <= cap)
    return vx, vy, take


def sums(v, ic2, take):
    """One component's rows -> its 28 sums as Python integers, in the header's order."""
    v = [a[take] for a in v]
    out = []
    for i, j in [(i, j) for i in range(6) for j in range(i, 6)] + [(i, 6) for i in range(7)]:
        w = (v[i] * v[j]) * ic2
        assert w.size == 0 or float(np.abs(w).max()) <= 16.0 * (1.0 + 2.0 ** -50)
        out.append(int(np.rint(w * PR.FIX).astype(np.int64).sum()))
        assert abs(out[-1]) < 2 ** 61
    return out


def update(Rm, t, s, n):
    """One round from its sums -> (R, t), or None."""
    if n < SOLVE_MIN:
        return None
    N = [[0.0] * 8 for _ in range(8)]
    for i in range(6):
        for j in range(6):
            N[i][j] = float(s[PO.sum_index(min(i, j), max(i, j))]) * UNFIX
    N[6][6] = N[7][7] = 1.0
    b = [-(float(s[21 + i]) * UNFIX) for i in range(6)] + [0.0, 0.0]
    h = PR.solve(N, b)
    if h is None:
        return None
    W = PO.skew_times(h[:3], Rm)
    R2, det = PO.polar([Rm[i] + W[i] for i in range(9)])
    t2 = [t[0] + h[3], t[1] + h[4], t[2] + h[5]]
    return (R2, t2) if PO.valid(R2, t2, det) else None


def fit_list(Q, X32, seed12, cam, f, tol, K, seed, min_points, still=False, details=None):
    """Q int64 [A,2], X32 float32 [A,3]: every structure point with a correspondence, in ascending n; still: Q = P on all of them ->
    (pose float32 [12], label int8 [A], error float32 [A], (M, labelled 1, k, bits))."""
    A = Q.shape[0]
    M = min(A, LIST_MAX)
    still = bool(still) and A > 0
    bits = (8 if A > LIST_MAX else 0) | (32 if still else 0)
    none = (EYE32, np.zeros(A, dtype=np.int8), np.full(A, -1.0, dtype=np.float32))
    if M < min_points:
        return none + ((M, 0, -1, bits),)
    X = [X32[:, i].astype(np.float64) for i in range(3)]
    R0, t0 = seed_pose(seed12)
    t2 = tol2(tol)
    Xl, Ql = [v[:M] for v in X], Q[:M]
    a = [PO.dot(R0[i * 3:i * 3 + 3], Xl) for i in range(3)]
    cands = []
    for k in range(0 if still else K):
        i = R.sample(seed, f, k, M, R.TRANSLATION)[0]
        s = scale(cam, [float(a[0][i]), float(a[1][i]), float(a[2][i])], (int(Ql[i, 0]), int(Ql[i, 1])), t0)
        cands.append(s if (s > 0.0 and PO.finite(s)) else None)
    cands = [None] * (K + 2) + ["eye"] if still else cands + [1.0, 0.0, "eye"]
    best, bk = -1, -1
    memo = {}
    for k, s in enumerate(cands):
        if s is None:
            continue
        if s not in memo:
            Xc = Xl if s == "eye" else shift(a, s, t0)
            memo[s] = int((error(cam, Xc, Ql)[0] <= t2).sum())
        if memo[s] > best:
            best, bk = memo[s], k
    if best < min_points:
        return none + ((M, 0, -1, bits),)
    s = cands[bk]
    Rm, t = (list(EYE[0]), list(EYE[1])) if s == "eye" else (list(R0), [s * t0[0], s * t0[1], s * t0[2]])
    cc = c2(cam)
    for rnd in range(0 if still else ROUNDS):
        Xc = apply(Rm, t, Xl)
        e, uvd = error(cam, Xc, Ql)
        inl = e <= t2
        Xi, uvdi = [v[inl] for v in Xc], [v[inl] for v in uvd]
        vx, vy, take = entries(cam, cc, Xi, uvdi)
        if not take.all():
            bits |= 4
        sx, sy = sums(vx, div(1.0, cc), take), sums(vy, div(1.0, cc), take)
        new = update(Rm, t, [p + q for p, q in zip(sx, sy)], int(take.sum()))
        if new is None:
            bits |= ROUND_BITS[rnd]
        else:
            Rm, t = new
    e, _ = error(cam, apply(Rm, t, X), Q)
    label = (e <= t2).astype(np.int8)
    with np.errstate(all="ignore"):
        err = e.astype(np.float32)
    pose = np.array([Rm[0], Rm[1], Rm[2], t[0], Rm[3], Rm[4], Rm[5], t[1], Rm[6], Rm[7], Rm[8], t[2]], dtype=np.float64)
    if details is not None:
        details.update(R=np.array(Rm).reshape(3, 3), t=np.array(t), inliers=label[:M] == 1)
    return pose.astype(np.float32), label, err, (M, int(label.sum()), bk, bits)


def fit_resection(coords, intrinsics, structure, valid, seed_poses, visible=None, vis=None, conf=None, thresh=0.0, first_row=None,
                  N_out=None, f0=0, F=1, to=None, lag=None, anchor=None, tol=2.0, hypotheses=256, seed=0, min_points=16,
                  scale=(1.0, 1.0)):
    """coords float32 [G,R,N,2]; structure float32 [G,N,3], valid int8 [G,N], seed_poses float32 [G,F,3,4]; the source forms, first_row,
    visible or logits: pose_reference.fit_pose's -> (pose float32 [G,F,3,4], label int8 [G,F,N_out], error float32 [G,F,N_out],
    stats int32 [G,F,4])."""
    coords = np.asarray(coords, dtype=np.float32)
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    assert (to is not None) + (lag is not None) + (anchor is not None) == 1 and (lag is None or lag >= 1) and (to is None or to >= 0)
    assert MIN_POINTS <= min_points <= 8192 and 1 <= hypotheses <= HYPOTHESES_MAX
    cam = PO.camera(intrinsics)
    structure = np.asarray(structure, dtype=np.float32).reshape(G, N, 3)
    valid = np.asarray(valid).reshape(G, N)
    seed_poses = np.asarray(seed_poses, dtype=np.float32).reshape(G, F, 12)

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
    pose = np.zeros((G, F, 12), dtype=np.float32)
    label = np.full((G, F, N_out), -1, dtype=np.int8)
    err = np.full((G, F, N_out), -1.0, dtype=np.float32)
    stats = np.zeros((G, F, 4), dtype=np.int32)
    for g in range(G):
        first = np.zeros(N, dtype=np.int64) if first_row is None else np.asarray(first_row[g], dtype=np.int64)
        in_structure = (valid[g] != 0) & np.isfinite(structure[g]).all(axis=1)
        for jf in range(F):
            f = f0 + jf
            fs = anchor[2] if anchor is not None else (to if to is not None else f - lag)
            corr = np.zeros(N_out, dtype=bool)
            src = pos[g, 0]
            if fs >= 0:
                src, src_good = (a_pos[g], a_good[g]) if anchor is not None else (pos[g, fs % R_], good[g, fs % R_])
                corr = src_good[:N_out] & good[g, f % R_, :N_out] & (fs >= first[:N_out]) & (f >= first[:N_out])
            idx = np.nonzero(corr & in_structure[:N_out])[0]
            po, la, er, st = fit_list(pos[g, f % R_][idx], structure[g][idx], seed_poses[g, jf], cam, f, tol, hypotheses, seed, min_points,
                                      still=bool((src[idx] == pos[g, f % R_][idx]).all()))
            pose[g, jf], stats[g, jf] = po, st
            label[g, jf, idx], err[g, jf, idx] = la, er
    return pose.reshape(G, F, 3, 4), label, err, stats


# ---- planted camera paths ----------------------------------------------------------------------------------------------------------------
def scene(seed, G, T, N, src=0, hw=(270, 480), movers=0.2, noise=0.05, p_visible=0.95):
    """A stream-shaped history: a camera of focal length 0.9 W that translates and turns from frame to frame through G static scenes
    3..12 deep; a fraction `movers` of the points drifts on its own ->
    dict(coords float32 [G,T,N,2], visible uint8 [G,T,N], mover bool [G,N], structure float32 [G,N,3]: every point in the camera
    coordinates of frame `src`, truth float64 [G,T,3,4]: (R | t) from frame `src` to frame f, cam)."""
    from epipolar_reference import rotation
    rng = np.random.default_rng(seed)
    Hd, Wd = hw
    fl = 0.9 * Wd
    cam = (fl, fl, Wd / 2.0, Hd / 2.0)
    coords = np.zeros((G, T, N, 2), dtype=np.float32)
    mover = np.zeros((G, N), dtype=bool)
    structure = np.zeros((G, N, 3), dtype=np.float32)
    truth = np.zeros((G, T, 3, 4))
    for g in range(G):
        P = np.stack([rng.uniform(8, Wd - 8, N), rng.uniform(8, Hd - 8, N)], axis=1)
        z = rng.uniform(3.0, 12.0, N)
        X = np.stack([(P[:, 0] - cam[2]) / fl * z, (P[:, 1] - cam[3]) / fl * z, z], axis=1)  # frame 0's camera coordinates
        step, turn = np.array([0.05, 0.004, 0.01]) * (1.0 + 0.3 * g), rng.uniform(-0.004, 0.004, 3)
        ids = rng.permutation(N)[:int(N * movers)]
        mover[g, ids] = True
        drift = np.zeros((N, 2))
        drift[ids] = rng.uniform(3.0, 6.0) * np.array([np.cos(1.0 + g), np.sin(1.0 + g)])
        Rs, ts = rotation(*(turn * src)), step * src
        structure[g] = ((Rs @ X.T).T + ts).astype(np.float32)
        for t in range(T):
            Rt, tt = rotation(*(turn * t)), step * t
            Xt = (Rt @ X.T).T + tt
            coords[g, t] = np.stack([fl * Xt[:, 0] / Xt[:, 2] + cam[2], fl * Xt[:, 1] / Xt[:, 2] + cam[3]], axis=1) + \
                drift * (t - src) + rng.normal(0.0, noise, (N, 2))
            Rr = Rt @ Rs.T
            truth[g, t, :, :3], truth[g, t, :, 3] = Rr, tt - Rr @ ts
    visible = (rng.uniform(size=(G, T, N)) < p_visible).astype(np.uint8)
    return dict(coords=coords, visible=visible, mover=mover, structure=structure, truth=truth, cam=cam)


def unit_seeds(truth, frames):
    """truth [G,T,3,4] -> float32 [G,F,3,4]: the planted poses with |t| = 1 as ctk_fit_pose writes them ((R | 0) where t = 0)."""
    out = truth[:, list(frames)].copy()
    n = np.linalg.norm(out[..., 3], axis=-1, keepdims=True)
    out[..., 3] = np.where(n > 0, out[..., 3] / np.where(n > 0, n, 1.0), 0.0)
    return out.astype(np.float32)


def spoil_structure(structure, valid):
    """NaN, infinite and behind-the-camera structure points next to good ones; validity bytes of every kind."""
    structure[0, 5, 0], structure[0, 6, 1], structure[0, 8, 2], structure[-1, 9] = np.nan, np.inf, -np.inf, np.nan
    structure[0, 10, 2] *= -1.0
    structure[-1, 11, 2] = 0.0
    valid[0, 12:18] = (-1, 20, 0, -128, 127, 0)
    valid[-1, 20] = 0


def cases():
    """The shapes at which the kernel can go wrong -> (name, args, kwargs) of fit_resection, one after the other."""
    import objects_reference as O
    # an anchor the ring has dropped with a slot released after it; first rows; NaN and outside positions; spoiled structure and seeds
    G, T, N, N_out = 2, 8, 123, 120
    sc = scene(3, G, T, N, src=1)
    coords, visible = sc["coords"], sc["visible"]
    first = O.spoil(coords, N_out)
    first[1, 7] = 2
    visible[0, :, 10] = 1  # the point that spoil_structure puts behind the camera is seen
    valid = np.ones((G, N), dtype=np.int8)
    structure = sc["structure"].copy()
    spoil_structure(structure, valid)
    seeds = unit_seeds(sc["truth"], range(3, 6))
    seeds[1, 0], seeds[1, 1, 1, 2], seeds[1, 2, :, 3] = 0.0, np.nan, 0.0  # zero, NaN, t = 0 (a tie of the fixed candidates)
    seeds[0, 1, 2, 3] = np.inf
    anchor = (coords[:, 1].copy(), visible[:, 1].copy(), 1)
    yield "anchor_ring", (R.fold(coords, 6, 8), sc["cam"], structure, valid, seeds), dict(
        visible=R.fold(visible, 6, 8), first_row=first, N_out=N_out, f0=3, F=3, anchor=anchor, tol=2.0, hypotheses=256, seed=11, min_points=12)
    yield "anchor_no_first_row", (coords, sc["cam"], structure, valid, seeds), dict(
        visible=visible, N_out=N_out, f0=3, F=3, anchor=anchor, tol=1.0, hypotheses=33, seed=2, min_points=6)
    # a fixed frame, the frame itself among the rows (the (I, 0) candidate), one hypothesis
    sc = scene(4, 2, 5, 64, src=2)
    seeds = unit_seeds(sc["truth"], range(1, 4))
    yield "fixed_to", (sc["coords"], sc["cam"], sc["structure"], np.ones((2, 64), dtype=np.int8), seeds), dict(
        visible=sc["visible"], f0=1, F=3, to=2, tol=2.0, hypotheses=1, seed=5, min_points=16)
    yield "valid_all_zero", (sc["coords"], sc["cam"], sc["structure"], np.zeros((2, 64), dtype=np.int8), seeds), dict(
        visible=sc["visible"], f0=1, F=3, to=2, tol=2.0, hypotheses=7, seed=5, min_points=6)
    # lag across a ring wrap, logits instead of `visible`, a scale
    sc = scene(5, 1, 8, 257, src=2)
    rng = np.random.default_rng(5)
    vis_l = np.where(sc["visible"] != 0, 4.0, -4.0).astype(np.float32) + rng.uniform(-1, 1, sc["visible"].shape).astype(np.float32)
    cam = (1.37 * sc["cam"][0], 0.81 * sc["cam"][1], 1.37 * sc["cam"][2], 0.81 * sc["cam"][3])
    seeds = unit_seeds(sc["truth"], (5, 5, 5))
    yield "lag_wrap_logits", (R.fold(sc["coords"], 6, 8), cam, sc["structure"], np.ones((1, 257), dtype=np.int8), seeds), dict(
        vis=R.fold(vis_l, 6, 8), conf=np.full((1, 6, 257), 5.0, dtype=np.float32), thresh=0.6, N_out=257, f0=5, F=3, lag=3, tol=2.0,
        hypotheses=257, seed=1, min_points=16, scale=(1.37, 0.81))
    # M exactly min_points and one below: six clean points, more hypotheses than entries (ties between candidates)
    sc = scene(6, 1, 3, 6, src=0, movers=0.0, noise=0.0, p_visible=2.0)
    seeds = unit_seeds(sc["truth"], (2,))
    for one_less in (False, True):
        valid = np.ones((1, 6), dtype=np.int8)
        valid[0, 3] = 0 if one_less else 1
        yield "six_points_%d" % (5 if one_less else 6), (sc["coords"], sc["cam"], sc["structure"], valid, seeds), dict(
            visible=sc["visible"], f0=2, F=1, to=0, tol=2.0, hypotheses=256, seed=3, min_points=6)
    # a wide tolerance lets the fixed candidates (R0, t0), (R0, 0) and (I, 0) win on the rows whose seed is zero, NaN or has t = 0
    sc = scene(3, 2, 8, 123, src=1)
    seeds = unit_seeds(sc["truth"], range(3, 6))
    seeds[1, 0], seeds[1, 1, 1, 2], seeds[1, 2, :, 3] = 0.0, np.nan, 0.0
    seeds[0, 2, :, 3] *= 0.0875  # close to the planted length: (R0, t0) is in the running
    yield "fixed_candidates", (sc["coords"], sc["cam"], sc["structure"], np.ones((2, 123), dtype=np.int8), seeds), dict(
        visible=sc["visible"], f0=3, F=3, to=1, tol=24.0, hypotheses=4, seed=0, min_points=6)
    # a structure in a unit so large that every point is nearer than 1 / 64: the cap leaves every entry out, every round keeps its pose
    sc = scene(8, 1, 4, 40, src=0)
    yield "cap_leaves_out", (sc["coords"], sc["cam"], sc["structure"] / 4096.0, np.ones((1, 40), dtype=np.int8), unit_seeds(sc["truth"], (2, 3))), dict(
        visible=sc["visible"], f0=2, F=2, to=0, tol=2.0, hypotheses=64, seed=4, min_points=6)
    # sizes round the chunk and the largest
    for N, N_out, every, K in ((255, 255, 1, 1), (600, 600, 1, 1024), (8192, 8192, 2, 1024), (8192, 8192, 1, 33)):
        sc = scene(N, 1, 2, N, src=0, movers=0.1)
        valid = np.zeros((1, N), dtype=np.int8)
        valid[0, ::every] = 1
        yield "size_%d_%d_%d" % (N_out, every, K), (sc["coords"], sc["cam"], sc["structure"], valid, unit_seeds(sc["truth"], (1,))), dict(
            visible=sc["visible"], N_out=N_out, f0=1, F=1, lag=1, tol=2.0, hypotheses=K, seed=N, min_points=16)
    # the list cap itself: every slot a structure point with a correspondence, so the list holds exactly N_out entries -- 4096 fill it
    # (no bit), 4097 overflow it by the one entry of the last chunk (bit 3; the 4097th is classified all the same)
    sc = scene(4100, 1, 2, 4100, src=0, movers=0.1, p_visible=2.0)
    for N_out in (4096, 4097):
        yield "cap_%d" % N_out, (sc["coords"], sc["cam"], sc["structure"], np.ones((1, 4100), dtype=np.int8), unit_seeds(sc["truth"], (1,))), dict(
            visible=sc["visible"], N_out=N_out, f0=1, F=1, lag=1, tol=2.0, hypotheses=256, seed=7, min_points=16)


def structure_from_pose(coords_row, intrinsics, depth, label, max_depth=64.0, scale=(1.0, 1.0)):
    """ops.structure_from_pose in numpy float32: coords_row float32 [N,2] on the later frame of the pair, depth float32 [N,2] and label
    int8 [N] as ctk_fit_pose and ctk_fit_epipolar wrote them -> (points float32 [N,3], valid int8 [N])."""
    fx, fy, cx, cy = (np.float32(v) for v in intrinsics)
    c = np.asarray(coords_row, dtype=np.float32)
    zs, zf = depth[..., 0], depth[..., 1]
    with np.errstate(all="ignore"):
        rx, ry = (c[..., 0] * np.float32(scale[0]) - cx) / fx, (c[..., 1] * np.float32(scale[1]) - cy) / fy
        ok = (label == 1) & np.isfinite(zs) & np.isfinite(zf) & (zs > 0) & (zf > 0) & (zf <= np.float32(max_depth))
        pts = np.stack([rx * zf, ry * zf, zf], axis=-1)
    return np.where(ok[..., None], pts, np.float32(0)).astype(np.float32), ok.astype(np.int8)


def planted_path(seed, kind, T=12):
    """epipolar_reference.planted's scenes (1080p, focal length 1000 px, depths 3..12 m, 0.1 px noise, 25 % movers in three groups;
    "sideways", "forward", "few" = 90 points) extended to a camera path: row 0 is the earlier frame of the reconstruct pair, row 1 the
    later one (the structure's frame), rows 2 .. T the T frames that are localised: the first of them IS the structure's frame (the
    same positions), the last returns to its position with the camera turned, the others go on along the pair's direction with a
    sideways swing.  -> dict(coords float32 [1,T+2,N,2], mover bool [N], truth float64 [T,3,4]: (R | t) from the structure's frame to
    each localised frame in units of the pair's baseline, pair: that of the pair itself)."""
    from epipolar_reference import rotation
    rng = np.random.default_rng(seed)
    N = 90 if kind == "few" else 400
    Wd, Hd, fl = 1920.0, 1080.0, 1000.0
    P = np.stack([rng.uniform(40, Wd - 40, N), rng.uniform(40, Hd - 40, N)], axis=1)
    z = rng.uniform(3.0, 12.0, N)
    X = np.stack([(P[:, 0] - Wd / 2) / fl * z, (P[:, 1] - Hd / 2) / fl * z, z], axis=1)
    step = np.array([0.0, 0.02, 0.35]) if kind == "forward" else np.array([0.30, 0.03, 0.02])
    swing = np.array([0.12, -0.05, 0.0]) if kind == "forward" else np.array([0.0, 0.06, 0.10])
    mover = np.zeros(N, dtype=bool)
    order = rng.permutation(N)
    drift = np.zeros((N, 2))
    for grp in range(3):
        ids = order[grp * (N // 4) // 3:(grp + 1) * (N // 4) // 3]
        mover[ids] = True
        ang = rng.uniform(0, 2 * np.pi)
        drift[ids] = rng.uniform(25.0, 60.0) * np.array([np.cos(ang), np.sin(ang)])
    # camera j: X_j = R_j X + t_j in the earlier frame's coordinates; "time" in units of the pair
    times = [0.0, 1.0, 1.0] + [1.0 + 0.35 * j for j in range(1, T - 1)] + [1.0]
    poses = []
    for i, tm in enumerate(times):
        Rj = rotation(*(rng.uniform(-0.02, 0.02, 3) * (0.0 if i == 0 else 1.0 + 0.3 * (tm - 1.0))))
        tj = step * tm + swing * np.sin(0.6 * (tm - 1.0))
        if i == 2:
            Rj, tj = poses[1]
        elif i == len(times) - 1:  # back at the structure's position, turned
            tj = Rj @ (poses[1][0].T @ poses[1][1])
        poses.append((Rj, tj))
    coords = np.zeros((1, T + 2, N, 2))
    for i, (Rj, tj) in enumerate(poses):
        Xj = X @ Rj.T + tj
        coords[0, i] = np.stack([fl * Xj[:, 0] / Xj[:, 2] + Wd / 2, fl * Xj[:, 1] / Xj[:, 2] + Hd / 2], axis=1) + drift * times[i] + \
            rng.normal(0.0, 0.1, (N, 2))
    coords[0, 2] = coords[0, 1]
    Ra, ta = poses[1]
    base = float(np.linalg.norm(ta))
    truth = np.zeros((T, 3, 4))
    for j in range(T):
        Rj, tj = poses[2 + j]
        Rr = Rj @ Ra.T
        truth[j, :, :3], truth[j, :, 3] = Rr, (tj - Rr @ ta) / base
    truth[0, :, 3] = 0.0
    pair = np.concatenate([Ra, (ta / base)[:, None]], axis=1)
    return dict(coords=coords.astype(np.float32), mover=mover, truth=truth, pair=pair)
