"""The rules of ctk_fit_p3p (include/ctk.h, "fit p3p"; co-tracker_amd/csrc/p3p_math.h) restated in numpy and Python numbers: what the
kernel (tests/test_gpu_p3p.py) and the g++ build of the header (tests/test_p3p_host.py) are compared with, exactly.  Everything but
the candidates is resection_reference's, reused: the gather, the fit list, project and within, the still rule, the score, the rounds
and the outputs.  A candidate is what one lane does in the kernel: Python floats here, one IEEE operation per step in the header's
order; what every entry does is numpy over the entries."""
import numpy as np

import motion_reference as R
import planes_reference as PR
import pose_reference as PO
import resection_reference as RR

div = PR.div
ROUNDS = 6
LIST_MAX, MIN_POINTS, HYPOTHESES_MAX = RR.LIST_MAX, RR.MIN_POINTS, RR.HYPOTHESES_MAX
EYE, EYE32 = RR.EYE, RR.EYE32


def cofactors(A):
    """Nine floats row major -> (the cofactors, row r = cross(row r + 1, row r + 2); the determinant)."""
    C = PO.cross(A[3:6], A[6:9]) + PO.cross(A[6:9], A[0:3]) + PO.cross(A[0:3], A[3:6])
    return C, PO.dot(A[0:3], C[0:3])


def solve(J, r):
    """J x = r -> x, or None."""
    C, det = cofactors(J)
    if det == 0.0 or not PO.finite(det):
        return None
    inv = div(1.0, det)
    return [PO.dot([C[i], C[3 + i], C[6 + i]], r) * inv for i in range(3)]


def row(li, lj, yyi, yyj, c, d):
    """-> (the residual, the two non-zeros of the Jacobian's row)."""
    r = (((li * li) * yyi + (lj * lj) * yyj) - 2.0 * ((li * lj) * c)) - d
    return r, 2.0 * (li * yyi - lj * c), 2.0 * (lj * yyj - li * c)


def candidate(cam, X, q):
    """Three entries: X three lists of three floats, q three pairs of integers -> (R nine floats, t three floats), or None."""
    fx, fy, cx, cy = cam
    y = [[div(float(qx) / 16.0 - cx, fx), div(float(qy) / 16.0 - cy, fy), 1.0] for qx, qy in q]
    yy = [PO.dot(v, v) for v in y]
    l = []
    for i in range(3):
        XX = PO.dot(X[i], X[i])
        if not (XX > 0.0) or not PO.finite(XX):
            return None
        l.append(XX * PO.rsqrt(XX * yy[i]))
    pairs = ((0, 1), (0, 2), (1, 2))
    c = [PO.dot(y[i], y[j]) for i, j in pairs]
    d = []
    for i, j in pairs:
        e = [X[i][0] - X[j][0], X[i][1] - X[j][1], X[i][2] - X[j][2]]
        d.append(PO.dot(e, e))
    for _ in range(ROUNDS):
        J, r = [0.0] * 9, [0.0] * 3
        for n, (i, j) in enumerate(pairs):
            r[n], J[n * 3 + i], J[n * 3 + j] = row(l[i], l[j], yy[i], yy[j], c[n], d[n])
        x = solve(J, r)
        if x is None:
            return None
        l = [l[0] - x[0], l[1] - x[1], l[2] - x[2]]
    if not all(v > 0.0 and PO.finite(v) for v in l):
        return None
    Y = [[l[i] * y[i][j] for j in range(3)] for i in range(3)]

    def frame(P):
        a1, a2 = [P[1][j] - P[0][j] for j in range(3)], [P[2][j] - P[0][j] for j in range(3)]
        a3 = PO.cross(a1, a2)
        return [a1[0], a2[0], a3[0], a1[1], a2[1], a3[1], a1[2], a2[2], a3[2]]
    A, B = frame(X), frame(Y)
    C, detA = cofactors(A)
    if not (detA > 0.0):
        return None
    inv = div(1.0, detA)
    Rm, det = PO.polar([PO.dot(B[i * 3:i * 3 + 3], C[j * 3:j * 3 + 3]) * inv for i in range(3) for j in range(3)])
    t = [Y[0][i] - PO.dot(Rm[i * 3:i * 3 + 3], X[0]) for i in range(3)]
    return (Rm, t) if PO.valid(Rm, t, det) else None


def fit_list(Q, X32, cam, f, tol, K, seed, min_points, still=False, details=None):
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
    t2 = RR.tol2(tol)
    Xl, Ql = [v[:M] for v in X], Q[:M]
    cands = []
    for k in range(0 if still else K):
        idx = PR.sample(seed, f, k, M)[:3]
        cands.append(candidate(cam, [[float(Xl[0][i]), float(Xl[1][i]), float(Xl[2][i])] for i in idx],
                               [(int(Ql[i, 0]), int(Ql[i, 1])) for i in idx]))
    cands = [None] * K + [EYE] if still else cands + [EYE]
    best, bk = -1, -1
    counts = []
    for k, c in enumerate(cands):
        if c is None:
            counts.append(-1)
            continue
        counts.append(int((RR.error(cam, RR.apply(c[0], c[1], Xl), Ql)[0] <= t2).sum()))
        if counts[-1] > best:
            best, bk = counts[-1], k
    if details is not None:
        details.update(counts=counts, made=sum(c is not None for c in cands[:K]))
    if best < min_points:
        return none + ((M, 0, -1, bits),)
    Rm, t = list(cands[bk][0]), list(cands[bk][1])
    cc = RR.c2(cam)
    for rnd in range(0 if still else RR.ROUNDS):
        Xc = RR.apply(Rm, t, Xl)
        e, uvd = RR.error(cam, Xc, Ql)
        inl = e <= t2
        Xi, uvdi = [v[inl] for v in Xc], [v[inl] for v in uvd]
        vx, vy, take = RR.entries(cam, cc, Xi, uvdi)
        if not take.all():
            bits |= 4
        sx, sy = RR.sums(vx, div(1.0, cc), take), RR.sums(vy, div(1.0, cc), take)
        new = RR.update(Rm, t, [p + q for p, q in zip(sx, sy)], int(take.sum()))
        if new is None:
            bits |= RR.ROUND_BITS[rnd]
        else:
            Rm, t = new
    e, _ = RR.error(cam, RR.apply(Rm, t, X), Q)
    label = (e <= t2).astype(np.int8)
    with np.errstate(all="ignore"):
        err = e.astype(np.float32)
    pose = np.array([Rm[0], Rm[1], Rm[2], t[0], Rm[3], Rm[4], Rm[5], t[1], Rm[6], Rm[7], Rm[8], t[2]], dtype=np.float64)
    if details is not None:
        details.update(R=np.array(Rm).reshape(3, 3), t=np.array(t), inliers=label[:M] == 1)
    return pose.astype(np.float32), label, err, (M, int(label.sum()), bk, bits)


def fit_p3p(coords, intrinsics, structure, valid, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1,
            to=None, lag=None, anchor=None, tol=2.0, hypotheses=256, seed=0, min_points=16, scale=(1.0, 1.0), details=None):
    """coords float32 [G,R,N,2]; structure float32 [G,N,3], valid int8 [G,N]; the source forms, first_row, visible or logits:
    resection_reference.fit_resection's -> (pose float32 [G,F,3,4], label int8 [G,F,N_out], error float32 [G,F,N_out], stats int32
    [G,F,4]).  details: a dict that takes {(g, frame row): fit_list's details}."""
    coords = np.asarray(coords, dtype=np.float32)
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    assert (to is not None) + (lag is not None) + (anchor is not None) == 1 and (lag is None or lag >= 1) and (to is None or to >= 0)
    assert MIN_POINTS <= min_points <= 8192 and 1 <= hypotheses <= HYPOTHESES_MAX
    cam = PO.camera(intrinsics)
    structure = np.asarray(structure, dtype=np.float32).reshape(G, N, 3)
    valid = np.asarray(valid).reshape(G, N)

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
        with np.errstate(all="ignore"):
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
            d = None if details is None else details.setdefault((g, jf), {})
            po, la, er, st = fit_list(pos[g, f % R_][idx], structure[g][idx], cam, f, tol, hypotheses, seed, min_points,
                                      still=bool((src[idx] == pos[g, f % R_][idx]).all()), details=d)
            pose[g, jf], stats[g, jf] = po, st
            label[g, jf, idx], err[g, jf, idx] = la, er
    return pose.reshape(G, F, 3, 4), label, err, stats


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def cases():
    """The shapes at which the kernel can go wrong -> (name, args, kwargs) of fit_p3p, one after the other.  The scenes are
    resection_reference's; few large cases, since a candidate is a Python loop."""
    import objects_reference as O
    # an anchor the ring has dropped with a slot released after it; first rows; NaN and outside positions; spoiled structure; G = 2, F = 3
    G, T, N, N_out = 2, 8, 123, 120
    sc = RR.scene(3, G, T, N, src=1)
    coords, visible = sc["coords"], sc["visible"]
    first = O.spoil(coords, N_out)
    first[1, 7] = 2
    visible[0, :, 10] = 1  # the point that spoil_structure puts behind the camera is seen
    valid = np.ones((G, N), dtype=np.int8)
    structure = sc["structure"].copy()
    RR.spoil_structure(structure, valid)
    structure[1, 30:33] = 0.0  # zero points: XX = 0 skips the candidates that draw one
    anchor = (coords[:, 1].copy(), visible[:, 1].copy(), 1)
    yield "anchor_ring", (R.fold(coords, 6, 8), sc["cam"], structure, valid), dict(
        visible=R.fold(visible, 6, 8), first_row=first, N_out=N_out, f0=3, F=3, anchor=anchor, tol=2.0, hypotheses=65, seed=11, min_points=12)
    yield "anchor_no_first_row", (coords, sc["cam"], structure, valid), dict(
        visible=visible, N_out=N_out, f0=3, F=3, anchor=anchor, tol=1.0, hypotheses=33, seed=2, min_points=6)
    # a fixed frame, the frame itself among the rows (still: (I, 0) alone), one hypothesis
    sc = RR.scene(4, 2, 5, 64, src=2)
    yield "fixed_to", (sc["coords"], sc["cam"], sc["structure"], np.ones((2, 64), dtype=np.int8)), dict(
        visible=sc["visible"], f0=1, F=3, to=2, tol=2.0, hypotheses=1, seed=5, min_points=16)
    # the fixed-frame form across a ring wrap: a ring of 6 rows after 8 frames, frames 5..7 against frame 3
    sc8 = RR.scene(12, 1, 8, 96, src=3)
    yield "to_ring", (R.fold(sc8["coords"], 6, 8), sc8["cam"], sc8["structure"], np.ones((1, 96), dtype=np.int8)), dict(
        visible=R.fold(sc8["visible"], 6, 8), f0=5, F=3, to=3, tol=2.0, hypotheses=40, seed=8, min_points=16)
    yield "valid_all_zero", (sc["coords"], sc["cam"], sc["structure"], np.zeros((2, 64), dtype=np.int8)), dict(
        visible=sc["visible"], f0=1, F=3, to=2, tol=2.0, hypotheses=7, seed=5, min_points=6)
    # lag across a ring wrap, logits instead of `visible`, a scale; one more than a generation batch (256 candidates a workgroup)
    sc = RR.scene(5, 1, 8, 257, src=2)
    rng = np.random.default_rng(5)
    vis_l = np.where(sc["visible"] != 0, 4.0, -4.0).astype(np.float32) + rng.uniform(-1, 1, sc["visible"].shape).astype(np.float32)
    cam = (1.37 * sc["cam"][0], 0.81 * sc["cam"][1], 1.37 * sc["cam"][2], 0.81 * sc["cam"][3])
    yield "lag_wrap_logits", (R.fold(sc["coords"], 6, 8), cam, sc["structure"], np.ones((1, 257), dtype=np.int8)), dict(
        vis=R.fold(vis_l, 6, 8), conf=np.full((1, 6, 257), 5.0, dtype=np.float32), thresh=0.6, N_out=257, f0=5, F=3, lag=3, tol=2.0,
        hypotheses=257, seed=1, min_points=16, scale=(1.37, 0.81))
    # M exactly min_points and one below: six clean points, more hypotheses than triples (ties between candidates)
    sc = RR.scene(6, 1, 3, 6, src=0, movers=0.0, noise=0.0, p_visible=2.0)
    for one_less in (False, True):
        valid = np.ones((1, 6), dtype=np.int8)
        valid[0, 3] = 0 if one_less else 1
        yield "six_points_%d" % (5 if one_less else 6), (sc["coords"], sc["cam"], sc["structure"], valid), dict(
            visible=sc["visible"], f0=2, F=1, to=0, tol=2.0, hypotheses=256, seed=3, min_points=6)
    # hypotheses round the generation batch: a lane a candidate, 64 a wave, 256 a workgroup
    sc = RR.scene(9, 1, 3, 80, src=0)
    for K in (63, 64, 65, 255, 256):
        yield "batch_%d" % K, (sc["coords"], sc["cam"], sc["structure"], np.ones((1, 80), dtype=np.int8)), dict(
            visible=sc["visible"], f0=2, F=1, to=0, tol=2.0, hypotheses=K, seed=K, min_points=16)
    # triples that are collinear and triples with a repeated point: eight points on a line, eight copies of one point, among 24 good ones
    sc = RR.scene(10, 1, 3, 40, src=0, movers=0.0, p_visible=2.0)
    structure = sc["structure"].copy()
    structure[0, :8] = structure[0, 0] + np.arange(8, dtype=np.float32)[:, None] * np.array([0.25, 0.5, 0.125], dtype=np.float32)
    structure[0, 8:16] = structure[0, 8]
    yield "degenerate_triples", (sc["coords"], sc["cam"], structure, np.ones((1, 40), dtype=np.int8)), dict(
        visible=sc["visible"], f0=2, F=1, to=0, tol=2.0, hypotheses=128, seed=2, min_points=6)
    # every sampled candidate is skipped: all points on one line; (I, 0) alone is scored, and with a wide tolerance it wins
    line = sc["structure"].copy()
    line[0] = line[0, 0] + np.arange(40, dtype=np.float32)[:, None] * np.array([0.25, 0.5, 0.125], dtype=np.float32)
    for tol in (2.0, 4000.0):
        yield "all_skipped_%d" % tol, (sc["coords"], sc["cam"], line, np.ones((1, 40), dtype=np.int8)), dict(
            visible=sc["visible"], f0=2, F=1, to=0, tol=tol, hypotheses=70, seed=1, min_points=6)
    # a structure in a unit so large that every point is nearer than 1 / 64: the cap leaves every entry out, every round keeps its pose
    sc = RR.scene(8, 1, 4, 40, src=0)
    yield "cap_leaves_out", (sc["coords"], sc["cam"], sc["structure"] / 4096.0, np.ones((1, 40), dtype=np.int8)), dict(
        visible=sc["visible"], f0=2, F=2, to=0, tol=2.0, hypotheses=64, seed=4, min_points=6)
    # sizes round the chunk and the largest
    for N, N_out, every, K in ((255, 255, 1, 1), (256, 256, 1, 5), (600, 600, 1, 1024), (8192, 8192, 2, 40), (8192, 8192, 1, 33)):
        sc = RR.scene(N, 1, 2, N, src=0, movers=0.1)
        valid = np.zeros((1, N), dtype=np.int8)
        valid[0, ::every] = 1
        yield "size_%d_%d_%d" % (N_out, every, K), (sc["coords"], sc["cam"], sc["structure"], valid), dict(
            visible=sc["visible"], N_out=N_out, f0=1, F=1, lag=1, tol=2.0, hypotheses=K, seed=N, min_points=16)
    # the list cap itself: every slot a structure point with a correspondence, so the list holds exactly N_out entries -- 4096 fill it
    # (no bit), 4097 overflow it by the one entry of the last chunk (bit 3; the 4097th is classified all the same)
    sc = RR.scene(4100, 1, 2, 4100, src=0, movers=0.1, p_visible=2.0)
    for N_out in (4096, 4097):
        yield "cap_%d" % N_out, (sc["coords"], sc["cam"], sc["structure"], np.ones((1, 4100), dtype=np.int8)), dict(
            visible=sc["visible"], N_out=N_out, f0=1, F=1, lag=1, tol=2.0, hypotheses=48, seed=7, min_points=16)


# ---- planted scenes ----------------------------------------------------------------------------------------------------------------------
def contaminated(seed, share, frames=3, N=400, plane=False):
    """The scenes the feature is for: 1080p, focal length 1000 px, N points 3..12 deep (plane: on a slanted plane), 0.1 px noise;
    the camera moves 0.2..0.6 units sideways with up to +-0.02 rad of turn on each of `frames` frames; the structure is the truth with
    0.3 % depth noise, every point valid; a `share` of the points moves individually by 8..60 px on every frame ->
    dict(coords float32 [1,frames+1,N,2] (row 0: the structure's frame), structure float32 [N,3], mover bool [N],
    truth float64 [frames,3,4])."""
    from epipolar_reference import rotation
    rng = np.random.default_rng(seed)
    Wd, Hd, fl = 1920.0, 1080.0, 1000.0
    P = np.stack([rng.uniform(40, Wd - 40, N), rng.uniform(40, Hd - 40, N)], axis=1)
    rx, ry = (P[:, 0] - Wd / 2) / fl, (P[:, 1] - Hd / 2) / fl
    z = 6.0 / (1.0 + 0.45 * rx - 0.25 * ry) if plane else rng.uniform(3.0, 12.0, N)  # the plane 0.45 X - 0.25 Y + Z = 6
    X = np.stack([rx * z, ry * z, z], axis=1)
    mover = np.zeros(N, dtype=bool)
    mover[rng.permutation(N)[:int(round(N * share))]] = True
    coords = np.zeros((1, frames + 1, N, 2))
    coords[0, 0] = P + rng.normal(0.0, 0.1, (N, 2))
    truth = np.zeros((frames, 3, 4))
    for j in range(frames):
        Rj = rotation(*rng.uniform(-0.02, 0.02, 3))
        tj = np.array([rng.uniform(0.2, 0.6) * rng.choice([-1.0, 1.0]), rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05)])
        Xj = X @ Rj.T + tj
        ang, far = rng.uniform(0, 2 * np.pi, N), rng.uniform(8.0, 60.0, N)
        move = np.where(mover[:, None], np.stack([far * np.cos(ang), far * np.sin(ang)], axis=1), 0.0)
        coords[0, j + 1] = np.stack([fl * Xj[:, 0] / Xj[:, 2] + Wd / 2, fl * Xj[:, 1] / Xj[:, 2] + Hd / 2], axis=1) + move + \
            rng.normal(0.0, 0.1, (N, 2))
        truth[j, :, :3], truth[j, :, 3] = Rj, tj
    structure = (X * (1.0 + rng.normal(0.0, 0.003, N))[:, None]).astype(np.float32)
    return dict(coords=coords.astype(np.float32), structure=structure, mover=mover, truth=truth)
