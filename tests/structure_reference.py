"""The rules of ctk_fit_structure (include/ctk.h, "fit structure"; co-tracker_amd/csrc/structure_math.h) restated in numpy and Python
numbers: what the kernel (tests/test_gpu_structure.py) and the g++ build of the header (tests/test_structure_host.py) are compared
with, exactly.  Positions are motion_reference's, dot / cross / polar / valid / rays are pose_reference's, apply / error are
resection_reference's.  Everything in double is one float64 operation per step in the header's order; what one thread does per view
in the kernel is one numpy operation over all slots here, the views in ascending order: the sums are the kernel's, bit for bit."""
import math

import numpy as np

import motion_reference as R
import pose_reference as PO
import resection_reference as RR

VIEWS_MAX, POINTS_MAX, MIN_VIEWS, ROUNDS = 256, 8192, 2, 3
BIT_ROUNDS, BIT_NO_START, BIT_NO_PARALLAX, BIT_INTO, BIT_MINORITY = (1, 2, 4), 8, 16, 32, 64
GATES = (4.0, 2.0, 1.0)
EYE12 = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float32)


def min_sin2(degrees):
    """What the host layers hand to the kernel for min_parallax degrees: the float32 of sin^2."""
    return float(np.float32(math.sin(math.radians(float(degrees))) ** 2))


def view(m12, stats_ok=True):
    """Twelve float32 (R | t) -> (counts, R: nine floats, t: three floats, c: three floats)."""
    m = np.asarray(m12, dtype=np.float32).reshape(12)
    ok = bool(stats_ok) and bool(np.isfinite(m).all())
    Rm = [float(m[r * 4 + c]) for r in range(3) for c in range(3)] if ok else list(RR.EYE[0])
    t = [float(m[3]), float(m[7]), float(m[11])] if ok else [0.0, 0.0, 0.0]
    if ok:
        Rm, det = PO.polar(Rm)
        ok = PO.valid(Rm, t, det)
    c = [-PO.dot([Rm[i], Rm[3 + i], Rm[6 + i]], t) for i in range(3)]
    return ok, Rm, t, c


def cols(Rm):
    return [[Rm[i], Rm[3 + i], Rm[6 + i]] for i in range(3)]


def solve(A, b):
    """A: six arrays (00 01 02 11 12 22), b: three -> (x: three arrays, the solve stands bool [n])."""
    with np.errstate(all="ignore"):
        a00, a01, a02, a11, a12, a22 = A
        c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        det = PO.dot([a00, a01, a02], [c00, c01, c02])
        ok = (det > 0.0) & (np.abs(det) <= PO.DBL_MAX)
        inv = 1.0 / det
        x = [PO.dot(r, b) * inv for r in ([c00, c01, c02], [c01, c11, c12], [c02, c12, c22])]
        ok = ok & (np.abs(x[0]) <= PO.DBL_MAX) & (np.abs(x[1]) <= PO.DBL_MAX) & (np.abs(x[2]) <= PO.DBL_MAX)
    return x, ok


def to_out(into_view, X):
    """X: three float64 arrays -> (float32 [n,3] as written, finite bool [n])."""
    with np.errstate(all="ignore"):
        Xo = X if into_view is None else RR.apply(into_view[1], into_view[2], X)
        o = np.stack([v.astype(np.float32) for v in Xo], axis=-1)
    return o, np.isfinite(o).all(axis=-1)


def origin(origin_in, into_view):
    m = EYE12.copy() if origin_in is None else np.asarray(origin_in, dtype=np.float32).reshape(12).copy()
    if into_view is None:
        return m
    _, Rk, tk, _ = into_view
    o = np.zeros(12, dtype=np.float32)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(4):
                d = PO.dot(Rk[i * 3:i * 3 + 3], [float(m[j]), float(m[4 + j]), float(m[8 + j])])
                o[i * 4 + j] = np.float32(d) if j < 3 else np.float32(d + tk[i])
    return o


def slots(cam, views, obs, Q, into, tol, sin2, min_views, details=None):
    """views: [view()] of F views; obs bool [F,n] (false on a view that does not count); Q int64 [F,n,2]; into: a counting view or -1
    -> (label of the attempt int [n]: 1 accepted, 0 rejected, -1 where m < 2; point float32 [n,3]; error float32 [n]; stats int32
    [n,4])."""
    F, n = obs.shape
    z = np.zeros(n)
    A, b = [z.copy() for _ in range(6)], [z.copy() for _ in range(3)]
    m = np.zeros(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        for j in range(F):
            if not views[j][0]:
                continue
            o = obs[j]
            _, Rm, t, c = views[j]
            y = PO.rays(cam, Q[j])
            d = [PO.dot(y, cl) for cl in cols(Rm)]
            w = 1.0 / PO.dot(d, d)
            e = {(i, k): (d[i] * d[k]) * w for i in range(3) for k in range(i, 3)}
            P = [1.0 - e[0, 0], -e[0, 1], -e[0, 2], 1.0 - e[1, 1], -e[1, 2], 1.0 - e[2, 2]]
            for i in range(6):
                A[i] = A[i] + np.where(o, P[i], 0.0)
            rows = ([P[0], P[1], P[2]], [P[1], P[3], P[4]], [P[2], P[4], P[5]])
            for i in range(3):
                b[i] = b[i] + np.where(o, PO.dot(rows[i], c), 0.0)
            m += o
        X, started = solve(A, b)
        started = started & (m >= 2)
        bits = np.where(started, 0, BIT_NO_START).astype(np.int64)
        for rnd in range(ROUNDS):
            gt = GATES[rnd] * float(np.float32(tol))
            gate2 = gt * gt
            A, b = [z.copy() for _ in range(6)], [z.copy() for _ in range(3)]
            took = np.zeros(n, dtype=np.int64)
            for j in range(F):
                if not views[j][0]:
                    continue
                _, Rm, t, c = views[j]
                e, (u, v, dx, dy, iz) = RR.error(cam, RR.apply(Rm, t, X), Q[j])
                o = obs[j] & (e <= gate2)
                ax, ay = cam[0] * iz, cam[1] * iz
                bx, by = ax * u, ay * v
                zero = np.zeros(n)
                gx, gy = [ax, zero, -bx], [zero, ay, -by]
                jx, jy = [PO.dot(gx, cl) for cl in cols(Rm)], [PO.dot(gy, cl) for cl in cols(Rm)]
                k = 0
                for i in range(3):
                    for l in range(i, 3):
                        A[k] = A[k] + np.where(o, jx[i] * jx[l] + jy[i] * jy[l], 0.0)
                        k += 1
                for i in range(3):
                    b[i] = b[i] + np.where(o, jx[i] * dx + jy[i] * dy, 0.0)
                took += o
            delta, ok = solve(A, [-b[0], -b[1], -b[2]])
            Xn = [X[i] + delta[i] for i in range(3)]
            ok = ok & (took >= min_views) & (np.abs(Xn[0]) <= PO.DBL_MAX) & (np.abs(Xn[1]) <= PO.DBL_MAX) & (np.abs(Xn[2]) <= PO.DBL_MAX)
            X = [np.where(ok & started, Xn[i], X[i]) for i in range(3)]
            bits |= np.where(started & ~ok, BIT_ROUNDS[rnd], 0)
        t2 = RR.tol2(tol)
        counted, first = np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int64)
        wa, total, par = [z.copy() for _ in range(3)], z.copy(), np.zeros(n, dtype=bool)
        s2 = float(np.float32(sin2))
        for j in range(F):
            if not views[j][0]:
                continue
            _, Rm, t, c = views[j]
            e, _ = RR.error(cam, RR.apply(Rm, t, X), Q[j])
            o = obs[j] & (e <= t2) & started
            wj = [X[i] - c[i] for i in range(3)]
            new = o & (first < 0)
            first = np.where(new, j, first)
            wa = [np.where(new, wj[i], wa[i]) for i in range(3)]
            cr = PO.cross(wa, wj)
            par |= o & (PO.dot(cr, cr) >= (PO.dot(wa, wa) * PO.dot(wj, wj)) * s2)
            total = total + np.where(o, e, 0.0)
            counted += o
        bits |= np.where(started & ~par, BIT_NO_PARALLAX, 0)
        pt, writable = to_out(views[into] if into >= 0 else None, X)
        majority = 2 * counted >= m
        bits |= np.where(started & ~majority, BIT_MINORITY, 0)
        accepted = started & (counted >= min_views) & majority & par & writable
        err = np.where(accepted, (total / np.where(counted > 0, counted, 1).astype(np.float64)), -1.0).astype(np.float32)
    label = np.where(accepted, 1, np.where(m < 2, -1, 0)).astype(np.int64)
    pt = np.where(accepted[:, None], pt, np.float32(0)).astype(np.float32)
    stats = np.stack([m, counted, first, bits], axis=-1).astype(np.int32)
    if details is not None:
        details.update(X=np.stack(X, axis=-1), started=started)
    return label, pt, err, stats


def fit_structure(coords, intrinsics, pose, pose_stats=None, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None,
                  f0=0, F=None, into=-1, source_frame=0, structure=None, valid=None, origin_in=None, tol=2.0, min_views=3, sin2=None,
                  refine=0, scale=(1.0, 1.0)):
    """coords float32 [G,R,N,2]; pose float32 [G,F,3,4]; pose_stats int32 [G,F,4] or None; visible or logits; first_row; structure
    float32 [G,N,3] with valid int8 [G,N], or neither; origin_in float32 [G,3,4] or None ->
    (points float32 [G,N_out,3], label int8 [G,N_out], error float32 [G,N_out], stats int32 [G,N_out,4], origin float32 [G,3,4])."""
    coords = np.asarray(coords, dtype=np.float32)
    G, R_, N, _ = coords.shape
    pose = np.asarray(pose, dtype=np.float32)
    F = pose.shape[1] if F is None else F
    pose = pose.reshape(G, F, 12)
    N_out = N if N_out is None else N_out
    sin2 = min_sin2(1.0) if sin2 is None else sin2
    assert 1 <= F <= VIEWS_MAX and F <= R_ and -1 <= into < F and MIN_VIEWS <= min_views <= VIEWS_MAX and refine in (0, 1)
    assert (structure is None) == (valid is None) and 0.0 < sin2 <= 1.0
    cam = PO.camera(intrinsics)
    okx, px = R.quant(coords[..., 0], scale[0])
    oky, py = R.quant(coords[..., 1], scale[1])
    pos = np.stack([px, py], axis=-1)
    seen = np.asarray(visible) != 0 if visible is not None else R.visible_from_logits(vis, conf, thresh)
    good = okx & oky & seen
    points = np.zeros((G, N_out, 3), dtype=np.float32)
    label = np.full((G, N_out), -1, dtype=np.int8)
    err = np.full((G, N_out), -1.0, dtype=np.float32)
    stats = np.zeros((G, N_out, 4), dtype=np.int32)
    org = np.zeros((G, 12), dtype=np.float32)
    for g in range(G):
        views = [view(pose[g, j], pose_stats is None or int(pose_stats[g, j, 2]) >= 0) for j in range(F)]
        into_counts = into >= 0 and views[into][0]
        no_structure = into >= 0 and not into_counts
        into_view = views[into] if into_counts else None
        org[g] = origin(None if origin_in is None else np.asarray(origin_in, dtype=np.float32)[g], into_view)
        first = np.zeros(N_out, dtype=np.int64) if first_row is None else np.asarray(first_row[g], dtype=np.int64)[:N_out]
        rows = [(f0 + j) % R_ for j in range(F)]
        obs = np.stack([good[g, rows[j], :N_out] & (f0 + j >= first) & bool(views[j][0]) for j in range(F)])
        Q = np.stack([pos[g, rows[j], :N_out] for j in range(F)])
        in_old = np.zeros(N_out, dtype=bool)
        carried, old = in_old.copy(), np.zeros((N_out, 3), dtype=np.float32)
        if structure is not None:
            s = np.asarray(structure, dtype=np.float32).reshape(G, N, 3)[g, :N_out]
            in_old = (np.asarray(valid).reshape(G, N)[g, :N_out] != 0) & np.isfinite(s).all(axis=1)
            if first_row is not None:
                in_old &= first <= source_frame
            if not no_structure:
                old, writable = to_out(into_view, [s[:, i].astype(np.float64) for i in range(3)])
                carried = in_old & writable
        if no_structure:
            m = obs.sum(axis=0)
            label[g] = np.where((m >= 1) | in_old, 0, -1)
            stats[g] = np.stack([m, 0 * m, 0 * m - 1, 0 * m + BIT_INTO], axis=-1)
            continue
        la, pt, er, st = slots(cam, views, obs, Q, into if into_counts else -1, tol, sin2, min_views)
        skip = carried & (refine == 0)
        keep_old = carried & (la != 1)
        label[g] = np.where(skip | keep_old, 2, la)
        points[g] = np.where((skip | keep_old)[:, None], old, pt)
        err[g] = np.where(skip, np.float32(-1), er)
        stats[g] = np.where(skip[:, None], np.array([0, 0, -1, 0], dtype=np.int32), st)
    return points, label, err, stats, org.reshape(G, 3, 4)


# ---- the shapes at which the kernel can go wrong -------------------------------------------------------------------------------------------
def spoil_views(pose, stats, g):
    """Group g: view 1 has no fit (pose_stats), view 2 a NaN pose, view 3 a zero matrix (the polar steps leave a determinant of 0)."""
    stats[g, 1, 2] = -1
    pose[g, 2, 1, 2] = np.nan
    pose[g, 3, :, :3] = 0.0


def special_points(sc, f0):
    """Slots 0..3 of group 0: a point behind the cameras of the first two views, one grossly wrong view, parallel rays (a point at
    infinity), and a point at a camera centre (an observation is put there all the same); slot 9: a view that is wrong by 40 x tol."""
    fx, fy, cx, cy = sc["cam"]
    T = sc["coords"].shape[1]
    c3 = passed = None
    for f in range(T):
        Rt, tt = sc["truth"][0, f, :, :3], sc["truth"][0, f, :, 3]
        if f == f0 + 3:
            c3 = -Rt.T @ tt
        if f == f0 + 1:
            passed = Rt.T @ (np.array([-0.15, 0.0, -0.012]) - tt)  # behind the cameras of the first two views, in front of the later ones
    for f in range(T):
        Rt, tt = sc["truth"][0, f, :, :3], sc["truth"][0, f, :, 3]
        for n, X in ((0, passed), (1, np.array([0.5, 0.2, 5.0])), (2, np.array([2.0e8, 1.0e8, 1.0e9])), (3, c3), (9, np.array([-0.8, 0.3, 6.0]))):
            Xc = Rt @ X + tt
            with np.errstate(all="ignore"):
                sc["coords"][0, f, n] = (fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy)
        sc["visible"][0, f, :4] = sc["visible"][0, f, 9] = 1
    sc["coords"][0, f0 + 3, 3] = (cx, cy)
    sc["coords"][0, f0 + 5, 1, 0] += 10.0  # (5 x tol: the gates drop it; the start is not robust, so a far larger one rejects the slot)
    sc["coords"][0, f0 + 5, 9, 0] += 80.0


def cases():
    """-> (name, args, kwargs) of fit_structure, one after the other."""
    import objects_reference as O
    # a ring of 8 rows after 14 frames; first rows: a slot that arrived mid-window (6), one released after source_frame (7); NaN and
    # outside positions; spoiled views; the old structure carried into a view that counts; an origin
    G, T, N, N_out, Rr, f0, F, src = 2, 14, 70, 65, 8, 6, 8, 3
    sc = RR.scene(3, G, T, N, src=src, p_visible=0.9)
    coords, visible = sc["coords"], sc["visible"]
    first = O.spoil(coords[:, f0 - 2:], N_out)  # (its frames fall into the window)
    first[0, 6], first[0, 7], first[1, 8] = f0 + 3, src + 1, f0 + F
    special_points(sc, f0)
    pose = np.ascontiguousarray(sc["truth"][:, f0:f0 + F]).astype(np.float32)
    stats = np.zeros((G, F, 4), dtype=np.int32)
    spoil_views(pose, stats, 1)
    valid = np.ones((G, N), dtype=np.int8)
    valid[:, ::3] = 0
    structure = sc["structure"].copy()
    RR.spoil_structure(structure, valid)
    origin = np.ascontiguousarray(sc["truth"][:, 1]).astype(np.float32)
    ring = dict(visible=R.fold(visible, Rr, T), first_row=first, N_out=N_out, f0=f0, F=F, source_frame=src)
    old = dict(structure=structure, valid=valid)
    yield "ring_carry", (R.fold(coords, Rr, T), sc["cam"], pose), dict(ring, pose_stats=stats, into=7, origin_in=origin, min_views=3, **old)
    yield "ring_refine", (R.fold(coords, Rr, T), sc["cam"], pose), dict(ring, pose_stats=stats, into=0, refine=1, min_views=2, tol=1.0, **old)
    yield "ring_into_dead_view", (R.fold(coords, Rr, T), sc["cam"], pose), dict(ring, pose_stats=stats, into=2, origin_in=origin, refine=1, **old)
    yield "ring_into_no_fit_view", (R.fold(coords, Rr, T), sc["cam"], pose), dict(ring, pose_stats=stats, into=1, **old)
    yield "ring_stats_null", (R.fold(coords, Rr, T), sc["cam"], pose), dict(ring, into=1, min_views=F, **old)
    yield "ring_plain", (R.fold(coords, Rr, T), sc["cam"], pose), dict(ring, pose_stats=stats, into=-1, min_views=3, sin2=min_sin2(0.2))
    yield "ring_carry_no_into", (R.fold(coords, Rr, T), sc["cam"], pose), dict(ring, into=-1, origin_in=origin, **old)
    # logits instead of bytes, a scale, no first rows
    rng = np.random.default_rng(5)
    vis_l = np.where(visible != 0, 4.0, -4.0).astype(np.float32) + rng.uniform(-1, 1, visible.shape).astype(np.float32)
    cam = (1.37 * sc["cam"][0], 0.81 * sc["cam"][1], 1.37 * sc["cam"][2], 0.81 * sc["cam"][3])
    yield "ring_logits", (R.fold(coords, Rr, T), cam, pose), dict(
        vis=R.fold(vis_l, Rr, T), conf=np.full((G, Rr, N), 5.0, dtype=np.float32), thresh=0.6, N_out=N, f0=f0, F=F, into=4, min_views=3,
        scale=(1.37, 0.81), source_frame=src, **old)
    # sizes round the workgroup, the fewest and the most views, min_views = F
    for N_out, F, G in ((1, 1, 1), (1, 2, 2), (63, 2, 1), (64, 3, 2), (65, 8, 1), (300, 8, 2), (65, 256, 1), (9, 256, 2)):
        sc = RR.scene(N_out + F, G, F, max(N_out, 4) + 3, src=0, movers=0.1, p_visible=2.0 if N_out == 9 else 0.97)
        pose = sc["truth"].astype(np.float32)
        kw = dict(visible=sc["visible"], N_out=N_out, into=F - 1, min_views=max(F, 2) if N_out != 65 else 3)
        if F == 256 and N_out == 9:  # every view must lie within tol: the path stays short enough for that
            sc = RR.scene(9, G, F, 12, src=0, movers=0.0, noise=0.02, p_visible=2.0)
            pose = sc["truth"].astype(np.float32)
            kw = dict(visible=sc["visible"], N_out=N_out, into=F - 1, min_views=F, tol=3.0)
        yield "size_%d_%d_%d" % (N_out, F, G), (sc["coords"], sc["cam"], pose), kw
    # a standing camera: all views under one pose, no parallax, every label 0
    sc = RR.scene(8, 1, 6, 40, src=0, movers=0.0, p_visible=2.0)
    sc["coords"][:] = sc["coords"][:, :1] + np.random.default_rng(1).normal(0, 0.05, sc["coords"].shape).astype(np.float32)
    pose = np.repeat(sc["truth"][:, 2:3], 6, axis=1).astype(np.float32)
    yield "standing", (sc["coords"], sc["cam"], pose), dict(visible=sc["visible"], into=2, min_views=2)
