"""The rules of ctk_fit_objects (include/ctk.h, "fit objects"; co-tracker_amd/csrc/objects_math.h) restated in numpy and Python integers on
top of motion_reference.fit_frame, which is one round: what the kernel (tests/test_gpu_objects.py) and the g++ build of the header
(tests/test_objects_host.py) are compared with, exactly.  What is new here is the round loop, the three source forms, the box and
the labels."""
import numpy as np

import motion_reference as R

NONE = 127
IDENTITY = np.array([1, 0, 0, 0, 1, 0], dtype=np.float32)
NO_BOX = (0, 0, -1, -1)


def seed_of(seed, r):
    return (seed ^ R.mix(r)) & 0xffffffff


def fit_rounds(P, Q, f, labels, L, min_points, model, T, b2, K, seed):
    """P, Q int64 [M,2] in ascending n; labels int [M] (labels mode) or None (split mode) ->
    (rows float32 [L,6], label int8 [M], stats [L,4], box [L,4])."""
    M = P.shape[0]
    rows = np.tile(IDENTITY, (L, 1))
    label = np.full(M, NONE, dtype=np.int8)
    stats, box = np.zeros((L, 4), dtype=np.int32), np.zeros((L, 4), dtype=np.int32)
    left = np.arange(M)  # split mode: list_r, as places in the list of correspondences
    stopped = False
    for r in range(L):
        idx = np.nonzero(labels == r)[0] if labels is not None else left
        stats[r], box[r] = (len(idx), 0, -1, 0), NO_BOX
        if stopped:
            continue
        row, inl, st = R.fit_frame(P[idx], Q[idx], f, model, T, b2, K, seed_of(seed, r))
        if st[2] < 0 or st[1] < min_points:  # no admissible hypothesis, or too few inliers: nothing is fitted, no point is taken
            stopped = labels is None
            continue
        took = idx[inl != 0]
        rows[r], stats[r] = row, st
        label[took] = r
        box[r] = (Q[took, 0].min(), Q[took, 1].min(), Q[took, 0].max(), Q[took, 1].max())
        if labels is None:
            left = idx[inl == 0]
    return rows, label, stats, box


def fit_objects(coords, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1, to=None, lag=None,
                anchor=None, labels=None, L=4, min_points=8, model=R.SIMILARITY, tol=2.0, K=128, min_base=16.0, seed=0, scale=(1.0, 1.0)):
    """coords float32 [G,R,N,2]; visible [G,R,N] (or the logits vis, conf and thresh); first_row int [G,N] or None; exactly one of
    to (a frame), lag (>= 1) and anchor = (coords float32 [G,N,2], visible [G,N], frame); labels int8 [G,N] or None (split mode) ->
    (motion float32 [G,F,L,2,3], label int8 [G,F,N_out], stats int32 [G,F,L,4], box int32 [G,F,L,4])."""
    coords = np.asarray(coords, dtype=np.float32)
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    assert (to is not None) + (lag is not None) + (anchor is not None) == 1 and (lag is None or lag >= 1) and (to is None or to >= 0)
    assert 1 <= L <= 16 and 1 <= min_points <= 8192
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
    motion = np.zeros((G, F, L, 6), dtype=np.float32)
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
            lab = None if labels is None else np.asarray(labels[g], dtype=np.int64)[idx]
            rows, la, st, bx = fit_rounds(src[idx], pos[g, f % R_][idx], f, lab, L, min_points, model, T, b2, K, seed)
            motion[g, jf], stats[g, jf], box[g, jf] = rows, st, bx
            label[g, jf, idx] = la
    return motion.reshape(G, F, L, 2, 3), label, stats, box


# ---- scenes for the tests -----------------------------------------------------------------------------------------------------------
SHARES = (0.50, 0.25, 0.15, 0.10)
CENTRES = ((120.0, 90.0), (340.0, 180.0), (240.0, 60.0))
MOTIONS = ((0.02, 1.03, (3.0, -2.0)), (-0.05, 0.97, (14.0, 9.0)), (0.08, 1.0, (-12.0, 11.0)), (0.0, 1.1, (10.0, -13.0)))
PICTURE, OBJECT_SIDE = (270, 480), 80.0


def planted(seed, N=1024, noise=0.1):
    """A camera and three objects on a 480 x 270 picture: N points in shares 0.50 / 0.25 / 0.15 / 0.10, the first uniform over the
    picture, the others uniform in 80 x 80 boxes round CENTRES; every share moves under its own similarity (the camera about the
    picture's centre, the objects about their box centres); Gaussian noise on both frames; the slots are permuted ->
    (coords float32 [1,2,N,2], planted label int [N] -- 0 the camera, 1..3 the objects in size order --, the planted matrices)."""
    rng = np.random.default_rng(seed)
    H, W = PICTURE
    counts = [int(round(s * N)) for s in SHARES]
    counts[0] = N - sum(counts[1:])
    src, who, mats = [], [], []
    for k, (cnt, (theta, s, t)) in enumerate(zip(counts, MOTIONS)):
        if k == 0:
            centre, pts = (W / 2, H / 2), rng.uniform([0, 0], [W - 1, H - 1], size=(cnt, 2))
        else:
            centre = CENTRES[k - 1]
            pts = rng.uniform(-OBJECT_SIDE / 2, OBJECT_SIDE / 2, size=(cnt, 2)) + np.asarray(centre)
        src.append(pts), who.append(np.full(cnt, k)), mats.append(R.similarity(theta, s, t, centre))
    src, who = np.concatenate(src), np.concatenate(who)
    dst = np.stack([src[i] @ mats[w][:, :2].T + mats[w][:, 2] for i, w in enumerate(who)])
    src = src + rng.normal(0, 1, src.shape) * noise
    dst = dst + rng.normal(0, 1, dst.shape) * noise
    perm = rng.permutation(N)
    return np.stack([src[perm], dst[perm]])[None].astype(np.float32), who[perm], mats


def objects_scene(seed, G, T, N, groups=3):
    """A moving camera (motion_reference.scene without outliers) and `groups` sets of points that each shift on their own, rigidly:
    -> (coords, visible, who int [G,N]: 0 the camera, k the k-th set)."""
    coords, visible, _ = R.scene(seed, G, T, N, outliers=0.0, p_visible=0.93)
    rng = np.random.default_rng(seed + 100)
    who = np.zeros((G, N), dtype=np.int64)
    for g in range(G):
        order = rng.permutation(N)
        at = N // 2
        for k in range(1, groups + 1):
            size = max(N // (4 * k), 1)
            who[g, order[at:at + size]] = k
            at += size
    for k in range(1, groups + 1):
        step = rng.uniform(-6, 6, 2) + np.array([9.0, -7.0]) * (1 if k % 2 else -1)
        coords += (who == k)[:, None, :, None] * (np.arange(T)[None, :, None, None] * step).astype(np.float32)
    return coords, visible, who


def spoil(coords, N_out):
    """Positions that are not valid (slots 1, 2, 3 on one frame each), an empty slot (4) and a late first row (0) ->
    first_row int32 [G,N]."""
    G, T, N, _ = coords.shape
    coords[0, 2, 1] = np.nan
    coords[0, 3, 2, 1] = np.inf
    coords[-1, 4, 3, 0] = -9000.0
    first = np.zeros((G, N), dtype=np.int32)
    first[0, 4] = R.INT32_MAX
    first[-1, 0] = 3
    return first
