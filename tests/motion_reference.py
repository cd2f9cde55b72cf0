"""The rules of ctk_fit_motion (include/ctk.h, "fit motion"; co-tracker_amd/csrc/motion_math.h) restated in numpy and Python integers: what
the kernel (tests/test_gpu_motion.py) and the g++ build of the header (tests/test_motion_host.py) are compared with, exactly.  Positions
are quantised with float32 operations, the hypothesis sums D, A, B and the refit sums are Python integers (their stated bounds are
asserted as they arise), the scoring is int64 numpy whose operands are bounded by those assertions, the four divisions are float64."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
TRANSLATION, SIMILARITY = 0, 1
LIMIT = 2 ** 63


def quant(x, s):
    """float32 positions x * s -> (valid, P int64 in 1/16 pixel; 0 where not valid)."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(x, dtype=np.float32) * np.float32(s)
        ok = (v >= np.float32(-8192.0)) & (v <= np.float32(8192.0))
        p = np.rint(np.where(ok, v, np.float32(0)) * np.float32(16.0)).astype(np.int64)
    return ok, p


def tol_steps(tol):
    """T, or 0 where the C-ABI refuses."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.rint(np.float32(tol) * np.float32(16.0))
    return int(t) if 1.0 <= t <= 4096.0 else 0


def base2(min_base):
    mb = np.float32(min_base)
    if not (mb >= 0 and mb <= 8192):
        return -1
    return int(np.rint(mb * np.float32(16.0))) ** 2


def sigmoid32(x):
    with np.errstate(over="ignore"):
        return np.float32(1.0) / (np.float32(1.0) + np.exp(-np.asarray(x, dtype=np.float32)))


def visible_from_logits(vis, conf, thresh):
    with np.errstate(invalid="ignore"):
        return (sigmoid32(vis) * sigmoid32(conf)) > np.float32(thresh)


def mix(x):
    x &= 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def sample(seed, f, k, M, model):
    base = (f * 0x9e3779b9 + 2 * k) & 0xffffffff
    i = mix(seed ^ mix(base)) % M
    if model != SIMILARITY:
        return i, i
    j = mix(seed ^ mix((base + 1) & 0xffffffff)) % (M - 1)
    return i, j + (1 if j >= i else 0)


def fit_frame(P, Q, f, model, T, b2, K, seed):
    """P, Q int64 [M,2] -> (row float32 [6], inlier int8 [M], (M, count, best k, 0))."""
    M = P.shape[0]
    identity = np.array([1, 0, 0, 0, 1, 0], dtype=np.float32)
    if M < (2 if model == SIMILARITY else 1):
        return identity, np.zeros(M, dtype=np.int8), (M, 0, -1, 0)
    assert int(np.abs(P).max()) <= 2 ** 17 and int(np.abs(Q).max()) <= 2 ** 17
    ij = [sample(seed, f, k, M, model) for k in range(K)]
    i = np.array([a for a, _ in ij])
    j = np.array([b for _, b in ij])
    u = P[None, :, :] - P[i][:, None, :]  # [K,M,2], |.| <= 2^18
    w = Q[None, :, :] - Q[i][:, None, :]
    if model == SIMILARITY:
        D, A, B = [], [], []
        for a, b in ij:
            dx, dy, ex, ey = (int(v) for v in (*(P[b] - P[a]), *(Q[b] - Q[a])))
            D.append(dx * dx + dy * dy), A.append(dx * ex + dy * ey), B.append(dx * ey - dy * ex)
            assert D[-1] <= 2 ** 37 and abs(A[-1]) <= 2 ** 37 and abs(B[-1]) <= 2 ** 37
            assert max(D[-1], abs(A[-1]), abs(B[-1])) * 2 ** 18 <= 2 ** 55 and T * D[-1] <= 2 ** 49 and 3 * 2 ** 55 < LIMIT
        D, A, B = (np.array(v, dtype=np.int64)[:, None] for v in (D, A, B))
        admissible = (D[:, 0] >= b2) & (D[:, 0] >= 1)
        rx = D * w[..., 0] - (A * u[..., 0] - B * u[..., 1])
        ry = D * w[..., 1] - (B * u[..., 0] + A * u[..., 1])
        inl = (np.abs(rx) <= T * D) & (np.abs(ry) <= T * D)
    else:
        admissible = np.ones(K, dtype=bool)
        r = w - u
        inl = (np.abs(r[..., 0]) <= T) & (np.abs(r[..., 1]) <= T)
    counts = inl.sum(axis=1)
    keys = [(int(counts[k]) << 32) | (K - 1 - k) for k in range(K) if admissible[k]]
    if not keys:
        return identity, np.zeros(M, dtype=np.int8), (M, 0, -1, 0)
    best = max(keys)
    kb = K - 1 - (best & 0xffffffff)
    mask = inl[kb]
    pin, qin = P[mask].tolist(), Q[mask].tolist()
    n = len(pin)
    assert n == best >> 32 and 1 <= n <= 8192
    spx, spy = sum(p[0] for p in pin), sum(p[1] for p in pin)
    sqx, sqy = sum(q[0] for q in qin), sum(q[1] for q in qin)
    if model == SIMILARITY:
        spp = sum(p[0] * p[0] + p[1] * p[1] for p in pin)
        sdot = sum(p[0] * q[0] + p[1] * q[1] for p, q in zip(pin, qin))
        scr = sum(p[0] * q[1] - p[1] * q[0] for p, q in zip(pin, qin))
        den = n * spp - (spx * spx + spy * spy)
        na = n * sdot - (spx * sqx + spy * sqy)
        nb = n * scr - (spx * sqy - spy * sqx)
        for v in (n * spp, spx * spx + spy * spy, n * sdot, spx * sqx + spy * sqy, n * scr, spx * sqy - spy * sqx, den, na, nb):
            assert abs(v) < LIMIT
        assert den > 0
        a, b = float(na) / float(den), float(nb) / float(den)
        tx = (float(sqx) - (a * float(spx) - b * float(spy))) / (float(n) * 16.0)
        ty = (float(sqy) - (b * float(spx) + a * float(spy))) / (float(n) * 16.0)
    else:
        a, b = 1.0, 0.0
        tx = (float(sqx) - float(spx)) / (float(n) * 16.0)
        ty = (float(sqy) - float(spy)) / (float(n) * 16.0)
    row = np.array([a, -b, tx, b, a, ty], dtype=np.float64).astype(np.float32)
    return row, mask.astype(np.int8), (M, n, kb, 0)


def fit_motion(coords, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1, lag=1, model=SIMILARITY,
               tol=2.0, K=128, min_base=16.0, seed=0, scale=(1.0, 1.0)):
    """coords float32 [G,R,N,2]; visible [G,R,N] (or the logits vis, conf and thresh); first_row int [G,N] or None ->
    (motion float32 [G,F,2,3], inlier int8 [G,F,N_out], stats int32 [G,F,4])."""
    coords = np.asarray(coords, dtype=np.float32)
    G, R, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    T, b2 = tol_steps(tol), base2(min_base)
    assert T > 0 and b2 >= 0
    okx, px = quant(coords[..., 0], scale[0])
    oky, py = quant(coords[..., 1], scale[1])
    seen = np.asarray(visible) != 0 if visible is not None else visible_from_logits(vis, conf, thresh)
    good = okx & oky & seen
    pos = np.stack([px, py], axis=-1)
    motion = np.zeros((G, F, 6), dtype=np.float32)
    inlier = np.full((G, F, N_out), -1, dtype=np.int8)
    stats = np.zeros((G, F, 4), dtype=np.int32)
    for g in range(G):
        first = np.zeros(N, dtype=np.int64) if first_row is None else np.asarray(first_row[g], dtype=np.int64)
        for jf in range(F):
            f, fs = f0 + jf, f0 + jf - lag
            corr = np.zeros(N_out, dtype=bool)
            if fs >= 0:
                corr = good[g, fs % R, :N_out] & good[g, f % R, :N_out] & (fs >= first[:N_out])
            idx = np.nonzero(corr)[0]
            row, inl, st = fit_frame(pos[g, fs % R][idx], pos[g, f % R][idx], f, model, T, b2, K, seed)
            motion[g, jf], stats[g, jf] = row, st
            inlier[g, jf, idx] = inl
    return motion.reshape(G, F, 2, 3), inlier, stats


# ---- scenes for the tests -----------------------------------------------------------------------------------------------------------
def similarity(theta, s, t, centre):
    """-> A float64 [2,3]: x -> s Rot(theta) (x - centre) + centre + t."""
    c, n = s * np.cos(theta), s * np.sin(theta)
    lin = np.array([[c, -n], [n, c]])
    return np.concatenate([lin, (np.asarray(centre) - lin @ np.asarray(centre) + np.asarray(t))[:, None]], axis=1)


def scene(seed, G, T, N, hw=(64, 96), outliers=0.3, noise=0.0, p_visible=0.9):
    """A camera that turns, zooms and shifts a little from frame to frame over G sets of N points, a fraction of which move on their
    own -> (coords float32 [G,T,N,2], visible uint8 [G,T,N], planted outlier bool [G,N])."""
    rng = np.random.default_rng(seed)
    H, W = hw
    cur = rng.uniform([0, 0], [W - 1, H - 1], size=(G, N, 2))
    out = rng.random((G, N)) < outliers
    coords = np.empty((G, T, N, 2), dtype=np.float32)
    for r in range(T):
        coords[:, r] = cur + rng.normal(0, 1, cur.shape) * noise
        A = similarity(rng.uniform(-0.05, 0.05), rng.uniform(0.95, 1.05), rng.uniform(-8, 8, 2), (W / 2, H / 2))
        cur = cur @ A[:, :2].T + A[:, 2]
        cur = cur + out[..., None] * rng.uniform(-1, 1, cur.shape) * 20
    visible = (rng.random((G, T, N)) < p_visible).astype(np.uint8)
    return coords, visible, out


def fold(x, R, upto):
    """A linear history x [G,T,...] -> the ring of R rows after `upto` frames: row f % R holds frame f for the last R frames."""
    ring = np.zeros((x.shape[0], R) + x.shape[2:], dtype=x.dtype)
    for f in range(max(upto - R, 0), upto):
        ring[:, f % R] = x[:, f]
    return ring
