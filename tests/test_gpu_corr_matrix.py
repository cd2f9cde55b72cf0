"""The correlation samplers, the whole contract: every kernel x workgroup dealing x chunk x edge; exact gathers, canaries, bit identities.

Three kernels compute the 49 x 49 correlation volumes of a window -- corr_volume_kernel (f32, corr.hip), corr_volume_sh_kernel
(SH version 1) and corr_volume_sh3_kernel (SH version 3, under the five workgroup dealings of CTK_OPT_CORR_MAP; corr_sh.hip) --
and corrblock.hip / the patch and support samplers share their tap arithmetic.  The GPU tests carry the `gpu` mark one by one;
the host parts (test_dealing_*, test_case_list_*, test_exact_gather_share, test_footprints_*, test_injections_*) need no GPU.

  1. EXACT INPUTS.  support[l][n][q] is the one-hot channel vector e_{pi(n, l)(q)}: pi is a random injection of the 49 taps into the
     128 channels per (point, level) (test_injections_differ: two points that any dealing makes neighbours -- 1, 2, 16 or 32 apart --
     and two levels of a point differ in at least 40 of the 49 taps).  The pyramid holds non-zero multiples of 1/16 in [-1/2, 1/2],
     drawn independently per level and frame.  Times 2^8 these are integers of at most 128 and the support is 256: the f16 split is
     exact with a zero low half, every MFMA product is exact and each correlation sum has one non-zero term, so
     C[pixel][q] = f[pixel][pi(q)] to the bit on all three kernels and volume entry (p, q) is the bilinear blend of four known numbers.
       EXACT GATHERS, no tolerance: where the restated float32 weights of tap p (ctk_support.sampler_taps: the numpy restatement of
     the reference's coordinate arithmetic) are all 0 or 1 -- integer coordinates whose normalise / unnormalise round trip is the
     identity, and taps clamped at a border -- the output must be the feature value to the bit: the f32 value, or SH hi == value and
     lo == 0.  test_exact_gather_share asserts on the host that among the tracks with coordinates that are integers at every level
     (multiples of 8) at least one entry in eight per level is such a gather in every case and that every tap 0..48 occurs among
     them; the observed share per pyramid and level is in profiles/corr_matrix_errors.json.
       EVERY OTHER ENTRY against oracle/window_fp64.volume (tap positions from the float32 coordinates, values and blend in float64)
     within a DERIVED bound.  With u = 2^-24, |f| <= V = 1/2 and corner weights that sum to 1 the kernel differs from the float64
     blend of the same float32 axis weights by
         7 u V      four product and three sum roundings of results of at most V (the kernels fuse them into one product and three
                    FMAs, four roundings; seven covers the unfused order of sample_patches as well),
         1 u V      the float32 rounding of each corner weight wx * wy, which the oracle forms in float64,
         1 u V      the axis weight w0 = (floor + 1) - u, rounded in float32 (2^-25 per axis) where the oracle has 1 - w1,
         2^-40      the oracle's own float64 arithmetic,
     BOUND_F32 = 9 u V + 2^-40 = 2.68e-7; SH output adds the split of the result, relative 2^-22 plus one f16 subnormal step:
     BOUND_SH = BOUND_F32 + 2^-22 V + 2^-24 = 4.47e-7.  Not the 3e-6 of the parity tests.
       What this sees that a 3e-6 bar against another kernel does not: a wrong pixel or corner turns one multiple of 1/16 into another;
     a transposed (p, q), a wrong level, frame or point reads another channel (pi differs per (n, l)) of other features (they
     differ per frame and level); a dealing that swaps two workgroups' targets writes one point's values into another's rows.
  2. THE CASE LIST (CASES x KERNELS): N in {1, 2, 15, 16, 17, 18, 31, 32, 33, 48}, S in {1, 2, 15, 16, 17, 33} (one full frame chunk, a
     full chunk and one frame, three chunks; version 3's pipeline runs prologue tl < 2, body, epilogue tl <= nt + 1), three
     pyramids -- (48, 64) halved, an odd one (21, 27), (10, 13), (5, 6), (2, 3) whose coarse levels are smaller than a footprint, and
     9 x 9 at every level -- masks none / a third of the points dead / all dead.  `deal` restates the workgroup dealing of
     corr_volume_sh3_kernel; test_dealing_is_a_bijection asserts for every map, N and S of the list that it is onto (point, level,
     chunk), test_case_list_covers_every_axis that every branch is reached: map 4 with no full block, full blocks only, ragged tails
     of 1 and of 15 points; maps 1 and 2 with odd and even point counts; map 1 with a grid that is a multiple of 64 ids, one
     below 64 and one of 72 (N = 18: a whole block and a partial one); map 3 with 1, 2 and 15 points.  Coordinates per case
     (coords_of): multiples of 8, integers, half-integers, the four corners, up to 8 units outside every border, (-50, 1000),
     random interior; the kinds walk along a track, so a track's frames differ.  test_footprints_cover_every_size: 8 x 8, 9 x 8,
     8 x 9, 9 x 9 and clamped footprints narrower than 8 all occur (version 3 loads extra row tiles above 64 pixels).
     Dead points' rows are exact zeros and live rows keep the bits of the unmasked run.
  3. CANARIES.  The volume sits between guard rows pre-filled with the NaN pattern 0x7FC17FC1 like itself: the guards keep their
     bits, columns 2401..2431 of every row are exact zeros, the volume holds no NaN.  The entry points fix the level stride at N * S
     rows, so guard rows lie in front of level 0 and behind level 3 only; a row written behind N * S at an inner level lands in the next
     level's rows, where the exact check reads it.  Every pyramid level and support tensor lies inside a NaN-filled allocation, 16-byte
     aligned: a clamped read that left the operand would put a NaN into the volume.  A read by a lane whose result is discarded
     cannot be seen this way, and the SH kernels read the pyramid through its split copy in the workspace, so for them only the
     support frame and the split kernel's own reads are covered.
  4. BIT IDENTITIES the code documents.  Version 3 under maps 0, 1, 2 and 4 == map 3 on every case (both kinds of operands).
     ctk_corr_embed with points_per_chunk in {1, 5, 16, 17} == the unchunked call (n0 > 0 with ncount odd, even, a multiple of 16, ragged), under
     every map and both versions and on the f32 path, with and without a mask whose dead points straddle the cuts.
     ctk_corr_embed_batch(shared) == unshared for three groups of 11 points in chunks of 16, 5 and 33, which straddle group
     boundaries, masked, on all seven kernels.  Rewriting one point's coordinates and support changes that point's rows only.
  5. THE REST OF THE FAMILY at the same inputs.  ctk_corrblock_sample with one-hot targets: every output is blend(f) / sqrt(128);
     against float64 within 10 u V' + 2^-40 = 2.63e-8, V' = V / sqrt(128) (the blend terms above on values of at most V' and one
     IEEE division), on the odd and the 9 x 9 pyramid, S in {1, 17}.  sample_patches and sample_support bit for bit against the numpy
     restatement in oracle/ on the odd and the 9 x 9 pyramid, T in {1, 17}, fractional and out-of-range frames, the case's coordinates.
  6. RANDOM OPERANDS: L2-normalised randn features, real sample_support patches, the same cases and kernels against float64 at the
     bars the project asserts already (tests/test_gpu_parity.py): 2e-6 for the f32 kernel, 3e-6 for SH.

Not asserted: non-finite operands, and which kernel a launch ran (the recorder names the sampler by its use): `deal` documents the
dealing and cannot prove it; the maps are pinned through what differs, the rows each workgroup writes.

Observed on an MI355X.  No finding: on all seven kernels every exact gather is the feature value to the bit, every canary is intact,
every identity holds, and the five dealings are bijections.  Largest error of the blended entries on exact inputs: f32 6.7e-8 (bound
2.68e-7); SH 9.3e-8 on version 1 and on version 3 under every map (bound 4.47e-7); corrblock 6.1e-9 (bound 2.63e-8).  Random
operands: f32 6.2e-7 (bar 2e-6), version 1 2.5e-7, version 3 4.2e-7 under every map (bar 3e-6).  Per level:
profiles/corr_matrix_errors.json.  Share of exact gathers among the entries of the multiple-of-8 tracks, levels 0..3: (48, 64)
pyramid 0.49 / 0.74 / 0.50 / 0.60, odd pyramid 0.59 / 0.80 / 0.93 / 1.00, 9 x 9 all of them (2 / 8 is a power of two).
Sensitivity, shown once on scratch copies of corr_sh.hip, one planted fault each (test_exact has 16 cases x 7 kernels):
  1. w10 and w01 exchanged in version 3's blend -> the 75 test_exact cases of version 3 that have a blended entry (15 cases x 5 maps;
     the 1 x 1 case is all gathers), at the derived bound with errors up to 1.0; no gather moves (a gather has one weight 1).
  2. `lvl` and `tc` exchanged in map 4's tail branch -> not run as written: it hands tc >= tchunks to the kernel, nt <= 0, and the
     kernel would read through an unwritten tap table.  On the restatement: test_dealing_notices_a_swapped_tail.  On the GPU with tc
     clamped to the chunk count, so that every access stays in bounds: the 11
     test_exact cases of map 4 whose N is no multiple of 16 (levels 1..3 of the tail's points are never written).
  3. `n` for coord_column in the grouped version-1 kernel -> test_grouped_launch_equals_per_group_launches[sh1] at all three chunk
     sizes (289 of 561 rows differ); the grouped kernels are reachable behind corr_mlp only, so no test_exact case can see them.
  4. the epilogue bound `tl <= nt` (the last frame of a chunk is never stored) -> all 80 test_exact cases of version 3: the canary
     pattern is still in the volume.
  5. p and q exchanged in the output column -> all 80 test_exact cases of version 3 (1 x 1 case: 2214 of 2401 gathers).
  6. the footprint read one pixel to the left when fw == 9 -> the 50 test_exact cases of version 3 whose coordinates have a 9-wide
     footprint (10 cases x 5 maps; none on the 9 x 9 pyramid, whose round trips are exact).
The module's 294 GPU tests (16 cases x 7 kernels, twice, and 70 identity and family tests) take 6.7 s (the attention matrix: 299
tests, 5.0 s); the 6 host tests 2.6 s.
"""
import dataclasses
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch

import ctk_support
from ctk_support import corr_volume_raw, dev, maxdiff, nan_framed, same_bits, sampler_taps
from test_gpu_gemm_matrix import CANARY

gpu = pytest.mark.gpu

LEVELS, TAPS, CH, TC = 4, 49, 128, 16
CORR_K, CORR_LD = ctk_support.CORR_K, ctk_support.CORR_LD
PYRAMIDS = {"p48": ((48, 64), (24, 32), (12, 16), (6, 8)), "odd": ((21, 27), (10, 13), (5, 6), (2, 3)), "p9": ((9, 9),) * 4}
KERNELS = ("f32", "sh1", "sh3m0", "sh3m1", "sh3m2", "sh3m3", "sh3m4")
MASKS = ("none", "third", "all")
KINDS = ("mult8", "int", "half", "corner", "out", "far", "rand")  # coords_of
U, V = 2.0 ** -24, 0.5
BOUND_F32 = 9 * U * V + 2.0 ** -40
BOUND_SH = BOUND_F32 + 2.0 ** -22 * V + 2.0 ** -24
BOUND_CORRBLOCK = 10 * U * V / np.sqrt(128.0) + 2.0 ** -40
BAR = {"f32": 2e-6, "sh": 3e-6}  # tests/test_gpu_parity.py
ERRORS = {}  # (test, kernel, level) -> largest |out - float64 reference|


@dataclasses.dataclass(frozen=True)
class Case:
    N: int
    S: int
    pyr: str = "p48"
    mask: str = "none"

    @property
    def id(self):
        return f"n{self.N}-s{self.S}-{self.pyr}-{self.mask}"

    @property
    def sizes(self):
        return PYRAMIDS[self.pyr]

    @property
    def tchunks(self):
        return cdiv(self.S, TC)

    @property
    def grid(self):
        return self.N * LEVELS * self.tchunks


def cdiv(a, b):
    return -(-a // b)


CASES = [Case(1, 1, "p9"), Case(2, 2, "odd"), Case(15, 15, "odd", "third"), Case(16, 16, "p48"), Case(17, 17, "p9"),
         Case(31, 2, "p48", "third"), Case(32, 1, "odd"), Case(33, 17, "odd", "third"), Case(16, 2, "odd", "all"), Case(48, 16, "p9"),
         Case(48, 2, "p48"), Case(2, 33, "odd"), Case(1, 33, "p9"), Case(1, 17, "p48"), Case(17, 16, "odd", "third"), Case(18, 1, "odd")]
IDS = [c.id for c in CASES]
BOTH = [(c, k) for c in CASES for k in KERNELS]
BOTH_IDS = [f"{c.id}-{k}" for c, k in BOTH]


# ---- the workgroup dealing of corr_volume_sh3_kernel, restated (corr_sh.hip) ------------------------------------------------------------
def xcd_remap(pid, nblk):
    """ctk_xcd_remap (ctk_common.h): the id a workgroup deals from."""
    q, r, xcd, idx = nblk >> 3, nblk & 7, pid & 7, pid >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


def deal(m, bid, ncount, tchunks, grid, swap_tail=False):
    """-> (branch, local point, level, frame chunk) of workgroup id `bid` (after the XCD remap) under CTK_OPT_CORR_MAP = m.  Version 1 and
    the f32 kernel deal like map 0.  swap_tail: the planted fault of test_dealing_notices_a_swapped_tail."""
    if m == 3:  # level-major
        return "level_major", bid % ncount, bid // ncount % LEVELS, bid // ncount // LEVELS
    if m == 4:  # blocks of 16 points
        per = 16 * LEVELS * tchunks
        blk, r = divmod(bid, per)
        if (blk + 1) * 16 <= ncount:
            return "block16", blk * 16 + (r & 15), (r >> 4) % LEVELS, (r >> 4) // LEVELS
        t = bid - blk * per
        lvl, tc = t // tchunks % LEVELS, t % tchunks
        if swap_tail:
            lvl, tc = tc, lvl
        return "block16_tail", blk * 16 + t // (tchunks * LEVELS), lvl, tc
    if m != 0 and ncount % 2 == 0:  # point pairs
        u, branch = bid, "pairs"
        if m == 1:
            branch = "pairs64_partial"
            if (bid // 64 + 1) * 64 <= grid:
                u, branch = bid // 64 * 64 + (bid & 31) * 2 + ((bid >> 5) & 1), "pairs64"
        v = u >> 1
        return branch, v // tchunks // LEVELS * 2 + (u & 1), v // tchunks % LEVELS, v % tchunks
    return ("plain" if m == 0 else "plain_odd"), bid // tchunks // LEVELS, bid // tchunks % LEVELS, bid % tchunks


def branches(m, c):
    return {deal(m, b, c.N, c.tchunks, c.grid)[0] for b in range(c.grid)}


def test_dealing_is_a_bijection():
    for c in CASES:
        want = {(n, l, tc) for n in range(c.N) for l in range(LEVELS) for tc in range(c.tchunks)}
        assert sorted(xcd_remap(p, c.grid) for p in range(c.grid)) == list(range(c.grid)), c.id
        for m in range(5):
            got = [deal(m, b, c.N, c.tchunks, c.grid)[1:] for b in range(c.grid)]
            assert len(got) == len(want) and set(got) == want, (c.id, m)


def test_dealing_notices_a_swapped_tail():
    """Negative control of the test above: `lvl` and `tc` exchanged in map 4's tail is no bijection for any case with a tail."""
    for c in CASES:
        if "block16_tail" in branches(4, c):
            got = {deal(4, b, c.N, c.tchunks, c.grid, swap_tail=True)[1:] for b in range(c.grid)}
            assert got != {(n, l, tc) for n in range(c.N) for l in range(LEVELS) for tc in range(c.tchunks)}, c.id


def test_case_list_covers_every_axis():
    assert len(set(IDS)) == len(IDS)
    assert {c.N for c in CASES} >= {1, 2, 15, 16, 17, 31, 32, 33, 48} and max(c.N for c in CASES) <= 48
    assert {c.S for c in CASES} == {1, 2, 15, 16, 17, 33}
    assert all(c.N <= 2 for c in CASES if c.S == 33)
    assert {c.pyr for c in CASES} == set(PYRAMIDS) and {c.mask for c in CASES} == set(MASKS)
    assert {c.tchunks for c in CASES} == {1, 2, 3}
    # one chunk of 1, 2, 15 and exactly 16 frames; a full chunk and nt = 1; three chunks
    assert {(c.tchunks, c.S % TC) for c in CASES} == {(1, 1), (1, 2), (1, 15), (1, 0), (2, 1), (3, 1)}
    seen = {m: {} for m in range(5)}
    for c in CASES:
        for m in range(5):
            for b in branches(m, c):
                seen[m].setdefault(b, []).append(c)
    assert set(seen[0]) == {"plain"} and set(seen[3]) == {"level_major"}
    assert {c.N for c in seen[3]["level_major"]} >= {1, 2, 15}
    for m in (1, 2):
        assert {c.N % 2 for c in seen[m]["plain_odd"]} == {1}
    assert {c.N % 2 for c in seen[2]["pairs"]} == {0}
    assert set(seen[1]) == {"plain_odd", "pairs64", "pairs64_partial"} and set(seen[2]) == {"plain_odd", "pairs"}
    # whole blocks of 64 ids only | no whole block | a whole block and a partial one in the same grid (N = 18: 72 ids)
    assert any(c.grid % 64 == 0 for c in seen[1]["pairs64"]) and any(c.grid < 64 for c in seen[1]["pairs64_partial"])
    assert any(c in seen[1]["pairs64_partial"] for c in seen[1]["pairs64"])
    assert set(seen[4]) == {"block16", "block16_tail"}
    tails = {(c.N // 16 > 0, c.N % 16) for c in CASES}
    assert {(False, 1), (False, 15), (True, 0), (True, 1), (True, 15)} <= tails  # no full block | full blocks only | ragged tails
    assert {c.tchunks for c in seen[4]["block16_tail"]} == {1, 2, 3} and {c.tchunks for c in seen[4]["block16"]} >= {1, 2}


# ---- coordinates and their tap tables (host) ---------------------------------------------------------------------------------------------
def seed_of(c, salt=0):
    return zlib.crc32(c.id.encode()) + salt


@functools.lru_cache(maxsize=None)
def good_multiples(size0, sizes):
    """The multiples of 8 in [0, size0) (level-0 units of one axis), most round-trip-exact taps over the four levels first."""
    cand = np.arange(0, size0, 8, dtype=np.float32)
    c = np.stack([cand, cand], -1)[None]  # [1,K,2]
    score = np.zeros(len(cand))
    for l, tab in enumerate(sampler_taps(c, [(s, s) for s in sizes])):
        score += ((tab["wx0"] == 1) & (tab["wx1"] == 0)).sum(-1)[0]
    return tuple(cand[np.argsort(-score, kind="stable")].tolist())


def kind_of(c):
    """[S,N] indices into KINDS: the kinds walk along a track and from point to point."""
    return (np.arange(c.N)[None] + np.arange(c.S)[:, None]) % len(KINDS)


@functools.lru_cache(maxsize=None)
def coords_of(c):
    """[S,N,2] float32 (x, y) in level-0 units."""
    H0, W0 = c.sizes[0]
    r = np.random.RandomState(seed_of(c) % 2 ** 31)
    S, N = c.S, c.N
    kind = kind_of(c)
    xy = np.empty((S, N, 2))
    gx = good_multiples(W0, tuple(s[1] for s in c.sizes))
    gy = good_multiples(H0, tuple(s[0] for s in c.sizes))
    size = np.array([W0, H0])
    for t in range(S):
        for n in range(N):
            k = KINDS[kind[t, n]]
            i = n * S + t
            if k == "mult8":    # integers at every level; the better half of the candidates
                xy[t, n] = gx[r.randint((len(gx) + 1) // 2)], gy[r.randint((len(gy) + 1) // 2)]
            elif k == "int":
                xy[t, n] = r.randint(0, W0), r.randint(0, H0)
            elif k == "half":
                xy[t, n] = r.randint(0, W0 - 1) + 0.5, r.randint(0, H0 - 1) + 0.5
            elif k == "corner":
                xy[t, n] = ((0, 0), (W0 - 1, 0), (0, H0 - 1), (W0 - 1, H0 - 1))[i // len(KINDS) % 4]
            elif k == "out":    # up to 8 units outside one border (every border in turn), the other axis anywhere up to 8 outside
                side, ax = divmod(i // len(KINDS) % 4, 2)
                p = r.uniform(-8, size + 7)
                p[ax] = -r.uniform(0, 8) if side == 0 else size[ax] - 1 + r.uniform(0, 8)
                if i % 2:
                    p = np.round(p)
                xy[t, n] = p
            elif k == "far":
                xy[t, n] = (-50.0, 1000.0) if i // len(KINDS) % 2 == 0 else (1000.0, -50.0)
            else:
                xy[t, n] = r.uniform(0, size - 1)
    return xy.astype(np.float32)


@functools.lru_cache(maxsize=None)
def taps_of(c):
    return sampler_taps(coords_of(c), c.sizes)


def exact_taps(tab):
    """-> [S,N,49] bool: the four corner weights of tap p = 7 * (x index) + (y index) are all 0 or 1 (then w0 == 1: the value is the
    pixel (y0, x0))."""
    ex = (tab["wx0"] == 1) & (tab["wx1"] == 0)
    ey = (tab["wy0"] == 1) & (tab["wy1"] == 0)
    return (ex[..., :, None] & ey[..., None, :]).reshape(*ex.shape[:2], TAPS)


def footprints(tab):
    """-> (fw, fh) [S,N]: the footprint of the 49 taps, as the SH kernels size it."""
    return tab["x1"][..., 6] - tab["x0"][..., 0] + 1, tab["y1"][..., 6] - tab["y0"][..., 0] + 1


def gather_share():
    """pyramid -> level -> share of exact gathers among the entries of the tracks at multiples of 8, over the case list."""
    out = {}
    for name in PYRAMIDS:
        cs = [c for c in CASES if c.pyr == name]
        out[name] = [float(np.concatenate([exact_taps(taps_of(c)[l])[kind_of(c) == 0].ravel() for c in cs]).mean()) for l in range(LEVELS)]
    return out


def test_exact_gather_share():
    for c in CASES:
        ints = kind_of(c) == 0
        assert ints.any(), c.id
        union = np.zeros(TAPS, bool)
        for l, tab in enumerate(taps_of(c)):
            ex = exact_taps(tab)[ints]  # [pairs,49]
            assert ex.mean() >= 1 / 8, (c.id, l, ex.mean())
            union |= ex.any(0)
        assert union.all(), (c.id, np.nonzero(~union)[0])
    # the far points are clamped on both axes at every level: exact on every tap
    c = CASES[3]
    assert all(exact_taps(tab)[kind_of(c) == KINDS.index("far")].all() for tab in taps_of(c))


def test_footprints_cover_every_size():
    seen, kinds = {name: set() for name in PYRAMIDS}, set()
    for c in CASES:
        kinds |= set(kind_of(c).ravel().tolist())
        for tab in taps_of(c):
            fw, fh = footprints(tab)
            assert fw.min() >= 1 and fh.min() >= 1 and fw.max() <= 9 and fh.max() <= 9, c.id  # (FROWS = 88 >= 81)
            seen[c.pyr] |= set(zip(fw.ravel().tolist(), fh.ravel().tolist()))
    assert kinds == set(range(len(KINDS)))
    assert {(8, 8), (9, 8), (8, 9), (9, 9)} <= seen["p48"], seen["p48"]          # (version 3 loads extra row tiles above 64 pixels)
    assert {(8, 8), (9, 9)} <= seen["odd"] | seen["p9"]
    for name in PYRAMIDS:
        assert any(fw < 8 for fw, _ in seen[name]) and any(fh < 8 for _, fh in seen[name]), name
        assert {(2, 1), (1, 2)} <= seen[name], name  # (-50, 1000) and (1000, -50): pixels 0 and 1 on one axis, the last one on the other
    assert any(fw * fh > 64 for fw, fh in seen["odd"]) and any(fw * fh > 80 for fw, fh in seen["p48"])
    corners = set()
    for c in CASES:
        H0, W0 = c.sizes[0]
        xy = coords_of(c)[kind_of(c) == KINDS.index("corner")]
        corners |= {(x == 0, y == 0) for x, y in xy.tolist() if x in (0, W0 - 1) and y in (0, H0 - 1)}
    assert len(corners) == 4


@functools.lru_cache(maxsize=None)
def injections(N):
    """pi [4][N][49]: per (level, point) an injection of the taps into the channels."""
    r = np.random.RandomState(4900 + N)
    return np.stack([np.stack([r.permutation(CH)[:TAPS] for _ in range(N)]) for _ in range(LEVELS)])


def test_injections_differ():
    for N in sorted({c.N for c in CASES} | {33}):
        pi = injections(N)
        assert all(len(set(row.tolist())) == TAPS for row in pi.reshape(-1, TAPS))
        for d in (1, 2, 16, 32):  # neighbours under some dealing
            if d < N:
                assert ((pi[:, d:] != pi[:, :-d]).sum(-1) >= 40).all(), (N, d)
        for a in range(LEVELS):
            for b in range(a):
                assert ((pi[a] != pi[b]).sum(-1) >= 40).all(), (N, a, b)


# ---- operands (GPU) ---------------------------------------------------------------------------------------------------------------------
class Problem:
    """One case on the GPU: pyramid and support inside NaN frames, the float64 reference volume [4][S][N][2401], and for exact
    inputs the expected gathers [4][S][N][49][49] (f32) with the mask of the taps on which they are exact, [4][S][N][49]."""

    def __init__(self, c, kind, support_from=None):
        from cotracker_amd import ops
        from oracle import window_fp64 as W
        g = torch.Generator(device=dev()).manual_seed(seed_of(c, 1 if kind == "exact" else 2))
        S, N = c.S, c.N
        self.c, self.kind = c, kind
        self.coords = torch.from_numpy(coords_of(c)).to(dev())
        pyr = []
        for H, Wd in c.sizes:
            if kind == "exact":
                f = torch.randint(1, 9, (S, H, Wd, CH), generator=g, device=dev()).float() / 16
                f = f * (torch.randint(0, 2, f.shape, generator=g, device=dev()).float() * 2 - 1)
            else:
                f = torch.randn(S, H, Wd, CH, generator=g, device=dev())
                f = f / f.norm(dim=-1, keepdim=True)
            pyr.append(nan_framed(f))
        if kind == "exact":
            pi = torch.from_numpy(injections(N)).to(dev())  # [4][N][49]
            sup = [nan_framed(torch.zeros(N, TAPS, CH, device=dev()).scatter_(2, pi[l][..., None], 1.0)) for l in range(LEVELS)]
        else:
            q = self.coords[0]
            sup = [nan_framed(ops.sample_support(pyr[l], torch.zeros(N, device=dev()), (q / 2 ** l).contiguous())) for l in range(LEVELS)]
        self.pyr, self.sup = pyr, sup
        self.ref = [W.volume(pyr[l].permute(0, 3, 1, 2).double(), sup[l].permute(1, 0, 2).double(), self.coords / 2 ** l)
                    for l in range(LEVELS)]
        if kind == "exact":
            self.exact, self.gather = [], []
            tt = torch.arange(S, device=dev())[:, None, None, None, None]
            for l, tab in enumerate(taps_of(c)):
                x0, y0 = (torch.from_numpy(tab[a]).to(dev()) for a in ("x0", "y0"))
                self.exact.append(torch.from_numpy(exact_taps(tab)).to(dev()))
                # value of the floor pixel (y0[j], x0[i]) in channel pi(q): [S][N][7 (i)][7 (j)][49 (q)] -> tap p = 7 i + j
                v = pyr[l][tt, y0[:, :, None, :, None], x0[:, :, :, None, None], pi[l][None, :, None, None, :]]
                self.gather.append(v.reshape(S, N, TAPS, TAPS))

    def mask(self, kind=None):
        kind = self.c.mask if kind is None else kind
        if kind == "none":
            return None
        m = torch.ones(self.c.N, dtype=torch.uint8, device=dev())
        if kind == "all":
            m[:] = 0
        else:
            m[1::3] = 0
        return m

    def window(self, mask=None, coords=None, sup=None, **kw):
        from cotracker_amd import ops
        c = self.c
        z = torch.zeros(c.S, c.N, device=dev())
        H0, W0 = c.sizes[0]
        return ops.Window(self.pyr, self.sup if sup is None else sup, self.coords if coords is None else coords, z, z.clone(),
                          (float(W0), float(H0)), iters=1, point_mask=mask, **kw)


@functools.lru_cache(maxsize=None)
def problem(c, kind):
    return Problem(c, kind)


def select(kern, ctk_option):
    """Makes `kern` the sampler of the SH path -> whether the volume is SH."""
    from cotracker_amd import _lib
    if kern == "f32":
        return False
    ctk_option(_lib.OPT_CORR_VERSION, 1 if kern == "sh1" else 3)
    if kern.startswith("sh3m"):
        ctk_option(_lib.OPT_CORR_MAP, int(kern[4:]))
    return True


def launch(win, kern, ctk_option, tag=""):
    """One volume call after the canary checks -> (raw volume, its values as float64 [4][S][N][2401])."""
    sh = select(kern, ctk_option)
    vol, intact = corr_volume_raw(win, sh, CANARY)
    assert intact, f"{tag}: a store outside the 4 x N * S volume rows"
    flat = vol.reshape(LEVELS, win.N * win.S, -1)
    assert not bool(torch.isnan(flat).any()), f"{tag}: NaN in the volume: a read outside the operands, or an element never written"
    pad = vol[:, :, CORR_LD // 32 - 1, :, CORR_K % 32:] if sh else vol[:, :, CORR_K:]
    assert bool((pad.contiguous().view(torch.int16 if sh else torch.int32) == 0).all()), f"{tag}: columns 2401..2431 are not exact zeros"
    val = (vol[:, :, :, 0].double() + vol[:, :, :, 1].double()).reshape(LEVELS, win.N * win.S, CORR_LD) if sh else vol.double()
    return vol, val[:, :, :CORR_K].reshape(LEVELS, win.N, win.S, CORR_K).transpose(1, 2)


def halves(vol):
    """SH volume -> (hi, lo) f16 [4][S][N][2401]."""
    L_, R = vol.shape[:2]
    return tuple(vol[:, :, :, h].reshape(L_, R, CORR_LD)[:, :, :CORR_K] for h in (0, 1))


def check_mask(c, kern, full, masked, mask, tag):
    """Dead points' rows are exact zeros, live rows keep the bits of the unmasked run."""
    dead = (mask == 0).nonzero()[:, 0]
    live = (mask != 0).nonzero()[:, 0]
    a, b = (v.reshape(LEVELS, c.N, c.S, -1) for v in (full, masked))
    assert bool((b[:, dead].contiguous().view(torch.int16) == 0).all()), f"{tag}: a dead point's rows are not exact zeros"
    assert same_bits(a[:, live], b[:, live]), f"{tag}: a live point's rows differ from the unmasked run"


# ---- 1 - 3: exact gathers, the derived bound, masks, canaries --------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c,kern", BOTH, ids=BOTH_IDS)
def test_exact(c, kern, ctk_option):
    P = problem(c, "exact")
    tag = f"{c.id}-{kern}"
    vol, val = launch(P.window(), kern, ctk_option, tag)
    sh = kern != "f32"
    bound = BOUND_SH if sh else BOUND_F32
    S, N = c.S, c.N
    if sh:
        hi, lo = (h.reshape(LEVELS, N, S, TAPS, TAPS).transpose(1, 2) for h in halves(vol))
    else:
        f32v = vol[:, :, :CORR_K].reshape(LEVELS, N, S, TAPS, TAPS).transpose(1, 2)
    for l in range(LEVELS):
        ex = P.exact[l][..., None].expand(S, N, TAPS, TAPS)
        want = P.gather[l]
        assert bool(ex.any())
        # (the restatement and the oracle agree on where the exact taps land)
        assert maxdiff(P.ref[l].reshape(S, N, TAPS, TAPS)[ex], want[ex]) < 1e-12
        if sh:
            bad = ((hi[l].contiguous().view(torch.int16) != want.half().view(torch.int16)) | (lo[l] != 0)) & ex
        else:
            bad = (f32v[l].contiguous().view(torch.int32) != want.view(torch.int32)) & ex
        assert not bool(bad.any()), f"{tag} level {l}: {int(bad.sum())} of {int(ex.sum())} exact gathers are not the feature value to the " \
                                    f"bit; first (frame, point, tap p, tap q) {bad.nonzero()[0].tolist()}"
        err = (val[l] - P.ref[l]).abs().reshape(S, N, TAPS, TAPS)
        e = float(err[~ex].max()) if bool((~ex).any()) else 0.0
        ERRORS[("exact", kern, l)] = max(ERRORS.get(("exact", kern, l), 0.0), e)
        print(f"{tag} level {l}: blended entries max |out - float64| {e:.3e} (bound {bound:.3e})")
        assert e <= bound, (tag, l, e, bound)
    if c.mask != "none":
        m = P.mask()
        mvol, _ = launch(P.window(mask=m), kern, ctk_option, tag + "-masked")
        check_mask(c, kern, vol, mvol, m, tag)


# ---- 6: random operands against float64 at the project's bars -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c,kern", BOTH, ids=BOTH_IDS)
def test_fp64(c, kern, ctk_option):
    P = problem(c, "real")
    tag = f"{c.id}-{kern}"
    m = P.mask()
    vol, val = launch(P.window(mask=m), kern, ctk_option, tag)
    live = torch.ones(c.N, dtype=torch.bool, device=dev()) if m is None else m.bool()
    for l in range(LEVELS):
        want = P.ref[l] * live[None, :, None]
        e = maxdiff(val[l], want)
        ERRORS[("fp64", kern, l)] = max(ERRORS.get(("fp64", kern, l), 0.0), e)
        print(f"{tag} level {l}: max |out - float64| {e:.3e}")
        assert e < BAR["f32" if kern == "f32" else "sh"], (tag, l, e)
    if m is not None and c.mask != "all":
        full, _ = launch(P.window(), kern, ctk_option, tag + "-unmasked")
        check_mask(c, kern, full, vol, m, tag)


@pytest.fixture(scope="module", autouse=True)
def error_record():
    """CTK_CORR_MATRIX_ERRORS=<file>: the largest error per kernel and level (profiles/corr_matrix_errors.json)."""
    yield
    path = os.environ.get("CTK_CORR_MATRIX_ERRORS")
    if path and ERRORS:
        def table(test):
            return {k: [float(f"{ERRORS[(test, k, l)]:.3e}") for l in range(LEVELS)] for k in KERNELS if (test, k, 0) in ERRORS}
        rec = {"what": "tests/test_gpu_corr_matrix.py: largest |out - float64 reference| per kernel (sh3mK: version 3 under CTK_OPT_CORR_MAP "
                       "= K) and pyramid level over the case list; MI355X",
               "module_cases": len(CASES), "kernels": list(KERNELS),
               "exact_inputs_blended_entries": {"bound_f32": BOUND_F32, "bound_sh": BOUND_SH, "max": table("exact")},
               "random_operands": {"bar_f32": BAR["f32"], "bar_sh": BAR["sh"], "max": table("fp64")},
               "corrblock_one_hot": {"bound": BOUND_CORRBLOCK, "max": {k[1]: float(f"{v:.3e}") for k, v in ERRORS.items() if k[0] == "corrblock"}},
               "exact_gather_share_of_integer_tracks": gather_share()}
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)


# ---- 4: bit identities --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_maps_do_not_change_a_bit(c, ctk_option):
    """Version 3 under maps 0, 1, 2 and 4 == map 3: the dealing must not change any point's arithmetic."""
    for kind in ("real", "exact"):
        P = problem(c, kind)
        win = P.window(mask=P.mask())
        base, _ = launch(win, "sh3m3", ctk_option, c.id)
        base = base.clone()
        for m in (0, 1, 2, 4):
            vol, _ = launch(win, f"sh3m{m}", ctk_option, c.id)
            assert same_bits(vol, base), f"{c.id} ({kind} operands): map {m} differs from map 3 in " \
                                         f"{int((vol.view(torch.int16) != base.view(torch.int16)).any(-1).any(-1).any(-1).sum())} rows"


ISOLATION = Case(17, 17, "odd")


@gpu
@pytest.mark.parametrize("kern", KERNELS)
def test_point_isolation(kern, ctk_option):
    """Other coordinates and another support patch for one point: every other point keeps its bits (and that point does not)."""
    c = ISOLATION
    P = problem(c, "real")
    first, _ = launch(P.window(), kern, ctk_option, c.id)
    first = first.clone()
    j = 8
    coords = P.coords.clone()
    coords[:, j] = coords[:, j].flip(0) + 1.25
    sup = [s.clone() for s in P.sup]
    for s in sup:
        s[j] = s[j].flip(0) * 1.5
    second, _ = launch(P.window(coords=coords, sup=sup), kern, ctk_option, c.id)
    a, b = (v.reshape(LEVELS, c.N, c.S, -1) for v in (first, second))
    others = torch.arange(c.N, device=dev()) != j
    assert same_bits(a[:, others], b[:, others]), kern
    assert not same_bits(a[:, j], b[:, j]), kern


_models = {}
CHUNKED = Case(33, 17, "odd")
EMBED_KERNELS = KERNELS


def weights(kern):
    return ctk_support.small_model(_models, "f32" if kern == "f32" else "f16x3", window_len=CHUNKED.S).packed(dev())


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("kern", EMBED_KERNELS)
def test_chunked_corr_embed_equals_unchunked(kern, masked, ctk_option):
    """ctk_corr_embed of 33 points in pieces of 1, 5, 16 and 17 (n0 > 0; ncount odd, even, a multiple of 16, ragged last pieces of
    3, 1 and 16) == one piece; the mask's dead points straddle the cuts at 5, 16 and 17 and fill the last piece."""
    from cotracker_amd import ops
    c = CHUNKED
    P = problem(c, "real")
    select(kern, ctk_option)
    pw = weights(kern)
    m = None
    if masked:
        m = torch.ones(c.N, dtype=torch.uint8, device=dev())
        m[[4, 5, 15, 16, 17, 32]] = 0
    whole = ops.corr_embed(P.window(mask=m), pw)
    assert torch.isfinite(whole).all() and float(whole[:, :1024].abs().max()) > 0
    for k in (1, 5, 16, 17):
        win = P.window(mask=m, max_corr_rows=k * c.S)
        assert win.args.points_per_chunk == k
        part = ops.corr_embed(win, pw)
        assert same_bits(part, whole), f"{kern}: points_per_chunk = {k} changes {int((part != whole).any(-1).sum())} rows"


@gpu
@pytest.mark.parametrize("chunk", [16, 5, 33])
@pytest.mark.parametrize("kern", EMBED_KERNELS)
def test_grouped_launch_equals_per_group_launches(kern, chunk, ctk_option):
    """ctk_corr_embed_batch over three query groups of 11 points of one video, masked: ONE grouped sampler launch per piece
    (CTK_BATCH_SHARED_FMAPS) == one launch per group and piece.  Pieces of 16 (11 + 5 | 6 + 10 | 1), of 5 and one of 33 stacked
    points straddle the group boundaries at 11 and 22; dead points sit on either side of them."""
    from cotracker_amd import ops
    c = CHUNKED
    P = problem(c, "real")
    select(kern, ctk_option)
    pw = weights(kern)
    G, n = 3, 11
    coords = P.coords.reshape(c.S, G, n, 2).permute(1, 0, 2, 3).contiguous()  # [G][S][n][2]: group g holds points g * n ..
    m = torch.ones(G, n, dtype=torch.uint8, device=dev())
    m.view(-1)[[3, 10, 11, 15, 16, 21, 32]] = 0
    z = torch.zeros(G, c.S, n, device=dev())
    H0, W0 = c.sizes[0]
    wins = ops.group_windows(P.pyr, P.sup, coords, z, z.clone(), (float(W0), float(H0)), point_mask=m, iters=1)
    shared = ops.corr_embed_batch(wins, pw, points_per_chunk=chunk, shared=True)
    unshared = ops.corr_embed_batch(wins, pw, points_per_chunk=chunk, shared=False)
    assert torch.isfinite(shared).all() and float(shared[:, :1024].abs().max()) > 0
    assert same_bits(shared, unshared), f"{kern}, chunk {chunk}: {int((shared != unshared).any(-1).sum())} rows differ"
    # the groups really are the stacked points of the single window: the same rows as its own (masked) corr_embed, to fp32 class
    one = ops.corr_embed(P.window(mask=m.view(-1).contiguous()), pw)
    assert maxdiff(shared, one) <= 1e-5 * max(1.0, float(one.abs().max()))


# ---- 5: the rest of the family ---------------------------------------------------------------------------------------------------------
FAMILY = [Case(17, 1, "odd"), Case(17, 17, "odd"), Case(15, 1, "p9"), Case(16, 17, "p9")]


@gpu
@pytest.mark.parametrize("c", FAMILY, ids=[c.id for c in FAMILY])
def test_corrblock_one_hot(c):
    """ctk_corrblock_sample with targets e_ch(t, n): out[n][t][49 l + p] = blend of f[.][ch] / sqrt(128)."""
    from cotracker_amd import ops
    from oracle import window_fp64 as W
    P = problem(c, "exact")
    S, N = c.S, c.N
    g = torch.Generator(device=dev()).manual_seed(seed_of(c, 3))
    ch = torch.randint(0, CH, (S, N), generator=g, device=dev())
    tg = nan_framed(torch.zeros(S, N, CH, device=dev()).scatter_(2, ch[..., None], 1.0))
    out = ops.corrblock_sample(P.pyr, tg, P.coords)  # [N][S][196]
    assert torch.isfinite(out).all()
    sqrt_c = float(np.sqrt(np.float32(CH)))  # torch.sqrt(torch.tensor(C).float()): the float32 root
    worst = 0.0
    for l in range(LEVELS):
        pat = W.patches(P.pyr[l].permute(0, 3, 1, 2).double(), P.coords / 2 ** l)  # [S][N][49][128]
        want = pat.gather(3, ch[:, :, None, None].expand(S, N, TAPS, 1))[..., 0] / sqrt_c
        got = out[:, :, l * TAPS:(l + 1) * TAPS].transpose(0, 1)
        worst = max(worst, maxdiff(got, want))
        ex = P.exact[l]  # one rounding only: the division
        x0, y0 = (torch.from_numpy(taps_of(c)[l][a]).to(dev()) for a in ("x0", "y0"))
        tt = torch.arange(S, device=dev())[:, None, None, None]
        v = P.pyr[l][tt, y0[:, :, None, :], x0[:, :, :, None], ch[:, :, None, None]].reshape(S, N, TAPS)
        one = torch.from_numpy(v.cpu().numpy() / np.sqrt(np.float32(CH))).to(dev())  # (numpy: an IEEE float32 division)
        assert same_bits(got[ex], one[ex]), (c.id, l)
    ERRORS[("corrblock", c.id, 0)] = worst
    print(f"{c.id}: corrblock max |out - float64| {worst:.3e} (bound {BOUND_CORRBLOCK:.3e})")
    assert worst <= BOUND_CORRBLOCK, (c.id, worst)


@gpu
@pytest.mark.parametrize("c", FAMILY, ids=[c.id for c in FAMILY])
@pytest.mark.parametrize("kind", ["exact", "real"])
def test_patch_and_support_samplers_bit_exact(c, kind):
    """sample_patches (every level, the case's coordinates) and sample_support (T = S frames, fractional and out-of-range frames)
    against the numpy restatement of the reference, bit for bit."""
    from cotracker_amd import ops
    from oracle import cotracker_oracle as O
    P = problem(c, kind)
    S, N = c.S, c.N
    xy = coords_of(c)
    r = np.random.RandomState(seed_of(c, 4) % 2 ** 31)
    frames = r.randint(0, S, N).astype(np.float32)
    frames[::3] += np.float32(0.25)
    frames[1::5] = -1.0  # out of range on either side: clamped to the first / last frame
    frames[4::5] = S + 0.5
    for l in range(LEVELS):
        fm = P.pyr[l].cpu().numpy()                              # [S,H,W,128]
        nchw = np.ascontiguousarray(fm.transpose(0, 3, 1, 2))[None]  # [1,S,128,H,W]
        out = ops.sample_patches(P.pyr[l], P.coords, l).cpu().numpy()
        ref = O.get_correlation_feat(nchw, (xy / np.float32(2 ** l)).astype(np.float32))
        assert np.array_equal(out, ref[0].reshape(S, N, TAPS, CH)), (c.id, l, "sample_patches")
        qc = (xy[S // 2] / np.float32(2 ** l)).astype(np.float32)
        out = ops.sample_support(P.pyr[l], torch.from_numpy(frames).to(dev()), torch.from_numpy(qc).to(dev())).cpu().numpy()
        ref = O.get_track_feat(nchw, frames[None], qc[None])  # [1,49,N,128]
        assert np.array_equal(out, ref[0].transpose(1, 0, 2)), (c.id, l, "sample_support")
