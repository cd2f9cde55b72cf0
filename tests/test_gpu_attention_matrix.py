"""ctk_attention_ex, the whole contract: every kernel x mask x stride x batch form, exact gathers, canaries, bit identities (-m gpu).

One entry point fans out to six compute kernels plus the split merge (attention.hip).  This module drives it through
`ctk_support.attention_raw` (every field of ctk_attn_args and ctk_attn_batch2 under the test's control) and checks

  1. EXACT INPUTS, no tolerance.  Per (batch, head) the keys are distinct +-1 sign vectors in 48 dimensions (distinctness is
     asserted on the host), query i is 512 * k[pi(i)] and V holds non-zero multiples of 1/16 in [-128, 128) (integers in [-8, 8]
     in the cases built around uniform rows).  Two distinct keys differ in a coordinate, so the winning logit leads by at least
     2 * 512 * 48^-0.5 = 147.8 nats = 213 in the log2 domain: every other probability is exactly 0 in f32, the winner's exactly 1,
     every rescale factor `alpha` and every merge weight 0 or 1, and 4096 * V and its sums are exact in f16 x f16 -> f32.  The
     output must be V[pi(i)] to the bit -- on the VALU kernel, on every MFMA kernel, through the 4-wave merge of the 64-query
     kernel and through attention_merge_kernel.  TWO-HOT: pairs of identical key rows with different V rows, placed in one tile,
     in two tiles of one wave (128 keys apart), in two waves (32 apart), in two splits and at the last (ragged) key; a query
     that points at a pair must return (V[j1] + V[j2]) / 2 exactly, which pins alpha == 1, the merge weights and the sums of l
     across tiles, waves and splits.  UNIFORM (n2 a power of two): a masked query, a row whose keys are all masked and a row
     with q = 0 return the exact mean of V.  Where n2 is no power of two a masked query's mean is not exact; those rows are
     left to 4.  pi is drawn over the unmasked keys, half of the draws from the keys next to a 16-key boundary and the last two
     keys, query 0 on the first and query n1 - 1 on the last unmasked key.
  2. THE CASE LIST comes from `route`, a restatement of the dispatcher's conditions; test_route_covers_every_kernel_and_axis
     asserts that each of the seven kernels gets every shape of its row of the table, both leading dimensions of q (384, 1152),
     k / v as column windows of a [rows][768] and a [rows][1152] matrix, o_ld at and above the minimum, o_bs != q_bs (always),
     both inner strides, single- and two-level batches (different outer strides for q, kv and out, per-video mask strides) and
     every mask kind it accepts: none, key, query, both, all keys masked, one split dead beside a live one.  Every case runs
     with f32 and with SH output.  The recorder names attention launches by their use on the path, not by kernel, so `route`
     documents which kernel a case is meant for and cannot prove it; CASES pins the dispatcher's thresholds only through the
     behaviours that differ (masks the persistent kernel does not take, the effective split count that bounds the writes
     into `partial`).
  3. CANARIES.  Every output allocation and `partial` are pre-filled with the NaN pattern 0x7FC17FC1 and must be bit-unchanged
     outside the addressed rows x 384 columns (the gaps o_ld, o_bs, o_is and the outer stride leave, the rows past the last
     batch) and outside partial[effective splits][nbatch][8][n1][50]; every operand allocation is NaN outside the addressed rows
     and head columns and the output may hold no NaN (a clamped padding read that left the operands would put one there:
     0 * NaN).  A read by a lane whose result is discarded cannot be seen this way.
  4. fp64 on randn operands with the masks of test_attention_masks, on the same case list, at the bound the project asserts
     already: max |out - ref| < 5e-6 on the f32 output.
  5. BIT IDENTITIES the code documents: the persistent time kernel == attention_self_kernel<2> (CTK_OPT_ATTENTION_TIME_PERSISTENT,
     small shapes and nbatch = 1031: a full persistent grid whose last pass of the job loop is partial); SH output ==
     split(f32 output) on every case (numpy's split of the GEMM matrix); rewriting one batch's q, k and v leaves every other
     batch's bits alone (two batches share a score tile on the pack-2 kernels, up to eight share a wave on the VALU kernel).

Not asserted: non-finite operands (on the pack-2 kernels 0 * inf from the tile partner is NaN; include/ctk.h says non-finite
values are not handled and range_guard re-runs such windows) and numeric range (tests/test_gpu_range.py).

Observed on an MI355X.  One finding: attention_self_kernel<2> ignored the QUERY mask (a masked query kept its logits: 376 of the
392 masked rows of the 16 x 16 x 7 query-mask case returned their gather instead of the mean; the other 16 were q = 0 rows).  The
source was right and the compiled kernel had lost the store -- a conditional `sacc[e] = NEG_MAX` behind the two short-circuit mask
loads; attention.hip now reads the query's flag once and selects.  With that every exact case is exact to the bit, every canary
intact and every identity holds.  Largest fp64 error per kernel over all mask kinds (profiles/attention_matrix_errors.json has
kernel x mask): kv64 9.8e-7, q64 6.5e-7, self<2> 6.7e-7, self<1> 1.3e-6, time16 1.2e-6, VALU 7.6e-7, through the merge kernel 7.5e-7
(bound 5e-6).  Sensitivity, shown once on scratch copies of attention.hip (which exact cases failed): no `alpha` rescale of oacc in
the 64-query kernel -> 6 q64 cases with n2 >= 1024 (a wave sees more than one tile); the V positions of keys 0 and 1 swapped in the
64-key kernel -> 5 kv64 cases (the key-masked ones: unmasked, keys 0 and 1 are a two-hot pair and the swap is no change); the last
key dropped from the VALU kernel's chunk loop -> 33 VALU cases; split 0 weighted by 1 in the merge kernel -> 26 cases with splits on
both paths; qm_obs ignored in the 64-key kernel -> the two two-level kv64 cases with a query mask.  The module's 299 tests (134
cases) take 5.0 s (the GEMM matrix: 170 cases, 4.2 s).
"""
import dataclasses
import json
import os
import zlib

import pytest
import torch

from ctk_support import attention_raw, dev, maxdiff, same_bits
from test_gpu_gemm_matrix import CANARY, np_split

pytestmark = pytest.mark.gpu

KERNELS = ("kv64", "q64", "self2", "self1", "time16", "valu", "merge")  # the six compute kernels and attention_merge_kernel
MASKS = ("none", "key", "query", "both", "allkeys", "deadsplit")
NEG = -torch.finfo(torch.float32).max
ERRORS = {}  # (kernel, mask) -> largest fp64 error of test_fp64


@dataclasses.dataclass(frozen=True)
class Case:
    kern: str           # the kernel the case is meant for: route() must agree
    n1: int
    n2: int
    nbatch: int
    splits: int = 1
    mask: str = "none"
    q_ld: int = 384     # 1152: q is the last 384 columns of a [rows][1152] matrix
    kvw: int = 768      # k | v are the last 768 columns of one [rows][kvw] matrix
    inner: str = "1"    # "1": the rows of a batch are contiguous | "S": they lie an inner batch count (and more) apart
    outer: int = 0      # 0: single level (b2 == NULL) | Bo: two-level batch of Bo x nbatch / Bo
    wide: bool = False  # o_ld above the minimum, the output a column window
    valu: bool = False  # CTK_OPT_ATTENTION_VALU = 1
    persistent: bool = True  # CTK_OPT_ATTENTION_TIME_PERSISTENT

    @property
    def id(self):
        return (f"{self.kern}-{self.n1}x{self.n2}-b{self.nbatch}-s{self.splits}-{self.mask}-q{self.q_ld}-kv{self.kvw}-is{self.inner}"
                f"-o{self.outer}" + ("-wide" if self.wide else "") + ("-valu" if self.valu else "") + ("" if self.persistent else "-np"))

    @property
    def binner(self):
        return self.nbatch // self.outer if self.outer else self.nbatch


# ---- the dispatcher's conditions, restated (attention.hip, ctk_attention_ex) ----------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def route(n1, n2, splits=1, two_level=False, masked=False, valu=False, persistent=True):
    """-> (compute kernel, effective splits); attention_merge_kernel follows when the effective splits exceed 1."""
    splits = max(splits, 1)

    def eff(tile):
        return cdiv(n2, cdiv(cdiv(n2, splits), tile) * tile)  # keys per split in whole tiles; empty splits are dropped
    if not valu and n2 == 64:
        return "kv64", 1
    if not valu and n1 == 64 and n2 > 64:
        return "q64", eff(32)
    if not valu and n1 == n2 and splits == 1 and not two_level:
        if n1 <= 16:
            return ("time16" if persistent and not masked else "self2"), 1
        return "self1", 1
    return "valu", eff(16)


def keys_per_split(c):
    tile = 32 if route_of(c)[0] == "q64" else 16
    return cdiv(cdiv(c.n2, max(c.splits, 1)), tile) * tile


def route_of(c):
    return route(c.n1, c.n2, c.splits, bool(c.outer), c.mask != "none", c.valu, c.persistent)


ACCEPTS = {"kv64": MASKS[:5], "q64": MASKS, "self2": MASKS[:5], "self1": MASKS[:5], "time16": ("none",), "valu": MASKS, "merge": MASKS}
TWO_LEVEL = ("kv64", "q64", "valu", "merge")
TABLE = {  # the shapes every kernel must see: n1, n2, nbatch, splits (None: not prescribed)
    "kv64": ({1, 31, 32, 33, 64, 127, 129, 511, 513, 641}, {64}, {1, 3}, None),
    "q64": ({64}, {65, 95, 96, 97, 128, 129, 1024, 1100}, None, {1, 2, 3, 4, 32}),
    "self2": ({1, 2, 8, 15, 16}, {1, 2, 8, 15, 16}, {1, 2, 7}, None),
    "time16": ({1, 2, 8, 15, 16}, {1, 2, 8, 15, 16}, {1, 2, 7, 1031}, None),
    "self1": ({17, 31, 32, 33, 63, 65, 100}, {17, 31, 32, 33, 63, 65, 100}, {1, 3}, None),
    "valu": ({1, 3, 5, 7, 9, 63, 65, 130}, {1, 15, 16, 17, 50}, {1, 8, 9, 13}, {1, 3}),
}


def _axes(i):
    """The addressing axes, cycled: eight consecutive cases hold every value of every axis."""
    return dict(q_ld=(384, 1152)[i & 1], kvw=(768, 1152)[(i >> 1) & 1], inner=("1", "S")[(i >> 2) & 1], wide=bool((i + (i >> 1)) & 1))


def _cases():
    cs = []

    def add(kern, n1, n2, nbatch, **kw):
        cs.append(Case(kern, n1, n2, nbatch, **dict(_axes(len(cs)), **kw)))

    # kv64: ragged 32-query tiles, one and two workgroups along the queries (512 per workgroup), the last one ragged
    for i, n1 in enumerate([1, 31, 32, 33, 64, 127, 129, 511, 513, 641]):
        add("kv64", n1, 64, (1, 3)[i & 1])
    for m in MASKS[1:5]:
        add("kv64", 129, 64, 3, mask=m)                    # (a key mask on a ragged query tile)
        add("kv64", 33, 64, 6, mask=m, outer=2)            # per-video masks
    add("kv64", 513, 64, 1, mask="key")
    add("kv64", 33, 64, 6, outer=3)
    # q64: ragged last tiles, 1..4 waves with work, splits (65 keys in 4 splits: 3 x 32, the empty one dropped; 1100 in 3: 384
    # each, the last one 10 tiles and 12 keys; 1100 in 32: 18 of 64)
    for i, (n2, s) in enumerate([(65, 1), (65, 4), (95, 2), (96, 3), (97, 1), (97, 4), (128, 1), (128, 2), (129, 3), (1024, 4),
                                 (1024, 32), (1100, 1), (1100, 3), (1100, 32)]):
        add("q64", 64, n2, (1, 2, 3)[i % 3], splits=s)
    for m, n2, s in [("query", 128, 1), ("key", 1024, 4), ("both", 1100, 3), ("allkeys", 128, 2), ("allkeys", 1024, 1), ("deadsplit", 128, 4),
                     ("query", 1024, 32), ("key", 97, 1), ("deadsplit", 1100, 3)]:
        add("q64", 64, n2, 2, splits=s, mask=m)
    for m in MASKS:
        add("q64", 64, 256, 4, splits=2, mask=m, outer=2)
    # square, n <= 16: two batches per score tile; odd batch counts leave the last tile half empty.  The same shapes on the
    # persistent kernel and on attention_self_kernel<2>; nbatch = 1031 -> 516 pairs x 8 heads = 4128 jobs on 2048 waves: two full
    # passes of the job loop and a third that 32 waves take
    for n in (1, 2, 8, 15, 16):
        for nb in (1, 2, 7):
            add("time16", n, n, nb)
            cs.append(dataclasses.replace(cs[-1], kern="self2", persistent=False))
    add("time16", 16, 16, 1031, q_ld=384, kvw=768)
    for m in MASKS[1:5]:
        add("self2", 16, 16, 7, mask=m)
    add("self2", 8, 8, 2, mask="both")
    add("self2", 15, 15, 3, mask="key")
    add("self2", 2, 2, 7, mask="query")
    # square, n > 16: 32-query tiles x 32-key tiles with the online softmax
    for i, n in enumerate([17, 31, 32, 33, 63, 65, 100]):
        add("self1", n, n, (1, 3)[i & 1])
    for m in MASKS[1:5]:
        add("self1", 32, 32, 3, mask=m)
    add("self1", 33, 33, 1, mask="key")
    add("self1", 100, 100, 3, mask="both")
    add("self1", 65, 65, 2, mask="query")
    # VALU: the natural fallback (neither side 64, not square) ...
    for i, n1 in enumerate([1, 3, 5, 7, 9, 63, 65, 130]):
        add("valu", n1, (15, 16, 17, 50, 1)[i % 5], (1, 8, 9, 13)[i % 4], splits=(1, 3)[i & 1])
    add("valu", 9, 50, 13, splits=3)
    add("valu", 3, 17, 9, splits=3)
    add("valu", 16, 16, 8, outer=2)                        # a two-level square shape other than 64 x 64
    add("valu", 17, 17, 6, outer=3)
    add("valu", 16, 16, 3, splits=2)                       # a square shape with splits
    for m in MASKS[1:5]:
        add("valu", 9, 16, 9, mask=m)
        add("valu", 5, 16, 8, mask=m, outer=2)
    add("valu", 65, 50, 3, splits=3, mask="key")
    add("valu", 65, 50, 3, splits=3, mask="deadsplit")
    add("valu", 130, 64, 2, splits=2, mask="deadsplit", outer=2, valu=True)
    # ... and forced onto the shapes of every MFMA kernel
    for n1, n2, nb, s, m in [(129, 64, 3, 1, "none"), (64, 129, 2, 3, "none"), (64, 128, 2, 2, "allkeys"), (16, 16, 7, 1, "none"),
                             (33, 33, 3, 1, "none"), (64, 64, 2, 1, "both"), (15, 15, 9, 1, "query"), (64, 1024, 1, 32, "deadsplit")]:
        add("valu", n1, n2, nb, splits=s, mask=m, valu=True)
    add("valu", 7, 17, 13, splits=3, valu=True)
    return cs


CASES = _cases()
IDS = [c.id for c in CASES]


def kernels_of(c):
    k, eff = route_of(c)
    return (k, "merge") if eff > 1 else (k,)


def test_route_covers_every_kernel_and_axis():
    assert len(set(IDS)) == len(IDS)
    for c in CASES:
        assert route_of(c)[0] == c.kern, c.id
        assert c.mask != "deadsplit" or route_of(c)[1] > 1, c.id
        assert not c.outer or c.nbatch % c.outer == 0, c.id
    seen = {k: [c for c in CASES if k in kernels_of(c)] for k in KERNELS}
    for k in KERNELS:
        cs = seen[k]
        assert cs, f"no case reaches {k}"
        # (every case runs with f32 and with SH output: test_exact, test_fp64)
        assert {c.q_ld for c in cs} == {384, 1152} and {c.kvw for c in cs} == {768, 1152}, k
        assert {c.inner for c in cs} == {"1", "S"} and {c.wide for c in cs} == {False, True}, k
        assert {c.mask for c in cs} == set(ACCEPTS[k]), (k, {c.mask for c in cs})
        assert {bool(c.outer) for c in cs} == ({False, True} if k in TWO_LEVEL else {False}), k
        if k in TABLE:
            n1s, n2s, nbs, sps = TABLE[k]
            assert n1s <= {c.n1 for c in cs} and n2s <= {c.n2 for c in cs}, k
            assert nbs is None or nbs <= {c.nbatch for c in cs}, k
            assert sps is None or sps <= {c.splits for c in cs}, k
    q64 = {(c.n2, c.splits): route_of(c)[1] for c in seen["q64"]}
    assert q64[(65, 4)] == 3 and q64[(1100, 32)] == 18 and q64[(1100, 3)] == 3 and 1100 % 32 != 0  # dropped splits, a ragged tile in the last
    assert any(c.valu for c in seen["valu"]) and any(not c.valu for c in seen["valu"])
    assert any(c.outer and c.n1 == c.n2 != 64 and not c.valu for c in seen["valu"])
    big = [c for c in seen["time16"] if c.nbatch > 512]
    assert big and all((c.nbatch + 1) // 2 * 8 > 2048 and ((c.nbatch + 1) // 2 * 8) % 2048 for c in big)


# ---- addressing ---------------------------------------------------------------------------------------------------------------------
class Layout:
    """Strides of a case and the row of every (batch, index) on the three sides.  Gaps differ from side to side: o_bs != q_bs."""

    def __init__(self, c):
        bi = c.binner
        self.side = {}
        for name, n, gap, ogap, igap, bs_s in (("q", c.n1, 1, 3, 0, 1), ("kv", c.n2, 2, 5, 1, 1), ("o", c.n1, 3, 7, 2, 2)):
            if c.inner == "1":
                is_, bs = 1, n + gap
                os_ = bi * bs + ogap
            else:
                is_, bs = bs_s * bi + igap, bs_s
                os_ = n * is_ + ogap
            b = torch.arange(c.nbatch)
            rows = ((b // bi) * os_ + (b % bi) * bs)[:, None] + torch.arange(n)[None] * is_
            assert rows.unique().numel() == rows.numel()
            self.side[name] = (bs, is_, os_, rows.reshape(-1).to(dev()), int(rows.max()) + 3)
        self.km_os, self.qm_os = c.n2 + 5, c.n1 + 3
        self.batch2 = None
        if c.outer:
            self.batch2 = dict(inner=bi, q_os=self.side["q"][2], kv_os=self.side["kv"][2], o_os=self.side["o"][2],
                               key_mask_os=self.km_os, query_mask_os=self.qm_os)


def launch(c, Q, K, V, km, qm, sh):
    """One call on operands Q [nbatch][n1][384], K / V [nbatch][n2][384], masks [Bo][n2] / [Bo][n1] uint8 or None, laid out as the
    case says inside NaN-filled allocations -> the output window [nbatch * n1][384] f32, or its SH form [.][12][2][32], after the
    canary checks."""
    lay = Layout(c)
    B, n1, n2 = c.nbatch, c.n1, c.n2
    (q_bs, q_is, _, qrows, qR), (kv_bs, kv_is, _, kvrows, kvR), (o_bs, o_is, _, orows, oR) = lay.side["q"], lay.side["kv"], lay.side["o"]
    qc, kc = c.q_ld - 384, c.kvw - 768
    qbuf = torch.full((qR, c.q_ld), float("nan"), device=dev())
    qbuf[qrows, qc:] = Q.reshape(-1, 384)
    kvbuf = torch.full((kvR, c.kvw), float("nan"), device=dev())
    kvbuf[kvrows, kc:kc + 384] = K.reshape(-1, 384)
    kvbuf[kvrows, kc + 384:] = V.reshape(-1, 384)
    ow, oc = (448, 32) if c.wide else (384, 0)  # in 4-byte units: an f32 row and an SH row are the same
    obuf = torch.full((oR, ow), CANARY, dtype=torch.int32, device=dev())
    part = torch.full((c.splits * B * 8 * n1 * 50 + 1024,), CANARY, dtype=torch.int32, device=dev()) if c.splits > 1 else None

    def mask_buf(m, n, stride):
        if m is None:
            return None
        buf = torch.zeros(m.shape[0], stride, dtype=torch.uint8, device=dev())
        buf[:, :n] = m
        return buf
    kmb, qmb = mask_buf(km, n2, lay.km_os), mask_buf(qm, n1, lay.qm_os)
    rc = attention_raw(qbuf[0, qc:], c.q_ld, q_bs, q_is, kvbuf[0, kc:], kvbuf[0, kc + 384:], c.kvw, kv_bs, kv_is,
                       obuf[0, oc:], ow * (2 if sh else 1), o_bs, o_is, B, n1, n2, splits=c.splits, partial=part, o_split=sh,
                       key_mask=kmb, query_mask=qmb, batch2=lay.batch2)
    assert rc == 0, rc
    written = torch.zeros(oR, ow, dtype=torch.bool, device=dev())
    written[orows, oc:oc + 384] = True
    assert bool((obuf[~written] == CANARY).all()), f"{c.id}: a store outside the addressed output rows and columns"
    if part is not None:
        eff = route_of(c)[1]
        used = eff * B * 8 * n1 * 50 if eff > 1 else 0
        assert bool((part[used:] == CANARY).all()), f"{c.id}: a store into `partial` outside [{eff}][nbatch][8][n1][50]"
    win = obuf[orows, oc:oc + 384].contiguous()
    out = win.view(torch.float16).reshape(B * n1, 12, 2, 32) if sh else win.view(torch.float32)
    assert not bool(torch.isnan(out).any()), f"{c.id}: NaN in the output: a read outside the operands, or an element never written"
    return out


def run_both(c, Q, K, V, km, qm, ctk_option):
    """f32 and SH output of one case -> the f32 output [nbatch][8][n1][48] after asserting SH == split(f32)."""
    from cotracker_amd import _lib
    ctk_option(_lib.OPT_ATTENTION_VALU, int(c.valu))
    ctk_option(_lib.OPT_ATTENTION_TIME_PERSISTENT, int(c.persistent))
    out = launch(c, Q, K, V, km, qm, False)
    osh = launch(c, Q, K, V, km, qm, True)
    assert same_bits(osh, torch.from_numpy(np_split(out.cpu().numpy()))), f"{c.id}: SH output != split(f32 output)"
    return out.reshape(c.nbatch, c.n1, 8, 48).permute(0, 2, 1, 3)


# ---- operands -----------------------------------------------------------------------------------------------------------------------
def gen(c, salt=0):
    return torch.Generator(device=dev()).manual_seed(zlib.crc32(c.id.encode()) + salt)


def masks(c, g):
    """-> (key mask [Bo][n2] or None, query mask [Bo][n1] or None), uint8, one row per video."""
    Bo = c.outer or 1
    km = qm = None
    if c.mask in ("key", "both"):
        km = (torch.rand(Bo, c.n2, generator=g, device=dev()) > 0.3).to(torch.uint8)
        for bo in range(Bo):
            km[bo, (7 * bo + 3) % c.n2] = 1
    if c.mask in ("query", "both"):
        qm = (torch.rand(Bo, c.n1, generator=g, device=dev()) > 0.3).to(torch.uint8)
    if c.mask == "allkeys":
        km = torch.zeros(Bo, c.n2, dtype=torch.uint8, device=dev())
    if c.mask == "deadsplit":  # every key of one split masked, another split beside it in every video
        eff, kps = route_of(c)[1], keys_per_split(c)
        km = torch.ones(Bo, c.n2, dtype=torch.uint8, device=dev())
        for bo in range(Bo):
            dead = (1 + bo) % eff
            km[bo, dead * kps:(dead + 1) * kps] = 0
    return km, qm


def two_hot_pairs(c):
    """Pairs of key slots that hold the same key row: one tile | two tiles of a wave of the 64-query kernel | two waves | two splits
    | the last key."""
    n2, kps = c.n2, keys_per_split(c)
    want = [(0, 1), (2, 130), (3, 35), (4, kps + 4), (5, n2 - 1)]
    used, pairs = set(), []
    for a, b in want:
        if b < n2 and a < b and not {a, b} & used:
            pairs.append((a, b))
            used |= {a, b}
    return pairs


def exact_problem(c):
    """-> Q, K, V, masks, the expected output [nbatch][8][n1][48] and the rows on which it is exact."""
    g = gen(c)
    B, n1, n2, bi = c.nbatch, c.n1, c.n2, c.binner
    km, qm = masks(c, g)
    pow2 = n2 & (n2 - 1) == 0
    sign = torch.randint(0, 2, (B, 8, n2, 48), generator=g, device=dev()).float() * 2 - 1
    pairs = two_hot_pairs(c) if km is None else []
    partner = torch.full((n2,), -1, dtype=torch.long, device=dev())
    single = torch.ones(n2, dtype=torch.bool, device=dev())
    for a, b in pairs:
        sign[:, :, b] = sign[:, :, a]
        partner[a], partner[b], single[b] = b, a, False
    code = ((sign > 0).long() << torch.arange(48, device=dev())).sum(-1)[:, :, single].sort(dim=2).values
    assert bool((code[:, :, 1:] != code[:, :, :-1]).all()), "two keys of one (batch, head) are the same sign vector"
    if c.mask in ("query", "both", "allkeys"):  # the cases built around uniform rows
        V = torch.randint(1, 9, (B, 8, n2, 48), generator=g, device=dev()).float()
    else:
        V = torch.randint(1, 2049, (B, 8, n2, 48), generator=g, device=dev()).float() / 16
    V = V * (torch.randint(0, 2, V.shape, generator=g, device=dev()).float() * 2 - 1)
    V[V == 128.0] = -128.0  # [-128, 128)
    pi = torch.zeros(B, 8, n1, dtype=torch.long, device=dev())
    dead = torch.zeros(B, dtype=torch.bool, device=dev())  # every key of the batch's video is masked
    edge = (torch.arange(n2) % 16 == 0) | (torch.arange(n2) % 16 == 15) | (torch.arange(n2) >= n2 - 2)
    for a, b in pairs:
        edge[a] = edge[b] = True
    for bo in range(c.outer or 1):
        sl = slice(bo * bi, (bo + 1) * bi) if c.outer else slice(None)
        ok = torch.ones(n2, dtype=torch.bool) if km is None else km[bo].bool().cpu()
        allowed = ok.nonzero()[:, 0].to(dev())
        if allowed.numel() == 0:
            dead[sl] = True
            continue
        near = (ok & edge).nonzero()[:, 0].to(dev())
        shape = pi[sl].shape
        p = allowed[torch.randint(0, allowed.numel(), shape, generator=g, device=dev())]
        if near.numel():
            pn = near[torch.randint(0, near.numel(), shape, generator=g, device=dev())]
            p = torch.where(torch.rand(shape, generator=g, device=dev()) < 0.5, pn, p)
        p[:, :, 0], p[:, :, -1] = allowed[0], allowed[-1]
        pi[sl] = p
    # q = 0: uniform over the keys that are not masked -- planted where that is all of them
    zero = torch.rand(B, 8, n1, generator=g, device=dev()) < (0.06 if pow2 and km is None else -1.0)
    uniform = zero | dead[:, None, None]
    if qm is not None:
        bo_of_b = torch.arange(B, device=dev()) // bi if c.outer else torch.zeros(B, dtype=torch.long, device=dev())
        uniform = uniform | ~qm.bool()[bo_of_b][:, None, :]
    idx = pi[..., None].expand(-1, -1, -1, 48)
    Qh = 512.0 * sign.gather(2, idx)
    Qh[zero] = 0.0
    second = torch.where(partner[pi] < 0, pi, partner[pi])[..., None].expand(-1, -1, -1, 48)
    want = (V.gather(2, idx) + V.gather(2, second)) / 2
    mean = (V.double().sum(2, keepdim=True) / n2).float().expand(-1, -1, n1, -1)
    want = torch.where(uniform[..., None], mean, want)
    exact = ~uniform if not pow2 else torch.ones_like(uniform)

    def rows(x):  # [B][8][n][48] -> [B][n][384]
        return x.permute(0, 2, 1, 3).reshape(B, -1, 384).contiguous()
    return rows(Qh), rows(sign), rows(V), km, qm, want, exact


def real_problem(c, salt=0):
    g = gen(c, 1 + salt)
    km, qm = masks(c, g)
    Q, K, V = (torch.randn(c.nbatch, n, 384, generator=g, device=dev()) for n in (c.n1, c.n2, c.n2))
    return Q, K, V, km, qm


def fp64_reference(c, Q, K, V, km, qm):
    """test_attention_masks' reference, the masks taken per video -> [nbatch][8][n1][48]."""
    B = c.nbatch
    bo = torch.arange(B, device=dev()) // c.binner if c.outer else torch.zeros(B, dtype=torch.long, device=dev())
    qh, kh, vh = (x.double().reshape(B, -1, 8, 48).transpose(1, 2) for x in (Q, K, V))
    sim = qh @ kh.transpose(-1, -2) * 48 ** -0.5
    if km is not None:
        sim = torch.where(km.bool()[bo][:, None, None, :], sim, torch.full_like(sim, NEG))
    if qm is not None:
        sim = torch.where(qm.bool()[bo][:, None, :, None], sim, torch.full_like(sim, NEG))
    return torch.softmax(sim, -1) @ vh


# ---- 1 - 3: exact gathers and means, canaries, SH == split(f32) ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_exact(c, ctk_option):
    Q, K, V, km, qm, want, exact = exact_problem(c)
    out = run_both(c, Q, K, V, km, qm, ctk_option)
    assert bool(exact.any())
    bad = (out.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).any(-1) & exact
    assert not bool(bad.any()), f"{c.id}: {int(bad.sum())} of {int(exact.sum())} rows are not the exact gather / mean; first (batch, head, " \
                                f"query) {bad.nonzero()[0].tolist()}"
    assert same_bits(out[exact], want[exact])


# ---- 4: randn operands against fp64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_fp64(c, ctk_option):
    Q, K, V, km, qm = real_problem(c)
    out = run_both(c, Q, K, V, km, qm, ctk_option)
    e = maxdiff(out, fp64_reference(c, Q, K, V, km, qm))
    for k in kernels_of(c):
        ERRORS[(k, c.mask)] = max(ERRORS.get((k, c.mask), 0.0), e)
    assert e < 5e-6, (c.id, e)


@pytest.fixture(scope="module", autouse=True)
def error_record():
    """CTK_ATTENTION_MATRIX_ERRORS=<file>: the largest fp64 error per kernel and mask kind (profiles/attention_matrix_errors.json)."""
    yield
    path = os.environ.get("CTK_ATTENTION_MATRIX_ERRORS")
    if path and ERRORS:
        rec = {"what": "tests/test_gpu_attention_matrix.py, test_fp64: largest |out - float64 reference| per kernel and mask kind over the "
                       "cases that reach the kernel (randn operands, f32 output); MI355X", "bound": "5e-6", "module_cases": len(CASES),
               "kernels": {k: {m: float(f"{ERRORS[(k, m)]:.3e}") for m in MASKS if (k, m) in ERRORS} for k in KERNELS}}
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)


# ---- 5: bit identities ----------------------------------------------------------------------------------------------------------------------
TIME16 = [c for c in CASES if c.kern == "time16"]


@pytest.mark.parametrize("c", TIME16, ids=[c.id for c in TIME16])
def test_persistent_time_kernel_equals_self2(c, ctk_option):
    from cotracker_amd import _lib
    ctk_option(_lib.OPT_ATTENTION_VALU, 0)
    assert route_of(c)[0] == "time16" and route_of(dataclasses.replace(c, persistent=False))[0] == "self2"
    for Q, K, V in (real_problem(c)[:3], exact_problem(c)[:3]):
        for sh in (False, True):
            ctk_option(_lib.OPT_ATTENTION_TIME_PERSISTENT, 1)
            a = launch(c, Q, K, V, None, None, sh)
            ctk_option(_lib.OPT_ATTENTION_TIME_PERSISTENT, 0)
            b = launch(c, Q, K, V, None, None, sh)
            assert same_bits(a, b), (c.id, sh)


def _isolation_cases():
    pick = [("kv64", 33, 64, "none"), ("kv64", 129, 64, "both"), ("q64", 64, 129, "none"), ("q64", 64, 256, "key"), ("self2", 15, 15, "none"),
            ("self2", 16, 16, "both"), ("time16", 15, 15, "none"), ("time16", 1, 1, "none"), ("self1", 33, 33, "none"), ("self1", 100, 100, "both"),
            ("valu", 9, 50, "none"), ("valu", 3, 17, "none"), ("valu", 5, 16, "both"), ("valu", 16, 16, "none")]
    return [max((c for c in CASES if (c.kern, c.n1, c.n2, c.mask) == p and c.nbatch > 1), key=lambda c: c.nbatch) for p in pick]


ISOLATION = _isolation_cases()


@pytest.mark.parametrize("c", ISOLATION, ids=[c.id for c in ISOLATION])
def test_batch_isolation(c, ctk_option):
    """Other finite values in one batch's q, k and v: every other batch keeps its bits (and the rewritten batch does not)."""
    Q, K, V, km, qm = real_problem(c)
    first = run_both(c, Q, K, V, km, qm, ctk_option)
    j = c.nbatch // 2  # (on the pack-2 kernels batches 2g and 2g + 1 share a tile: both parities occur over the cases)
    Q2, K2, V2, _, _ = real_problem(c, salt=7)
    for x, y in ((Q, Q2), (K, K2), (V, V2)):
        x[j] = 3.0 * y[j] + 1.0
    second = run_both(c, Q, K, V, km, qm, ctk_option)
    others = torch.arange(c.nbatch, device=dev()) != j
    assert same_bits(first[others], second[others]), c.id
    assert not same_bits(first[j], second[j]), c.id
