"""Stream-state contract matrix (-m gpu): every kernel of csrc/stream.hip -- begin, support, commit, assign, resident assign, emit,
health, each in its linear and its ring form -- through the C ABI, at block, wave and ring edges.

WHAT IS EXACT, AND WHY.  Everything.  The kernels move bytes, do single float32 multiplications and additions with explicit IEEE
intrinsics in a translation unit built without contraction, and count integers; tests/stream_reference.py restates them in numpy
from the rules of include/ctk.h, one float32 operation per step (tests/test_stream_reference_host.py holds the restatement against
the torch glue of the reference on the CPU).  After each call EVERY buffer handed over -- outputs, inputs, buffers the call has no
business with -- equals the restatement's as integers, so an untouched byte is one where the random pre-fill is still in place.  The
one inexact device step is expf inside `visible` / `alive`: the restatement forms sigmoid(vis) * sigmoid(conf) in float64 and the
logits are chosen so that the product is decisive or at least 0.02 from the threshold (asserted on the CPU, over every logit pair of
every case): a condition on the inputs, five orders above the device's rounding, not a tolerance on the kernel.

INPUTS.  Every buffer is pre-filled with random bytes (NaN patterns, infinities and subnormals included).  On top of that a case
writes finite values where a kernel does ARITHMETIC on what it reads (the carry rows of begin, the window of commit, accumulator
rows that are added to, the pyramid, emit's coordinates, logits that are thresholded): a NaN payload through a multiplication is not
a thing the header defines.  What is only copied (begin's carried logits, a plain assign's new queries) stays random bytes.

CANARIES.  Every buffer is a view into a ctk_support.nan_framed allocation (pattern 0x7FC17FC1, 2048 words on either side) and
frame_intact is asserted for every frame after every call: a store one row past a tensor lands there, and a sampler read that left
the pyramid would put a NaN into an accumulator.

THE CASE LIST (tests/test_stream_reference_host.py::test_case_list_covers_every_axis asserts that it reaches every branch):
  begin / commit  N in {1, 63, 64, 65, 255, 256, 257, 513} x G in {1, 3}; (S, step) in {(8, 4), (16, 8), (8, 3), (8, 7), (8, 1), (2, 1)};
                  T_valid in {1, S - 1, S}; linear ind in {0, step, later}, G * S * N no multiple of 256, N no divisor of 256; ring sizes
                  S, S + 1, 13, 2 S with ind such that the carry rows wrap, the commit rows wrap, both, neither; S = 64 at ind = 2^30 - 64
                  with a query at CTK_STREAM_EMPTY_FRAME == ind + S (mask 0) and one at ind + S - 64 (mask 1)
  query frames    left - 1, left, right - 1, right, ind + overlap - 1, ind + overlap, -0.5 (frame 0: sampled at ind == 0), a fraction,
                  a negative frame, EMPTY_FRAME, and NaN, +-inf, +-1e30, 2^31 (no window: mask 0, no accumulator byte, begun from the query)
  commit flag     NaN / +inf / -inf in x, y, vis, conf at lane 0, lane 63, wave 3, the last live lane; ring: the only live thread of
                  block 1 (N = 257), lane 1 of block 1 (N = 258), lane 0 of wave 1 of block 1 (N = 321); 6 -> 7; NULL; t >= T_valid
  support         P = G * N in {1, 2, 3, 4, 67} (P * 49 % 4 takes every residue) on the model's (16, 24) halving pyramid, the odd
                  pyramid (21, 27), (10, 13), (5, 6), (2, 3) and (1, 1) at every level; positions interior, integer, half-integer, the
                  corners, 8 units outside every border, NaN, +-inf, 1e30
  assign          M in {1, G * N, a list in no order with the first and last slot of every group}, out-of-range indices, rows in
                  {0, 1, T_cap, between}; resident: the nine kinds of test_gpu_stream_resident.py and the six frames of no window at
                  (8, 4), (16, 8), (8, 3), linear with the rows .. ind gap, ring with the carry rows wrapping, R == S
  emit            N_out in {N, N - 1, 1, 256, 257}, f1 - f0 == R, ranges that wrap, every optional output absent in turn, first_row with
                  INT32_MAX, f1 == 2^30
  health          1 and 2 cells at N_out = 513 (blocks that own no cell), 4096 cells at N_out = 1, 35 cells over 3 blocks
  identities      every linear case again through the ring entry point with R = T_cap >= ind + S: the same bits; a resident assign
                  with every frame outside the pyramid == ctk_stream_assign; begin_ring after assign_resident_ring starts the slot from
                  its query, at the wrapping shapes

NOT ASSERTED.  Speed.  The refusals of the entry points (tests/test_stream_*_cabi.py).  Subnormal or NaN operands of the float steps.
Two writers of one slot (the header leaves it undefined).

PLANTED FAULTS, each on a scratch copy of stream.hip with every access kept in bounds, the module run once against each -> what fails:
  the parent's bare (long)f conversion             17 begin, 2 support (ind == 0), 3 resident, 5 health cases: NaN, +inf and 1e30 frames
                                                   get point_mask 1 and are carried over, sampled at ind == 0 and judged as tracked
  begin: min(t, overlap - 1) -> min(t, overlap)    every begin case with ind > 0 (16), and the begin after 11 resident assigns
  ring commit: ring_row(ind) + t (clamped to R - 1) instead of ring_row(ind + t)
                                                   the 6 ring commit cases whose rows wrap, 3 ring flag cases
  support: left = ind + step at ind == 0 too       the 3 support cases with ind == 0
  resident: the `t >= rows && t < ind` skip removed   the 3 linear resident cases with rows < ind
  commit flag: lane 0 reports its own `bad` without the wave vote
                                                   4 of the 5 flag cases (lane 63, wave 3, last live lane, lane 1 of block 1)
  ring commit: idle threads return before the vote  NOTHING, and nothing can: the threads past N are the highest lanes of a wave, so
                                                   lane 0 of a wave is live whenever any of its lanes is, and the vote of the live lanes
                                                   reaches it.  The change alters no result; it is not a gap of the list.

Observed on an MI355X: 98 tests, 3.3 s for the module (the slowest test 0.26 s, the first launch of the process); every comparison
bit for bit, every frame intact."""
import ctypes as C
import dataclasses
import zlib

import numpy as np
import pytest

import stream_reference as ref
from ctk_support import lib  # noqa: F401  (the fixture)
from stream_reference import BIG, EMPTY_FRAME, LEVELS, f32

pytestmark = pytest.mark.gpu

PAD = 2048  # words of NaN pattern on either side of every buffer
NAN, INF = float("nan"), float("inf")
NO_WINDOW = (NAN, INF, -INF, 1e30, -1e30, 2.0 ** 31)  # the frames of "no window"
THRESH = 0.6
MARGIN = 0.02
PYRAMIDS = {"model": [(16, 24), (8, 12), (4, 6), (2, 3)], "odd": [(21, 27), (10, 13), (5, 6), (2, 3)], "ones": [(1, 1)] * 4}
LOGITS = np.array([-6.0, -2.5, -1.0, 0.0, 0.3, 1.2, 2.0, 3.7, 6.0, 88.0, -88.0, 104.0, -104.0, INF, -INF, NAN], f32)


@dataclasses.dataclass(frozen=True)
class Case:
    kernel: str
    ring: bool
    G: int
    N: int
    S: int = 8
    step: int = 4
    ind: int = 0
    R: int = 0          # T_cap of a linear history, the ring size of a ring
    T_valid: int = 0    # commit
    stride: float = 4.0
    pyr: str = "model"  # support, resident
    kw: tuple = ()      # what only one kernel reads, as (key, value) pairs

    def get(self, key, default=None):
        return dict(self.kw).get(key, default)

    @property
    def id(self):
        tail = "-".join(f"{k}{v}" for k, v in self.kw if k != "tag")
        return (f"{'ring' if self.ring else 'lin'}-G{self.G}-N{self.N}-S{self.S}.{self.step}-i{self.ind}-R{self.R}" +
                (f"-T{self.T_valid}" if self.T_valid else "") + (f"-st{self.stride:g}" if self.stride != 4.0 else "") +
                (f"-{self.pyr}" if self.kernel in ("support", "resident") else "") + (f"-{tail}" if tail else ""))

    @property
    def overlap(self):
        return self.S - self.step

    def rng(self, salt=0):
        return np.random.default_rng(zlib.crc32(f"{self.kernel}/{self.id}/{salt}".encode()))


def carry_wraps(c):
    return c.ring and c.ind > 0 and (c.ind % c.R) + c.overlap > c.R


def commit_wraps(c):
    return c.ring and (c.ind % c.R) + c.T_valid > c.R


LIMIT = 2 ** 30 - 64  # ind of the S = 64 window that ends on the admitted limit

# (ring, G, N, S, step, ind, R, T_valid, stride): begin reads all but T_valid, commit all; the ring rows of either list are the other's
_STEPS = [
    (False, 1, 1, 8, 4, 0, 8, 8, 4.0), (False, 3, 63, 8, 4, 4, 12, 7, 4.0), (False, 1, 64, 16, 8, 16, 35, 1, 4.0),
    (False, 3, 65, 8, 3, 6, 14, 8, 3.0), (False, 1, 255, 8, 7, 14, 22, 7, 4.0), (False, 1, 256, 8, 1, 5, 13, 1, 4.0),
    (False, 3, 257, 2, 1, 3, 5, 2, 4.0), (False, 1, 513, 8, 4, 8, 16, 7, 4.0),
    (True, 3, 1, 8, 4, 4, 8, 8, 4.0),      # R == S: the commit rows wrap, the carry rows do not
    (True, 1, 63, 8, 4, 8, 9, 7, 4.0),     # R == S + 1: both wrap
    (True, 3, 64, 16, 8, 16, 17, 1, 4.0),  # the carry rows wrap, the one commit row does not
    (True, 1, 65, 8, 3, 9, 13, 8, 3.0),    # both wrap
    (True, 3, 255, 8, 7, 21, 16, 7, 4.0),  # R == 2 S, neither wraps
    (True, 1, 256, 8, 1, 3, 8, 1, 4.0),    # overlap 7: the carry rows wrap
    (True, 1, 257, 2, 1, 5, 2, 2, 4.0),    # R == S == 2
    (True, 3, 513, 8, 4, 12, 13, 8, 4.0),  # both wrap
    (True, 1, 65, 8, 4, 0, 8, 1, 4.0),     # ind == 0 in a ring
    (True, 1, 5, 64, 32, LIMIT, 67, 64, 4.0), (True, 1, 5, 64, 32, LIMIT, 64, 63, 4.0),  # at the admitted limit
]
BEGIN = [Case("begin", r, G, N, S, st, ind, R, S, sd) for r, G, N, S, st, ind, R, tv, sd in _STEPS]
COMMIT = [Case("commit", r, G, N, S, st, ind, R, tv, sd) for r, G, N, S, st, ind, R, tv, sd in _STEPS]

# commit flag: (ring, G, N, S, T_valid) and the planted positions, as flat thread numbers of the launch
# linear: thread i = (g * T_valid + t) * N + n; ring: thread n of the blocks of (t, g), planted in the last (t, g)
FLAG = [
    (Case("commit", False, 3, 65, 8, 4, 4, 12, 7), {"lane0": 0, "lane63": 63, "wave3": 197, "wave3-block1": 448, "last-live": 3 * 7 * 65 - 1}),
    (Case("commit", True, 1, 65, 8, 4, 12, 13, 8), {"lane0": 0, "lane63": 63, "last-live": 64}),
    (Case("commit", True, 3, 257, 8, 4, 12, 13, 7), {"wave3": 199, "only-live-of-block1": 256}),
    (Case("commit", True, 1, 258, 8, 4, 4, 8, 8), {"lane1-of-block1": 257}),
    (Case("commit", True, 1, 321, 8, 4, 8, 9, 1), {"lane0-wave1-block1": 320}),
]

SUPPORT = [
    Case("support", False, 1, 1, 8, 4, 0, 8, pyr="model"), Case("support", False, 1, 2, 8, 4, 8, 16, pyr="odd"),
    Case("support", True, 3, 1, 2, 1, 3, 2, pyr="ones"), Case("support", False, 2, 2, 16, 8, 8, 24, pyr="model"),
    Case("support", False, 1, 67, 8, 4, 4, 12, pyr="model"), Case("support", True, 1, 67, 8, 3, 6, 13, stride=3.0, pyr="odd"),
    Case("support", False, 1, 67, 8, 7, 0, 8, pyr="ones"), Case("support", False, 1, 4, 8, 1, 2, 10, pyr="odd"),
    Case("support", True, 3, 11, 8, 4, 0, 8, pyr="odd"),
]

# assign: M = "one" | "all" | "list" (no order, first and last slot of every group) | "list+out" (and out-of-range indices)
ASSIGN = [
    Case("assign", False, 1, 1, 8, 4, 4, 12, kw=(("M", "one"), ("rows", 0))), Case("assign", False, 1, 2, 8, 4, 4, 12, kw=(("M", "all"), ("rows", 1))),
    Case("assign", False, 3, 1, 8, 4, 4, 12, kw=(("M", "list"), ("rows", 12))), Case("assign", False, 2, 2, 16, 8, 8, 24, kw=(("M", "list"), ("rows", 5))),
    Case("assign", False, 1, 67, 8, 4, 8, 16, kw=(("M", "list+out"), ("rows", 5))), Case("assign", False, 3, 11, 8, 3, 6, 14, kw=(("M", "list+out"), ("rows", 7))),
    Case("assign", True, 3, 11, 8, 4, 12, 13, kw=(("M", "list+out"),)), Case("assign", True, 1, 67, 8, 4, 4, 8, kw=(("M", "all"),)),
    Case("assign", True, 1, 1, 8, 4, 8, 9, kw=(("M", "one"),)),
]

# resident: frames = "kinds" (the nine of test_gpu_stream_resident.py + the six of no window) | "outside" (no resident frame)
RESIDENT = [
    Case("resident", False, 3, 11, 8, 4, 4, 12, kw=(("M", "list+out"), ("rows", 8))),
    Case("resident", False, 3, 11, 8, 4, 12, 20, kw=(("M", "list"), ("rows", 5))),   # rows 5 .. 11 are nobody's
    Case("resident", False, 3, 11, 16, 8, 8, 24, kw=(("M", "list"), ("rows", 0))),
    Case("resident", False, 3, 11, 16, 8, 24, 41, kw=(("M", "list"), ("rows", 41)), pyr="odd"),
    Case("resident", False, 3, 11, 8, 3, 6, 14, kw=(("M", "list"), ("rows", 3)), stride=3.0, pyr="odd"),
    Case("resident", True, 3, 11, 8, 4, 12, 15, kw=(("M", "list+out"),)),             # carry rows 12, 13, 14, 0
    Case("resident", True, 3, 11, 16, 8, 24, 27, kw=(("M", "list"),)),                # carry rows 24, 25, 26, 0 .. 4
    Case("resident", True, 3, 11, 8, 4, 4, 8, kw=(("M", "list"),)),                   # R == S
    Case("resident", True, 3, 11, 8, 3, 9, 13, kw=(("M", "list"),), stride=3.0, pyr="odd"),  # carry rows 9 .. 12, 0
    Case("resident", False, 1, 1, 8, 4, 4, 12, kw=(("M", "one"), ("rows", 4))), Case("resident", True, 1, 4, 8, 4, 8, 9, kw=(("M", "all"),), pyr="ones"),
    Case("resident", False, 3, 11, 8, 4, 12, 20, kw=(("M", "list"), ("rows", 5), ("frames", "outside"))),
    Case("resident", True, 3, 11, 8, 4, 12, 15, kw=(("M", "list"), ("frames", "outside"))),
]


def _emit(ring, G, N, N_out, R, f0, f1, scale=(1.0, 1.0), absent=(), first=True):
    return Case("emit", ring, G, N, R=R, kw=(("No", N_out), ("f0", f0), ("f1", f1), ("scale", scale), ("absent", absent), ("first", first)))


EMIT = [
    _emit(False, 1, 1, 1, 8, 0, 8), _emit(False, 3, 63, 62, 12, 2, 9, (1.5, 0.75)), _emit(True, 1, 64, 64, 13, 20, 33, (1.3, 0.7)),
    _emit(True, 3, 65, 1, 13, 24, 29), _emit(True, 1, 255, 254, 9, 9, 18, (1.3, 0.7)), _emit(False, 3, 256, 256, 16, 8, 16),
    _emit(True, 1, 257, 257, 8, 3, 4), _emit(False, 1, 513, 257, 16, 0, 16, (1.5, 0.75)), _emit(True, 3, 513, 256, 13, 11, 15),
    _emit(True, 1, 513, 513, 13, 24, 29, (1.3, 0.7)), _emit(False, 1, 513, 512, 8, 4, 8),
    _emit(True, 3, 65, 64, 13, 24, 29, absent=("vis_logit",)), _emit(True, 3, 65, 64, 13, 24, 29, absent=("conf_logit",)),
    _emit(True, 3, 65, 64, 13, 24, 29, absent=("visible",), first=False), _emit(True, 3, 65, 64, 13, 24, 29, first=False),
    _emit(True, 3, 65, 64, 13, 24, 29, absent=("vis_logit", "conf_logit", "visible"), first=False),
    _emit(True, 1, 5, 4, 67, LIMIT, 2 ** 30, (1.5, 0.75)),
]


def _health(ring, G, N, N_out, R, f1, look, ind_next, grid, bounds=(-2.0, 94.0, -2.0, 62.0)):
    return Case("health", ring, G, N, R=R, kw=(("No", N_out), ("f1", f1), ("look", look), ("next", ind_next), ("grid", grid), ("bounds", bounds)))


HEALTH = [
    _health(False, 1, 513, 513, 20, 20, 8, 16, (1, 1)), _health(True, 3, 513, 513, 15, 33, 15, 32, (1, 2)),
    _health(False, 1, 4, 1, 20, 20, 8, 16, (64, 64), (0.0, 95.0, 0.0, 63.0)), _health(True, 1, 513, 513, 13, 30, 5, 28, (5, 7), (0.0, 95.0, 0.0, 63.0)),
    _health(False, 3, 300, 257, 32, 20, 1, 16, (8, 12)), _health(True, 3, 65, 1, 9, 18, 9, 16, (2, 3)),
    _health(True, 1, 256, 255, 8, 12, 8, 8, (64, 64)),
]
CASES = {"begin": BEGIN, "commit": COMMIT, "support": SUPPORT, "assign": ASSIGN, "resident": RESIDENT, "emit": EMIT, "health": HEALTH}


# ---- inputs: numpy only (tests/test_stream_reference_host.py builds the same states on the CPU) ---------------------------------------
def rbytes(rng, shape, dtype=np.float32):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return rng.integers(0, 256, n, dtype=np.uint8).view(dtype).reshape(shape).copy()


def finite(rng, shape, scale=30.0):
    return (rng.standard_normal(shape) * scale).astype(f32)


def frame_list(c):
    """The query frames every case cycles through: the edges of the sample range and of the carry-over, fractions, a negative
    frame, an empty slot, and the frames of no window."""
    if c.ind == LIMIT:  # multiples of 64: exact in float32
        return [float(EMPTY_FRAME), float(c.ind + c.S - 64), float(c.ind - 64), 0.0, NAN, 2.0 ** 31, float(c.ind + 3 * c.S)]
    left, right = (0 if c.ind == 0 else c.ind + c.step), c.ind + c.S
    edges = [left - 1, left, right - 1, right, c.ind + c.overlap - 1, c.ind + c.overlap]
    return [float(f) for f in edges] + [-0.5, c.ind + 0.75, -3.0, 0.0, float(EMPTY_FRAME), *NO_WINDOW, -2.0 ** 31]


def position_list(c, sizes):
    """(x, y) in pixels for a level-0 map of sizes[0]."""
    s = c.stride
    xm, ym = (sizes[0][1] - 1) * s, (sizes[0][0] - 1) * s
    return [(33.3, 20.7), (40.0, 24.0), (12.5, 8.5), (0.0, 0.0), (xm, 0.0), (0.0, ym), (xm, ym), (-8 * s, 10.0), (xm + 8 * s, 10.0),
            (10.0, -8 * s), (10.0, ym + 8 * s), (-7.3, -2.0), (NAN, 5.0), (5.0, NAN), (INF, -INF), (-INF, INF), (1e30, -1e30), (NAN, NAN)]


def queries_of(c, rng, sizes=None, hit_first=False):
    """[G*N,3]: frames cycle through frame_list from a case-dependent start, positions are random (or, with a pyramid, cycle through
    position_list over the points that are sampled)."""
    P = c.G * c.N
    frames = frame_list(c)
    if hit_first:  # small P: start on the frames inside the sample range
        frames = frames[1:3] + [f for f in frames if f not in frames[1:3]]
    off = 0 if (hit_first or c.ind == LIMIT) else int(rng.integers(0, len(frames)))
    q = np.empty((P, 3), f32)
    q[:, 0] = [frames[(i + off) % len(frames)] for i in range(P)]
    q[:, 1:] = (rng.random((P, 2)) * np.array([112.0, 80.0]) - 8.0).astype(f32)
    if sizes is not None:
        pos = position_list(c, sizes)
        qf = ref.qframe(q[:, 0])
        left, right = (0 if c.ind == 0 else c.ind + c.step), c.ind + c.S
        hit = np.nonzero((qf >= left) & (qf < right))[0]
        start = int(rng.integers(0, len(pos)))
        for k, i in enumerate(hit):
            q[i, 1:] = pos[(k + start) % len(pos)]
    return q


def history_of(c, rng, rows_finite=()):
    """hist_coords / vis / conf of random bytes, the coordinates of `rows_finite` finite."""
    hc, hv, hf = rbytes(rng, (c.G, c.R, c.N, 2)), rbytes(rng, (c.G, c.R, c.N)), rbytes(rng, (c.G, c.R, c.N))
    for r in rows_finite:
        hc[:, r] = finite(rng, (c.G, c.N, 2))
    return hc, hv, hf


def window_of(c, rng):
    return {"coords": rbytes(rng, (c.G, c.S, c.N, 2)), "vis": rbytes(rng, (c.G, c.S, c.N)), "conf": rbytes(rng, (c.G, c.S, c.N)),
            "mask": rbytes(rng, (c.G * c.N,), np.uint8)}


def pyramid_of(c, rng):
    return [finite(rng, (c.S, H, W, ref.CH), 1.0) for H, W in PYRAMIDS[c.pyr]]


def logits_of(rng, shape, thresh=THRESH):
    """Two logit arrays from LOGITS whose float64 product is NaN or at least MARGIN from thresh (a pair that is not becomes (4, 4))."""
    v, w = (LOGITS[rng.integers(0, len(LOGITS), shape)] for _ in range(2))
    p = ref.visible_product(v, w)
    near = np.abs(p - np.float64(f32(thresh))) < MARGIN  # (NaN: False)
    v[near], w[near] = 4.0, 4.0
    return v, w


def state_begin(c):
    rng = c.rng()
    carry = [ref.row_of(c.ind + t, c.R, c.ring) for t in range(c.overlap)] if c.ind > 0 else []
    hc, hv, hf = history_of(c, rng, carry)
    return {"queries": queries_of(c, rng).reshape(-1), "hc": hc, "hv": hv, "hf": hf, **window_of(c, rng)}


def want_begin(c, st, ring=None):
    ring = c.ring if ring is None else ring
    coords, vis, conf, mask = ref.begin(ring, c.G, c.N, c.S, c.step, c.ind, c.R, c.stride, st["queries"], st["hc"], st["hv"], st["hf"])
    return {**st, "coords": coords, "vis": vis, "conf": conf, "mask": mask}


def state_commit(c, plant=None, flag=0):
    """plant: (name, (g, t, n[, k]), value) written into the window after the finite fill."""
    rng = c.rng()
    hc, hv, hf = history_of(c, rng)
    st = {"hc": hc, "hv": hv, "hf": hf, "coords": finite(rng, (c.G, c.S, c.N, 2), 9.0), "vis": finite(rng, (c.G, c.S, c.N), 9.0),
          "conf": finite(rng, (c.G, c.S, c.N), 9.0), "flag": np.array([flag], np.int32)}
    if plant is None and c.T_valid < c.S:  # a non-finite value beyond the chunk: not committed, not flagged
        st["vis"][c.G - 1, c.T_valid, c.N - 1] = INF
        st["coords"][0, c.S - 1, 0, 1] = NAN
    if plant is not None:
        name, idx, value = plant
        st[name][idx] = value
    return st


def want_commit(c, st, ring=None, null_flag=False):
    ring = c.ring if ring is None else ring
    hc, hv, hf, flag = ref.commit(ring, c.G, c.N, c.S, c.ind, c.T_valid, c.R, c.stride, st["coords"], st["vis"], st["conf"], st["hc"],
                                  st["hv"], st["hf"], None if null_flag else int(st["flag"][0]))
    return {**st, "hc": hc, "hv": hv, "hf": hf, "flag": st["flag"] if null_flag else np.array([flag], np.int32)}


def flag_plants(c, places):
    """(label, plant) for every place x every one of x, y, vis, conf; the value goes round NaN, +inf, -inf."""
    out = []
    for i, (label, thread) in enumerate(places.items()):
        if c.ring:
            g, t, n = c.G - 1, c.T_valid - 1, thread
        else:
            g, rem = divmod(thread, c.T_valid * c.N)
            t, n = divmod(rem, c.N)
        for j, (name, idx) in enumerate((("coords", (g, t, n, 0)), ("coords", (g, t, n, 1)), ("vis", (g, t, n)), ("conf", (g, t, n)))):
            value = (NAN, INF, -INF)[(4 * i + j) % 3]
            out.append((f"{label}-{'xyvc'[j]}-{value}", (name, idx, value)))
    return out


def state_support(c):
    rng = c.rng()
    sizes = PYRAMIDS[c.pyr]
    q = queries_of(c, rng, sizes, hit_first=c.G * c.N <= 4)
    qf = ref.qframe(q[:, 0])
    left, right = (0 if c.ind == 0 else c.ind + c.step), c.ind + c.S
    hit = (qf >= left) & (qf < right)
    st = {"queries": q.reshape(-1)}
    for l, fm in enumerate(pyramid_of(c, rng)):
        st[f"fm{l}"] = fm
        acc = rbytes(rng, (c.G * c.N, ref.TAPS, ref.CH))
        acc[hit] = finite(rng, (int(hit.sum()), ref.TAPS, ref.CH), 1.0)  # added to: finite
        st[f"acc{l}"] = acc
    return st


def want_support(c, st, ring=None):
    acc = ref.support(c.ring, c.G, c.N, c.S, c.step, c.ind, c.stride, st["queries"], [st[f"fm{l}"] for l in range(LEVELS)],
                      [st[f"acc{l}"] for l in range(LEVELS)])
    return {**st, **{f"acc{l}": acc[l] for l in range(LEVELS)}}


def slots_of(c, rng):
    P, kind = c.G * c.N, c.get("M")
    if kind == "one":
        return np.array([P - 1], np.int32)
    if kind == "all":
        return rng.permutation(P).astype(np.int32)
    ends = list(dict.fromkeys([g * c.N + c.N - 1 for g in reversed(range(c.G))] + [g * c.N for g in range(c.G)]))
    want = min(P, 20) - (3 if kind == "list+out" else 0)
    rest = [s for s in rng.permutation(P).tolist() if s not in ends]
    slots = ends + rest[:max(0, want - len(ends))]
    slots = [slots[i] for i in rng.permutation(len(slots))]
    if kind == "list+out":  # indices outside [0, G*N): nothing is written for them
        slots += [-1, P, BIG]
    return np.array(slots, np.int32)


def resident_kinds(c):
    ind, ov, s = c.ind, c.overlap, c.stride
    xm, ym = (PYRAMIDS[c.pyr][0][1] - 1) * s, (PYRAMIDS[c.pyr][0][0] - 1) * s
    if c.get("frames") == "outside":
        rows = [[ind + ov, 50.0, 30.0], [ind + ov + 9.0, 10.0, 10.0], [float(EMPTY_FRAME), 0.0, 0.0], [ind - c.step - 1.0, 20.0, 20.0],
                [ind - c.step - 0.5 - 1.0, 3.0, 4.0]]
        return rows + [[f, 7.0, 9.0] for f in NO_WINDOW]
    return [[ind - c.step, 33.3, 20.7],        # the pyramid's first frame, interior
            [ind - 1.0, 40.0, 24.0],           # integer position
            [float(ind), 12.5, 8.5],           # half-integer
            [ind + ov - 1.0, xm, ym],          # the pyramid's last frame, on the far corner
            [ind + 0.5, -7.3, -2.0],           # a fractional frame (truncated), outside on the low side
            [ind - c.step + 0.75, xm + 8 * s, ym + 8.5],  # outside on the high side
            [float(ind + ov), 50.0, 30.0],     # the first frame that is not resident: the plain assign
            [ind + ov + 9.0, 10.0, 10.0],      # further ahead
            [float(EMPTY_FRAME), 0.0, 0.0],    # an empty slot
            *[[f, 7.0 + k, 9.0] for k, f in enumerate(NO_WINDOW)],  # no window: the plain assign
            [ind - 0.5, NAN, INF], [ind + 0.0, -INF, 1e30]]          # resident at positions the sampler clamps


def state_assign(c):
    rng = c.rng()
    hc, hv, hf = history_of(c, rng)
    slots = slots_of(c, rng)
    st = {"queries": rbytes(rng, (c.G * c.N * 3,)), "hc": hc, "hv": hv, "hf": hf, "slots": slots}
    for l in range(LEVELS):
        st[f"acc{l}"] = rbytes(rng, (c.G * c.N, ref.TAPS, ref.CH))
    if c.kernel == "assign":
        st["newq"] = rbytes(rng, (len(slots) * 3,))  # copied only
    else:
        kinds = resident_kinds(c)
        st["newq"] = np.array([kinds[m % len(kinds)] for m in range(len(slots))], f32).reshape(-1)
        for l, fm in enumerate(pyramid_of(c, rng)):
            st[f"fm{l}"] = fm
    return st


def want_assign(c, st, ring=None, plain=False):
    ring = c.ring if ring is None else ring
    acc = [st[f"acc{l}"] for l in range(LEVELS)]
    rows = c.get("rows", 0)
    if c.kernel == "assign" or plain:
        out = ref.assign(ring, c.G, c.N, c.R, rows, st["slots"], st["newq"], st["queries"], acc, st["hc"], st["hv"], st["hf"])
    else:
        out = ref.assign_resident(ring, c.G, c.N, c.S, c.step, c.ind, c.R, rows, c.stride, [st[f"fm{l}"] for l in range(LEVELS)],
                                  st["slots"], st["newq"], st["queries"], acc, st["hc"], st["hv"], st["hf"])
    q, acc, hc, hv, hf = out
    return {**st, "queries": q, "hc": hc, "hv": hv, "hf": hf, **{f"acc{l}": acc[l] for l in range(LEVELS)}}


def first_rows_of(c, rng, f1, ind_next):
    vals = np.array([0, 0, 0, max(f1 - 6, 0), max(f1 - 2, 0), max(ind_next - 1, 0), ind_next, ind_next + 4, BIG], np.int64)
    return vals[rng.integers(0, len(vals), (c.G, c.N))].astype(np.int32)


def state_emit(c):
    rng = c.rng()
    No, F = c.get("No"), c.get("f1") - c.get("f0")
    v, w = logits_of(rng, (c.G, c.R, c.N))
    st = {"hc": finite(rng, (c.G, c.R, c.N, 2)), "hv": v, "hf": w, "tracks": rbytes(rng, (c.G, F, No, 2))}
    for name, dtype in (("vis_logit", np.float32), ("conf_logit", np.float32), ("visible", np.uint8)):
        st[name] = rbytes(rng, (c.G, F, No), dtype)  # an absent output is allocated all the same: it must keep its bytes
    st["first_row"] = first_rows_of(c, rng, c.get("f1"), c.get("f1"))
    return st


def want_emit(c, st):
    sx, sy = c.get("scale")
    first = st["first_row"] if c.get("first") else None
    tracks, v, w, on, p = ref.emit(c.ring, c.G, c.N, c.get("No"), c.R, c.get("f0"), c.get("f1"), sx, sy, THRESH, st["hc"], st["hv"], st["hf"], first)
    out = {**st, "tracks": tracks}
    for name, val in (("vis_logit", v), ("conf_logit", w), ("visible", on)):
        if name not in c.get("absent"):
            out[name] = val
    return out, p


def state_health(c):
    rng = c.rng()
    No, f1, nxt, (gh, gw) = c.get("No"), c.get("f1"), c.get("next"), c.get("grid")
    x_lo, x_hi, y_lo, y_hi = c.get("bounds")
    v, w = logits_of(rng, (c.G, c.R, c.N))
    hc = (rng.random((c.G, c.R, c.N, 2)) * np.array([x_hi - x_lo + 20.0, y_hi - y_lo + 20.0]) + np.array([x_lo - 10.0, y_lo - 10.0])).astype(f32)
    hc[rng.random((c.G, c.R, c.N)) < 0.02] = NAN
    hc[rng.random((c.G, c.R, c.N)) < 0.02] = (x_hi, y_lo)  # on a border: inside
    frames = [0.0, 0.0, 0.0, 3.5, -0.5, f1 - 5.0, f1 - 1.0, f1 - 0.5, float(f1), f1 + 7.0, float(EMPTY_FRAME), *NO_WINDOW, -2.0 ** 31]
    q = np.empty((c.G * c.N, 3), f32)
    q[:, 0] = np.array(frames, f32)[rng.integers(0, len(frames), c.G * c.N)]
    q[:, 1:] = (rng.random((c.G * c.N, 2)) * np.array([x_hi - x_lo + 20.0, y_hi - y_lo + 20.0]) + np.array([x_lo - 10.0, y_lo - 10.0])).astype(f32)
    return {"queries": q.reshape(-1), "hc": hc, "hv": v, "hf": w, "first_row": first_rows_of(c, rng, f1, nxt),
            "lost": rbytes(rng, (c.G, No), np.int32), "cell": rbytes(rng, (c.G, No), np.int32), "cover": rbytes(rng, (c.G, gh * gw), np.int32)}


def want_health(c, st):
    lost, cell, cover, p = ref.health(c.ring, c.G, c.N, c.get("No"), c.R, c.get("f1"), c.get("look"), c.get("next"), THRESH, c.get("bounds"),
                                      c.get("grid"), st["queries"], st["hc"], st["hv"], st["hf"], st["first_row"])
    return {**st, "lost": lost, "cell": cell, "cover": cover}, p


# ---- the device side -----------------------------------------------------------------------------------------------------------------
def _words(a):
    """An array as int32 words, its bytes padded to a multiple of four with 0xA5."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    tail = (-len(raw)) % 4
    return np.concatenate([raw, np.full(tail, 0xA5, np.uint8)]).view(np.int32)


class Device:
    """Every array of a state as a view into its own NaN-framed allocation."""

    def __init__(self, st):
        import torch
        from ctk_support import NAN_PATTERN, nan_framed
        self.bufs = {}
        for name, a in st.items():
            x = torch.from_numpy(_words(a).view(np.float32))
            self.bufs[name] = nan_framed(x, pad=PAD, pattern=NAN_PATTERN, whole=True)

    def ptr(self, name):
        return self.bufs[name][0].data_ptr()

    def check(self, want, tag):
        """Every buffer equals `want`, bit for bit, and every frame is intact."""
        import torch
        from ctk_support import frame_intact
        torch.cuda.synchronize()
        assert set(want) == set(self.bufs)
        for name, (view, flat) in self.bufs.items():
            assert frame_intact(flat, view), (tag, name, "a store outside the buffer")
            got, exp = view.view(torch.int32).cpu().numpy(), _words(want[name])
            if not np.array_equal(got, exp):
                bad = np.nonzero(got != exp)[0]
                raise AssertionError(f"{tag}: {name}: {len(bad)} of {len(exp)} words differ, first at {bad[:6].tolist()}: "
                                     f"got {got[bad[:6]].tolist()}, want {exp[bad[:6]].tolist()}")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def stream_args(c, d, ring):
    import ctk_support
    a = ctk_support.abi_structs()["ctk_stream_args"]()
    a.G, a.N, a.S, a.step, a.ind, a.T_valid, a.T_cap, a.stride = c.G, c.N, c.S, c.step, c.ind, c.T_valid or c.S, c.R, c.stride
    for field, name in (("queries", "queries"), ("hist_coords", "hc"), ("hist_vis", "hv"), ("hist_conf", "hf"), ("coords", "coords"),
                        ("vis", "vis"), ("conf", "conf"), ("point_mask", "mask"), ("nonfinite", "flag")):
        if name in d.bufs:
            setattr(a, field, d.ptr(name))
    for l, (H, W) in enumerate(PYRAMIDS[c.pyr]):
        a.H[l], a.W[l] = H, W
        if f"fm{l}" in d.bufs:
            a.fmaps[l] = d.ptr(f"fm{l}")
        if f"acc{l}" in d.bufs:
            a.support[l] = d.ptr(f"acc{l}")
    return a


def call(name, ring, *args):
    from cotracker_amd import _lib as L
    rc = getattr(L.load(), name + ("_ring" if ring else ""))(*args, _stream())
    assert rc == 0, (name, ring, rc)


def forms(c):
    """The case's own form and, for a linear case, the ring entry point on the same buffers: R = T_cap >= ind + S addresses the
    very rows the linear form addresses."""
    return [c.ring] if c.ring else [False, True]


def ids(cases):
    return [c.id for c in cases]


# ---- begin ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", BEGIN, ids=ids(BEGIN))
def test_begin(lib, c):
    st = state_begin(c)
    want = want_begin(c, st)
    q = st["queries"].reshape(c.G * c.N, 3)
    none = ~((q[:, 0] >= f32(-2.0 ** 31)) & (q[:, 0] < f32(2.0 ** 31)))
    gone = np.isin(q[:, 0], np.array(NO_WINDOW, f32)) | np.isnan(q[:, 0])
    assert np.array_equal(none, gone)
    # a frame of no window: mask 0 and the query position at every t, zero logits
    assert not want["mask"][none].any()
    fresh = (q[none, 1:] * ref.inv_stride(c.stride)).astype(f32)
    cw = want["coords"].reshape(c.G, c.S, c.N, 2).transpose(0, 2, 1, 3).reshape(c.G * c.N, c.S, 2)[none]
    assert np.array_equal(cw.view(np.int32), np.repeat(fresh[:, None], c.S, 1).view(np.int32))
    if c.ind == LIMIT:
        assert want["mask"].tolist()[:3] == [0, 1, 1] and q[0, 0] == c.ind + c.S
    for ring in forms(c):
        assert all(np.array_equal(_words(a), _words(b)) for a, b in zip(want_begin(c, st, ring).values(), want.values()))
        d = Device(st)
        a = stream_args(c, d, ring)
        call("ctk_stream_begin", ring, C.byref(a))
        d.check(want, (c.id, ring))


# ---- commit -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", COMMIT, ids=ids(COMMIT))
def test_commit(lib, c):
    st = state_commit(c)
    want = want_commit(c, st)
    assert int(want["flag"][0]) == 0  # the non-finite values beyond T_valid do not flag
    for ring in forms(c):
        d = Device(st)
        call("ctk_stream_commit", ring, C.byref(stream_args(c, d, ring)))
        d.check(want, (c.id, ring))


FLAG_RUNS = [(c, label, plant) for c, places in FLAG for label, plant in flag_plants(c, places)]


@pytest.mark.parametrize("k", range(len(FLAG)), ids=[c.id for c, _ in FLAG])
def test_commit_flag(lib, k):
    """One non-finite value per call: the flag word goes from 6 to 7, whichever lane, wave and block holds the value."""
    c, places = FLAG[k]
    for label, plant in flag_plants(c, places):
        st = state_commit(c, plant, flag=6)
        want = want_commit(c, st)
        assert int(want["flag"][0]) == 7, label
        d = Device(st)
        call("ctk_stream_commit", c.ring, C.byref(stream_args(c, d, c.ring)))
        d.check(want, (c.id, label))
    # clean: 6 stays 6; a NULL flag: the word keeps its bytes although a value is not finite
    st = state_commit(c, None, flag=6)
    d = Device(st)
    call("ctk_stream_commit", c.ring, C.byref(stream_args(c, d, c.ring)))
    d.check(want_commit(c, st), (c.id, "clean"))
    st = state_commit(c, plant, flag=6)
    d = Device(st)
    a = stream_args(c, d, c.ring)
    a.nonfinite = None
    call("ctk_stream_commit", c.ring, C.byref(a))
    d.check(want_commit(c, st, null_flag=True), (c.id, "null flag"))


# ---- support ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SUPPORT, ids=ids(SUPPORT))
def test_support(lib, c):
    st = state_support(c)
    want = want_support(c, st)
    for ring in ([True] if c.ring else [False, True]):  # (the ring form's capacity rule R >= S holds for every T_cap >= ind + S)
        d = Device(st)
        call("ctk_stream_support", ring, C.byref(stream_args(c, d, ring)))
        d.check(want, (c.id, ring))


# ---- assign and resident assign -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ASSIGN, ids=ids(ASSIGN))
def test_assign(lib, c):
    st = state_assign(c)
    want = want_assign(c, st)
    M = len(st["slots"])
    d = Device(st)
    a = stream_args(c, d, c.ring)
    if c.ring:
        call("ctk_stream_assign", True, C.byref(a), d.ptr("slots"), d.ptr("newq"), M)
    else:
        call("ctk_stream_assign", False, C.byref(a), d.ptr("slots"), d.ptr("newq"), M, c.get("rows"))
    d.check(want, c.id)
    if not c.ring and c.get("rows") == c.R:  # every row cleared: what the ring form does with R = T_cap
        d = Device(st)
        call("ctk_stream_assign", True, C.byref(stream_args(c, d, True)), d.ptr("slots"), d.ptr("newq"), M)
        d.check(want, (c.id, "ring"))


@pytest.mark.parametrize("c", RESIDENT, ids=ids(RESIDENT))
def test_assign_resident(lib, c):
    st = state_assign(c)
    want = want_assign(c, st)
    M = len(st["slots"])
    newq = st["newq"].reshape(M, 3)
    qf = ref.qframe(newq[:, 0])
    resident = (qf >= c.ind - c.step) & (qf < c.ind + c.overlap)
    listed = (st["slots"] >= 0) & (st["slots"] < c.G * c.N)
    if c.get("frames") == "outside":  # no frame inside the pyramid: exactly ctk_stream_assign
        assert not resident.any()
        plain = want_assign(c, st, plain=True)
        assert all(np.array_equal(_words(plain[k]), _words(want[k])) for k in want)
    d = Device(st)
    a = stream_args(c, d, c.ring)
    if c.ring:
        call("ctk_stream_assign_resident", True, C.byref(a), d.ptr("slots"), d.ptr("newq"), M)
    else:
        call("ctk_stream_assign_resident", False, C.byref(a), d.ptr("slots"), d.ptr("newq"), M, c.get("rows"))
    d.check(want, c.id)
    # the unmodified begin starts a resident slot as it starts a fresh point: x / stride at every t, zero logits, mask 1
    rng = c.rng(1)
    st2 = {k: want[k] for k in ("queries", "hc", "hv", "hf")}
    st2.update(window_of(c, rng))
    d = Device(st2)
    call("ctk_stream_begin", c.ring, C.byref(stream_args(c, d, c.ring)))
    import torch
    torch.cuda.synchronize()
    got = {k: d.bufs[k][0].view(torch.int32).cpu().numpy() for k in ("coords", "vis", "conf", "mask")}
    coords = got["coords"].view(np.float32).reshape(c.G, c.S, c.N, 2)
    vis, conf = (got[k].reshape(c.G, c.S, c.N) for k in ("vis", "conf"))
    mask = got["mask"].view(np.uint8)[:c.G * c.N]
    for m in np.nonzero(resident & listed)[0]:
        g, n = divmod(int(st["slots"][m]), c.N)
        fresh = (newq[m, 1:] * ref.inv_stride(c.stride)).astype(f32)
        assert np.array_equal(coords[g, :, n].view(np.int32), np.repeat(fresh[None], c.S, 0).view(np.int32)), (c.id, m)
        assert not vis[g, :, n].any() and not conf[g, :, n].any() and mask[g * c.N + n] == 1, (c.id, m)
    if c.get("frames") != "outside":
        assert resident.sum() >= 1


# ---- emit and health ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", EMIT, ids=ids(EMIT))
def test_emit(lib, c):
    from cotracker_amd import _lib as L
    st = state_emit(c)
    want, _ = want_emit(c, st)
    d = Device(st)
    a = L.StreamEmit.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.f1, a.thresh, a.reserved = c.G, c.N, c.get("No"), c.R, c.get("f0"), c.get("f1"), THRESH, 0
    a.sx, a.sy = c.get("scale")
    a.hist_coords, a.hist_vis, a.hist_conf, a.tracks = d.ptr("hc"), d.ptr("hv"), d.ptr("hf"), d.ptr("tracks")
    a.first_row = d.ptr("first_row") if c.get("first") else None
    for name in ("vis_logit", "conf_logit", "visible"):
        setattr(a, name, None if name in c.get("absent") else d.ptr(name))
    call("ctk_stream_emit", False, C.byref(a))
    d.check(want, c.id)


@pytest.mark.parametrize("c", HEALTH, ids=ids(HEALTH))
def test_health(lib, c):
    from cotracker_amd import _lib as L
    st = state_health(c)
    want, _ = want_health(c, st)
    d = Device(st)
    a = L.StreamHealth.Args()
    a.G, a.N, a.N_out, a.R, a.f1, a.look, a.ind_next = c.G, c.N, c.get("No"), c.R, c.get("f1"), c.get("look"), c.get("next")
    a.thresh, a.reserved = THRESH, 0
    a.gh, a.gw = c.get("grid")
    a.x_lo, a.x_hi, a.y_lo, a.y_hi = c.get("bounds")
    a.inv_cw = float(f32(a.gw) / f32(f32(a.x_hi) - f32(a.x_lo)))
    a.inv_ch = float(f32(a.gh) / f32(f32(a.y_hi) - f32(a.y_lo)))
    a.queries, a.hist_coords, a.hist_vis, a.hist_conf, a.first_row = (d.ptr(k) for k in ("queries", "hc", "hv", "hf", "first_row"))
    a.lost, a.cell, a.cover = d.ptr("lost"), d.ptr("cell"), d.ptr("cover")
    call("ctk_stream_health", False, C.byref(a))
    d.check(want, c.id)
    # a frame of no window is a pending slot (lost 0) unless first_row says empty
    q = st["queries"].reshape(c.G, c.N, 3)[:, :c.get("No")]
    none = (np.isnan(q[..., 0]) | np.isin(q[..., 0], np.array(NO_WINDOW, f32))) & (st["first_row"][:, :c.get("No")] != BIG)
    assert (want["lost"][none] == 0).all()
