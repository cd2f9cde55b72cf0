"""ctk_conv2d_sh, the whole contract: both kernels x channel groups x K-tile counts x column cuts x geometry, canaries (-m gpu).

One entry point fans out to conv_pp128_kernel<32> and conv3x3_halo_kernel<32, true / false> (csrc/conv_pp.hip).  This module drives
it through `ctk_support.conv_raw` (every argument of ctk_conv2d_sh in caller-owned memory; weights repacked as encoder_hip._Conv
does: W'[n_pad][(ky*KW + kx)*Cin + c], rows >= n_out zero, bias n_pad floats) and checks

  1. WHICH KERNEL RAN.  Every launch is wrapped in the profile recorder; the one recorder row must be `route(c)`, a restatement of
     the dispatcher's rule (halo kernel iff 3 x 3 / stride 1 / pad 1 / H % 8 == 0 / W % 32 == 0), AND carry the prefix of the kernel
     the case names: a threshold moved in the dispatcher fails the named case instead of turning it into a test of the other kernel.
  2. EXACT INTEGERS.  Activations and weights integer-valued in [-4, 4] (one |w| = 4: asserted), bias in [-64, 64].  The integers
     are their own f16 `hi` with `lo` = 0 (asserted on the SH tensor); ctk_pack_weight scales W by 2^11 (asserted on the blob's
     header; test_gpu_gemm_matrix.py item 2 has the derivation), so every product is a multiple of 2^11 and every partial sum is
     bounded by 16 * K * 2^11 -- at the largest K here, 9 * 416 = 3744, 16 * 3744 = 59904 and 59904 * 2^11 < 2^27 (asserted per
     case): f32 accumulation is exact in ANY K-tile order, which is why the halo kernel (channel group outer) and conv_pp128_kernel
     (tap outer) must hit the same integers; the epilogue's * 2^-11 and + bias (|out| <= 59904 + 64 < 2^24) are exact too.  The
     reference is torch.nn.functional.conv2d in float64 on the CPU, where these integers and their sums are exact (it IS the int64
     product), and the assertion is torch.equal: no tolerance.  A dropped, repeated or misplaced K-tile, tap, row or column block
     cannot hide.  Every case is launched twice (same bits) and, with F > 1, once more on frame 0 alone (the bits it has in the batch).
  3. ADDRESSING, on every case of 2.  The output lies inside an allocation pre-filled with the NaN pattern 0x7FC17FC1, GUARD rows
     in front and behind: bit-unchanged outside [M][n_out], no NaN inside.  The SH input lies in the middle of an allocation of the
     same pattern (two f16 NaNs per word; the guard holds more than KH + pad + 2 image rows): a tap that leaves the tensor turns an
     exact integer into NaN.  `zeros` is exactly 128 zero bytes and the bias exactly n_pad floats inside NaN; the weight blob is
     packed into the middle of a 0xFF-filled buffer (f16 NaNs again).
  4. fp64 on randn operands (weights / sqrt(K), bias 0.1 randn, as test_conv2d_sh_vs_fp64 builds them): one shape per kernel
     instantiation and K class, K = 32 ... 3744, bound 4e-6 * max(1, max|ref|) -- the bound the project asserts for this operator.
     For K > 1440 (beyond what test_conv2d_sh_vs_fp64 covers) the error of torch's float32 CPU conv2d against the same reference is
     recorded next to the kernel's.  The halo kernel and conv_pp128_kernel are not bit-identical on real values (K-tile order) and
     are not compared with each other.

The persistent-loop cases (more tiles than CUs, a partial second round: `tiles` asserted against the device's CU count in the test)
run on integers like every other case: the second round of a workgroup reuses the LDS its first tile's epilogue has just read.  Two
`load` cases add deep K to that (two channel groups / 18 K-tiles per tile on every CU at once).

Entry-point argument rules, and the range of the row origin that conv_pp128_kernel packs into 15 + 16 bits (the entry point took
pad > 16384 and (Hout-1)*stride - pad > 16383, e.g. Hin = 16000 / 3 x 3 / pad 400, and the kernel then gathered other rows; it
returns CTK_E_SHAPE now): tests/test_cabi_and_host.py, on the CPU.  No GPU case relies on the rejection.

Observed on an MI355X with 256 CUs: all 55 integer cases exact on both kernels, every canary intact, no shape had to be routed
away; the matrix found no fault in conv_pp.hip or pp_common.h.  Persistent-loop tiles: halo 280 and 320, conv_pp128 320 and 272.
Largest fp64 error per kernel and K (bound 4e-6 * max(1, max|ref|) = 1.1e-5 ... 2.5e-5, max|ref| 2.8 ... 6.2;
profiles/conv_matrix_errors.json has every case): halo N64 1.8e-6 (K = 288), 3.5e-6 (864); halo 128-column 2.4e-6 (576), 6.2e-6
(2304), 6.4e-6 (3744); conv_pp128 5.9e-7 / 9.5e-7 (32), 8.1e-7 (64), 3.1e-6 (1152), 2.3e-6 (1568), 4.9e-6 (2304), 5.5e-6 (3744).
No case at K > 1440 needed more than the project's bound (torch's float32 CPU conv2d on the same operands: 1.1e-6 ... 2.1e-6).
The 67 tests take 1.0 ... 1.4 s behind the first one's set-up (3.1 ... 3.7 s for the pytest process).

Planted faults (scratch copies of the library, one line each, run against the 65 tests without the two `load` cases;
profiles/conv_matrix_errors.json lists the failing cases).  Caught, each by an exact mismatch or a canary: the halo double
buffer's parity ((cg + 1) & 1 -> cg & 1: every halo case with cl > 1, 13 integer and 4 real), a tap shifted by one column in
conv_pp128 (every case with KH >= 3: 20 integer, 4 real), one column block too many in pp_epilogue (>= -> >: every n_out that is
not a multiple of 128, on both kernels, 36 integer and 7 real; the first report is "a store behind row M - 1"), the halo
kernel's weight wait one K-tile short (base = D * NB: 4 integer cases and 1 real, all on the N64 template at n_out = 64).
NOT caught: conv_pp128's phase-1 wait relaxed from vmcnt(6) to (12), the halo kernel's stricter wait at tap 8 removed, the barrier
at tile end removed (either kernel) -- at these sizes, the loaded cases included, the requests have landed long before the relaxed
wait and no wave runs an epilogue ahead, so the race never opens; tools/check_pp_schedule.py proves conv_pp128's counts
statically.  Dropping the `cg + 1 < cl` guard of the A prefetch only reads a resident buffer into registers nobody uses: same
output, nothing to catch.
"""
import dataclasses
import json
import os
import time

import pytest
import torch

from ctk_support import conv_raw, dev, recorded, same_bits

pytestmark = pytest.mark.gpu

CANARY = 0x7FC17FC1  # NaN as one f32 and as two f16
GUARD = 320          # output guard rows on either side: more than one 256-row tile
FRAME = 4096         # bytes / elements of NaN or 0xFF on either side of the small operands


@dataclasses.dataclass(frozen=True)
class Case:
    kernel: str   # the kernel the case names: "halo" or "pp128"
    edge: str
    F: int        # F = 0 or H = 0: sized from the device's CU count (persistent-loop cases)
    H: int
    W: int
    Cin: int
    n_out: int
    KH: int = 3
    KW: int = 3
    stride: int = 1
    pad: int = 1

    @property
    def id(self):
        return f"{self.kernel}-{self.edge}-{self.F}x{self.H}x{self.W}-c{self.Cin}-n{self.n_out}-k{self.KH}x{self.KW}s{self.stride}p{self.pad}"

    @property
    def K(self):
        return self.KH * self.KW * self.Cin

    @property
    def n_pad(self):
        return (self.n_out + 127) // 128 * 128

    @property
    def out_hw(self):
        return (self.H + 2 * self.pad - self.KH) // self.stride + 1, (self.W + 2 * self.pad - self.KW) // self.stride + 1

    @property
    def M(self):
        return self.F * self.out_hw[0] * self.out_hw[1]


def halo(edge, F, H, W, Cin, n_out):
    return Case("halo", edge, F, H, W, Cin, n_out)


def pp(edge, F, H, W, Cin, n_out, k=(3, 3, 1, 1)):
    return Case("pp128", edge, F, H, W, Cin, n_out, *k)


K1, K1S2, K3S2, K3 = (1, 1, 1, 0), (1, 1, 2, 0), (3, 3, 2, 1), (3, 3, 1, 1)
CASES = (
    # ---- conv3x3_halo_kernel: 3 x 3 / stride 1 / pad 1 on tile-aligned maps
    # channel groups cl = 1 (no `cg + 1 < cl` branch taken, KT = 9 against the N64 ring's look-ahead of 7), 2, 3 (odd: the double
    # buffer ends on buffer 0), 13 (conv2); n_out = 64: the N64 template (ring of 8), 128: ring of 4
    [halo("groups", 1, 8, 32, cin, n) for cin in (32, 64, 96) for n in (64, 128)] + [halo("groups", 1, 8, 32, 416, 256)] +
    # column cut: one 32-column block on the N64 template ... a second column block with 32 valid columns ... two full blocks
    [halo("columns", 2, 16, 64, 64, n) for n in (32, 64, 96, 128, 160, 256)] +
    # geometry: ((1, 8, 32), one tile touching all four borders, is every `groups` case); three tiles in one tile row; three tile
    # rows and the frame stride; ((2, 16, 64) is every `columns` case)
    [halo("geometry", 1, 8, 96, 96, 96), halo("geometry", 3, 24, 32, 64, 64)] +
    # persistent loop: cus < tiles < 2 cus, tiles % cus != 0; with n_out = 160 two column blocks interleave in the tile index
    [halo("loop", 0, 64, 160, 32, 64), halo("loop", 0, 64, 160, 32, 160)] +
    # the same round and a bit under load: every CU streams halos and weights at once, two channel groups (N64 template)
    [halo("load", 0, 64, 160, 64, 32)] +
    # ---- conv_pp128_kernel
    # ring depth: KT = 1, 2, 3, 4 on the ring of 3 (the prologue requests K-tiles 0 and 1, the loop kt + 2: clamped duplicates);
    # the stem's class (160 -> 64) and conv3 (256 -> 128, cl = 8)
    [pp("ring", 2, 9, 31, cin, 128, K1) for cin in (32, 64, 96, 128)] + [pp("ring", 2, 9, 31, 160, 64, K1), pp("ring", 2, 9, 31, 256, 128, K1)] +
    # encoder classes no operator test ran: the 1 x 1 stride-2 downsample, stride 2 on odd maps, 3 x 3 / s1 / p1 off the halo tiling
    [pp("class", 2, 16, 64, 64, 96, K1S2), pp("class", 2, 15, 21, 64, 96, K1S2)] +
    [pp("class", 2, h, w, cin, n, K3S2) for (cin, n) in ((64, 96), (128, 128)) for (h, w) in ((16, 64), (15, 21))] +
    [pp("class", 2, 12, 40, 64, 64, K3), pp("class", 2, 8, 24, 96, 96, K3), pp("class", 2, 7, 9, 128, 128, K3)] +
    # ragged M: the min(r, M - 1) row clamp and the epilogue's row guard.  M = 1 (eight of nine taps are padding), 63, 255, 257, 511
    [pp("ragged", 1, 1, 1, 64, 64, K3), pp("ragged", 1, 7, 9, 64, 96, K1)] + [pp("ragged", 1, 1, w, 64, 64, K1) for w in (255, 257, 511)] +
    # column cut: 32; 64 (`ph1` skipped); 96; 128; 160 (`ph1` differs between the two column blocks); 256; 384 (three blocks)
    [pp("columns", 3, 15, 21, 64, n, K3S2) for n in (32, 64, 96, 128, 160, 256, 384)] +
    # promised by include/ctk.h, used by nobody: nn.Conv2d(Cin, n_out, (KH, KW), stride, padding=pad) in general
    [pp("general", 2, 11, 13, 32, 32, k) for k in ((1, 3, 1, 1), (3, 1, 1, 0), (5, 5, 1, 2), (7, 7, 2, 3), (3, 3, 1, 0), (3, 3, 3, 1),
                                                   (2, 2, 2, 0), (3, 3, 1, 2))] +
    # persistent loop: ceil(M / 256) * (n_pad / 128) between cus and 2 cus (H sized from the CU count, W = 251)
    [pp("loop", 1, 0, 251, 32, 160, K1)] +
    # ... and 18 K-tiles per tile on every CU at once: the ring's steady state with the memory system busy
    [pp("load", 0, 128, 128, 64, 32, K3S2)]
)

# fp64 on real values: one shape per kernel instantiation and K class
REAL = [
    halo("n64", 1, 8, 32, 32, 64),         # K = 288
    halo("n64", 2, 16, 64, 96, 64),        # K = 864
    halo("n128", 2, 16, 64, 64, 160),      # K = 576, two column blocks
    halo("n128", 1, 8, 96, 256, 128),      # K = 2304
    halo("n128", 1, 8, 32, 416, 256),      # K = 3744 (conv2)
    pp("real", 1, 1, 257, 32, 32, K1),     # K = 32
    pp("real", 2, 15, 21, 64, 96, K1S2),   # K = 64
    pp("real", 2, 15, 21, 128, 128, K3S2), # K = 1152
    pp("real", 2, 11, 13, 32, 32, (7, 7, 2, 3)),  # K = 1568
    pp("real", 2, 12, 40, 256, 128, K3),   # K = 2304
    pp("real", 2, 7, 9, 416, 256, K3),     # K = 3744
    pp("loop", 1, 0, 251, 32, 160, K1),    # K = 32, more tiles than CUs
]


# ---- the dispatcher's rule, restated (conv_pp.hip: ctk_conv2d_sh) -------------------------------------------------------------------------
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def route(c):
    if c.KH == 3 and c.KW == 3 and c.stride == 1 and c.pad == 1 and c.H % 8 == 0 and c.W % 32 == 0:
        return f"conv_halo_3x3_c{c.Cin}_n{c.n_out}"
    return f"conv_pp128_{c.KH}x{c.KW}_s{c.stride}_c{c.Cin}_n{c.n_out}"


def tiles(c):
    """Tiles of the launch, as the kernel the case names counts them."""
    if c.kernel == "halo":
        return c.F * (c.H // 8) * (c.W // 32) * (c.n_pad // 128)
    return -(-c.M // 256) * (c.n_pad // 128)


def sized(c):
    """The persistent-loop cases, sized from the CU count: F = 0 -> the fewest frames that pass one round, H = 0 -> the rows of about
    5/4 of a round (check_route asserts cus < tiles < 2 cus and the partial last round on what comes out)."""
    if c.edge not in ("loop", "load"):
        return c
    n = cus()
    if c.F == 0:
        return dataclasses.replace(c, F=n // tiles(dataclasses.replace(c, F=1)) + 1)
    mb = (n + n // 4) // (c.n_pad // 128) + 1
    return dataclasses.replace(c, H=(mb * 256 - 100) // c.W)


# ---- operands ---------------------------------------------------------------------------------------------------------------------------------
def framed(x, pad, fill=CANARY):
    """x (4-byte or 2-byte elements, contiguous, a multiple of 16 bytes) in the middle of an allocation of int32 `fill`, `pad`
    words on either side (a multiple of 4: 16-byte alignment is kept) -> (the allocation, the view of x's bytes as int32)."""
    assert pad % 4 == 0
    w = x.contiguous().view(torch.int32).reshape(-1)
    buf = torch.full((w.numel() + 2 * pad,), fill, dtype=torch.int32, device=dev())
    buf[pad:pad + w.numel()] = w
    return buf, buf[pad:pad + w.numel()]


class Problem:
    """One convolution on the device, every operand framed, and its float64 reference on the CPU (computed once)."""

    def __init__(self, c, oracle):
        from cotracker_amd import _lib as L
        from cotracker_amd import ops
        self.c = c
        g = torch.Generator().manual_seed(c.F * 7 + c.H * 5 + c.W * 3 + c.K + c.n_out)
        if oracle == "int":
            x = torch.randint(-4, 5, (c.F, c.Cin, c.H, c.W), generator=g).float()
            w = torch.randint(-4, 5, (c.n_out, c.Cin, c.KH, c.KW), generator=g).float()
            w[0, 0, 0, 0] = 4.0  # max|W| = 4: the packed scale is 2^11
            b = torch.randint(-64, 65, (c.n_out,), generator=g).float()
        else:
            x = torch.randn(c.F, c.Cin, c.H, c.W, generator=g)
            w = torch.randn(c.n_out, c.Cin, c.KH, c.KW, generator=g) / c.K ** 0.5
            b = torch.randn(c.n_out, generator=g) * 0.1
        self.x, self.w, self.b = x, w, b
        ref = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), stride=c.stride, padding=c.pad)
        assert tuple(ref.shape[2:]) == c.out_hw
        self.ref = ref.permute(0, 2, 3, 1).reshape(c.M, c.n_out).contiguous()  # [pixel][n]
        # SH input, NHWC, inside NaN: the guard holds KH + pad + 2 image rows (a tap a row or a column off lands in it)
        sh = ops.split_rows(x.permute(0, 2, 3, 1).reshape(c.F * c.H * c.W, c.Cin).contiguous().to(dev()))
        self.lo_zero = bool((sh[:, :, 1] == 0).all())
        guard = max(16384, ((c.KH + c.pad + 2) * c.W + 64) * c.Cin)
        self.x_buf, self.x_sh = framed(sh, guard)
        # weights as encoder_hip._Conv repacks them, packed into the middle of a 0xFF-filled buffer
        mp = torch.zeros(c.n_pad, c.K)
        mp[:c.n_out] = w.permute(0, 2, 3, 1).reshape(c.n_out, c.K)
        mp = mp.to(dev())
        nbytes = ops._query_bytes("ctk_pack_weight_bytes", c.n_pad, c.K)
        assert nbytes % 16 == 0
        self.w_buf = torch.full((nbytes + 2 * FRAME,), 0xFF, dtype=torch.uint8, device=dev())
        self.wp = self.w_buf[FRAME:FRAME + nbytes]
        L.check(L.load().ctk_pack_weight(mp.data_ptr(), c.K, c.n_pad, c.K, self.wp.data_ptr(), torch.cuda.current_stream().cuda_stream),
                "ctk_pack_weight")
        assert bool((self.w_buf[:FRAME] == 0xFF).all()) and bool((self.w_buf[FRAME + nbytes:] == 0xFF).all())
        self.w_scale = float(self.wp[:4].view(torch.float32)[0])
        bp = torch.zeros(c.n_pad)
        bp[:c.n_out] = b
        self.b_buf, self.bias = framed(bp.to(dev()), FRAME)
        self.z_buf, self.zeros = framed(torch.zeros(32, device=dev()), FRAME)  # exactly 128 zero bytes

    def launch(self, F=None):
        """One launch on frames [0, F) into a canary-filled allocation -> (out f32 [M][n_out], recorder rows), after asserting that
        nothing outside [M][n_out] changed and nothing inside is NaN."""
        c = self.c if F is None else dataclasses.replace(self.c, F=F)
        buf = torch.full((c.M + 2 * GUARD, c.n_out), CANARY, dtype=torch.int32, device=dev())
        rc, rows = recorded(lambda: conv_raw(self.x_sh, c.F, c.H, c.W, c.Cin, self.wp, self.bias, c.n_out, c.n_pad, c.KH, c.KW, c.stride,
                                             c.pad, buf[GUARD:], self.zeros))
        assert rc == 0, (c.id, rc)
        assert bool((buf[:GUARD] == CANARY).all()), f"{c.id}: a store in front of row 0"
        assert bool((buf[GUARD + c.M:] == CANARY).all()), f"{c.id}: a store behind row M - 1"
        out = buf[GUARD:GUARD + c.M].view(torch.float32)
        nan = torch.isnan(out)
        assert not bool(nan.any()), f"{c.id}: {int(nan.sum())} NaN in the output (a read outside an operand, or an element never " \
                                    f"written); first (row, column) {nan.nonzero()[0].tolist()}"
        return out, rows


def check_route(c, rows):
    name = route(c)
    assert rows == {name: 1}, (c.id, rows, name)
    assert name.startswith("conv_halo_3x3_" if c.kernel == "halo" else "conv_pp128_"), f"{c.id} no longer reaches the kernel it names: {name}"
    if c.edge in ("loop", "load"):
        n, t = cus(), tiles(c)
        assert n < t < 2 * n and t % n != 0, f"{c.id}: {t} tiles on {n} CUs is not a partial second round"


# ---- 1 + 2 + 3: exact integers on the named kernel, every operand framed ------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_exact_integers_on_the_named_kernel(c):
    c = sized(c)
    p = Problem(c, "int")
    assert float(p.w.abs().max()) == 4.0 and p.w_scale == 2048.0 and p.lo_zero
    assert c.K * 16 * 2048 < 2 ** 27
    out, rows = p.launch()
    check_route(c, rows)
    got = out.double().cpu()
    bad = got != p.ref
    assert torch.equal(got, p.ref), f"{c.id}: {int(bad.sum())} of {bad.numel()} outputs differ from the integer product; first (row, column) " \
                                    f"{bad.nonzero()[0].tolist()}: {float(got[bad][0])} for {float(p.ref[bad][0])}; rows affected " \
                                    f"{int(bad.any(1).sum())}, columns {int(bad.any(0).sum())}"
    again, _ = p.launch()
    assert same_bits(again, out), f"{c.id}: a second launch gives other bits"
    if c.F > 1:
        one, rows = p.launch(F=1)
        check_route(dataclasses.replace(c, F=1, edge="frame0"), rows)
        assert same_bits(one, out[:one.shape[0]]), f"{c.id}: frame 0 alone differs from frame 0 in the batch"


# ---- 4: fp64 on real values ---------------------------------------------------------------------------------------------------------------------
ERRORS = {}


@pytest.mark.parametrize("c", REAL, ids=[c.id for c in REAL])
def test_fp64_real_values(c, capsys):
    c = sized(c)
    p = Problem(c, "real")
    out, rows = p.launch()
    check_route(c, rows)
    scale = float(p.ref.abs().max())
    err = float((out.double().cpu() - p.ref).abs().max())
    bound = 4e-6 * max(1.0, scale)
    rec = dict(kernel=route(c), K=c.K, M=c.M, max_ref=float(f"{scale:.4g}"), err=float(f"{err:.3e}"), bound=float(f"{bound:.3e}"))
    if c.K > 1440:  # beyond test_conv2d_sh_vs_fp64: what the float32 convolution of the reference gives on the same operands
        f32 = torch.nn.functional.conv2d(p.x, p.w, p.b, stride=c.stride, padding=c.pad).permute(0, 2, 3, 1).reshape(c.M, c.n_out)
        rec["torch_f32_cpu_err"] = float(f"{float((f32.double() - p.ref).abs().max()):.3e}")
    ERRORS[c.id] = rec
    with capsys.disabled():
        print(f"\nfp64-error {c.id}: {rec}")
    assert err <= bound, (c.id, rec)
    again, _ = p.launch()
    assert same_bits(again, out)
    if c.F > 1:
        one, _ = p.launch(F=1)
        assert same_bits(one, out[:one.shape[0]])


@pytest.fixture(scope="module", autouse=True)
def error_record():
    """CTK_CONV_MATRIX_ERRORS=<file>: the fp64 error of every real-valued case and the module's wall time
    (profiles/conv_matrix_errors.json)."""
    t0 = time.time()
    yield
    path = os.environ.get("CTK_CONV_MATRIX_ERRORS")
    if path and ERRORS:
        rec = {"what": "tests/test_gpu_conv_matrix.py, test_fp64_real_values: max |out - float64 reference| per case (randn activations, "
                       "weights / sqrt(K), bias 0.1 randn); bound 4e-6 * max(1, max|ref|); for K > 1440 also the error of torch's float32 "
                       "CPU conv2d against the same reference", "cus": cus(), "integer_cases": len(CASES), "real_cases": len(REAL),
               "module_seconds": float(f"{time.time() - t0:.1f}"), "cases": ERRORS}
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)
