"""ctk_gemm, the whole contract: every kernel family x epilogue x K x N x ragged M, batch strides, leading dimensions, canaries (-m gpu).

One entry point fans out to nine kernel families (gemm.hip, gemm_f16x3.hip, gemm_pp.hip) plus the tail split.  This module
drives it through `ctk_support.gemm_raw` (every field of ctk_gemm_args under the test's control) and checks

  1. WHICH KERNEL RAN.  Every launch is wrapped in the profile recorder and the recorder's row names are compared with `route`, a
     restatement of the dispatcher's thresholds (M comes from the device's CU count): a threshold moved in the dispatcher fails
     the case that names the kernel instead of silently turning it into a second test of another kernel.
  2. EXACT INTEGERS.  A, W integer-valued in [-4, 4] (one |W| = 4), bias / bias rows / residual in [-64, 64], act = NONE: the
     integers are their own f16 `hi` with `lo` = 0, ctk_pack_weight scales W by 2^11, every partial sum is a multiple of 2^11
     below 2^27 (f32 accumulation exact in any order, the persistent kernel's `resid * s` included), |out| <= 16 * 800 + 192
     < 65504 so an SH output's hi + lo is exact as well.  The reference is the product in float64, where these integers and
     their sums are exact (it IS the int64 product), and the assertion is torch.equal: no tolerance.  A dropped, repeated or
     misplaced K-tile, row or column block cannot hide.  K brackets the pipeline depths (1..5 K-tiles), the ring parity (13 and
     25 K-tiles) and the K > 768 form of the 256 x 192 kernel.
  3. fp64 for the GELU epilogues and real-valued operands, with the bounds the project asserts already: test_gemm's 2e-5
     (exact f32) / 4e-5 (split-half on f32 activations) and test_gpu_gemm_pp's 4e-5 * max(1, max|ref| / 4) on SH operands;
     without a residual the SH families must agree bit for bit on the same rows (same products, same K order), with one they
     are one rounding apart (test_gpu_gemm_pp's 4e-6 * max(1, max|ref|)).
     (CTK_HOT_EPILOGUES holds TWO GELU codes -- erf and tanh, both bias + SH output; the third GELU epilogue here is the
     generic erf + bias with f32 output.)
  4. ADDRESSING: batch > 1 in the corr_mlp.fc2 -> x pattern (a_bs, c_bs, ldc, f32 and SH output, residual advancing by c_bs),
     column windows (lda > K on f32 and SH operands, ldr != ldc, resid == C), bias-row periods that do and do not divide the
     tail cut.  Every output allocation is pre-filled with a NaN pattern and must be bit-unchanged outside [batch][M][N]; the A
     allocation is NaN outside [batch][M][K] and no output element may be NaN.
  5. ctk_split_rows / ctk_pack_weight to the bit against a numpy restatement (numpy's float16 cast rounds to nearest even).

Observed on an MI355X with 256 CUs, the smallest (M, K, N, batch) that reached each family: 64 x 64 kernels (1, 32, 64, 1);
gemm_f32 / gemm_f16x3 / gemm_sh 128 tiles (16257, 32, 384, 1); gemm_sh_256 (130817, 32, 256, 1); gemm_sh_pp256 (65281, 32, 256, 1),
batched (16385, 384, 256, 4); gemm_sh_pp192 (32513, 32, 384, 1); tail split (32769, 32, 384, 1).  Every kernel was exact on the
integers, short K on the persistent kernels included; no shape had to be routed away from them.  Largest fp64 error per family
(K = 32 ... 800; profiles/gemm_matrix_errors.json has every case): gemm_f32 64 / 128 tile 3.6e-6 / 4.8e-6, gemm_f16x3 2.2e-6 /
2.9e-6, gemm_sh_64 3.4e-6, gemm_sh_128 4.4e-6, gemm_sh_256 and gemm_sh_pp256 3.8e-6, gemm_sh_pp192 2.1e-5 (residual epilogue at
K = 800, max|ref| ~ 17).  The 170 cases take 4.2 s.
"""
import math

import numpy as np
import pytest
import torch

from ctk_support import dev, gemm_raw, recorded, same_bits

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_ERF, ACT_TANH = 0, 1, 2
CANARY = 0x7FC17FC1  # NaN as one f32 and as two f16
PERIOD = 16


# ---- epilogues ------------------------------------------------------------------------------------------------------------------
def epi_code(act=0, res=False, sh=False, brows=False, bias=False):
    """ctk_epi_code (gemm_params.h)."""
    return act | (4 if res else 0) | (8 if sh else 0) | (16 if brows else 0) | (32 if bias else 0)


HOT = {epi_code(ACT_ERF, sh=True, bias=True), epi_code(sh=True, bias=True), epi_code(brows=True), epi_code(bias=True),
       epi_code(res=True, bias=True), epi_code(ACT_TANH, sh=True, bias=True)}                                  # CTK_HOT_EPILOGUES
HOT_N256 = {epi_code(sh=True, bias=True), epi_code(bias=True), epi_code(ACT_TANH, sh=True, bias=True)}         # ..._N256
# act = NONE: the four hot codes and two generic ones
EPIS = {"bias": dict(bias=True), "bias_sh": dict(bias=True, sh=True), "brows": dict(brows=True), "bias_res": dict(bias=True, res=True),
        "none": dict(), "all": dict(bias=True, brows=True, res=True)}
GELUS = {"erf_bias_sh": dict(act=ACT_ERF, bias=True, sh=True), "tanh_bias_sh": dict(act=ACT_TANH, bias=True, sh=True),
         "erf_bias": dict(act=ACT_ERF, bias=True)}


# ---- the dispatcher's thresholds, restated (gemm.hip:163, gemm_f16x3.hip ctk_launch_gemm_f16x3, gemm_pp.hip ctk_launch_gemm_pp) ----
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def tail_pct():
    """CTK_OPT_GEMM_TAIL_PCT as the library holds it (default 25)."""
    import ctypes as C

    from cotracker_amd import _lib
    v = C.c_int(0)
    _lib.check(_lib.load().ctk_get_option(_lib.OPT_GEMM_TAIL_PCT, C.byref(v)), "ctk_get_option")
    return v.value


def small_last_round(tiles):
    """The tile count leaves a last round that the tail split would hand to the 64 x 64 kernel (were batch 1 and the split on)."""
    rem = tiles % cus()
    return tiles > cus() and rem > 0 and rem * 100 <= cus() * tail_pct()


def _pp_cut(M, N, batch, mode, brows, period):
    """-> (tiles, rows the persistent launch keeps, tail rows) of a shape the persistent kernels take."""
    nb = N // (256 if N % 256 == 0 else 192)
    tiles, cu = -(-M // 256) * nb * batch, cus()
    rem = tiles % cu
    if (mode & 32) and batch == 1 and small_last_round(tiles):
        rows_full = (tiles - rem) // nb * 256
        if rows_full > 0 and (not brows or rows_full % period == 0):
            return tiles, rows_full, M - rows_full
    return tiles, M, 0


def route(kind, M, K, N, batch=1, code=0, mode=33, period=PERIOD):
    """kind: "f32" (Wp = NULL), "f16x3" (f32 activations, packed W), "sh" (SH activations) -> the recorder rows of the launch."""
    big = N % 128 == 0 and -(-M // 128) * (N // 128) * batch >= 384
    if kind != "sh":
        return {f"gemm_{kind}_128x128" if big else f"gemm_{kind}_64x64"}
    sh64 = f"gemm_sh_64_k{K}_n{N}"
    res, brows = bool(code & 4), bool(code & 16)
    if (mode & 1) and (N % 256 == 0 or N % 192 == 0) and code in HOT and not (res and (K < 256 or N % 256 == 0)):
        tiles, _, tail = _pp_cut(M, N, batch, mode, brows, period)
        if tiles >= cus():
            return {f"gemm_sh_pp{256 if N % 256 == 0 else 192}_k{K}_n{N}"} | ({sh64} if tail else set())
    if not big:
        return {sh64}
    if N % 256 == 0 and -(-M // 256) * (N // 256) * batch >= 512 and code in HOT_N256:
        return {f"gemm_sh_256_k{K}_n{N}"}
    return {f"gemm_sh_128_k{K}_n{N}"}


# family -> (kind, CTK_OPT_GEMM_PP mode, row prefix, N values)
ALL_N = [64, 128, 192, 256, 320, 384]
FAMILIES = {
    "f32_64": ("f32", 33, "gemm_f32_64x64", ALL_N), "f32_128": ("f32", 33, "gemm_f32_128x128", [128, 256, 384]),
    "f16x3_64": ("f16x3", 33, "gemm_f16x3_64x64", ALL_N), "f16x3_128": ("f16x3", 33, "gemm_f16x3_128x128", [128, 256, 384]),
    "sh64": ("sh", 33, "gemm_sh_64_k", ALL_N), "sh128": ("sh", 32, "gemm_sh_128_k", [128, 256, 384]),
    "sh256": ("sh", 32, "gemm_sh_256_k", [256]), "pp256": ("sh", 33, "gemm_sh_pp256_k", [256]),
    "pp192": ("sh", 33, "gemm_sh_pp192_k", [192, 384]), "tail": ("sh", 33, "gemm_sh_pp192_k", [192, 384]),
}
SMALL = ("f32_64", "f16x3_64", "sh64")


def reach_m(fam, N, batch=1):
    """The M values of a family: 1, one past a tile and one short of three for the 64 x 64 kernels; for the others the smallest
    row-block count that reaches the kernel, ragged by 1 and by tile - 1."""
    if fam in SMALL:
        return [1, 65, 191]
    if fam in ("f32_128", "f16x3_128", "sh128"):
        T, mb = 128, -(-384 // ((N // 128) * batch))
    elif fam == "sh256":
        T, mb = 256, -(-512 // ((N // 256) * batch))
    else:
        T, nb = 256, N // (256 if N % 256 == 0 else 192)
        mb = -(-cus() // (nb * batch))
        want_tail = fam == "tail"
        if want_tail:
            mb += 1
        while bool(_pp_cut(mb * 256, N, batch, 33, False, PERIOD)[2]) != want_tail:  # (pp: whole launch persistent; tail: cut)
            mb += 1
            assert mb < 4 * cus(), "no such row-block count"
    return [(mb - 1) * T + 1, mb * T - 1]


def supports(fam, code, K):
    """Does the family have this epilogue?  (Otherwise the dispatcher falls back and the recorder must show it.)"""
    if fam == "sh256":
        return code in HOT_N256
    if fam == "pp256":
        return code in HOT and not code & 4
    if fam in ("pp192", "tail"):
        return code in HOT and (not code & 4 or K >= 256)
    return True


# ---- operands: one set per (oracle, rows, K, N), the float64 product computed once ------------------------------------------------------
class Operands:
    def __init__(self, oracle, rows, K, N, resid_scale=1.0):
        from cotracker_amd import ops
        g = torch.Generator(device=dev()).manual_seed(rows * 7 + K * 3 + N)
        if oracle == "int":
            def ints(lim, *shape):
                return torch.randint(-lim, lim + 1, shape, generator=g, device=dev()).float()
            self.a, self.w = ints(4, rows, K), ints(4, N, K)
            self.w[0, 0] = 4.0  # max|W| = 4: the packed scale is 2^11
            self.bias, self.brows, self.resid = ints(64, N), ints(64, PERIOD, N), ints(64, rows, N)
        else:
            def randn(*shape):
                return torch.randn(*shape, generator=g, device=dev())
            self.a, self.w = randn(rows, K), randn(N, K) / K ** 0.5
            self.bias, self.brows, self.resid = randn(N), randn(PERIOD, N), resid_scale * randn(rows, N)
        # the bias-row table is the first PERIOD rows of a table that is NaN from there on: a kernel that indexes it by the row
        # instead of row % period reads the NaN (and stays inside the allocation at the small shapes)
        guard = torch.full((256, N), float("nan"), device=dev())
        guard[:PERIOD] = self.brows
        self.brows = guard[:PERIOD]
        self.oracle, self.rows, self.K, self.N = oracle, rows, K, N
        self.a_sh, self.wp = ops.split_rows(self.a), ops.pack_weight(self.w)
        self.P = self.a.double() @ self.w.double().t()

    def ref(self, M, e, period=PERIOD, rows=slice(None)):
        """float64 reference of rows [0, M) (or rows `rows` of the operands, M of them) under epilogue e."""
        r = self.P[rows][:M].clone()
        if e.get("bias"):
            r += self.bias.double()
        if e.get("brows"):
            r += self.brows.double()[torch.arange(M, device=dev()) % period]
        if e.get("act") == ACT_ERF:
            r = torch.nn.functional.gelu(r)
        elif e.get("act") == ACT_TANH:
            r = torch.nn.functional.gelu(r, approximate="tanh")
        if e.get("res"):
            r += self.resid[rows][:M].double()
        return r


_OPERANDS = {}


def operands(oracle, rows, K, N, resid_scale=1.0):
    key = (oracle, rows, K, N, resid_scale)
    if key not in _OPERANDS:
        if len(_OPERANDS) >= 2:  # the big families hold ~1 GiB per set
            _OPERANDS.pop(next(iter(_OPERANDS)))
        _OPERANDS[key] = Operands(*key)
    return _OPERANDS[key]


def unsplit(sh):
    from cotracker_amd import ops
    return ops.unsplit(sh)


def dense(kind, d, M, e, period=PERIOD):
    """One unbatched launch on rows [0, M) of d, dense leading dimensions, NaN-filled output -> (out as f32 [M][N], rows)."""
    K, N, sh = d.K, d.N, bool(e.get("sh"))
    out = torch.full((M, N // 32, 2, 32), float("nan"), dtype=torch.float16, device=dev()) if sh else \
        torch.full((M, N), float("nan"), device=dev())
    rc, rows = recorded(lambda: gemm_raw(
        d.a_sh if kind == "sh" else d.a, 2 * K if kind == "sh" else K, M, N, K, out, 2 * N if sh else N, W=d.w, ldw=K,
        Wp=None if kind == "f32" else d.wp, bias=d.bias if e.get("bias") else None, bias_rows=d.brows if e.get("brows") else None,
        period=period if e.get("brows") else 0, resid=d.resid if e.get("res") else None, ldr=N, act=e.get("act", 0),
        a_split=kind == "sh", c_split=sh))
    assert rc == 0, rc
    return (unsplit(out) if sh else out), rows


def tol_for(kind, ref):
    """The project's bounds for randn operands: test_gemm (f32 activations), test_gpu_gemm_pp (SH operands)."""
    if kind == "f32":
        return 2e-5
    if kind == "f16x3":
        return 4e-5
    return 4e-5 * max(1.0, float(ref.abs().max()) / 4)


def err(out, ref):
    return float((out.double() - ref).abs().max())


# ---- 1 + 2: every family x epilogue x K x N x ragged M on integers, exact ---------------------------------------------------------------
K_LIST = [32, 64, 96, 128, 160, 384, 416, 800]


@pytest.mark.parametrize("K", K_LIST)
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_exact_integers_on_the_named_kernel(fam, K, ctk_option):
    from cotracker_amd import _lib
    kind, mode, prefix, ns = FAMILIES[fam]
    ctk_option(_lib.OPT_GEMM_PP, mode)
    reached = 0
    for N in ns:
        ms = reach_m(fam, N)
        d = operands("int", max(ms), K, N)
        for M in ms:
            for name, e in EPIS.items():
                if e.get("sh") and kind == "f32":
                    continue  # SH output exists on the split-half back end only
                code = epi_code(**e)
                out, rows = dense(kind, d, M, e)
                where = f"{fam} M={M} K={K} N={N} {name}: rows {sorted(rows)}"
                assert set(rows) == route(kind, M, K, N, code=code, mode=mode), where
                if supports(fam, code, K):
                    assert any(r.startswith(prefix) for r in rows), where
                    assert fam != "tail" or f"gemm_sh_64_k{K}_n{N}" in rows, where
                    reached += 1
                else:
                    assert not any(r.startswith(prefix) for r in rows), where  # the fallback, and the row shows it
                assert torch.equal(out.double(), d.ref(M, e)), where
    assert reached, f"{fam}: no launch reached the kernel"


# ---- 3: fp64 on real-valued operands: GELU epilogues, and the same bits from every SH family ------------------------------------------
@pytest.mark.parametrize("K", [32, 96, 384])
@pytest.mark.parametrize("fam", ["f32_64", "f32_128", "f16x3_64", "f16x3_128"])
def test_fp64_f32_activations(fam, K, capsys):
    """test_gemm's operands and bounds (bias + bias rows + residual under each activation, and the bare product) on the four
    kernels that read f32 activations, at one ragged M each and the K range the primitive tests never ran."""
    kind, _, prefix, _ = FAMILIES[fam]
    N = 384
    M = reach_m(fam, N)[-1]
    d = operands("real", M, K, N)
    worst = 0.0
    for act in (ACT_NONE, ACT_ERF, ACT_TANH):
        for e in (dict(act=act, bias=True, brows=True, res=True), dict(act=act, bias=True, sh=True), dict()):
            if e.get("sh") and kind == "f32":
                continue
            out, rows = dense(kind, d, M, e)
            assert set(rows) == {prefix}, (fam, rows)
            ref = d.ref(M, e)
            worst = max(worst, err(out, ref))
            assert err(out, ref) < tol_for(kind, ref), (fam, K, e, err(out, ref))
    with capsys.disabled():
        print(f"\nfp64-error {fam} M={M} K={K} N={N}: {worst:.3e} (bound {tol_for(kind, None):.0e})")


@pytest.mark.parametrize("N,K", [(256, 32), (256, 96), (256, 384), (384, 32), (384, 96), (384, 384),
                                 (384, 800)])  # (K = 800: the K > 768 form of the 256 x 192 kernel, residual on its first 8 of 25 K-tiles)
def test_fp64_and_same_bits_across_sh_families(N, K, ctk_option, capsys):
    """Every SH family on the same operands: the persistent kernel and the old 256 / 128 tiles on the full (ragged) M, the 64 x 64
    kernel and (N = 256) the 128 tile on a row prefix -- rows are independent, so a prefix launch must give the prefix's bits."""
    from cotracker_amd import _lib
    pp = "pp256" if N == 256 else "pp192"
    M = max(reach_m(pp, N)[0], reach_m("sh256", N)[0] if N == 256 else 0)
    m128, m64 = reach_m("sh128", N)[0], 321
    d = operands("real", M, K, N, 3.0)  # (residual 3 * randn: test_gpu_gemm_pp's)
    worst = {}
    epis = dict(GELUS, **EPIS)
    for name, e in epis.items():
        code = epi_code(**e)
        ref = d.ref(M, e)
        tol = tol_for("sh", ref)
        outs = {}
        for fam, mode, rows_m in ((pp, 1, M), ("sh256", 0, M), ("sh128", 0, M if N == 384 else m128), ("sh64", 0, m64)):
            if fam == "sh256" and N != 256:
                continue
            ctk_option(_lib.OPT_GEMM_PP, mode)
            out, rows = dense("sh", d, rows_m, e)
            assert set(rows) == route("sh", rows_m, K, N, code=code, mode=mode), (fam, name, rows)
            on_family = any(r.startswith(FAMILIES[fam][2]) for r in rows)
            assert on_family == supports(fam, code, K), (fam, name, rows)
            e_ = err(out, ref[:rows_m])
            assert e_ < tol, (fam, name, K, N, e_, tol)
            if on_family:
                worst[fam] = max(worst.get(fam, 0.0), e_)
            outs[fam] = (out, on_family)
        first = outs[pp][0]
        for fam, (out, on_family) in outs.items():
            if e.get("res") and outs[pp][1] and fam != pp:
                # the 256 x 192 kernel adds residual * s into the accumulators, the others add the residual last: one rounding
                assert err(out, first[:out.shape[0]]) <= 4e-6 * max(1.0, float(ref.abs().max())), (fam, name)
            else:
                assert torch.equal(out, first[:out.shape[0]]), f"{fam} and {pp} differ on {name}, K={K} N={N}"
    with capsys.disabled():
        print(f"\nfp64-error K={K} N={N} M={M}: " + ", ".join(f"{f} {v:.3e}" for f, v in sorted(worst.items())))


# ---- 4: addressing ------------------------------------------------------------------------------------------------------------------
def windowed(kind, d, M, e, batch=1, ldc=1120, c_bs=0, c0=0, lda_pad=64, k0=32, resid="separate", ldr=1024, period=PERIOD, pad_rows=2):
    """A launch with every stride in play.  A is batch blocks of M + pad_rows rows, row b*(M+pad_rows)+m = row b*M+m of d, inside an
    allocation that is NaN outside the [M][K] windows (columns [k0, k0 + K) of rows K + lda_pad wide); the output is columns
    [c0 + b*c_bs, + N) of an [M + pad_rows][ldc] allocation pre-filled with CANARY.  -> (out f32 [batch][M][N], recorder rows)
    after asserting that nothing outside the window changed and nothing inside is NaN.  resid: "separate" (its own [.][ldr]
    matrix, advancing by c_bs like C) or "inplace" (resid == C)."""
    K, N, sh_in, sh_out = d.K, d.N, kind == "sh", bool(e.get("sh"))
    Ma, LDA = M + pad_rows, K + lda_pad
    # (in 4-byte units an SH row and an f32 row are the same: K units per row of A, N per row of C)
    abuf = torch.full((batch * Ma, LDA), CANARY, dtype=torch.int32, device=dev())
    src = (d.a_sh.view(torch.int32).reshape(d.rows, K) if sh_in else d.a.view(torch.int32))[:batch * M].reshape(batch, M, K)
    abuf.view(batch, Ma, LDA)[:, :M, k0:k0 + K] = src
    unit = 2 if sh_in else 1  # halves per 4-byte unit
    cbuf = torch.full((Ma, ldc), CANARY, dtype=torch.int32, device=dev())
    mask = torch.zeros(Ma, ldc, dtype=torch.bool, device=dev())
    for b in range(batch):
        mask[:M, c0 + b * c_bs:c0 + b * c_bs + N] = True
    res_t = None
    if e.get("res"):
        assert not sh_out
        r = d.resid[:batch * M].reshape(batch, M, N)
        if resid == "inplace":
            res_t, ldr = cbuf, ldc
        else:
            res_t = torch.full((Ma, ldr), CANARY, dtype=torch.int32, device=dev())
        for b in range(batch):
            res_t.view(torch.float32)[:M, c0 + b * c_bs:c0 + b * c_bs + N] = r[b]
    ounit = 2 if sh_out else 1
    rc, rows = recorded(lambda: gemm_raw(
        abuf[0, k0:], LDA * unit, M, N, K, cbuf[0, c0:], ldc * ounit, W=d.w, ldw=K, Wp=None if kind == "f32" else d.wp,
        bias=d.bias if e.get("bias") else None, bias_rows=d.brows if e.get("brows") else None, period=period if e.get("brows") else 0,
        resid=None if res_t is None else res_t[0, c0:], ldr=ldr, act=e.get("act", 0), batch=batch, a_bs=Ma * LDA * unit,
        c_bs=c_bs * ounit, a_split=sh_in, c_split=sh_out))
    assert rc == 0, rc
    assert bool((cbuf[~mask] == CANARY).all()), "a store outside the [batch][M][N] window"
    outs = []
    for b in range(batch):
        w = cbuf[:M, c0 + b * c_bs:c0 + b * c_bs + N].contiguous()
        outs.append(unsplit(w.view(torch.float16).reshape(M, N // 32, 2, 32)) if sh_out else w.view(torch.float32))
    out = torch.stack(outs)
    assert not bool(torch.isnan(out).any()), "NaN in the output: read outside the A window, or an element never written"
    return out, rows


def batched_ref(d, M, e, batch, period=PERIOD):
    return torch.stack([d.ref(M, e, period, rows=slice(b * M, (b + 1) * M)) for b in range(batch)])


def judge(d, kind, out, ref):
    if d.oracle == "int":
        assert torch.equal(out.double(), ref)
    else:
        assert err(out, ref) < tol_for(kind, ref), (err(out, ref), tol_for(kind, ref))


def pp_rows(N, batch):
    """Rows per batch (batch > 1, ragged by 1) that reach the persistent kernel with a small, non-empty last round: the tile count
    at which a batch-1 launch would be split, so that "batch > 1 is never split" is what the recorder row shows."""
    nb = N // (256 if N % 256 == 0 else 192)
    mb = -(-cus() // (nb * batch))
    while not small_last_round(mb * nb * batch):
        mb += 1
        assert mb < 4 * cus(), "no such row-block count"
    return (mb - 1) * 256 + 1


@pytest.mark.parametrize("oracle", ["int", "real"])
@pytest.mark.parametrize("sh_out", [False, True], ids=["f32out", "shout"])
@pytest.mark.parametrize("batch,c_bs", [(4, 256), (3, 320)])
@pytest.mark.parametrize("fam", ["sh64", "pp256"])
def test_batched_column_blocks_of_a_wider_matrix(fam, batch, c_bs, sh_out, oracle):
    """corr_mlp.fc2 -> x: one batch per level, A advancing by a_bs, C by c_bs columns of an [.][1120] matrix (f32 or SH), and a
    batch stride that is not N.  batch > 1 never takes the tail split."""
    N, K = 256, 384
    M = 301 if fam == "sh64" else pp_rows(N, batch)
    d = operands(oracle, batch * M, K, N)
    e = dict(bias=True, sh=sh_out)
    out, rows = windowed("sh", d, M, e, batch=batch, c_bs=c_bs, c0=32)
    assert set(rows) == route("sh", M, K, N, batch=batch, code=epi_code(**e)), rows
    assert set(rows) == {f"gemm_sh_64_k{K}_n{N}" if fam == "sh64" else f"gemm_sh_pp256_k{K}_n{N}"}, rows  # (pp256: no gemm_sh_64 row)
    judge(d, "sh", out, batched_ref(d, M, e, batch))


@pytest.mark.parametrize("oracle", ["int", "real"])
@pytest.mark.parametrize("resid", ["separate", "inplace"])
@pytest.mark.parametrize("fam", ["sh64", "sh128", "pp192"])
def test_batched_residual_advances_by_c_bs(fam, resid, oracle, ctk_option):
    """include/ctk.h: the residual's batch stride is c_bs, whatever ldr is -- in its own matrix (ldr != ldc) and in place."""
    from cotracker_amd import _lib
    N, K, batch = 384, 384, 2
    if fam == "sh128":
        ctk_option(_lib.OPT_GEMM_PP, 32)
    M = {"sh64": 301, "sh128": (-(-384 // (3 * batch)) - 1) * 128 + 1, "pp192": pp_rows(N, batch)}[fam]
    d = operands(oracle, batch * M, K, N, 3.0)
    e = dict(bias=True, res=True)
    out, rows = windowed("sh", d, M, e, batch=batch, c_bs=512, resid=resid)
    assert set(rows) == {FAMILIES[fam][2] + f"{K}_n{N}"}, rows
    judge(d, "sh", out, batched_ref(d, M, e, batch))


@pytest.mark.parametrize("oracle", ["int", "real"])
@pytest.mark.parametrize("fam,name", [(f, n) for f in ("f32_64", "f16x3_64", "sh64", "pp192") for n in ("bias", "bias_sh", "bias_res", "all")
                                      if (f, n) != ("f32_64", "bias_sh")])  # (SH output exists on the split-half back end only)
def test_column_windows(fam, name, oracle):
    """lda > K (A a column window of a wider f32 or SH matrix), C a column window, ldr != ldc."""
    kind = FAMILIES[fam][0]
    e = EPIS[name]
    N, K = 384, 96 if name == "bias" else 384
    M = 191 if fam != "pp192" else reach_m("pp192", N)[0]
    d = operands(oracle, M, K, N, 3.0)
    out, rows = windowed(kind, d, M, e, c0=64, ldc=1120, ldr=512)
    assert set(rows) == route(kind, M, K, N, code=epi_code(**e)), rows
    if supports(fam, epi_code(**e), K):
        assert any(r.startswith(FAMILIES[fam][2]) for r in rows), rows
    judge(d, kind, out[0], d.ref(M, e))


@pytest.mark.parametrize("oracle", ["int", "real"])
@pytest.mark.parametrize("K", [32, 384])
def test_bias_row_period_and_the_tail_cut(K, oracle, ctk_option):
    """A period that divides the cut (16) leaves the tail split on; one that does not (12) turns it off -- the recorder shows it --
    and gives the bits of a launch with the split disabled.  The 64 x 64 kernel alone takes any period."""
    from cotracker_amd import _lib
    N = 384
    M = reach_m("tail", N)[0]
    d = operands(oracle, M, K, N)
    e = dict(brows=True)
    pp, sh64 = f"gemm_sh_pp192_k{K}_n{N}", f"gemm_sh_64_k{K}_n{N}"
    out16, rows = dense("sh", d, M, e, period=16)
    assert set(rows) == {pp, sh64}, rows
    judge(d, "sh", out16, d.ref(M, e, 16))
    out12, rows = dense("sh", d, M, e, period=12)
    assert set(rows) == {pp} == route("sh", M, K, N, code=16, period=12), rows
    judge(d, "sh", out12, d.ref(M, e, 12))
    ctk_option(_lib.OPT_GEMM_PP, 1)
    whole, rows = dense("sh", d, M, e, period=12)
    assert set(rows) == {pp}, rows
    assert torch.equal(out12, whole)
    small, rows = dense("sh", d, 191, e, period=12)
    assert set(rows) == {sh64}, rows
    assert torch.equal(small, whole[:191])


# ---- 5: ctk_split_rows and ctk_pack_weight, to the bit ----------------------------------------------------------------------------------
def np_split(x):
    """hi = rn16(x), lo = rn16(x - hi) -> SH layout [M][K/32][2][32]."""
    M, K = x.shape
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return np.stack([hi.reshape(M, K // 32, 32), lo.reshape(M, K // 32, 32)], axis=2)


def special_values(rows, K, seed):
    """Random rows with the corners in front: ties to even, -0, the top of the f16 range, lo subnormal, hi subnormal, zeros."""
    r = np.random.RandomState(seed)
    x = (r.standard_normal((rows, K)) * np.exp2(r.randint(-12, 12, (rows, K)))).astype(np.float32)
    corners = [2049.0, 2051.0, -2049.0, 4098.0, 4102.0, -0.0, 0.0, 65503.996, -65503.996, 65472.0, 1.0 + 2.0 ** -20, 0.1, -0.3,
               2.0 ** -14, 2.0 ** -15 * 1.5, 2.0 ** -24, 2.0 ** -25, 3.0 * 2.0 ** -25, 6.1e-5, 1e-7, 1.0, 2048.0]
    x[0, :len(corners)] = np.array(corners, np.float32)
    x[1] = 0.0  # a zero row
    return x


@pytest.mark.parametrize("K,pad", [(32, 0), (96, 36), (384, 4)])
def test_split_rows_bit_exact(K, pad):
    from cotracker_amd import _lib as L
    M = 37
    wide = np.full((M, K + pad), np.nan, np.float32)  # ld > K: columns outside the window are never read
    wide[:, :K] = special_values(M, K, K)
    x = torch.from_numpy(wide).to(dev())
    out = torch.full((M, K // 32, 2, 32), float("nan"), dtype=torch.float16, device=dev())
    L.check(L.load().ctk_split_rows(x.data_ptr(), K + pad, M, K, out.data_ptr(), torch.cuda.current_stream().cuda_stream), "ctk_split_rows")
    assert same_bits(out, torch.from_numpy(np_split(wide[:, :K])))


def np_pack(w):
    """-> (s, 1/s, hi / lo of s * W in the blob's [N][K/32][2][32] layout): s = 2^(13 - floor(log2 max|W|)), 1 for a zero matrix."""
    mx = float(np.abs(w).max())
    e = 13 - (math.frexp(mx)[1] - 1) if 0.0 < mx < math.inf else 0
    e = max(-100, min(100, e))
    s = np.float32(math.ldexp(1.0, e))
    return s, np.float32(math.ldexp(1.0, -e)), np_split((w * s).astype(np.float32))


@pytest.mark.parametrize("case", ["pow2", "below_pow2", "tiny", "huge", "zero", "window"])
def test_pack_weight_bit_exact(case):
    from cotracker_amd import _lib as L
    from cotracker_amd import ops
    N, K, pad = 70, 96, 8 if case == "window" else 0
    w = special_values(N, K, 5)
    w = np.clip(w, -3.9, 3.9).astype(np.float32)
    w[2, :6] = np.array([2049, 2051, -2049, 4098, 4102, 8191.5], np.float32) / 2048  # ties once scaled by 2^11
    w[0, 0] = {"pow2": 4.0, "below_pow2": np.nextafter(np.float32(4.0), np.float32(0.0)), "window": -5.5}.get(case, 3.9)
    if case == "tiny":
        w *= np.float32(2.0 ** -40)
    elif case == "huge":
        w *= np.float32(2.0 ** 30)
    elif case == "zero":
        w[:] = 0.0
    wide = np.full((N, K + pad), np.nan, np.float32)
    wide[:, :K] = w
    x = torch.from_numpy(wide).to(dev())
    blob = torch.full((ops._query_bytes("ctk_pack_weight_bytes", N, K),), 0xFF, dtype=torch.uint8, device=dev())
    L.check(L.load().ctk_pack_weight(x.data_ptr(), K + pad, N, K, blob.data_ptr(), torch.cuda.current_stream().cuda_stream), "ctk_pack_weight")
    s, inv, body = np_pack(w)
    hdr = blob[:8].cpu().numpy().view(np.float32)
    assert hdr[0] == s and hdr[1] == inv and s * inv == 1.0, (hdr, s, inv)
    if case in ("pow2", "below_pow2"):
        assert s == {"pow2": 2.0 ** 11, "below_pow2": 2.0 ** 12}[case]
    got = blob[64:].view(torch.float16).reshape(N, K // 32, 2, 32)
    assert same_bits(got, torch.from_numpy(body))
