"""attention_time_rows_kernel: time attention with one workgroup per track pair, q | k | v read as whole blocks (-m gpu).

ctk_attention_ex sends a call to this kernel where the old persistent kernel ran and the operands are one row-contiguous block:
k == q + 384, v == q + 768, q_ld == kv_ld == 1152, 16 frames per track on consecutive rows, the tracks one after the other, no
masks, a single-level batch, and with CTK_OPT_ATTENTION_TIME_PERSISTENT at its default 1 at least 8 track pairs per CU (below
that count the old kernel is the faster one).  Value 3 of the option drops the count, so that small shapes reach the kernel;
value 2 keeps the wave-per-job persistent kernel (attention_time16_kernel) on every layout and 0 selects
attention_self_kernel<2>: the two old routes.  The new kernel promises their bits.  Checked here, on shapes far below the
workload's, with value 3 for the new kernel:

  1. BIT IDENTITY with both old routes, f32 and SH output, on the randn operands and on the exact-gather operands of
     tests/test_gpu_attention_matrix.py (the same generators and, where that module has the shape, the same seeds): S = 16 with
     nbatch 1 (a lone half pair), 2, 7 (three pairs and a half), 33 and 1031 (516 pairs: more than one per workgroup on a 256-CU
     device -- the walk and the register prefetch across pairs -- and a half-empty last pair; 76 MB of operands).
     The operand buffer ends with the last track and 16 rows of NaN follow it: the missing track of a half pair must not be
     read there (0 * NaN would reach the output), and the output allocation is a canary pattern outside the addressed rows.
  2. FLOAT64 attention on the same operands, at the bound tests/test_gpu_attention_matrix.py records for attention_time16_kernel
     (profiles/attention_matrix_errors.json, kernels.time16.none = 1.188e-6, asserted as 1.2e-6).  The bound is the old kernel's
     record and not this kernel's error; with identical bits the error is the old kernel's.
  3. FALLBACK LAYOUTS at the option's default and at 3: separate q (leading dimension 384) and k | v (768) buffers, one q | k | v buffer of
     leading dimension 1156, a masked call on the block layout, and S = 8 on the block layout (the new kernel takes 16 frames
     only).  Each returns the bits of the old routes.
  4. DETERMINISM: two launches on the same operands are bit-equal.
  5. THE DEFAULT: 8 pairs per CU and one track more (4097 tracks on a 256-CU device, randn operands made on the device) return
     the bits of the wave-per-job kernel with the option at 1, and so does a shape below the count.

The recorder names every one of these launches `attention_time`, so which kernel ran cannot be read back from Python: the
conditions are restated in `takes_block_kernel` and the window- and stage-level suites are the check that run_transformer's
calls meet them.
"""
import functools

import pytest
import torch

import test_gpu_attention_matrix as M
from ctk_support import attention_raw, dev, maxdiff, same_bits
from test_gpu_gemm_matrix import CANARY

pytestmark = pytest.mark.gpu

S = 16
TIME16_FP64_BOUND = 1.2e-6  # profiles/attention_matrix_errors.json: kernels.time16.none = 1.188e-06
DEFAULT, NEW, WAVE, SELF2 = 1, 3, 2, 0  # CTK_OPT_ATTENTION_TIME_PERSISTENT
MIN_ROUNDS = 8  # attention.hip, TR_MIN_ROUNDS: pairs per CU from which the default picks the new kernel
NBATCH = (1, 2, 7, 33, 1031)


def takes_block_kernel(n1, q_ld, kv_ld, one_buffer, masked, mode, nbatch=None):
    """ctk_attention_ex's conditions for attention_time_rows_kernel, restated (rows of a track consecutive, tracks n1 rows apart)."""
    enough = mode == NEW or (mode == DEFAULT and nbatch is not None and
                             (nbatch + 1) // 2 >= MIN_ROUNDS * torch.cuda.get_device_properties(0).multi_processor_count)
    return enough and n1 == 16 and q_ld == kv_ld == 1152 and one_buffer and not masked


def case_for(nbatch, n=S):
    """The matrix module's case of this shape where it has one (the same id, so the same operands), else a new one."""
    return next((c for c in M.TIME16 if c.n1 == n and c.nbatch == nbatch), M.Case("time16", n, n, nbatch))


@functools.lru_cache(maxsize=None)
def operands(nbatch, n=S):
    """-> ((Q, K, V) randn, (Q, K, V, expected [nbatch][8][n][48], rows where it is exact) exact gather); Q, K, V [nbatch][n][384].
    Shared by the tests and left unchanged."""
    c = case_for(nbatch, n)
    ex = M.exact_problem(c)
    return M.real_problem(c)[:3], (ex[0], ex[1], ex[2], ex[5], ex[6])


def launch(Q, K, V, sh, ctk_option, mode, layout="block", key_mask=None):
    """One single-level call -> the output rows [nbatch * n][384] f32 or [.][12][2][32] halves.
    layout: "block" q | k | v in one [rows][1152] buffer | "ld1156" the same with four floats more per row | "split" q in a
    [rows][384] buffer, k | v in a [rows][768] buffer."""
    from cotracker_amd import _lib
    ctk_option(_lib.OPT_ATTENTION_VALU, 0)
    ctk_option(_lib.OPT_ATTENTION_TIME_PERSISTENT, mode)
    B, n = Q.shape[0], Q.shape[1]
    R = B * n
    nan_rows = 16  # behind the last track
    if layout == "split":
        qbuf = torch.full((R + nan_rows, 384), float("nan"), device=dev())
        kvbuf = torch.full((R + nan_rows, 768), float("nan"), device=dev())
        qbuf[:R] = Q.reshape(R, 384)
        kvbuf[:R, :384], kvbuf[:R, 384:] = K.reshape(R, 384), V.reshape(R, 384)
        q, k, v, q_ld, kv_ld = qbuf, kvbuf, kvbuf[0, 384:], 384, 768
    else:
        ld = 1152 if layout == "block" else 1156
        buf = torch.full((R + nan_rows, ld), float("nan"), device=dev())
        buf[:R, :384], buf[:R, 384:768], buf[:R, 768:1152] = Q.reshape(R, 384), K.reshape(R, 384), V.reshape(R, 384)
        q, k, v, q_ld, kv_ld = buf, buf[0, 384:], buf[0, 768:], ld, ld
    obuf = torch.full((R + 32, 384), CANARY, dtype=torch.int32, device=dev())
    rc = attention_raw(q, q_ld, n, 1, k, v, kv_ld, n, 1, obuf, 768 if sh else 384, n, 1, B, n, n, o_split=sh, key_mask=key_mask)
    assert rc == 0, rc
    assert bool((obuf[R:] == CANARY).all()), "a store behind the last output row"
    out = obuf[:R].view(torch.float16).reshape(R, 12, 2, 32) if sh else obuf[:R].view(torch.float32)
    assert not bool(torch.isnan(out).any()), "NaN in the output: a read behind the last track, or an element never written"
    return out


# ---- 1: the bits of both old routes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbatch", NBATCH)
def test_block_kernel_equals_both_old_routes(nbatch, ctk_option):
    assert takes_block_kernel(S, 1152, 1152, True, False, NEW) and not takes_block_kernel(S, 1152, 1152, True, False, WAVE)
    real, exact = operands(nbatch)
    for Q, K, V in (real, exact[:3]):
        for sh in (False, True):
            new = launch(Q, K, V, sh, ctk_option, NEW)
            assert same_bits(new, launch(Q, K, V, sh, ctk_option, WAVE)), (nbatch, sh, "attention_time16_kernel")
            assert same_bits(new, launch(Q, K, V, sh, ctk_option, SELF2)), (nbatch, sh, "attention_self_kernel<2>")


@pytest.mark.parametrize("nbatch", NBATCH)
def test_block_kernel_returns_the_exact_gather(nbatch, ctk_option):
    """The exact-gather operands of the matrix module: every output row is a V row (or the mean of two), to the bit."""
    Q, K, V, want, exact = operands(nbatch)[1]
    out = launch(Q, K, V, False, ctk_option, NEW).reshape(nbatch, S, 8, 48).permute(0, 2, 1, 3)
    assert bool(exact.any()) and same_bits(out[exact], want[exact])


# ---- 2: float64 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbatch", NBATCH)
def test_block_kernel_against_float64(nbatch, ctk_option):
    c = case_for(nbatch)
    for Q, K, V in (operands(nbatch)[0], operands(nbatch)[1][:3]):
        out = launch(Q, K, V, False, ctk_option, NEW).reshape(nbatch, S, 8, 48).permute(0, 2, 1, 3)
        e = maxdiff(out, M.fp64_reference(c, Q, K, V, None, None))
        print(f"attention_time_rows fp64: nbatch {nbatch} max |out - ref| = {e:.3e} (bound {TIME16_FP64_BOUND:.1e})")
        assert e < TIME16_FP64_BOUND, (nbatch, e)


# ---- 3: every other layout takes the path it took ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["split", "ld1156"])
def test_fallback_layouts_keep_their_route(layout, ctk_option):
    assert not takes_block_kernel(S, 384 if layout == "split" else 1156, 768 if layout == "split" else 1156, layout != "split", False, NEW)
    Q, K, V = operands(7)[0]
    for sh in (False, True):
        default = launch(Q, K, V, sh, ctk_option, DEFAULT, layout)
        assert same_bits(default, launch(Q, K, V, sh, ctk_option, NEW, layout)), (layout, sh)
        assert same_bits(default, launch(Q, K, V, sh, ctk_option, WAVE, layout)), (layout, sh)
        assert same_bits(default, launch(Q, K, V, sh, ctk_option, SELF2, layout)), (layout, sh)
        assert same_bits(default, launch(Q, K, V, sh, ctk_option, NEW, "block")), (layout, sh)  # the layout is no part of the result


def test_masked_call_on_the_block_layout_keeps_its_route(ctk_option):
    assert not takes_block_kernel(S, 1152, 1152, True, True, NEW)
    Q, K, V = operands(7)[0]
    km = torch.ones(1, S, dtype=torch.uint8, device=dev())
    km[0, 3] = km[0, 15] = 0
    for sh in (False, True):
        default = launch(Q, K, V, sh, ctk_option, DEFAULT, key_mask=km)
        assert same_bits(default, launch(Q, K, V, sh, ctk_option, NEW, key_mask=km)), sh
        assert same_bits(default, launch(Q, K, V, sh, ctk_option, WAVE, key_mask=km)), sh
        assert same_bits(default, launch(Q, K, V, sh, ctk_option, SELF2, key_mask=km)), sh
        assert not same_bits(default, launch(Q, K, V, sh, ctk_option, NEW)), sh  # the mask was applied
    c = case_for(7)
    out = launch(Q, K, V, False, ctk_option, NEW, key_mask=km).reshape(7, S, 8, 48).permute(0, 2, 1, 3)
    assert maxdiff(out, M.fp64_reference(c, Q, K, V, km, None)) < 5e-6  # (the matrix module's bound for the masked kernels)


@pytest.mark.parametrize("n", [1, 2, 8, 15])
def test_short_tracks_on_the_block_layout_keep_their_route(n, ctk_option):
    """Fewer than 16 frames: a pair is no 147 456-byte block; the wave-per-job kernel keeps these calls."""
    assert not takes_block_kernel(n, 1152, 1152, True, False, NEW)
    Q, K, V = operands(7, n)[0]
    for sh in (False, True):
        default = launch(Q, K, V, sh, ctk_option, DEFAULT)
        assert same_bits(default, launch(Q, K, V, sh, ctk_option, NEW)), (n, sh)
        assert same_bits(default, launch(Q, K, V, sh, ctk_option, WAVE)), (n, sh)
        assert same_bits(default, launch(Q, K, V, sh, ctk_option, SELF2)), (n, sh)


# ---- 4: determinism ---------------------------------------------------------------------------------------------------------------------------
def test_two_launches_are_bit_equal(ctk_option):
    Q, K, V = operands(1031)[0]
    for sh in (False, True):
        assert same_bits(launch(Q, K, V, sh, ctk_option, NEW), launch(Q, K, V, sh, ctk_option, NEW)), sh


# ---- 5: the default ------------------------------------------------------------------------------------------------------------------------------
def test_default_picks_the_block_kernel_from_eight_pairs_per_cu(ctk_option):
    nbatch = 2 * MIN_ROUNDS * torch.cuda.get_device_properties(0).multi_processor_count + 1  # the count, and a half pair behind it
    assert takes_block_kernel(S, 1152, 1152, True, False, DEFAULT, nbatch) and not takes_block_kernel(S, 1152, 1152, True, False, DEFAULT, 1031)
    g = torch.Generator(device=dev()).manual_seed(5)
    Q, K, V = (torch.randn(nbatch, S, 384, generator=g, device=dev()) for _ in range(3))
    for sh in (False, True):
        assert same_bits(launch(Q, K, V, sh, ctk_option, DEFAULT), launch(Q, K, V, sh, ctk_option, WAVE)), sh
    Q, K, V = operands(1031)[0]
    assert same_bits(launch(Q, K, V, True, ctk_option, DEFAULT), launch(Q, K, V, True, ctk_option, NEW))


def test_option_range():
    """0 .. 3 are values of the option; 1 stays the default (tests/test_cabi_and_host.py pins it)."""
    from cotracker_amd import _lib
    lib = _lib.load()
    for v in (0, 2, 3, 1):
        assert lib.ctk_set_option(_lib.OPT_ATTENTION_TIME_PERSISTENT, v) == 0
    assert lib.ctk_set_option(_lib.OPT_ATTENTION_TIME_PERSISTENT, 4) == -2 and lib.ctk_set_option(_lib.OPT_ATTENTION_TIME_PERSISTENT, -1) == -2
