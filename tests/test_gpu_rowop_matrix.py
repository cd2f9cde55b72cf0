"""The CoTracker3 row kernels (csrc/rowops.hip), the whole contract: LayerNorm (single and DUAL), token assembly (single and joint),
virtual-token broadcast and the output heads with the fused state update (single and joint), each on its own (-m gpu).

Every kernel is reached through the entry point that makes exactly its launch (ctk_layernorm, ctk_layernorm_dual,
ctk_assemble_tokens_batch, ctk_virtual_init, ctk_heads_update; raw calls in ctk_support, every pointer the test's own).  On every
launch of this module
  - every operand lies inside an allocation filled with the NaN pattern 0x7FC17FC1 (NaN as one f32 and as two f16), and so does
    every output: after the launch the frame is bit-unchanged outside the documented output and the output holds no NaN (rows
    poisoned on purpose aside).  The frames are wider than one workgroup's reach: 16 rows of 384 for LayerNorm and the heads, 256
    threads x 8 columns = 22 rows of `ld` for the assembly;
  - the profile recorder must show ONE row, `layernorm`, `assemble_tokens`, `virtual_init` or `heads_update`;
  - the launch is repeated into fresh memory and must give the same bits.

LayerNorm, R in {1, 2, 7, 8, 9, 15, 16, 17, 263} x affine x {f32, SH} x {single, DUAL} (two rows share a 64-lane wave; odd R
retires half a wave):
  - fp64 (F.layer_norm in float64 on the CPU) on the project's distribution 3 randn + 0.5 at the project's bounds, 5e-6 f32 and
    8e-6 SH; on four ill-conditioned classes (mean 1e3 / sigma 1e-2, mean 1e4 / sigma 1, sigma 1e-4, sigma 1e4) within 4 x the error
    of torch's float32 CPU layer_norm on the same rows (measured in the test; the margin is for the other summation tree), SH
    + 2^-21 |ref|;
  - the SH output is ops.split_rows of the f32 output, as halves, on every case and with gamma up to 1e3 on a spike row (|y| = 1.96e4);
  - DUAL's y / y2 are the bits of ctk_layernorm(gamma, beta, eps) / ctk_layernorm(None, None, eps2), eps / eps2 = 1e-5 / 1e-6 and
    1e-2 / 1e-6;
  - a row replaced by NaN, Inf or 1e30 -- lower half of a wave, upper half, last row of an odd R -- changes no bit of another row;
    16 rows rotated through all 16 slots keep their bits (no dependence on slot or wave-mate);
  - constant rows c in {0, 1, -2, 2^-10, 2^10} give exactly 0 (exactly beta with affine); alternating +-1 gives |y| within 1 ulp of
    fl(1 / sqrtf(1 + eps)) and y[c] == -y[c ^ 1] bit for bit.
Heads, exact integers (tokens and head_w in [-4, 4] with one |w| = 4, head_b in [-64, 64], state in [-1000, 1000]; every sum is
below 384 * 16 + 64 + 1000 < 2^24, exact in f32 in any order; reference int64 on the CPU, torch.equal): (S, N) in (1,1), (8,1),
(3,5), (7,9), (8,12), (13,1263) -- 16419 rows = 2048 x 8 + 35, the second pass of the grid-stride loop -- as delta only, state only
and both (delta == the state's change); joint at B in {2, 3, 16} with separately allocated, framed state per video, and B = 2 past
16384 rows.  Then randn per instantiation against float64 at 20 * 2^-24 * (sum |x w| + |b|) per output (+ 2^-24 |new value| for the state).
Assembly, S in {1, 2, 3, 8, 16} x N in {1, 5, 33} x {(CTK_X_LD, CTK_X_VIS), (CTK_XF_LD, CTK_XF_SMALL)} x {f32, SH} x B in {1, 2, 16}
(B = 16 at S = 3 / N = 5): the reference is the reference model's own float32 chain in numpy float32 (sub, / scale, * 2^deg,
+ f32(pi/2)), then sin in float64 OF THAT float32 ARGUMENT: only sinf differs.  vis / conf, the 4 raw relative columns and the ten
+0 columns are exact, every word outside [base, base + 96) keeps its bits, SH is the split of f32, the joint kernel's rows are the
bits of B single calls, a missing neighbour frame gives the columns of rel = 0, NaN coordinates on one track stay in that track's
rows.  Sine columns: 2.5e-7 absolute at small (|dc| <= 2), large (3e2) and off-frame (3e4: arguments to 1e7) motions; torch's
float32 CPU sin on the same arguments is checked against the same bound first (it measures 3.6e-8 at every magnitude).
Virtual init, S in {1, 3, 8, 16} x B in {1, 2, 3, 16}: the table v * 384 + c (exact), dst torch.equal to the broadcast.

Observed on an MI355X: all 231 tests pass, every exact assertion without a tolerance, every canary intact; the matrix found no fault
in rowops.hip.  What it did find is in the entry points: none of them checked alignment although every kernel here moves 16 bytes
at a time -- ctk_layernorm, ctk_assemble_tokens, the window calls (head_w, virtual_tokens, ctx_gamma / ctx_beta) and
ctk_update_former (delta) now answer CTK_E_ALIGN before any launch (tests/test_rowop_cabi.py).  Measured, kernel | torch float32 CPU
on the same operands (profiles/rowop_matrix_errors.json has every number):
  LayerNorm f32 output, plain / affine: project 5.3e-7 | 6.4e-7 / 1.2e-6 | 1.4e-6 (SH 7.7e-7 / 1.4e-6); mean 1e3 sigma 1e-2
    1.25e-2 | 9.3e-3 / 3.2e-2 | 2.4e-2; mean 1e4 sigma 1 1.1e-3 | 1.6e-3 / 3.1e-3 | 4.0e-3; sigma 1e-4 5.0e-8 | 5.0e-8 / 1.3e-7 | 1.3e-7
    (SH 7.8e-8 / 3.6e-7); sigma 1e4 5.6e-7 | 5.6e-7 / 1.2e-6 | 1.2e-6 (SH 1.0e-6 / 1.4e-6).  The ill-conditioned classes lose what
    float32 loses on x - mean; the kernel is never above 1.35 x torch.
  Heads: delta at 16419 rows 6.1e-7 | 1.2e-6 (smallest bound 1.2e-5); state, single 3.6e-6 and joint 3.8e-6 (coordinates of size 1e2:
    their own rounding; delta alone | 6.4e-7, 7.0e-7).
  Assembly, sinf: small 6.2e-8 | 3.6e-8 (arguments to 3.4e2), large 6.9e-8 | 3.6e-8 (5.1e4), off-frame 6.9e-8 | 3.5e-8 (9.9e6): the
    device sinf reduces large arguments properly, the bound holds at every magnitude and include/ctk.h says so.
The module takes 3.6 s for the pytest process, 1.6 s behind its set-up; no test above 0.4 s.
Planted faults (scratch copies of the library, one line of rowops.hip each, the module run once against each; the JSON lists the
failing cases) -- all caught, each by an exact mismatch:
  1. ctk_half_sum starting at o = 32: 123 tests -- every LayerNorm case with R >= 2 (a row takes in its wave-mate: row isolation,
     slots, exact values, fp64) and, as the heads use the same sum, the integer heads at more than one row;
  2. the SH store's `odd ? hi : lo` swapped: 62 tests, every SH LayerNorm case (SH != split of f32, fp64);
  3. DUAL's second store with eps: 40 tests, every DUAL case (y2 != ctk_layernorm(None, None, eps2)) and the exact values;
  4. heads update with sn = n*S + t: HeadsOne 9 tests (state and both at every (S, N) with S, N > 1; fp64 state), HeadsBatch 5 tests
     (every joint case; fp64 batch);
  5. assemble's comp < 2 turned to comp >= 2: 55 tests (every matrix case with S >= 2, the NaN track, the three sine classes);
  6. virtual_init's divisor without * S: 12 tests, every case with S > 1.
Argument rules, CTK_E_ALIGN included: tests/test_rowop_cabi.py, on the CPU; no case here relies on a rejection.
Not tested: R beyond a launch's grid limit, a sanitizer run, the ISA.
"""
import functools
import json
import os
import time

import numpy as np
import pytest
import torch

from ctk_support import (NAN_PATTERN, assemble_raw, bits, dev, frame_intact, heads_raw, layernorm_raw, nan_framed, recorded,
                         same_bits, virtual_init_raw)

pytestmark = pytest.mark.gpu

HID, VIRT = 384, 64
ROWS16 = 16 * HID      # frame of the 384-column operands: 16 rows, two workgroups' reach
SMALL = 4096           # frame of the small operands (gamma, beta, head_w, head_b, the state), in elements
ERRORS = {"layernorm": {}, "heads": {}, "assemble": {}}


def canary(n_words, pad):
    """-> (the allocation of n_words + 2 pad NaN-pattern words, its middle n_words as int32)."""
    assert pad % 4 == 0
    flat = torch.full((n_words + 2 * pad,), NAN_PATTERN, dtype=torch.int32, device=dev())
    return flat, flat[pad:pad + n_words]


def framed_ok(flat, body, what):
    pad = (flat.numel() - body.numel()) // 2
    assert bool((flat[:pad] == NAN_PATTERN).all()), f"{what}: a store in front of the output"
    assert bool((flat[pad + body.numel():] == NAN_PATTERN).all()), f"{what}: a store behind the output"


def put(x, pad=SMALL):
    return None if x is None else nan_framed(x.contiguous().float(), pad, NAN_PATTERN)


def split_rows(x):
    from cotracker_amd import ops
    return ops.split_rows(x.contiguous())


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------------
LN_R = (1, 2, 7, 8, 9, 15, 16, 17, 263)


def ln_once(x, gamma, beta, eps, split, eps2, poisoned):
    R = x.shape[0]
    outs = [canary(R * HID, ROWS16) for _ in range(1 if eps2 is None else 2)]
    rc, rows = recorded(lambda: layernorm_raw(x, outs[0][1], R, gamma, beta, eps, split, None if eps2 is None else outs[1][1],
                                              0.0 if eps2 is None else eps2))
    assert rc == 0 and rows == {"layernorm": 1}, (rc, rows)
    ys = []
    for k, (flat, body) in enumerate(outs):
        framed_ok(flat, body, f"layernorm R={R} split={split} output {k}")
        y = body.view(torch.float16).view(R, HID // 32, 2, 32) if split else body.view(torch.float32).view(R, HID)
        clean = [r for r in range(R) if r not in poisoned]
        assert not bool(torch.isnan(y[clean]).any()), f"layernorm R={R}: NaN in the output (a read outside x, or an element never written)"
        ys.append(y)
    return ys


def ln(x, gamma=None, beta=None, eps=1e-6, split=False, eps2=None, poisoned=()):
    """x [R,384] (CPU) -> [y] or [y, y2] (DUAL when eps2 is given) on the device; launched twice into fresh memory: the same bits."""
    xd, gd, bd = put(x, ROWS16), put(gamma), put(beta)
    first = ln_once(xd, gd, bd, eps, split, eps2, poisoned)
    again = ln_once(xd, gd, bd, eps, split, eps2, poisoned)
    for a, b in zip(first, again):
        assert same_bits(a, b), "a second launch gives other bits"
    return first


def ln_ref(x, gamma, beta, eps):
    return torch.nn.functional.layer_norm(x.double(), (HID,), None if gamma is None else gamma.double(),
                                          None if beta is None else beta.double(), eps)


def unsplit(y):
    return (y[:, :, 0].float().double() + y[:, :, 1].float().double()).reshape(y.shape[0], -1).cpu()


def as_f64(y, split):
    return unsplit(y) if split else y.double().cpu()


def held(v, split):
    """The float32 vector v [384] as an output row of the format holds it, in float64 (SH: hi + lo of its split)."""
    return unsplit(split_rows(v.float().view(1, HID).to(dev())))[0] if split else v.double()


@functools.lru_cache(maxsize=None)
def ln_operands(R, affine):
    g = torch.Generator().manual_seed(1000 + R)
    x = torch.randn(R, HID, generator=g) * 3 + 0.5
    return x, (torch.randn(HID, generator=g) if affine else None), (torch.randn(HID, generator=g) if affine else None)


@pytest.mark.parametrize("dual", [False, True], ids=["single", "dual"])
@pytest.mark.parametrize("split", [False, True], ids=["f32", "sh"])
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("R", LN_R)
def test_layernorm_matrix(R, affine, split, dual):
    x, gamma, beta = ln_operands(R, affine)
    bound = 8e-6 if split else 5e-6
    for eps, eps2 in ((1e-5, 1e-6), (1e-2, 1e-6)) if dual else ((1e-5 if affine else 1e-6, None),):
        y = ln(x, gamma, beta, eps, split)[0]
        err = float((as_f64(y, split) - ln_ref(x, gamma, beta, eps)).abs().max())
        assert err < bound, (R, affine, split, eps, err)
        if split:
            assert same_bits(y, split_rows(ln(x, gamma, beta, eps, False)[0])), "the SH output is not the split of the f32 output"
        if dual:
            d, d2 = ln(x, gamma, beta, eps, split, eps2)
            y2 = ln(x, None, None, eps2, split)[0]
            assert same_bits(d, y), f"DUAL y differs from ctk_layernorm(gamma, beta, {eps})"
            assert same_bits(d2, y2), f"DUAL y2 differs from ctk_layernorm(None, None, {eps2})"
            err2 = float((as_f64(d2, split) - ln_ref(x, None, None, eps2)).abs().max())
            assert err2 < bound, (R, affine, split, eps2, err2)


@pytest.mark.parametrize("split", [False, True], ids=["f32", "sh"])
@pytest.mark.parametrize("dual", [False, True], ids=["single", "dual"])
@pytest.mark.parametrize("R,victim", [(7, 6), (8, 2), (8, 3), (9, 8), (9, 4), (17, 16), (17, 11), (2, 0), (2, 1)])
def test_layernorm_row_isolation(R, victim, dual, split):
    """A poisoned row stays in its row: lower half of a wave (even index), upper half (odd), the last row of an odd R (alone in its wave)."""
    x, gamma, beta = ln_operands(R, True)
    eps, eps2 = 1e-5, (1e-6 if dual else None)
    clean = ln(x, gamma, beta, eps, split, eps2)
    others = [r for r in range(R) if r != victim]
    for name, value in (("nan", float("nan")), ("inf", float("inf")), ("-inf", float("-inf")), ("1e30", 1e30)):
        xp = x.clone()
        xp[victim] = value
        got = ln(xp, gamma, beta, eps, split, eps2, poisoned=(victim,))
        for k, (a, b) in enumerate(zip(got, clean)):
            assert same_bits(a[others], b[others]), f"R={R}: row {victim} = {name} changed another row of output {k}"
            row = as_f64(a[victim:victim + 1], split)[0]
            if name == "1e30":  # a constant row: sum and mean exact, y exactly 0 (beta)
                assert torch.equal(row, held(beta, split) if k == 0 else torch.zeros(HID, dtype=torch.float64)), (R, victim, k)
            else:
                assert not bool(torch.isfinite(row).any()), f"R={R}: row {victim} = {name} has finite outputs"
    xp = x.clone()
    xp[victim, 77] = float("inf")  # one element: the mean is inf, every element of the row is NaN
    got = ln(xp, gamma, beta, eps, split, eps2, poisoned=(victim,))
    for a, b in zip(got, clean):
        assert same_bits(a[others], b[others]) and not bool(torch.isfinite(as_f64(a[victim:victim + 1], split)).any())


@pytest.mark.parametrize("split", [False, True], ids=["f32", "sh"])
@pytest.mark.parametrize("dual", [False, True], ids=["single", "dual"])
def test_layernorm_rows_do_not_depend_on_their_slot(dual, split):
    x, gamma, beta = ln_operands(16, True)
    base = ln(x, gamma, beta, 1e-5, split, 1e-6 if dual else None)
    for s in range(1, 16):  # row i moves to slot (i + s) % 16: every row visits every slot, odd s changes its wave-mate
        got = ln(torch.roll(x, s, 0), gamma, beta, 1e-5, split, 1e-6 if dual else None)
        for a, b in zip(got, base):
            assert same_bits(a, torch.roll(b, s, 0)), f"rotation by {s}: a row's bits depend on its slot or its wave-mate"


@pytest.mark.parametrize("split", [False, True], ids=["f32", "sh"])
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
def test_layernorm_exact_values(affine, split):
    consts = (0.0, 1.0, -2.0, 2.0 ** -10, 2.0 ** 10)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(9, HID, generator=g)
    for r, c in enumerate(consts):
        x[r] = c
    alt = torch.tensor([1.0, -1.0]).repeat(HID // 2)
    x[5], x[6] = alt, -alt   # row 7, 8: random (8 is the odd last row)
    gamma, beta = (torch.randn(HID, generator=g), torch.randn(HID, generator=g)) if affine else (None, None)
    for eps, eps2 in ((1e-5, 1e-6), (1e-2, 1e-6)):
        for k, y in enumerate(ln(x, gamma, beta, eps, split, eps2)):
            e = eps if k == 0 else eps2
            v = as_f64(y, split)
            want = held(beta, split) if (affine and k == 0) else torch.zeros(HID, dtype=torch.float64)
            for r, c in enumerate(consts):
                assert torch.equal(v[r], want), f"constant row {c}: output {k} is not exactly {'beta' if affine and k == 0 else '0'}"
            if affine and k == 0:
                continue
            # mean 0 and var 1 exactly: y = +-fl(1 / sqrtf(fl(1 + eps))); the f32 output to 1 ulp, the SH one carries >= 21 bits
            r32 = np.float32(1.0) / np.sqrt(np.float32(1.0) + np.float32(e))
            tol = float(np.spacing(r32)) if not split else float(r32) * 2.0 ** -21
            for r, sign in ((5, alt), (6, -alt)):
                assert float((v[r] - sign.double() * float(r32)).abs().max()) <= tol, (k, r, e)
            flip = (-y[5:7]).view(2, 12, 2, 16, 2).flip(4).reshape(2, 12, 2, 32) if split else (-y[5:7]).view(2, HID // 2, 2).flip(2).reshape(2, HID)
            assert same_bits(y[5:7], flip), "y[c] != -y[c ^ 1] on the alternating rows"


def test_layernorm_sh_is_the_split_at_the_top_of_the_f16_range():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(17, HID, generator=g) * 3 + 0.5
    x[3] = 0.0
    x[3, 200] = 5.0     # a spike row: the normalised spike is sqrt(383) = 19.57
    x[16] = 0.0
    x[16, 1] = -2.0     # ... in the half-wave that is alone in its wave
    gamma = (torch.randn(HID, generator=g) * 300).clamp(-1e3, 1e3)
    gamma[200], gamma[1] = 1e3, -1e3
    beta = torch.randn(HID, generator=g) * 10
    y, y2 = ln(x, gamma, beta, 1e-5, False, 1e-6)
    s, s2 = ln(x, gamma, beta, 1e-5, True, 1e-6)
    assert 1.9e4 < float(y.abs().max()) < 2.1e4
    assert same_bits(s, split_rows(y)) and same_bits(s2, split_rows(y2))
    assert same_bits(ln(x, gamma, beta, 1e-5, True)[0], s)


LN_CLASSES = {"project": (0.5, 3.0), "mean1e3_sigma1e-2": (1e3, 1e-2), "mean1e4_sigma1": (1e4, 1.0), "sigma1e-4": (0.0, 1e-4),
              "sigma1e4": (0.0, 1e4)}


@pytest.mark.parametrize("cls", list(LN_CLASSES))
def test_layernorm_fp64_classes(cls, capsys):
    mean, sigma = LN_CLASSES[cls]
    g = torch.Generator().manual_seed(42)
    x = torch.randn(263, HID, generator=g) * sigma + mean
    gamma, beta = torch.randn(HID, generator=g), torch.randn(HID, generator=g)
    rec = {}
    for name, ga, be, eps in (("plain", None, None, 1e-6), ("affine", gamma, beta, 1e-5)):
        ref = ln_ref(x, ga, be, eps)
        torch_f32 = float((torch.nn.functional.layer_norm(x, (HID,), ga, be, eps).double() - ref).abs().max())
        y = ln(x, ga, be, eps, False)[0]
        s = ln(x, ga, be, eps, True)[0]
        assert same_bits(s, split_rows(y))
        e32, esh = float((y.double().cpu() - ref).abs().max()), float((unsplit(s) - ref).abs().max())
        over_sh = float(((unsplit(s) - ref).abs() - 2.0 ** -21 * ref.abs()).max())
        rec[name] = dict(torch_f32_cpu_err=float(f"{torch_f32:.3e}"), kernel_f32_err=float(f"{e32:.3e}"), kernel_sh_err=float(f"{esh:.3e}"),
                         max_ref=float(f"{float(ref.abs().max()):.4g}"))
        with capsys.disabled():
            print(f"\nlayernorm-error {cls} {name}: {rec[name]}")
        if cls == "project":
            assert e32 < 5e-6 and esh < 8e-6, (cls, name, rec[name])
        else:
            assert e32 <= 4 * torch_f32, (cls, name, rec[name])
            assert over_sh <= 4 * torch_f32, (cls, name, rec[name], over_sh)
    ERRORS["layernorm"][cls] = rec


# ---- heads ----------------------------------------------------------------------------------------------------------------------------------
def heads_once(S, N, tok, hw, hb, states, want_delta):
    rows = len(states) * S * N
    st_dev, st_flat = [], []
    for st in states:
        if st is None:
            st_dev.append((None, None, None))
            continue
        pairs = [nan_framed(t_.contiguous(), SMALL, NAN_PATTERN, whole=True) for t_ in st]
        st_dev.append(tuple(p[0] for p in pairs))
        st_flat.append(pairs)
    dflat, dbody = canary(rows * 4, SMALL) if want_delta else (None, None)
    rc, rec = recorded(lambda: heads_raw(st_dev, S, N, tok, hw, hb, dbody))
    assert rc == 0 and rec == {"heads_update": 1}, (rc, rec)
    delta = None
    if want_delta:
        framed_ok(dflat, dbody, f"heads S={S} N={N}: delta")
        delta = dbody.view(torch.float32).view(rows, 4)
        assert not bool(torch.isnan(delta).any()), "NaN in delta"
    for b, pairs in enumerate(st_flat):
        for (view, flat), name in zip(pairs, ("coords", "vis", "conf")):
            assert frame_intact(flat, view), f"heads S={S} N={N}: a store outside video {b}'s {name}"
            assert not bool(torch.isnan(view).any()), f"NaN in video {b}'s {name}"
    return delta, st_dev


def heads(S, N, tokens, hw, hb, states, want_delta):
    """states: per video (coords [S,N,2], vis [S,N], conf [S,N]) on the CPU, or None (delta only) -> (delta or None, the new state
    per video); two launches on fresh copies of the state: the same bits."""
    tok, hwd, hbd = put(tokens, ROWS16), put(hw), put(hb)
    d1, s1 = heads_once(S, N, tok, hwd, hbd, states, want_delta)
    d2, s2 = heads_once(S, N, tok, hwd, hbd, states, want_delta)
    assert d1 is None or same_bits(d1, d2), "a second launch gives another delta"
    for a, b in zip(s1, s2):
        assert all(x is None or same_bits(x, y) for x, y in zip(a, b)), "a second launch gives another state"
    return d1, s1


def int_problem(S, N, B, seed):
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(-4, 5, (B * S * N, HID), generator=g).float()
    hw = torch.randint(-4, 5, (4, HID), generator=g).float()
    hw[0, 0] = 4.0
    hb = torch.randint(-64, 65, (4,), generator=g).float()
    states = [(torch.randint(-1000, 1001, (S, N, 2), generator=g).float(), torch.randint(-1000, 1001, (S, N), generator=g).float(),
               torch.randint(-1000, 1001, (S, N), generator=g).float()) for _ in range(B)]
    assert float(hw.abs().max()) == 4.0 and HID * 16 + 64 + 1000 < 2 ** 24
    d = tokens.long() @ hw.long().T + hb.long()       # [rows, 4], row (b*N + n)*S + t
    per = d.view(B, N, S, 4).permute(0, 2, 1, 3)       # [b][t][n]
    want = [(st[0].long() + per[b, :, :, :2], st[1].long() + per[b, :, :, 2], st[2].long() + per[b, :, :, 3]) for b, st in enumerate(states)]
    return tokens, hw, hb, states, d, want


def check_state(got, want, what):
    for b, (g_, w_) in enumerate(zip(got, want)):
        for name, a, r in zip(("coords", "vis", "conf"), g_, w_):
            a = a.double().cpu()
            bad = a != r.double()
            assert torch.equal(a, r.double()), f"{what}: video {b} {name}: {int(bad.sum())} of {bad.numel()} differ; first (t, n) " \
                                               f"{bad.nonzero()[0].tolist()}: {float(a[bad][0])} for {float(r.double()[bad][0])}"


HEADS_SN = ((1, 1), (8, 1), (3, 5), (7, 9), (8, 12), (13, 1263))


@pytest.mark.parametrize("mode", ["delta", "state", "both"])
@pytest.mark.parametrize("S,N", HEADS_SN)
def test_heads_exact_integers(S, N, mode):
    assert S == 1 or N == 1 or S != N
    tokens, hw, hb, states, d, want = int_problem(S, N, 1, S * 100 + N)
    delta, st = heads(S, N, tokens, hw, hb, [None] if mode == "delta" else states, mode != "state")
    if mode != "state":
        got = delta.double().cpu()
        bad = got != d.double()
        assert torch.equal(got, d.double()), f"S={S} N={N}: {int(bad.sum())} delta values differ; first (row, o) {bad.nonzero()[0].tolist()}"
    if mode != "delta":
        check_state(st, want, f"S={S} N={N} {mode}")


@pytest.mark.parametrize("B,S,N", [(2, 7, 5), (3, 7, 5), (16, 7, 5), (2, 13, 640)])
def test_heads_batch_exact_integers(B, S, N):
    tokens, hw, hb, states, d, want = int_problem(S, N, B, B * 1000 + N)
    assert (B, S, N) != (2, 13, 640) or B * S * N > 16384
    _, st = heads(S, N, tokens, hw, hb, states, False)
    check_state(st, want, f"B={B} S={S} N={N}")


@pytest.mark.parametrize("kind", ["one_delta", "one_state", "batch"])
def test_heads_fp64(kind, capsys):
    B, S, N = (3, 7, 9) if kind == "batch" else (1, 13, 1263) if kind == "one_delta" else (1, 7, 9)
    g = torch.Generator().manual_seed(5)
    tokens = torch.randn(B * S * N, HID, generator=g)
    hw, hb = torch.randn(4, HID, generator=g) / HID ** 0.5, torch.randn(4, generator=g)
    states = [(torch.randn(S, N, 2, generator=g) * 30, torch.randn(S, N, generator=g), torch.randn(S, N, generator=g)) for _ in range(B)]
    ref = tokens.double() @ hw.double().T + hb.double()
    mag = tokens.double().abs() @ hw.double().abs().T + hb.double().abs()
    bound = 20 * 2.0 ** -24 * mag
    f32 = tokens @ hw.T + hb
    delta, st = heads(S, N, tokens, hw, hb, [None] if kind == "one_delta" else states, kind == "one_delta")
    rec = dict(rows=B * S * N, torch_f32_cpu_err=float(f"{float((f32.double() - ref).abs().max()):.3e}"), bound_min=float(f"{float(bound.min()):.3e}"))
    if kind == "one_delta":
        err = (delta.double().cpu() - ref).abs()
        rec["kernel_err"] = float(f"{float(err.max()):.3e}")
        ok = bool((err <= bound).all())
    else:
        per, pb = ref.view(B, N, S, 4).permute(0, 2, 1, 3), bound.view(B, N, S, 4).permute(0, 2, 1, 3)
        worst, ok = 0.0, True
        for b in range(B):
            for a, r, lim in ((st[b][0], states[b][0].double() + per[b, :, :, :2], pb[b, :, :, :2]),
                              (st[b][1], states[b][1].double() + per[b, :, :, 2], pb[b, :, :, 2]),
                              (st[b][2], states[b][2].double() + per[b, :, :, 3], pb[b, :, :, 3])):
                err = (a.double().cpu() - r).abs()
                worst = max(worst, float(err.max()))
                ok = ok and bool((err <= lim + 2.0 ** -24 * r.abs()).all())
        rec["kernel_err"] = float(f"{worst:.3e}")
    ERRORS["heads"][kind] = rec
    with capsys.disabled():
        print(f"\nheads-error {kind}: {rec}")
    assert ok, (kind, rec)


# ---- token assembly -------------------------------------------------------------------------------------------------------------------------
X_LD, X_VIS, XF_LD, XF_SMALL = 1120, 1024, 1632, 1536
SCALE = (4.0, 3.0)
SIN_BOUND = 2.5e-7
HALF_PI = np.float32(0.5 * np.pi)


def asm_reference(coords, vis, conf):
    """coords [S,N,2], vis / conf [S,N] float32 numpy -> rows n*S + t: (vis|conf [rows,2], rel [rows,4] float32, the 80 sine ARGUMENTS
    [rows,80] float32: 40 plain, 40 shifted), by the reference model's float32 chain."""
    S, N = vis.shape
    zero = np.zeros((1, N, 2), np.float32)
    with np.errstate(invalid="ignore"):
        fwd = np.concatenate([coords[:-1] - coords[1:], zero], 0)     # c[t] - c[t+1], 0 at t = S - 1
        bwd = np.concatenate([zero, coords[1:] - coords[:-1]], 0)     # c[t] - c[t-1], 0 at t = 0
        rel = (np.concatenate([fwd, bwd], -1) / np.array(SCALE * 2, np.float32)).astype(np.float32)   # [S,N,4]: fwd x, fwd y, bwd x, bwd y
        arg = (rel[:, :, None, :] * (np.float32(2.0) ** np.arange(10, dtype=np.float32))[None, None, :, None]).astype(np.float32)
        arg = arg.reshape(S, N, 40)
        args = np.concatenate([arg, (arg + HALF_PI).astype(np.float32)], -1)

    def rows(a):
        return np.ascontiguousarray(np.swapaxes(a, 0, 1)).reshape(N * S, -1)
    return rows(np.stack([vis, conf], -1)), rows(rel), rows(args)


def asm_once(states_dev, B, S, N, ld, base, split):
    rows = B * N * S
    flat, body = canary(rows * ld, 40960)   # > 256 threads x 8 columns = 21.3 rows of 1632
    rc, rec = recorded(lambda: assemble_raw(states_dev, S, N, SCALE, body, split, ld, base))
    assert rc == 0 and rec == {"assemble_tokens": 1}, (rc, rec)
    framed_ok(flat, body, f"assemble B={B} S={S} N={N} ld={ld}")
    w = body.view(rows, ld)
    assert bool((w[:, :base] == NAN_PATTERN).all()) and bool((w[:, base + 96:] == NAN_PATTERN).all()), "a word outside [base, base + 96) changed"
    out = w[:, base:base + 96].contiguous()
    return out.view(torch.float16).view(rows, 3, 2, 32) if split else out.view(torch.float32)


def assemble(states, ld, base, split):
    """states: per video (coords, vis, conf) float32 numpy -> the 96 written columns, f32 [rows,96] or SH [rows,3,2,32]."""
    S, N = states[0][1].shape
    sd = [tuple(put(torch.from_numpy(np.ascontiguousarray(a)), 8192) for a in st) for st in states]
    first = asm_once(sd, len(states), S, N, ld, base, split)
    assert same_bits(first, asm_once(sd, len(states), S, N, ld, base, split)), "a second launch gives other bits"
    return first


def asm_states(B, S, N, mag, seed):
    r = np.random.RandomState(seed)
    out = []
    for _ in range(B):
        start = r.uniform(-mag, mag, size=(1, N, 2)) if mag > 1e3 else r.uniform(0, 100, size=(1, N, 2))
        c = (start + r.uniform(-mag, mag, size=(S, N, 2))).astype(np.float32) if mag > 1e3 else \
            (start + np.cumsum(r.uniform(-mag, mag, size=(S, N, 2)), 0)).astype(np.float32)
        out.append((c, r.standard_normal((S, N)).astype(np.float32), r.standard_normal((S, N)).astype(np.float32)))
    return out


def asm_check(x, states, what, sin_bound=SIN_BOUND):
    """x f32 [B*N*S, 96] against the reference of every video -> the largest sine error."""
    S, N = states[0][1].shape
    worst = 0.0
    x = x.cpu()
    for b, st in enumerate(states):
        vc, rel, args = asm_reference(*st)
        xb = x[b * N * S:(b + 1) * N * S]
        assert same_bits(xb[:, 0:2], torch.from_numpy(vc)), f"{what}: video {b}: vis / conf are not copies"
        got_rel, want_rel = xb[:, 2:6], torch.from_numpy(rel)
        nan = torch.isnan(want_rel)
        assert torch.equal(torch.isnan(got_rel), nan) and same_bits(torch.where(nan, torch.zeros(()), got_rel), torch.where(nan, torch.zeros(()), want_rel)), \
            f"{what}: video {b}: the raw relative columns are not the float32 sub / div"
        assert bool((bits(xb[:, 86:96]) == 0).all()), f"{what}: video {b}: columns 86..95 are not +0"
        ref = np.sin(args.astype(np.float64))
        got = xb[:, 6:86].double().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: video {b}: NaN where the argument is finite, or the reverse"
        err = np.nan_to_num(np.abs(got - ref), nan=0.0)
        worst = max(worst, float(err.max()))
        assert err.max() <= sin_bound, f"{what}: video {b}: sine error {err.max():.3e} at argument {args.flat[err.argmax()]!r}"
    return worst


ASM_CASES = [(B, S, N) for B in (1, 2) for S in (1, 2, 3, 8, 16) for N in (1, 5, 33)] + [(16, 3, 5)]


@pytest.mark.parametrize("layout", ["x", "xf"])
@pytest.mark.parametrize("B,S,N", ASM_CASES)
def test_assemble_matrix(B, S, N, layout):
    ld, base = (X_LD, X_VIS) if layout == "x" else (XF_LD, XF_SMALL)
    states = asm_states(B, S, N, 2.0, B * 10000 + S * 100 + N)
    x = assemble(states, ld, base, False)
    asm_check(x, states, f"B={B} S={S} N={N} {layout}")
    sh = assemble(states, ld, base, True)
    assert same_bits(sh, split_rows(x)), "the SH form is not the split of the f32 form"
    if B > 1:  # the joint kernel: the bits of B single calls
        for b in range(B):
            assert same_bits(x[b * N * S:(b + 1) * N * S], assemble(states[b:b + 1], ld, base, False)), f"video {b} differs from its single call"
            assert B > 2 or same_bits(sh[b * N * S:(b + 1) * N * S], assemble(states[b:b + 1], ld, base, True))
    vc, rel, args = asm_reference(*states[0])
    first, last = np.arange(N) * S, np.arange(N) * S + S - 1       # rows of t = 0 and of t = S - 1
    xc = x[:N * S].cpu()
    zero_cols = lambda comps: [2 + c for c in comps] + [6 + 4 * d + c for d in range(10) for c in comps]  # noqa: E731
    one_cols = lambda comps: [46 + 4 * d + c for d in range(10) for c in comps]  # noqa: E731
    sin_half_pi = xc[first][:, one_cols((2, 3))]
    assert bool((bits(xc[first][:, zero_cols((2, 3))]) == 0).all()) and bool((bits(xc[last][:, zero_cols((0, 1))]) == 0).all()), \
        "a missing neighbour frame does not give rel = +0 and sin(+0) = +0"
    assert same_bits(xc[last][:, one_cols((0, 1))], sin_half_pi) and bool((sin_half_pi == sin_half_pi[0, 0]).all())
    assert abs(float(sin_half_pi[0, 0]) - 1.0) <= SIN_BOUND
    if S == 1:
        assert bool((bits(xc[:, 2:46]) == 0).all()) and bool((xc[:, 46:86] == sin_half_pi[0, 0]).all())


def test_assemble_thread_tails():
    """S * N * 12 threads: below one workgroup, and past a multiple of 256 by less than a row."""
    tails = {(S, N): (S * N * 12) % 256 for B, S, N in ASM_CASES if B == 1}
    assert tails[(1, 1)] == 12 and tails[(3, 5)] == 180 and tails[(8, 33)] == 96 and tails[(16, 33)] == 192 and tails[(2, 33)] == 24
    assert sum(1 for v in tails.values() if v) >= 12 and 16 * 3 * 5 * 12 % 256 == 64


@pytest.mark.parametrize("cls,mag", [("small", 2.0), ("large", 3e2), ("off_frame", 3e4)])
def test_assemble_sine_by_magnitude(cls, mag, capsys):
    states = asm_states(2, 16, 33, mag, 77)
    worst_arg, torch_err = 0.0, 0.0
    for st in states:   # first, on the CPU: torch's float32 sin on the same arguments stays inside the bound against the same reference
        args = asm_reference(*st)[2]
        worst_arg = max(worst_arg, float(np.abs(args).max()))
        torch_err = max(torch_err, float(np.abs(torch.sin(torch.from_numpy(args)).double().numpy() - np.sin(args.astype(np.float64))).max()))
    assert torch_err <= SIN_BOUND, (cls, torch_err)
    expect = {"small": (1e2, 5e3), "large": (1e4, 5e5), "off_frame": (2e6, 2e7)}[cls]
    assert expect[0] < worst_arg < expect[1], (cls, worst_arg)
    x = assemble(states, XF_LD, XF_SMALL, False)
    rec = dict(max_argument=float(f"{worst_arg:.4g}"), torch_f32_cpu_err=float(f"{torch_err:.3e}"))
    try:
        rec["kernel_err"] = float(f"{asm_check(x, states, cls, sin_bound=float('inf')):.3e}")
    finally:
        ERRORS["assemble"][cls] = rec
        with capsys.disabled():
            print(f"\nassemble-sine {cls}: {rec}")
    assert rec["kernel_err"] <= SIN_BOUND, (cls, rec)
    assert same_bits(assemble(states, XF_LD, XF_SMALL, True), split_rows(x))


@pytest.mark.parametrize("B", [1, 3])
def test_assemble_nan_coords_stay_in_their_track(B):
    S, N, victim = 8, 5, 3
    states = asm_states(B, S, N, 2.0, 5)
    clean = assemble(states, X_LD, X_VIS, False).cpu()
    c = states[B - 1][0].copy()
    c[:, victim] = np.nan
    bad = states[:B - 1] + [(c,) + states[B - 1][1:]]
    got = assemble(bad, X_LD, X_VIS, False).cpu()
    asm_check(got, bad, "NaN track")   # NaN exactly where the reference has it: that track's columns with a neighbour frame
    rows = torch.arange((B - 1) * N * S + victim * S, (B - 1) * N * S + (victim + 1) * S)
    keep = torch.ones(B * N * S, dtype=torch.bool)
    keep[rows] = False
    assert same_bits(got[keep], clean[keep]), "NaN coordinates of one track changed another row"
    mid = got[rows[1:-1]]
    assert bool(torch.isnan(mid[:, 2:86]).all()) and same_bits(mid[:, :2], clean[rows[1:-1]][:, :2]) and bool((bits(mid[:, 86:]) == 0).all())


# ---- virtual init ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 3, 16])
@pytest.mark.parametrize("S", [1, 3, 8, 16])
def test_virtual_init(S, B):
    table = (torch.arange(VIRT).view(VIRT, 1) * HID + torch.arange(HID).view(1, HID)).float()   # distinct, exact
    vt = put(table, ROWS16)                                                                      # an index past the table reads NaN
    want = table.view(1, VIRT, 1, HID).expand(B, VIRT, S, HID).reshape(B * VIRT * S, HID)
    outs = []
    for _ in range(2):
        flat, body = canary(B * VIRT * S * HID, ROWS16)
        rc, rec = recorded(lambda: virtual_init_raw(vt, S, B, body))
        assert rc == 0 and rec == {"virtual_init": 1}, (rc, rec)
        framed_ok(flat, body, f"virtual_init S={S} B={B}")
        outs.append(body.view(torch.float32).view(B * VIRT * S, HID))
    assert torch.equal(outs[0].cpu(), want), f"S={S} B={B}: dst is not the broadcast of the table"
    assert same_bits(outs[0], outs[1])


@pytest.fixture(scope="module", autouse=True)
def error_record():
    """CTK_ROWOP_MATRIX_ERRORS=<file>: the measured errors with their torch-float32 companions and the module's wall time (the
    `measured` part of profiles/rowop_matrix_errors.json)."""
    t0 = time.time()
    yield
    path = os.environ.get("CTK_ROWOP_MATRIX_ERRORS")
    if path and any(ERRORS.values()):
        with open(path, "w") as f:
            json.dump({"module_seconds": float(f"{time.time() - t0:.1f}"), **ERRORS}, f, indent=1)
