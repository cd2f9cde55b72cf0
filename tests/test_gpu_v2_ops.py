"""The row kernels of the CoTracker2 iteration (co-tracker_amd/csrc/v2ops.hip), one by one, against float64:
ctk_v2_assemble, ctk_v2_apply_delta, ctk_v2_vis_head, through their front ends in cotracker_amd.ops.  The CoTracker2 goldens reach
them at one S and one N; here S != N, every input carries (t, n, c) in its value (each has its own layout, so a transposed row
cannot pass), the row count is not a multiple of the rows per workgroup, and the leading dimensions take every value the
entry points allow."""
import numpy as np
import pytest
import torch

from ctk_support import dev, same_bits

pytestmark = pytest.mark.gpu


# ---- token assembly --------------------------------------------------------------------------------------------------------------
def assemble_inputs(S, N, flow_scale, seed):
    """Values that name their own index: fcorrs [N,S,196] = n + t/32 + c/8192, track_feat [S,N,128] = -(t + n/512 + c/65536)
    (all exact in float32), mask and vis patterns of (t, n); random coords and positional embedding."""
    g = torch.Generator().manual_seed(seed)
    t, n = torch.arange(S).float(), torch.arange(N).float()
    coords = torch.rand(1, N, 2, generator=g) * 60.0 + (torch.rand(S, N, 2, generator=g) * 2.0 - 1.0) * flow_scale
    fcorrs = n[:, None, None] + t[None, :, None] / 32.0 + torch.arange(196).float()[None, None, :] / 8192.0
    feat = -(t[:, None, None] + n[None, :, None] / 512.0 + torch.arange(128).float()[None, None, :] / 65536.0)
    mask = ((t[:, None] + n[None, :]) % 2).contiguous()
    vis = (0.25 * t[:, None] - 0.125 * n[None, :]).contiguous()
    pos = torch.rand(N, 456, generator=g) * 2.0 - 1.0
    return coords.contiguous(), fcorrs.contiguous(), feat.contiguous(), mask, vis, pos


def assemble_reference(coords, fcorrs, feat, mask, vis, pos, in_ld):
    """cotracker.py:135-150 without the time embedding.  flows = coords - coords[0] and the argument flows * div of
    get_2d_embedding (embeddings.py:87-120, div = arange(0, 64, 2) * (1000 / 64)) in float32, sin / cos of that float32 value in
    float64; cat(flows 2 | pe_x 64 | pe_y 64 | fcorrs 196 | track_feat 128 | mask | vis) + pos[n]; row n*S + t.
    Returns (float32 reference with the exact columns, float64 reference, mask of the sin / cos columns)."""
    S, N = coords.shape[:2]
    flows = coords - coords[0:1]                                                    # float32
    div = torch.arange(0, 64, 2).float() * float(np.float32(1000.0 / 64.0))        # 15.625: exact
    x64 = torch.zeros(S, N, in_ld, dtype=torch.float64)
    x32 = torch.zeros(S, N, in_ld, dtype=torch.float32)
    x32[..., 0:2] = flows + pos[None, :, 0:2]
    for a in range(2):
        arg = (flows[..., a: a + 1] * div).double()                                 # the product is rounded to float32 first
        x64[..., 2 + 64 * a: 66 + 64 * a: 2] = torch.sin(arg)
        x64[..., 3 + 64 * a: 67 + 64 * a: 2] = torch.cos(arg)
    x64[..., 2:130] += pos[None, :, 2:130].double()
    x32[..., 130:326] = fcorrs.permute(1, 0, 2) + pos[None, :, 130:326]
    x32[..., 326:454] = feat + pos[None, :, 326:454]
    x32[..., 454] = mask + pos[None, :, 454]
    x32[..., 455] = vis + pos[None, :, 455]
    trig = torch.zeros(in_ld, dtype=torch.bool)
    trig[2:130] = True
    x64[..., ~trig] = x32[..., ~trig].double()
    rows = lambda x: x.permute(1, 0, 2).reshape(N * S, in_ld)                       # noqa: E731  row n*S + t
    return rows(x32), rows(x64), trig


@pytest.mark.parametrize("in_ld", [480, 512])
@pytest.mark.parametrize("S,N,flow_scale", [(1, 1, 3.0), (8, 5, 3.0), (16, 257, 3.0), (3, 64, 3.0), (8, 5, 100.0)])
def test_v2_assemble(S, N, flow_scale, in_ld):
    """flow_scale 100: arguments of sin / cos up to ~1e5 rad, where a fast-math sinf or a contracted flows * div would show."""
    from cotracker_amd import ops
    inp = assemble_inputs(S, N, flow_scale, S * 1000 + N)
    ref32, ref64, trig = assemble_reference(*inp, in_ld)
    d = [a.to(dev()) for a in inp]
    x = ops.v2_assemble(*d, in_ld, False)
    got = x.cpu()
    assert got.shape == (N * S, in_ld)
    assert same_bits(got[:, ~trig], ref32[:, ~trig]), (S, N, in_ld)                  # exact columns, the zero padding among them
    assert int(got[:, 456:].view(torch.int32).abs().max()) == 0
    err = float((got.double() - ref64)[:, trig].abs().max())
    assert err <= 1e-6, (S, N, in_ld, err)
    if flow_scale > 50:
        assert float((inp[0] - inp[0][0:1]).abs().max()) * 15.625 * 62 > 5e4           # the large arguments are really there
    sh = ops.v2_assemble(*d, in_ld, True)
    assert same_bits(sh, ops.split_rows(x)), (S, N, in_ld)
    assert same_bits(ops.v2_assemble(*d, in_ld, False), x) and same_bits(ops.v2_assemble(*d, in_ld, True), sh)


# ---- state update ----------------------------------------------------------------------------------------------------------------
def apply_delta_raw(delta, coords, gamma, beta, eps=1e-5):
    """ops.v2_apply_delta, but the normalised rows start as NaN so a row that is never written shows."""
    import ctypes as C
    from cotracker_amd import _lib as L
    from cotracker_amd import ops
    S, N = coords.shape[:2]
    normed = torch.full((S * N, 128), float("nan"), device=dev(), dtype=torch.float32)
    L.check(L.load().ctk_v2_apply_delta(S, N, C.c_void_p(delta.data_ptr()), delta.shape[1], C.c_void_p(coords.data_ptr()),
                                        C.c_void_p(gamma.data_ptr()), C.c_void_p(beta.data_ptr()), eps, C.c_void_p(normed.data_ptr()),
                                        ops._stream()), "ctk_v2_apply_delta")
    return normed


@pytest.mark.parametrize("out_ld", [130, 160, 192])
@pytest.mark.parametrize("S,N", [(1, 1), (3, 1), (5, 7), (16, 257)])
def test_v2_apply_delta(S, N, out_ld):
    """cotracker.py:157-167: coords += delta[:, :2] (float32, in place: two calls are two steps) and GroupNorm(1, 128) of the 128
    feature deltas in float64.  delta rows are n*S + t, the normalised rows t*N + n; columns beyond 130 are NaN (never read)."""
    from cotracker_amd import ops
    g = torch.Generator().manual_seed(S * 100 + N + out_ld)
    R = S * N
    delta = torch.full((R, out_ld), float("nan"))
    delta[:, :2] = torch.randn(R, 2, generator=g)
    spread = 0.5 + torch.arange(R).float()[:, None] % 7                          # a different scale and offset per row
    delta[:, 2:130] = torch.randn(R, 128, generator=g) * spread + (torch.arange(R).float()[:, None] % 5 - 2.0)
    if R >= 3:
        delta[0, 2:130] = 1000.0 + torch.randn(128, generator=g)                 # offset 1e3, spread 1: the float32 row sum rounds at 1e3
        delta[1, 2:130] = 0.75                                                   # a constant row: variance 0 -> beta
        # the same offset on a grid of 1/16, where even a float32 sum is exact: this row isolates the two-pass variance
        # (E[x^2] - mean^2 in float32 would lose every digit here)
        delta[2, 2:130] = 1000.0 + torch.randint(-48, 49, (128,), generator=g).float() / 16.0
    if R > 40:
        delta[R - 1, 2:130] = -1000.0 + 0.1 * torch.randn(128, generator=g)      # offset 1e4 times the spread, in the last workgroup
    gamma, beta = torch.randn(128, generator=g), torch.randn(128, generator=g)
    coords = torch.randn(S, N, 2, generator=g) * 30.0
    step = delta[:, :2].view(N, S, 2).permute(1, 0, 2)                            # [S,N,2]
    d64 = delta[:, 2:130].double().view(N, S, 128).permute(1, 0, 2).reshape(R, 128)   # row t*N + n
    mu = d64.mean(dim=1, keepdim=True)
    var = ((d64 - mu) ** 2).mean(dim=1, keepdim=True)
    ref = (d64 - mu) / torch.sqrt(var + float(np.float32(1e-5))) * gamma.double() + beta.double()
    dd, cd, gd, bd = delta.to(dev()), coords.to(dev()), gamma.to(dev()), beta.to(dev())
    normed = apply_delta_raw(dd, cd, gd, bd)
    assert same_bits(cd.cpu(), coords + step), (S, N, out_ld)
    got = normed.cpu().double()
    assert torch.isfinite(got).all()
    # the kernel's documented limit (include/ctk.h): 2e-6 max|ref|, plus the rounding of the 7-level float32 sum behind the row
    # mean, <= 2^-21 |mean| rstd |gamma| -- below 1e-6 on ordinary rows, up to 5e-4 |gamma| on the offset-1e3 row (measured ~5e-5)
    rstd = 1.0 / torch.sqrt(var + float(np.float32(1e-5)))
    tol = 2e-6 * float(ref.abs().max()) + 2.0 ** -21 * mu.abs() * rstd * gamma.double().abs()[None, :]
    over = (got - ref).abs() - tol
    assert float(over.max()) <= 0.0, (S, N, out_ld, float(over.max()), np.unravel_index(int(over.argmax()), over.shape))
    strict = mu.abs()[:, 0] <= 10.0                                             # ordinary rows: the plain bound alone
    if R >= 3:
        strict[(2 % S) * N + 2 // S] = True                                      # and the grid row (delta row 2), whose float32 sum is exact
    assert float((got - ref)[strict].abs().max()) <= 2e-6 * float(ref.abs().max()), (S, N, out_ld)
    if R >= 3:
        assert float((got[N if S > 1 else 1] - beta.double()).abs().max()) <= 1e-6   # delta row 1 = (n 0, t 1) -> row 1*N + 0 (S > 1)
    normed2 = ops.v2_apply_delta(dd, cd, gd, bd)                                  # the front end; the second step on coords
    assert same_bits(normed2, normed)
    assert same_bits(cd.cpu(), (coords + step) + step), (S, N, out_ld)


# ---- visibility head -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 5, 4097])
def test_v2_vis_head(R):
    """vis_predictor (cotracker.py:81-83, 172): <track_feat[r], w> + b in float64.  The kernel accumulates in f64 too, so the
    result is the rounded exact value: one float32 ulp of the logit, however large the terms that cancel in it (a float32 sum
    would be held to 1e-6 sum|tf w|, which is 1e-4 on real rows); the bias is far above either bound."""
    from cotracker_amd import ops
    g = torch.Generator().manual_seed(R)
    tf = torch.randn(1, R, 128, generator=g) * (1.0 + torch.arange(R).float()[None, :, None] % 3)
    w, b = torch.randn(128, generator=g), torch.tensor([0.37])
    ref = (tf.double() * w.double()).sum(dim=-1) + b.double()
    terms = (tf.double() * w.double()).abs().sum(dim=-1)
    bound = 2.0 ** -23 * ref.abs() + 1e-9 * terms
    assert float(bound.max()) < 1e-4 and (R == 1 or float((terms / ref.abs().clamp_min(1e-3)).max()) > 100)   # rows that cancel heavily
    d = [a.to(dev()) for a in (tf, w, b)]
    out = ops.v2_vis_head(*d)
    assert out.shape == (1, R)
    assert bool(((out.cpu().double() - ref).abs() <= bound).all()), float(((out.cpu().double() - ref).abs() / bound).max())
    assert same_bits(ops.v2_vis_head(*d), out)
    for r in sorted({0, R // 2, R - 1}):
        assert same_bits(ops.v2_vis_head(d[0][:, r: r + 1].contiguous(), d[1], d[2]), out[:, r: r + 1]), (R, r)
