"""The encoder's pixel kernels (co-tracker_amd/csrc/encoder.hip), one by one, against a plain reference of the same operation:
ctk_enc_stem_im2col, ctk_enc_inorm_stats, ctk_enc_inorm_apply, ctk_enc_fuse, ctk_enc_l2norm.  The whole-encoder tests see them
in the chain only: test_gpu_parity.py through six more layers and at sizes that are multiples of 16, test_gpu_encoder_stages.py
stage by stage against float64 (also at 70 x 102 and on a constant frame), but always on the activations of a real encoder,
whose mean is about 0; here every kernel gets its own edges (odd sizes, one pixel, the 512-pixel partial-block seam, a channel count that
leaves threads idle, offsets that dominate the spread) and a reference in float64, or in float32 with one torch op per kernel
operation where the kernel promises the same bits.  Every test also asserts that a second call gives the same bits and that
frame f alone gives the bits it has inside a batch."""
import ctypes as C

import numpy as np
import pytest
import torch

from ctk_support import dev, same_bits

pytestmark = pytest.mark.gpu

EPS = float(np.float32(1e-5))  # the kernel receives eps as a float


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _lib():
    from cotracker_amd import _lib as L
    return L, L.load()


def _stream():
    from cotracker_amd import ops
    return ops._stream()


def sh_of(ref_f32_cpu):
    """SH form of a float32 matrix [M, K] (K % 32 == 0) through ctk_split_rows: what every SH-writing kernel must reproduce."""
    from cotracker_amd import ops
    return ops.split_rows(ref_f32_cpu.contiguous().to(dev()))


# ---- stem -----------------------------------------------------------------------------------------------------------------
def stem(frames):
    L, lib = _lib()
    F, _, H, W = frames.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.full((F * Ho * Wo, 5, 2, 32), float("nan"), device=dev(), dtype=torch.float16)
    L.check(lib.ctk_enc_stem_im2col(_p(frames), F, H, W, _p(out), _stream()), "ctk_enc_stem_im2col")
    return out


def stem_reference(frames_cpu):
    """cotracker3_online.py:320 (video = 2 * (video / 255.0) - 1.0, three rounded float32 operations) and the 7x7 stride-2
    pad-3 patches of blocks.py:150-157's conv1 as rows of 160 columns in (ky, kx, c) order, 147 used."""
    F, _, H, W = frames_cpu.shape
    x = frames_cpu / torch.full_like(frames_cpu, 255.0)      # an IEEE division (not a multiplication by 1/255)
    x = x * 2.0
    x = x - 1.0
    cols = torch.nn.functional.unfold(x, 7, padding=3, stride=2)              # [F, 3*49, L] in (c, ky, kx) order, zero padded
    L_ = cols.shape[-1]
    cols = cols.view(F, 3, 7, 7, L_).permute(0, 4, 2, 3, 1).reshape(F * L_, 147)
    return torch.nn.functional.pad(cols, (0, 13))


@pytest.mark.parametrize("shape", [(1, 7, 7), (2, 9, 11), (1, 63, 95), (2, 64, 96), (1, 384, 512)])
def test_stem_im2col_bits(shape):
    F, H, W = shape
    g = torch.Generator().manual_seed(H * 1000 + W)
    frames = torch.randint(0, 256, (F, 3, H, W), generator=g).float()
    frac = torch.rand(F, 3, H, W, generator=g) * 255.0
    frames = torch.where(torch.rand(F, 3, H, W, generator=g) < 0.5, frames, frac)   # integers 0..255 and non-integers
    frames[-1] = 255.0    # a constant frame: its padding must be 0 (normalised space), not the image of pixel value 0 (-1)
    if F == 1:
        frames[0, :, : H // 2] = frac[0, :, : H // 2]
    ref = stem_reference(frames)
    out = stem(frames.to(dev()))
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert out.shape[0] == F * Ho * Wo == ref.shape[0]
    assert same_bits(out, sh_of(ref)), shape
    flat = out.view(-1, 320).cpu()      # 5 lines of (32 hi | 32 lo): columns 147..159 sit in line 4 at 19..31 of either plane
    for plane in (0, 32):               # exactly +0 in the hi and in the lo plane
        pad = flat[:, 4 * 64 + plane + 19: 4 * 64 + plane + 32].contiguous().view(torch.int16)
        assert int(pad.abs().max()) == 0, (shape, plane)
    from cotracker_amd import ops
    assert float((ops.unsplit(out).cpu() - ref).abs().max()) <= 2.0 ** -21      # hi + lo is the value (independent of ctk_split_rows)
    assert same_bits(stem(frames.to(dev())), out)
    for f in range(F):
        assert same_bits(stem(frames[f: f + 1].contiguous().to(dev())), out[f * Ho * Wo: (f + 1) * Ho * Wo]), (shape, f)


# ---- instance-norm statistics -------------------------------------------------------------------------------------------------
def inorm_stats(x, F, HW, Cn):
    """ctk_enc_inorm_stats on x [F, HW, C]; the workspace starts as NaN so a partial sum that is read but never written shows."""
    L, lib = _lib()
    nb = C.c_size_t()
    L.check(lib.ctk_enc_inorm_workspace_bytes(F, HW, Cn, C.byref(nb)), "ctk_enc_inorm_workspace_bytes")
    assert nb.value == F * ((HW + 511) // 512) * Cn * 16
    ws = torch.full((nb.value // 8,), float("nan"), device=dev(), dtype=torch.float64)
    st = torch.full((F, Cn, 2), float("nan"), device=dev(), dtype=torch.float32)
    L.check(lib.ctk_enc_inorm_stats(_p(x), F, HW, Cn, 1e-5, _p(st), _p(ws), _stream()), "ctk_enc_inorm_stats")
    return st


def stats_reference(x_cpu):
    """nn.InstanceNorm2d (blocks.py:110-113, 147-148: no affine, eps 1e-5, biased variance) in float64: [F, C] mean, 1/sqrt(var + eps)."""
    x64 = x_cpu.double()
    mean = x64.mean(dim=1)
    var = ((x64 - mean[:, None, :]) ** 2).mean(dim=1)      # two passes: no cancellation in the reference
    return mean, 1.0 / torch.sqrt(var + EPS)


def check_stats(x_cpu, what):
    F, HW, Cn = x_cpu.shape
    xd = x_cpu.contiguous().to(dev())
    st = inorm_stats(xd, F, HW, Cn)
    mean64, rstd64 = stats_reference(x_cpu)
    got = st.cpu().double()
    assert torch.isfinite(got).all(), what
    em = (got[..., 0] - mean64).abs() - (2.0 ** -23 * mean64.abs() + 1e-9)
    er = (got[..., 1] / rstd64 - 1.0).abs()
    assert float(em.max()) <= 0.0, (what, "mean", float(em.max()), np.unravel_index(int(em.argmax()), em.shape))
    assert float(er.max()) <= 3e-7, (what, "rstd", float(er.max()), np.unravel_index(int(er.argmax()), er.shape))
    assert same_bits(inorm_stats(xd, F, HW, Cn), st), what
    for f in range(F):
        assert same_bits(inorm_stats(xd[f: f + 1].contiguous(), 1, HW, Cn), st[f: f + 1]), (what, f)
    return er


def _channel_data(F, HW, Cn, mean, std, seed):
    """x[f, :, c] = mean[f, c] + std[f, c] * randn, rounded to float32 (the reference starts from the rounded values)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(F, HW, Cn, generator=g)
    return x * std[:, None, :].float() + mean[:, None, :].float()


@pytest.mark.parametrize("Cn", [64, 96, 128, 256])
@pytest.mark.parametrize("HW", [1, 3, 24, 511, 512, 513, 1536, 49152])
def test_inorm_stats_zero_mean(HW, Cn):
    """(a) spread ~1, |mean| <= 0.25: a different mean and spread for every (frame, channel), so no swapped index can pass."""
    F = 3
    f, c = torch.arange(F)[:, None], torch.arange(Cn)[None, :]
    mean = 0.05 * ((c * 7 + f * 3) % 11 - 5).double()
    std = 1.0 + 0.1 * ((c + 5 * f) % 13).double()
    check_stats(_channel_data(F, HW, Cn, mean, std, HW + Cn), ("zero-mean", HW, Cn))


@pytest.mark.parametrize("HW,Cn", [(1536, 64), (1536, 96), (1536, 128), (1536, 256), (49152, 64), (49152, 256), (12288, 96)])
def test_inorm_stats_offset_dominated(HW, Cn):
    """(b) channels whose offset dominates their spread (a trained bias, a flat region of a real video): mean in
    +-{10, 100, 1000} x spread in {1, 0.1}.  var = E[x^2] - mean^2 amplifies an error of the mean by 2 |mean|, so the sum must not
    round at the scale of the offset."""
    F = 3
    f, c = torch.arange(F)[:, None], torch.arange(Cn)[None, :]
    k = (c + f) % 6
    mean = torch.tensor([10.0, 100.0, 1000.0]).double()[k % 3] * (1 - 2 * ((c // 6 + f) % 2)).double()
    std = torch.tensor([1.0, 0.1]).double()[k // 3] * (1.0 + 0.01 * (c % 5).double())
    check_stats(_channel_data(F, HW, Cn, mean, std, HW * 3 + Cn), ("offset", HW, Cn))


@pytest.mark.parametrize("HW,Cn", [(1, 64), (24, 96), (513, 128), (1536, 256)])
def test_inorm_stats_constant_channels(HW, Cn):
    """(c) variance exactly 0: rstd = 1 / sqrt(eps), the mean is the constant itself, no NaN."""
    F = 2
    g = torch.Generator().manual_seed(HW)
    x = torch.randn(F, HW, Cn, generator=g)
    consts = torch.tensor([3.25, -0.1, 100.7, 0.0, -4096.0, 1e-3])
    for i, v in enumerate(consts):
        x[i % F, :, (i * 11) % Cn] = v
    check_stats(x, ("constant", HW, Cn))
    st = inorm_stats(x.to(dev()), F, HW, Cn).cpu()
    for i, v in enumerate(consts):
        m, r = st[i % F, (i * 11) % Cn]
        assert m.item() == v.item() and abs(r.item() * EPS ** 0.5 - 1.0) <= 3e-7, (HW, Cn, v.item(), m.item(), r.item())


def test_inorm_stats_clamps_a_negative_variance():
    """(c) again, where E[x^2] - mean^2 comes out NEGATIVE: 49152 pixels of a large constant v with a full 24-bit mantissa.  The sum
    of v is exact (mean = v, mean^2 = v^2), every 512-pixel partial sum of squares is exact, and the 96 partial sums added one after
    the other round: numpy repeats that chain and finds differences down to -0.04, far beyond eps.  Whatever the order of the
    kernel's sums, the variance it uses must never be negative: rstd is finite and at most 1 / sqrt(eps)."""
    Cn, HW = 64, 49152
    k = np.arange(Cn)
    v = (3.0e6 * (1 + 0.0137 * k) + 0.25 + 0.5 * (k % 2)).astype(np.float32)
    v2 = v.astype(np.float64) ** 2
    ss = np.zeros(Cn)
    for _ in range(HW // 512):
        ss = ss + 512.0 * v2
    assert (ss / HW - v2 < -1e-3).sum() >= 8      # the clamp is exercised (in the kernel's present order; see above)
    x = torch.from_numpy(v)[None, None, :].repeat(1, HW, 1).contiguous()
    st = inorm_stats(x.to(dev()), 1, HW, Cn).cpu().double().numpy()[0]
    assert np.isfinite(st).all(), st[~np.isfinite(st).all(axis=1)]
    assert (st[:, 0] == v.astype(np.float64)).all()
    assert (st[:, 1] * np.sqrt(EPS) <= 1.0 + 3e-7).all() and (st[:, 1] > 0).all(), st[:, 1].max()


@pytest.mark.parametrize("scale", [1e4, 1e18])
def test_inorm_stats_large_values(scale):
    """(d) squares beyond float32's range (1e18^2 summed over 1536 pixels) are fine in the float64 accumulators."""
    F, HW, Cn = 2, 1536, 64
    std = torch.full((F, Cn), scale).double() * (1.0 + torch.arange(Cn)[None, :].double() / Cn)
    check_stats(_channel_data(F, HW, Cn, torch.zeros(F, Cn).double(), std, 5), ("large", scale))


# ---- normalise (+ ReLU) (+ skip, ReLU) ---------------------------------------------------------------------------------------------
def inorm_apply(x, st, F, HW, Cn, skip=None, skip_st=None, want_sh=True, want_f32=True):
    L, lib = _lib()
    sh = torch.full((F * HW, Cn // 32, 2, 32), float("nan"), device=dev(), dtype=torch.float16) if want_sh else None
    f32 = torch.full((F * HW, Cn), float("nan"), device=dev(), dtype=torch.float32) if want_f32 else None
    L.check(lib.ctk_enc_inorm_apply(_p(x), _p(st), _p(skip), _p(skip_st), F, HW, Cn, _p(sh), _p(f32), _stream()), "ctk_enc_inorm_apply")
    return sh, f32


def apply_reference(x, st, skip, skip_st):
    """blocks.py:130-138 in float32, one torch operation per kernel operation: relu((x - mean) * rstd); with a skip
    relu(skip' + y), skip' = skip or (skip - mean_s) * rstd_s (the 1x1 downsample branch, blocks.py:123-126)."""
    y = x - st[:, None, :, 0]
    y = y * st[:, None, :, 1]
    y = y.clamp_min(0.0)
    if skip is not None:
        k = skip
        if skip_st is not None:
            k = k - skip_st[:, None, :, 0]
            k = k * skip_st[:, None, :, 1]
        y = k + y
        y = y.clamp_min(0.0)
    return y


@pytest.mark.parametrize("Cn", [64, 96, 128, 256])
@pytest.mark.parametrize("mode", ["plain", "skip_f32", "skip_raw"])
def test_inorm_apply_bits(mode, Cn):
    F = 3
    for HW in (1, 35, 1536):
        g = torch.Generator().manual_seed(HW + Cn)
        x = torch.randn(F, HW, Cn, generator=g) * 2.0 + 0.5
        st = torch.stack([torch.randn(F, Cn, generator=g), 0.25 + 2.0 * torch.rand(F, Cn, generator=g)], dim=-1)   # differs by frame
        skip = torch.randn(F, HW, Cn, generator=g) if mode != "plain" else None
        skip_st = (torch.stack([torch.randn(F, Cn, generator=g), 0.25 + torch.rand(F, Cn, generator=g)], dim=-1)
                   if mode == "skip_raw" else None)
        ref = apply_reference(x, st, skip, skip_st).reshape(F * HW, Cn)
        assert float((ref == 0).float().mean()) > 0.1 and float((ref > 0).float().mean()) > 0.3      # the ReLU cuts, and not everything
        d = [None if a is None else a.contiguous().to(dev()) for a in (x, st, skip, skip_st)]
        ref_sh = sh_of(ref)
        for want_sh, want_f32 in ((True, False), (False, True), (True, True)):
            sh, f32 = inorm_apply(d[0], d[1], F, HW, Cn, d[2], d[3], want_sh, want_f32)
            what = (mode, Cn, HW, want_sh, want_f32)
            assert (sh is None) == (not want_sh) and (f32 is None) == (not want_f32)
            if want_f32:
                assert same_bits(f32.cpu(), ref), what
            if want_sh:
                assert same_bits(sh, ref_sh), what
        sh2, f322 = inorm_apply(d[0], d[1], F, HW, Cn, d[2], d[3])
        assert same_bits(sh2, sh) and same_bits(f322, f32)
        for f in range(F):
            one = [None if a is None else a[f: f + 1].contiguous() for a in d]
            sh1, f321 = inorm_apply(one[0], one[1], 1, HW, Cn, one[2], one[3])
            assert same_bits(sh1, sh[f * HW: (f + 1) * HW]) and same_bits(f321, f32[f * HW: (f + 1) * HW]), (mode, Cn, HW, f)


# ---- multi-scale fusion --------------------------------------------------------------------------------------------------------
FUSE_C = (64, 96, 128, 128)     # blocks.py:159-175: the output widths of layer1..layer4


def fuse(srcs, F, Ho, Wo):
    """srcs: four device tensors [F, H_k, W_k, C_k] -> SH [F*Ho*Wo, sum C_k / 32, 2, 32]."""
    L, lib = _lib()
    ctot = sum(s.shape[3] for s in srcs)
    out = torch.full((F * Ho * Wo, ctot // 32, 2, 32), float("nan"), device=dev(), dtype=torch.float16)
    ptr = (C.c_void_p * 4)(*[s.data_ptr() for s in srcs])
    hs = (C.c_int32 * 4)(*[s.shape[1] for s in srcs])
    ws = (C.c_int32 * 4)(*[s.shape[2] for s in srcs])
    cs = (C.c_int32 * 4)(*[s.shape[3] for s in srcs])
    L.check(lib.ctk_enc_fuse(ptr, hs, ws, cs, F, Ho, Wo, _p(out), _stream()), "ctk_enc_fuse")
    return out


def smooth_sources(F, sizes, seed):
    """Four stage outputs [F, H_k, W_k, C_k] that vary slowly over the image (at most 2 rad along y, 4.5 rad along x, a different
    phase per channel and frame).  The kernel forms the source position in float32 like ATen's float path (a few 1e-7 px at the
    small sizes, 2e-5 px at 192 x 256); against a float64 reference that is only invisible on data whose slope per pixel is
    moderate, while a wrong tap or weight still costs a visible fraction of that slope."""
    out = []
    for k, ((h, w), c) in enumerate(zip(sizes, FUSE_C)):
        f = torch.arange(F).double()[:, None, None, None]
        y = torch.arange(h).double()[None, :, None, None] / h
        x = torch.arange(w).double()[None, None, :, None] / w
        ch = torch.arange(c)[None, None, None, :]
        v = torch.sin(y * (1 + ch % 2).double() + 1.5 * x * (1 + ch % 3).double() + 0.37 * ch.double() + 1.3 * f + seed + k)
        out.append(((1.0 + 0.25 * k) * v).float().contiguous())
    return out


def fuse_reference(srcs_cpu, Ho, Wo):
    """blocks.py:198-215: F.interpolate(bilinear, align_corners=True) of every stage to (Ho, Wo) and torch.cat on channels, float64."""
    outs = [torch.nn.functional.interpolate(s.permute(0, 3, 1, 2).double(), (Ho, Wo), mode="bilinear", align_corners=True)
            for s in srcs_cpu]
    return torch.cat(outs, dim=1).permute(0, 2, 3, 1).reshape(-1, sum(s.shape[3] for s in srcs_cpu))


def in_one_arena(srcs_cpu):
    """The four sources as slices of ONE device buffer, 64 floats apart (16-byte aligned): neighbours in memory, as the stages of a
    real encoder call usually are."""
    n = [s.numel() for s in srcs_cpu]
    arena = torch.zeros(sum(n) + 64 * 5, device=dev(), dtype=torch.float32)
    out, off = [], 64
    for s, k in zip(srcs_cpu, n):
        v = arena[off: off + k].view(s.shape)
        v.copy_(s)
        out.append(v)
        off += k + 64
    return out


FUSE_CASES = {
    # name: (F, [(H_k, W_k)] * 4, (Ho, Wo))
    "frame_64x96": (2, [(32, 48), (16, 24), (8, 12), (4, 6)], (16, 24)),          # 1/2, 1/4, 1/8, 1/16 of the frame -> 1/4
    "frame_384x512": (1, [(192, 256), (96, 128), (48, 64), (24, 32)], (96, 128)),
    "frame_72x104": (2, [(36, 52), (18, 26), (9, 13), (5, 7)], (18, 26)),         # sizes that are not in exact ratio
    "one_output_row": (2, [(3, 9), (1, 5), (2, 3), (1, 1)], (1, 5)),              # Ho = 1: scale 0 along y; a 1 x 1 source
    "one_output_column": (2, [(9, 3), (5, 1), (1, 1), (4, 2)], (5, 1)),           # Wo = 1: scale 0 along x
    "one_output_pixel": (1, [(2, 2), (1, 1), (3, 5), (1, 4)], (1, 1)),
}


@pytest.mark.parametrize("case", sorted(FUSE_CASES))
def test_fuse_vs_fp64(case):
    from cotracker_amd import ops
    F, sizes, (Ho, Wo) = FUSE_CASES[case]
    srcs = smooth_sources(F, sizes, len(case))
    d = [s.to(dev()) for s in srcs]
    out = fuse(d, F, Ho, Wo)
    ref = fuse_reference(srcs, Ho, Wo)
    got = ops.unsplit(out).cpu().double()
    assert got.shape == ref.shape
    err = float((got - ref).abs().max())
    assert err <= 1e-6 * float(ref.abs().max()), (case, err, float(ref.abs().max()))
    c0 = 0
    for s in srcs:      # a source that already has the output size passes through with weights exactly 1 and 0: the bits of its split
        if tuple(s.shape[1:3]) == (Ho, Wo):
            assert same_bits(out[:, c0 // 32: (c0 + s.shape[3]) // 32], sh_of(s.reshape(-1, s.shape[3]))), (case, c0)
        c0 += s.shape[3]
    assert same_bits(fuse(d, F, Ho, Wo), out)
    for f in range(F):
        one = fuse([s[f: f + 1].contiguous() for s in d], 1, Ho, Wo)
        assert same_bits(one, out[f * Ho * Wo: (f + 1) * Ho * Wo]), (case, f)


def test_fuse_channel_seams():
    """Every source carries a ramp that is constant over its pixels, value 1000 k + c in channel c of source k: interpolation
    returns it unchanged, so the output must be the four ramps side by side; a first channel that is off (the seams are at 64, 160
    and 288) shows as a wrong channel, not as a small error."""
    from cotracker_amd import ops
    F, sizes, (Ho, Wo) = FUSE_CASES["frame_72x104"]
    srcs = [(1000.0 * k + torch.arange(c).float()).expand(F, h, w, c).contiguous() for k, ((h, w), c) in enumerate(zip(sizes, FUSE_C))]
    out = ops.unsplit(fuse(in_one_arena(srcs), F, Ho, Wo)).cpu()
    want = torch.cat([1000.0 * k + torch.arange(c).float() for k, c in enumerate(FUSE_C)])
    err = (out - want[None, :]).abs().max(dim=0).values
    assert float(err.max()) <= 1e-2, [(int(c), float(out[:, c].abs().max())) for c in torch.nonzero(err > 1e-2).flatten()[:8]]


# ---- channel L2 normalisation --------------------------------------------------------------------------------------------------
def l2norm(x, out=None):
    L, lib = _lib()
    if out is None:
        out = torch.full_like(x, float("nan"))
    L.check(lib.ctk_enc_l2norm(_p(x), x.shape[0], _p(out), _stream()), "ctk_enc_l2norm")
    return out


@pytest.mark.parametrize("P", [1, 5, 4097])
def test_l2norm_vs_fp64(P):
    """cotracker3_online.py:384-394: fmaps / sqrt(max(sum_c fmaps^2, 1e-12)), 128 channels, four pixels per workgroup."""
    g = torch.Generator().manual_seed(P)
    x = torch.randn(P, 128, generator=g)
    kinds = ["unit", "zero", "below_clamp", "near_clamp", "large", "one_hot"]
    for r in range(P):
        k = kinds[r % len(kinds)] if P > 1 else "unit"
        if k == "zero":
            x[r] = 0.0
        elif k == "below_clamp":
            x[r] *= 1e-8         # |x|^2 ~ 1e-14 < 1e-12: divided by 1e-6, not by its norm
        elif k == "near_clamp":
            x[r] *= 3e-7         # |x|^2 ~ 1e-11: just above the clamp
        elif k == "large":
            x[r] *= 1e3
        elif k == "one_hot":
            x[r] = 0.0
            x[r, r % 128] = -7.0
    x64 = x.double()
    ref = x64 / torch.sqrt((x64 * x64).sum(dim=1, keepdim=True).clamp_min(float(np.float32(1e-12))))
    xd = x.to(dev())
    out = l2norm(xd)
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    err = float((got - ref).abs().max())
    assert err <= 3e-7, (P, err)
    zero_rows = (x == 0).all(dim=1)
    assert (out.cpu()[zero_rows].view(torch.int32) == 0).all()          # exactly +0
    if P > 1:
        assert float(ref[2].abs().max()) < 0.1 and float(got[2].abs().max()) > 1e-3     # the clamped row is NOT unit length
    assert same_bits(l2norm(xd), out)
    alias = xd.clone()
    assert l2norm(alias, out=alias) is alias and same_bits(alias, out)            # in place
    for r in sorted({0, P // 2, P - 1}):
        assert same_bits(l2norm(xd[r: r + 1].contiguous()), out[r: r + 1]), (P, r)
