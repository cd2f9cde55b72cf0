"""Pin oracle/encoder_fp64.py -- the float64 reference of tests/test_gpu_encoder_stages.py -- on the CPU.  Needs no GPU.

  1. in float32 and in float64 against the `fnet` outputs the UNMODIFIED reference wrote (tests/golden/model_online.npz,
     model_offline.npz, cotracker2.npz), at the bars test_encoder_hip_vs_reference_fnet holds the HIP encoder to:
     5e-6 x max(1, scale) on the raw conv3 output, 2e-6 on the normalised features;
  2. in float64, stage by stage, against the repository's torch module (co-tracker_amd/encoder.py, `.double()`), its
     intermediates taken by forward hooks, at 70 x 102 and 128 x 256: 1e-12 x the stage scale (the same arithmetic, summed in
     another order);
  3. prints how far the float32 and the float64 run of the same text are apart at every stage: the yardstick for the errors the
     GPU stage tests measure (they record it in $CTK_SESSION_OUT/encoder_stages_<case>.json);
  4. every fault hook moves the stage it is planted in by at least 10 x that stage's bar, and no other stage by a bit.

What the yardstick shows about the CONSTANT frame (ctk_support.encoder_frames): in float64 every stage of it is exact -- each
convolution returns its bias, each norm sees (x - mean) = 0 -- but float32 torch is off by one ulp in a mean of identical values,
and 1 / sqrt(eps) = 316 per norm turns that into an error of the order of the features six norms later.  float32 torch is
therefore no yardstick on that frame, and the figures are printed for the textured frames and the constant one apart."""
import copy

import numpy as np
import pytest
import torch

from ctk_support import ENC_CASES, ENC_FAULTS, encoder_frames, encoder_model
from oracle import encoder_fp64 as E

DTYPES = [torch.float32, torch.float64]
BAR_RAW, BAR_FEATURES = 5e-6, 2e-6   # tests/test_gpu_parity.py: test_encoder_hip_vs_reference_fnet


def bar_of(stage, ref):
    """5e-6 x max(1, max |ref of the stage|) for every raw and normed stage, 2e-6 absolute for the unit-length features."""
    return BAR_FEATURES if stage == "features" else BAR_RAW * max(1.0, float(ref.abs().max()))


# ---- 1. the goldens of the unmodified reference ---------------------------------------------------------------------------------
def golden_model(which, golden):
    from cotracker_amd.weights import fill_synthetic_
    if which == "cotracker2":
        from cotracker_amd.model_v2 import CoTracker2
        g = golden("cotracker2")
        m = CoTracker2(stride=4, window_len=8, model_resolution=(64, 96)).eval()
        fill_synthetic_(m, seed=6, head_scale=1.0)
        return m, g["video"][0], g["fmaps"][0]
    from cotracker_amd.model import CoTrackerThreeOffline, CoTrackerThreeOnline
    cls, seed, key = (CoTrackerThreeOnline, 1, "on") if which == "online" else (CoTrackerThreeOffline, 2, "off")
    m = cls(stride=4, corr_radius=3, window_len=8, model_resolution=(64, 96)).eval()
    fill_synthetic_(m, seed=seed)
    g = golden(f"model_{which}")
    return m, g[f"{key}_video"][0], g[f"{key}_fnet"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("which", ["online", "offline", "cotracker2"])
def test_oracle_matches_the_reference_goldens(golden, which, dtype):
    m, video, ref = golden_model(which, golden)
    ref = torch.from_numpy(np.ascontiguousarray(ref)).double()                         # [T,128,16,24], raw conv3
    with torch.no_grad():
        out = E.forward(torch.from_numpy(np.ascontiguousarray(video)).float(), E.cast_params(m.state_dict(), "cpu", dtype))
    assert out["conv3"].dtype == dtype and out["conv3"].shape == ref.shape
    e = float((out["conv3"].double() - ref).abs().max())
    assert e <= bar_of("conv3", ref), (which, dtype, e, float(ref.abs().max()))
    ref_n = ref / torch.sqrt(torch.clamp((ref * ref).sum(1, keepdim=True), min=1e-12))
    e = float((out["features"].double() - ref_n).abs().max())
    assert e <= BAR_FEATURES, (which, dtype, e)


# ---- 2. the repository's module, stage by stage, in float64 -------------------------------------------------------------------
def module_stages(fnet, x):
    """The intermediates of BasicEncoder.forward by forward hooks: stage name -> tensor (norm1 and fused are the inputs of
    layer1.0 and conv2; the module has no layer of its own for either)."""
    got, hooks = {}, []

    def keep(name, what):
        def hook(mod, inp, out):
            got[name] = (inp[0] if what == "in" else out).detach()
        return hook

    hooks.append(fnet.conv1.register_forward_hook(keep("conv1", "out")))
    hooks.append(fnet.layer1[0].register_forward_hook(keep("norm1", "in")))
    for k, layer in enumerate((fnet.layer1, fnet.layer2, fnet.layer3, fnet.layer4), 1):
        for j in (0, 1):
            hooks.append(layer[j].register_forward_hook(keep(f"layer{k}.{j}", "out")))
    hooks.append(fnet.conv2.register_forward_hook(keep("fused", "in")))
    hooks.append(fnet.conv2.register_forward_hook(keep("conv2", "out")))
    hooks.append(fnet.conv3.register_forward_hook(keep("conv3", "out")))
    with torch.no_grad():
        fnet(x)
    for h in hooks:
        h.remove()
    return got


@pytest.fixture(scope="module")
def model():
    m = encoder_model()
    return {"m": m, "p64": E.cast_params(m.state_dict(), "cpu", torch.float64), "p32": E.cast_params(m.state_dict(), "cpu", torch.float32)}


@pytest.mark.parametrize("case", ["odd", "mixed"])
def test_oracle_matches_the_torch_module_stage_by_stage(model, case):
    """Teacher-forced: every stage of the oracle starts from the MODULE's output of the stage before.

    The textured frames meet 1e-12 x the stage scale (measured: <= 2e-14).  The constant frame cannot, in the three units behind
    the stem, and the op that reorders is the MEAN of F.instance_norm: where every pixel of a channel has the same value the oracle's
    mean returns it and (x - mean) is 0, the module's leaves 7e-16 in norm1.  From there on the module's constant frame is noise
    that each norm multiplies by up to 1 / sqrt(eps) = 316 (3.7e-11 after layer1.0, 2.5e-6 after layer1.1, O(1) from layer2.1 on),
    and a unit holds two norms in a row, so a rounding difference of 1e-17 in a mean may come out as 1e-12.  Measured on that
    frame: 3.1e-11 .. 6.9e-10 in layer1.0 .. layer2.0, <= 2.4e-13 elsewhere.  Its bar is 1e-12 x scale / eps."""
    frames = encoder_frames(case)
    assert tuple(frames.shape[-2:]) in ((70, 102), (128, 256))
    fnet = copy.deepcopy(model["m"].fnet).double()
    mod = module_stages(fnet, E.to_unit_range(frames, torch.float64))
    mod["features"] = mod["conv3"] / mod["conv3"].norm(dim=1, keepdim=True).clamp_min(1e-6)   # sqrt(max(ss, 1e-12)), another way
    size = (frames.shape[-2] // 4, frames.shape[-1] // 4)
    assert tuple(mod["fused"].shape) == (frames.shape[0], 416) + size
    with torch.no_grad():
        for stage in E.STAGES:
            ours = E.step(stage, E.inputs_of(stage, mod, frames), model["p64"], size)
            assert ours.dtype == torch.float64 and ours.shape == mod[stage].shape, stage
            scale = float(mod[stage].abs().max())
            e = float((ours[:-1] - mod[stage][:-1]).abs().max())
            assert e <= 1e-12 * scale, f"{case} {stage}: {e:.3e} > 1e-12 x {scale:.3f}"
            e = float((ours[-1] - mod[stage][-1]).abs().max())
            assert e <= 1e-12 * scale / E.EPS, f"{case} {stage}, constant frame: {e:.3e} > 1e-7 x {scale:.3f}"


# ---- 3 + 4. the three shapes of the GPU test: yardstick, the constant frame, the fault hooks --------------------------------------
_runs = {}


def run(model, case):
    if case not in _runs:
        frames = encoder_frames(case)
        with torch.no_grad():
            _runs[case] = (frames, E.forward(frames, model["p64"]), E.forward(frames, model["p32"]))
    return _runs[case]


def apart(a, b):
    d = a.double() - b.double()
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())


@pytest.mark.parametrize("case", list(ENC_CASES))
def test_float32_yardstick_and_the_constant_frame(model, case):
    frames, o64, o32 = run(model, case)
    H, W, Fn = ENC_CASES[case]
    assert tuple(frames.shape) == (Fn, 3, H, W) and float(frames[-1].min()) == float(frames[-1].max()) == 127.5
    assert tuple(o64["layer4.1"].shape[-2:]) == {"halo": (8, 32), "mixed": (8, 16), "odd": (5, 7)}[case]
    assert tuple(o64["features"].shape) == (Fn, 128, H // 4, W // 4)
    rows = []
    for stage in E.STAGES:
        assert bool(torch.isfinite(o64[stage]).all()), (case, stage)
        # the constant frame: every stage of it is constant over the pixels (so every norm behind it sees a variance of 0) ...
        const = o64[stage][-1]
        # (the channel sum of `features` runs in a different order at different pixels: a few ulps of 0.1 there)
        assert float((const - const[:, :1, :1]).abs().max()) <= (1e-16 if stage == "features" else 0.0), (case, stage)
        tex = apart(o32[stage][:-1], o64[stage][:-1])
        rows.append(f"{stage:9s} scale {float(o64[stage].abs().max()):7.3f}  textured max {tex[0]:.2e} rms {tex[1]:.2e}   "
                    f"constant frame max {apart(o32[stage][-1], o64[stage][-1])[0]:.2e}")
    # ... and normed stages of it are exactly 0 in float64 (x - mean = 0, times 1 / sqrt(eps))
    for stage in ["norm1"] + E.UNITS + ["fused"]:
        assert float(o64[stage][-1].abs().max()) == 0.0, (case, stage)
    print(f"\nfloat32 vs float64 of oracle/encoder_fp64.py, {case} ({Fn} x {H} x {W}), free-running from the frames:\n  " + "\n  ".join(rows))


@pytest.mark.parametrize("name", list(ENC_FAULTS))
def test_planted_faults_move_their_stage_and_no_other(model, name):
    """Teacher-forced on the float64 chain itself: with the hook, the stage it names moves by >= 10 x the bar the GPU test holds
    that stage to; every other stage returns the bits it returns without a hook.  All five faults meet the condition as narrow as
    they are (none had to be widened): measured 266 x (unbiased variance, layer4.0) to 2.7e5 x the bar."""
    case, where, faults = ENC_FAULTS[name]
    frames, o64, _ = run(model, case)
    size = tuple(o64["fused"].shape[-2:])
    with torch.no_grad():
        for stage in E.STAGES:
            bad = E.step(stage, E.inputs_of(stage, o64, frames), model["p64"], size, faults)
            moved = float((bad - o64[stage]).abs().max())
            if stage == where:
                assert moved >= 10 * bar_of(stage, o64[stage]), f"{name}: moves {stage} by {moved / bar_of(stage, o64[stage]):.1f} x its bar only"
                print(f"\n{name}: {stage} of `{case}` moves by {moved:.3e} = {moved / bar_of(stage, o64[stage]):.0f} x its bar")
            else:
                assert torch.equal(bad, o64[stage]), (name, stage, moved)
    if name == "dropped_tap_at_a_tile_seam":
        # the convolution itself changes in the two columns either side of the seam and nowhere else (the norm behind it then
        # spreads the change of the statistics over the map, so the unit's output moves everywhere, most at the seam)
        x = o64["layer3.0"]
        with torch.no_grad():
            d = (E.conv(x, model["p64"], "layer3.1.conv2", 1, 1, faults) - E.conv(x, model["p64"], "layer3.1.conv2", 1, 1)).abs()
        assert x.shape[-1] == 64 and sorted(torch.nonzero(d.amax(dim=(0, 1, 2))).flatten().tolist()) == [31, 32]


def test_unknown_fault_names_are_refused(model):
    with pytest.raises(AssertionError):
        E.norm1(torch.zeros(1, 64, 4, 4, dtype=torch.float64), faults={"norm1_frames": (1, 0)})
