"""Every stage of the HIP encoder chain against float64, on every pixel (-m gpu).

HipEncoder.__call__ (co-tracker_amd/encoder_hip.py) makes about 60 launches per call -- 23 convolutions, 19 instance norms, 8
residual units, the four-level fuse, the L2 norm.  tests/test_gpu_encoder_ops.py and test_gpu_conv_matrix.py own the kernels one by
one; what they cannot own is the HOST layer: the order of the launches, which tensor is the skip, which statistics go with which
activation, the want_sh / want_f32 choices, the Ho / Wo arithmetic on odd maps.  The whole-encoder tests of test_gpu_parity.py see
a fault there only through every layer behind it, against one max-norm bar on the output and (at model resolution) a float32
reference.  Here every one of the 14 stages (oracle/encoder_fp64.py: STAGES) is compared where it is written.

Every stage is teacher-forced: the HIP stage (HipEncoder.trace) and the float64 stage get the same input -- the HIP output of the
stage before, converted to double (for conv2 that is ops.unsplit of the fused SH rows) -- so one assertion measures ONE stage, over
all pixels, channels and frames.  A failure names the stage and the worst entry as (frame, y, x, channel).  The reference is
oracle/encoder_fp64.py in float64 on the CPU (F.conv2d), pinned by tests/test_encoder_fp64_reference.py on the goldens of the
unmodified reference and on the repository's torch module.

Shapes (ctk_support.ENC_CASES), the smallest at which each path engages:
  halo   128 x 512, 2 frames   maps 64 x 256, 32 x 128, 16 x 64, 8 x 32: every 3 x 3 / stride-1 layer on conv3x3_halo_kernel
  mixed  128 x 256, 2 frames   layer4 (8 x 16) falls back to conv_pp128_kernel, the others are halo
  odd    70 x 102, 3 frames    35 x 51, 18 x 26, 9 x 13, 5 x 7: stride 2 on odd maps, nothing tile-aligned, fused to 17 x 25 (no
                               multiple of any source size; rows of 25 pixels start off a 16-byte multiple in pixels)
Weights are fill_synthetic_(seed=3); the frames are synthetic_video(seed=9) plus, last, a CONSTANT frame of 127.5, on which every
instance norm of the chain sees a variance of exactly 0 (the eps path; the float64 chain of that frame is finite and exact,
test_encoder_fp64_reference.py).

Bars, all the project's own (test_encoder_hip_vs_reference_fnet): 5e-6 x max(1, max |ref of the stage|) for every raw and normed
stage, 2e-6 absolute for `features`.  A stage alone must meet what the whole chain is already held to.

Measured numbers go to $CTK_SESSION_OUT/encoder_stages_<case>.json (default session_out/; a copy of a run:
profiles/encoder_stages.json): max and RMS error of HIP against float64, the same for the float32 torch stage from the same input
(the yardstick, not a bar; textured frames -- float32 torch is no yardstick on the constant frame, see
test_encoder_fp64_reference.py), the stage scale."""
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from ctk_support import ENC_CASES, ENC_FAULTS, dev, encoder_frames, encoder_model, same_bits  # noqa: E402
from oracle import encoder_fp64 as E  # noqa: E402  (checker only)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR_RAW, BAR_FEATURES = 5e-6, 2e-6   # tests/test_gpu_parity.py: test_encoder_hip_vs_reference_fnet


def bar_of(stage, ref):
    return BAR_FEATURES if stage == "features" else BAR_RAW * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------------------------------
# the one checker every comparison goes through (the 4-d form of test_gpu_window_stages.check / expect)
# ------------------------------------------------------------------------------------------
def check(ours, ref):
    """ours, ref [F, h, w, C] -> (max |ours - ref|, frame, y, x, channel); a non-finite entry counts as infinite."""
    assert ours.shape == ref.shape and ours.dim() == 4, (ours.shape, ref.shape)
    d = (ours.double() - ref.double()).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, math.inf))
    i = int(d.argmax())
    _, h, w, c = d.shape
    return float(d.reshape(-1)[i]), i // (h * w * c), (i // (w * c)) % h, (i // c) % w, i % c


def expect(stage, w, bar):
    assert w[0] <= bar, f"{stage}: max |error| {w[0]:.3e} > bar {bar:.1e} at frame f={w[1]}, y={w[2]}, x={w[3]}, channel {w[4]}"


def rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())


def nhwc(x):
    return x.permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------
# measured numbers -> $CTK_SESSION_OUT/encoder_stages_<case>.json (default session_out/)
# ------------------------------------------------------------------------------------------
REPORT = {}


def record(case, section, key, **numbers):
    H, W, Fn = ENC_CASES[case]
    rep = REPORT.setdefault(case, {"case": case, "H": H, "W": W, "frames": Fn, "bars": {"raw_x_max1_scale": BAR_RAW, "features": BAR_FEATURES},
                                   "stages": {}, "whole_chain": {}, "controls": {}})
    rep[section].setdefault(key, {}).update(numbers)
    out = os.environ.get("CTK_SESSION_OUT") or os.path.join(ROOT, "session_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, f"encoder_stages_{case}.json"), "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------
# model, frames, the HIP trace and every reference: computed once per shape
# ------------------------------------------------------------------------------------------
_model = {}


def model():
    if not _model:
        m = encoder_model()
        _model.update(p64=E.cast_params(m.state_dict(), "cpu", torch.float64), p32=E.cast_params(m.state_dict(), "cpu", torch.float32),
                      fnet=m.fnet.to(dev()))
    return _model


class Case:
    def __init__(self, name):
        from cotracker_amd.encoder_hip import HipEncoder
        self.name = name
        self.frames = encoder_frames(name)
        Fn, _, H, W = self.frames.shape
        self.size = (H // 4, W // 4)
        self.enc = HipEncoder(model()["fnet"], dev())
        self.frames_dev = self.frames.to(dev())
        self.out = self.enc(self.frames_dev)                      # untraced
        self.enc.trace = {}
        self.out_traced = self.enc(self.frames_dev)
        torch.cuda.synchronize()
        trace, self.enc.trace = self.enc.trace, None
        self.trace_keys = sorted(trace)
        self.features_is_the_result = trace["features"].data_ptr() == self.out_traced.data_ptr()
        self.hip = {s: trace[s].cpu() for s in E.STAGES}          # [F,h,w,C] float32
        del trace
        hip64 = {s: v.permute(0, 3, 1, 2).double() for s, v in self.hip.items()}   # the oracle's layout
        p64, p32 = model()["p64"], model()["p32"]
        self.inputs, self.ref, self.f32, self._worst = {}, {}, {}, None
        with torch.no_grad():
            for s in E.STAGES:
                x = self.inputs[s] = E.inputs_of(s, hip64, self.frames)
                self.ref[s] = E.step(s, x, p64, self.size)
                self.f32[s] = E.step(s, [v.float() for v in x] if isinstance(x, list) else x.float(), p32, self.size)
            self.chain64 = E.forward(self.frames, p64)
            self.chain32 = E.forward(self.frames, p32)

    def worst(self, refs=None):
        """stage -> (check(...), bar) of the HIP trace against `refs` (default: the float64 stages)."""
        if self._worst is None:
            self._worst = {s: (check(self.hip[s], nhwc(self.ref[s])), bar_of(s, self.ref[s])) for s in E.STAGES}
        if refs is None:
            return self._worst
        return {s: self._worst[s] if refs[s] is self.ref[s] else (check(self.hip[s], nhwc(refs[s])), bar_of(s, refs[s])) for s in E.STAGES}

    def failing(self, refs=None):
        return [s for s, (w, bar) in self.worst(refs).items() if not w[0] <= bar]


_cases = {}


def get_case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.fixture(scope="module", params=list(ENC_CASES))
def case(request):
    return get_case(request.param)


# ------------------------------------------------------------------------------------------
# the trace costs nothing and changes nothing
# ------------------------------------------------------------------------------------------
def test_traced_call_returns_the_bits_of_an_untraced_one(case):
    assert same_bits(case.out_traced, case.out)
    assert set(E.STAGES) <= set(case.trace_keys), sorted(set(E.STAGES) - set(case.trace_keys))
    assert case.features_is_the_result and same_bits(case.hip["features"], case.out.cpu())
    assert same_bits(case.enc(case.frames_dev), case.out)         # and a third call, untraced again
    Fn, H, W = case.frames.shape[0], *case.frames.shape[-2:]
    assert tuple(case.hip["norm1"].shape) == (Fn, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64)
    assert tuple(case.hip["layer4.1"].shape[1:3]) == {"halo": (8, 32), "mixed": (8, 16), "odd": (5, 7)}[case.name]
    assert tuple(case.hip["fused"].shape) == (Fn, H // 4, W // 4, 416) and tuple(case.out.shape) == (Fn, H // 4, W // 4, 128)


# ------------------------------------------------------------------------------------------
# 14 stages x 3 shapes, each alone
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", E.STAGES)
def test_stage(case, stage):
    ours, ref, f32 = case.hip[stage], nhwc(case.ref[stage]), nhwc(case.f32[stage])
    w, bar = check(ours, ref), bar_of(stage, ref)
    tex = slice(0, ours.shape[0] - 1)                              # the textured frames; the last one is the constant frame
    record(case.name, "stages", stage, scale=float(ref.abs().max()), bar=bar,
           hip_max=w[0], hip_worst={"frame": w[1], "y": w[2], "x": w[3], "channel": w[4]}, hip_rms=rms(ours, ref),
           hip_max_textured=check(ours[tex], ref[tex])[0], hip_rms_textured=rms(ours[tex], ref[tex]),
           hip_max_constant_frame=check(ours[-1:], ref[-1:])[0],
           float32_torch_max_textured=check(f32[tex], ref[tex])[0], float32_torch_rms_textured=rms(f32[tex], ref[tex]),
           float32_torch_max_constant_frame=check(f32[-1:], ref[-1:])[0],
           chain_float32_vs_float64_max_textured=check(nhwc(case.chain32[stage])[tex], nhwc(case.chain64[stage])[tex])[0],
           chain_float32_vs_float64_rms_textured=rms(case.chain32[stage][tex], case.chain64[stage][tex]))
    print(f"\n{case.name} {stage}: HIP vs float64 max {w[0]:.3e} rms {rms(ours, ref):.3e}; bar {bar:.3e}; "
          f"float32 torch (textured) max {check(f32[tex], ref[tex])[0]:.3e}")
    assert bool(torch.isfinite(ref).all())
    expect(f"{case.name}, stage {stage} (teacher-forced)", w, bar)


# ------------------------------------------------------------------------------------------
# the whole chain, free-running from the frames, against float64
# ------------------------------------------------------------------------------------------
def test_whole_encoder_vs_float64_from_the_frames(case):
    from cotracker_amd.encoder_hip import HipEncoder
    raw = HipEncoder(model()["fnet"], dev(), normalize=False)(case.frames_dev)
    assert same_bits(raw.cpu(), case.hip["conv3"]), "normalize=False must return the conv3 bits"
    for s in E.STAGES:
        assert bool(torch.isfinite(case.chain64[s]).all()), s
    ref_raw, ref_n = nhwc(case.chain64["conv3"]), nhwc(case.chain64["features"])
    w_raw, w_n = check(raw.cpu(), ref_raw), check(case.out.cpu(), ref_n)
    free = {s: check(case.hip[s], nhwc(case.chain64[s]))[0] for s in E.STAGES}
    record(case.name, "whole_chain", "conv3", max=w_raw[0], rms=rms(raw.cpu(), ref_raw), scale=float(ref_raw.abs().max()),
           bar=bar_of("conv3", ref_raw), float32_torch_max_textured=check(nhwc(case.chain32["conv3"])[:-1], ref_raw[:-1])[0])
    record(case.name, "whole_chain", "features", max=w_n[0], rms=rms(case.out.cpu(), ref_n), bar=BAR_FEATURES,
           float32_torch_max_textured=check(nhwc(case.chain32["features"])[:-1], ref_n[:-1])[0])
    record(case.name, "whole_chain", "every_stage_free_running_max", **{s.replace(".", "_"): v for s, v in free.items()})
    expect(f"{case.name}, untraced conv3 against the float64 chain from the frames", w_raw, bar_of("conv3", ref_raw))
    expect(f"{case.name}, untraced features against the float64 chain from the frames", w_n, BAR_FEATURES)


def test_frame_alone_gives_the_bits_it_has_in_the_batch():
    """On `odd`: the existing tests assert this at aligned sizes only."""
    cs = get_case("odd")
    for f in range(cs.frames.shape[0]):
        assert same_bits(cs.enc(cs.frames_dev[f:f + 1].contiguous())[0], cs.out[f]), f
    assert same_bits(cs.enc(cs.frames_dev[1:3].contiguous()), cs.out[1:3])


# ------------------------------------------------------------------------------------------
# negative controls: the checker names the entry, and the bars have teeth
# ------------------------------------------------------------------------------------------
def test_checker_names_the_planted_entry():
    cs = get_case("odd")
    ref = nhwc(cs.ref["layer2.1"])                                   # [3,9,13,96]
    bar = bar_of("layer2.1", ref)
    bad = ref.clone()
    bad[1, 4:6, 7:9, 30:34] += 4 * bar
    bad[1, 5, 8, 33] += 1 * bar
    w = check(bad, ref)
    assert w[1:] == (1, 5, 8, 33) and abs(w[0] - 5 * bar) < 1e-9
    with pytest.raises(AssertionError, match=r"stage planted.*frame f=1, y=5, x=8, channel 33"):
        expect("stage planted", w, bar)
    bad = ref.clone()
    bad[2, 0, 12, 95] = float("nan")
    assert check(bad, ref) == (math.inf, 2, 0, 12, 95)


@pytest.mark.parametrize("name", list(ENC_FAULTS))
def test_planted_fault_fails_its_stage_and_no_other(name):
    """The float64 reference with ONE fault planted through the hooks of oracle/encoder_fp64.py (the kernels are not touched): the
    unchanged HIP stage must now FAIL at the stage of the fault and pass at every other one.  That each fault moves its stage by
    >= 10 x the bar in the float64 oracle alone, and no other stage by a bit, is asserted without a GPU in
    test_encoder_fp64_reference.py; every fault is as narrow as it reads (one tap over two columns, one norm, one level, one frame):
    none had to be widened to reach that."""
    where_case, where, faults = ENC_FAULTS[name]
    cs = get_case(where_case)
    with torch.no_grad():
        refs = dict(cs.ref)
        refs[where] = E.step(where, cs.inputs[where], model()["p64"], cs.size, faults)
    worst = cs.worst(refs)
    w, bar = worst[where]
    record(where_case, "controls", name, stage=where, ratio_to_bar=w[0] / bar,
           worst={"frame": w[1], "y": w[2], "x": w[3], "channel": w[4]}, unfaulted_ratio_to_bar=cs.worst()[where][0][0] / bar)
    assert cs.failing(refs) == [where], (name, cs.failing(refs))
    assert w[0] >= 10 * bar, f"{name}: HIP is only {w[0] / bar:.1f} x the bar from the faulted reference"
    with pytest.raises(AssertionError, match=rf"stage {where.replace('.', '[.]')} "):
        expect(f"stage {where} ", w, bar)
    if name == "dropped_tap_at_a_tile_seam":
        assert w[3] in (31, 32), w                                   # the worst entry sits at the seam
    if name == "norm1_stats_of_another_frame":
        assert w[1] == 1, w
