"""Every stage of one CoTracker2 update window (ctk_forward_window_v2) at FULL SIZE against float64, on every point (-m gpu).

The other GPU files compare the stages of the CoTracker2 iteration with an independent reference at S = 8, N = 10 only
(tests/golden/cotracker2.npz), where no persistent split-half GEMM runs, attention_q64_kernel takes no key split
(v2p_splits(N) = ceil(N / 1024)), nothing is merged and the mask covers ten keys; tests/test_gpu_v2_ops.py checks the three row
kernels alone.  Here the reference is computed: oracle/window_v2_fp64.py in float64 ON THE GPU (torch ops only; pinned on the CPU
against the unmodified reference's goldens by tests/test_window_v2_fp64_reference.py), at

  full         S = 8,  N = 6400   the window bench.py's v2_sliding times: persistent GEMMs and their tails, 7 key splits + merge
  full_masked  S = 8,  N = 6400   ~10 % of the points masked at random PLUS the run 1800..2999: key split 2 (keys 1856..2783) is
                                  masked as a whole, splits 1 and 3 in part; masked queries in points<-virtual; their track_feat is 0
  ragged       S = 8,  N = 4099   N not a multiple of 32 / 64 / 256 / 1024
  small        S = 8,  N = 300    below every persistent threshold, one key split
  long         S = 16, N = 1031   a window_len = 16 CoTracker2: time attention at n1 = 16 under 6 layers, 16 bias rows

on a 96 x 128 level-0 pyramid of UNNORMALISED random features (pixel norms spread over a decade: CoTracker2 runs the encoder without
the final L2 normalisation), fill_synthetic_(seed=0, head_scale=1.0) weights, the moving tracks of the CoTracker3 stage file
(make_tracks: ~2 % leave the frame on each side, some integer and half-integer coordinates), random vis, a 0/1 track_mask and a
track_feat of the features' scale.

Every stage is teacher-forced: the HIP stage and the float64 stage get the same input -- the HIP output of the stage before, converted
to double -- so each assertion measures ONE stage at that stage's own bar, over ALL rows.  With head_scale = 1 the CoTracker2 map
amplifies a rounding difference 15-20 x per iteration (tests/test_window_v2_fp64_reference.py prints it), so nothing free-running is
asserted on these weights; stage 6 walks along the HIP orbit one iteration at a time instead, and stage 7 runs six iterations free on
the damped weights (weights.fill_synthetic_v2_damped_) by the rule of tests/test_gpu_scale.py's scale_v2_c2.

The bars are the project's own, named by source in BAR; none is new.  Two quantities are MEASURED ON THE REFERENCE (float32 torch of
the same text against float64) and enter a bar only with a factor of 3: the floor of stage 4 and the floor of stage 7.

A failure names the stage and the worst entry as (track n, frame t, column).  Measured errors go to
$CTK_SESSION_OUT/window_v2_stages_<id>_<precision>.json (default session_out/; a copy of a run: profiles/window_v2_stages.json).
Stages 1-3 do not depend on the Linear back end and run once per shape; stages 4-7 run for both back ends (f16x3, f32)."""
import ctypes as C
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from ctk_support import dev, recorded, same_bits  # noqa: E402
from ctk_support import precision_param as precision  # noqa: E402,F401
from oracle import window_v2_fp64 as V  # noqa: E402  (checker only)
from test_gpu_gemm_matrix import tol_for  # noqa: E402  the Linear bound of the GEMM contract matrix
from test_gpu_window_stages import check, expect, make_tracks, w2d  # noqa: E402  the one checker, the C3 file's tracks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW, STRIDE = (96, 128), 4
SHAPES = {"full": (8, 6400, False), "full_masked": (8, 6400, True), "ragged": (8, 4099, False), "small": (8, 300, False),
          "long": (16, 1031, False)}
MASKED_RUN = (1800, 3000)
F64_CHUNK = 400  # points per float64 volume (8 x 400 x 96 x 128 doubles = 315 MB)
BAR = {"pos": 1e-6,            # the support bar of tests/test_gpu_window_stages.py
       "corrblock": 1e-6,      # x max(1, max |ref|): test_corrblock_vs_reference_golden's 3e-6 at |corr| ~ 3
       "trig": 1e-6,           # tests/test_gpu_v2_ops.py::test_v2_assemble
       "former": 3e-5,         # the project's former bar (test_oracle_golden, stage 5 of the C3 file)
       "apply_delta": 1.0,     # in units of the bound include/ctk.h documents (test_v2_apply_delta restates it)
       "vis_head": 1.0,        # in units of test_v2_vis_head's one-ulp bound
       "vis_out": 1e-4, "px": 1e-3, "logit": 1e-4}   # the end-to-end bars (test_gpu_scale.py)


def nsc(x):
    """[S,N,...] (the state's layout) -> [N,S,C] (the checker's)."""
    return (x if x.dim() == 3 else x[..., None]).permute(1, 0, 2)


def ratio(w, bar):
    return w[0] / bar


# ------------------------------------------------------------------------------------------
# measured numbers -> $CTK_SESSION_OUT/window_v2_stages_<id>_<precision>.json (default session_out/)
# ------------------------------------------------------------------------------------------
REPORT = {}


def record(name, precision, stage, **numbers):
    """precision None: a stage that does not depend on the Linear back end (written to both files)."""
    rep = REPORT.setdefault(name, {None: {}, "f16x3": {}, "f32": {}})
    rep[precision].setdefault(stage, {}).update(numbers)
    out = os.environ.get("CTK_SESSION_OUT") or os.path.join(ROOT, "session_out")
    os.makedirs(out, exist_ok=True)
    S, N, masked = SHAPES[name]
    for prec in ("f16x3", "f32") if precision is None else (precision,):
        with open(os.path.join(out, f"window_v2_stages_{name}_{prec}.json"), "w") as f:
            json.dump({"case": name, "S": S, "N": N, "masked": masked, "precision": prec, "bars": BAR,
                       "stages": {**rep[None], **rep[prec]}}, f, indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------
# models (head_scale = 1 and damped, window_len 8 and 16), inputs, and the HIP outputs of every stage (once per shape / back end)
# ------------------------------------------------------------------------------------------
_models = {}


def model(S, damped=False):
    key = (S, damped)
    if key not in _models:
        from cotracker_amd.model_v2 import CoTracker2
        from cotracker_amd.weights import fill_synthetic_, fill_synthetic_v2_damped_
        m = CoTracker2(window_len=S, stride=STRIDE, model_resolution=(HW[0] * STRIDE, HW[1] * STRIDE)).eval()
        if damped:
            fill_synthetic_v2_damped_(m, seed=0)
        else:
            fill_synthetic_(m, seed=0, head_scale=1.0)
        m = m.to(dev())
        _models[key] = dict(m=m, p64=V.cast_params(m.state_dict(), dev(), torch.float64), p32=V.cast_params(m.state_dict(), dev(), torch.float32))
    return _models[key]


def features(S, seed):
    """Level-0 features [S,96,128,128] channels-last, NOT normalised: unit normal channels times a log-normal factor per pixel."""
    g = torch.Generator().manual_seed(seed)
    f0 = torch.randn(S, HW[0], HW[1], 128, generator=g) * torch.exp(0.5 * torch.randn(S, HW[0], HW[1], 1, generator=g))
    return f0.to(dev()).contiguous()


def point_mask(N):
    m = torch.rand(N, generator=torch.Generator().manual_seed(3)) > 0.1
    m[MASKED_RUN[0]:MASKED_RUN[1]] = False
    return m


class Case:
    def __init__(self, name):
        from cotracker_amd import ops
        self.name = name
        self.S, self.N, masked = SHAPES[name]
        S, N = self.S, self.N
        self.pyr = ops.build_pyramid(features(S, seed=100))
        self.pyr64 = [f.permute(0, 3, 1, 2).double().contiguous() for f in self.pyr]
        _, _, coords, vis, _ = make_tracks(S, N, seed=7)
        g = torch.Generator().manual_seed(11)
        feat = torch.randn(S, N, 128, generator=g) * torch.exp(0.5 * torch.randn(1, N, 1, generator=g))
        self.track_mask = (torch.rand(S, N, generator=g) > 0.5).float().to(dev())
        self.mask = self.maskb = None
        if masked:
            self.maskb = point_mask(N).to(dev())
            self.mask = self.maskb.to(torch.uint8)
            feat = feat * point_mask(N).float()[None, :, None]          # as the model does (cotracker.py:346)
        self.coords, self.vis, self.feat = coords.to(dev()), vis.to(dev()), feat.to(dev()).contiguous()
        self.chunk = min(N, F64_CHUNK)
        self._cache = {}

    def cached(self, key, make):
        if key not in self._cache:
            with torch.no_grad():
                self._cache[key] = make()
            torch.cuda.synchronize()
        return self._cache[key]

    def pw(self, precision, damped=False):
        return model(self.S, damped)["m"].packed(dev(), precision)

    @property
    def p64(self):
        return model(self.S)["p64"]

    # ---- HIP outputs that do not depend on the back end ------------------------------------------------------------------------
    def pos(self):
        from cotracker_amd import ops
        return self.cached("pos", lambda: ops.sample_features4d(self.pw("f32").pos_hwc, self.coords[0].contiguous()))

    def fcorrs(self):
        from cotracker_amd import ops
        return self.cached("fcorrs", lambda: ops.corrblock_sample(self.pyr, self.feat, self.coords))

    def x(self, split=False):
        from cotracker_amd import ops
        from cotracker_amd.model_v2 import IN_LD
        return self.cached(("x", split), lambda: ops.v2_assemble(self.coords, self.fcorrs(), self.feat, self.track_mask, self.vis, self.pos(),
                                                                 IN_LD, split))

    # ---- HIP outputs per back end ----------------------------------------------------------------------------------------------
    def delta(self, precision, depth=6):
        """ctk_update_former_ex with the mask on a copy of the FormerWeights with `depth` layers; x in the form the window driver
        hands over (SH on the split-half back end): delta rows [N*S, 192]."""
        def make():
            from cotracker_amd import _lib as L, ops
            pw = self.pw(precision)
            fw = L.FormerWeights()
            C.memmove(C.byref(fw), C.byref(pw.former), C.sizeof(L.FormerWeights))
            fw.depth = depth
            return ops.update_former_ex(self.x(pw.split), pw.split, self.S, self.N, fw, self.mask)
        return self.cached(("delta", precision, depth), make)

    def applied(self, precision):
        """ctk_v2_apply_delta on the HIP delta -> (coords after the step, normed rows [S*N,128])."""
        def make():
            from cotracker_amd import ops
            pw, c = self.pw(precision), self.coords.clone()
            normed = ops.v2_apply_delta(self.delta(precision), c, pw.norm_w, pw.norm_b)
            return c, normed
        return self.cached(("applied", precision), make)

    def updated(self, precision):
        """The track_feat_updater Linear as the driver calls it: erf GELU, residual and output both track_feat (in place)."""
        def make():
            from cotracker_amd import _lib as L, ops
            pw, f = self.pw(precision), self.feat.clone()
            rows = f.view(self.S * self.N, 128)
            ops.gemm(self.applied(precision)[1], pw.upd_w, bias=pw.upd_b, act=L.ACT_GELU_ERF, resid=rows, out=rows, packed=pw.upd_p)
            return f
        return self.cached(("updated", precision), make)

    def vis_logits(self, precision):
        from cotracker_amd import ops
        pw = self.pw(precision)
        return self.cached(("vis", precision), lambda: ops.v2_vis_head(self.updated(precision), pw.vis_w, pw.vis_b))

    def orbit(self, precision):
        """The HIP orbit: states[k] = (coords, track_feat, vis_out) after k calls of ctk_forward_window_v2(iters=1), k = 0 .. 6."""
        def make():
            from cotracker_amd import ops
            c, f = self.coords.clone(), self.feat.clone()
            states = [(c.clone(), f.clone(), None)]
            for _ in range(6):
                win = ops.V2Window(self.pyr, c, f, self.vis, self.track_mask, self.mask, 1)
                ops.forward_window_v2(win, self.pw(precision))
                torch.cuda.synchronize()
                states.append((c.clone(), f.clone(), win.vis_out.clone()))
            return states
        return self.cached(("orbit", precision), make)

    # ---- the float64 side ------------------------------------------------------------------------------------------------------
    def x_ref(self, dtype=torch.float64, faults=None):
        """The HIP x as the former of the reference wants it: time embedding added (the library folds it into the per-frame bias
        rows of the input projection, ctk_former_weights.in_bias_t)."""
        p = model(self.S)["p64" if dtype == torch.float64 else "p32"]
        return self.x().view(self.N, self.S, -1)[..., :V.IN_DIM].to(dtype) + V.time_embed(p, self.S, faults)

    def former(self, precision):
        """Stage 4's measurement: the float64 former on the HIP x after every depth, the same text in float32 torch (the floor, measured
        on the reference alone), and the bar that follows: 3e-5, or 3 x the floor where the floor at depth 6 is above a third of it."""
        def make():
            ref = V.update_former(self.x_ref(), self.p64, self.maskb, each_depth=True)
            f32 = V.update_former(self.x_ref(torch.float32), model(self.S)["p32"], self.maskb, each_depth=True)
            floor = [check(a, b)[0] for a, b in zip(f32, ref)]
            bar = BAR["former"] if 3 * floor[-1] <= BAR["former"] else 3 * floor[-1]
            return {"ref": ref, "floor": floor, "bar": bar}
        return self.cached("former", make)

    def stage_errors(self, precision, faults=None, sub=None):
        """Stages 2-5, teacher-forced, with `faults` planted in the REFERENCE: stage -> (worst, bar).  sub: the correlation stage on
        the first `sub` points only (a float64 volume pass over all points is the expensive part)."""
        if faults is None:
            return self.cached(("errors", precision, sub), lambda: self._stage_errors(precision, None, sub))
        with torch.no_grad():
            return self._stage_errors(precision, faults, sub)

    def _stage_errors(self, precision, faults, sub):
        S, N, p = self.S, self.N, self.p64
        n1 = sub or N
        out = {}
        # 2: CorrBlock.corr + sample
        ref = V.corrblock(self.pyr64, self.feat[:, :n1].double(), self.coords[:, :n1], min(self.chunk, n1), faults=faults)
        scale = max(1.0, float(ref.abs().max()))
        out["2_corrblock_sample"] = (check(self.fcorrs()[:n1], ref), BAR["corrblock"] * scale)
        # 3: the sin / cos columns of the token rows
        ref = V.assemble(self.coords, self.fcorrs().double(), self.feat.double(), self.track_mask, self.vis, self.pos().double(), faults)
        xh = self.x().view(N, S, -1)
        out["3_v2_assemble_trig"] = (check(xh[..., 2:130], ref[..., 2:130]), BAR["trig"])
        # 4: the update former with the mask
        fm = self.former(precision)
        ref = fm["ref"][-1] if not faults else V.update_former(self.x_ref(faults=faults), p, self.maskb, faults=faults)
        dl = self.delta(precision).view(N, S, -1)
        out["4_update_former"] = (check(dl[..., :130], ref), fm["bar"])
        # 5: GroupNorm of the feature delta, in units of the kernel's documented bound; the updater Linear
        d64 = dl[..., :130].double()
        _, ref = V.apply_delta(self.coords, d64, p, faults)
        mu = d64[..., 2:].mean(dim=-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(d64[..., 2:].var(dim=-1, keepdim=True, unbiased=False) + 1e-5)
        tol = 2e-6 * float(ref.abs().max()) + 2.0 ** -21 * mu.abs() * rstd * p["norm.weight"].abs()
        normed = self.applied(precision)[1].view(S, N, 128).permute(1, 0, 2)
        out["5_v2_apply_delta"] = (check(normed / tol, ref / tol), BAR["apply_delta"])
        ref = V.updater(normed.double(), self.feat.double(), p, faults)
        out["5_updater"] = (check(nsc(self.updated(precision)), nsc(ref)), tol_for(precision, ref))
        return out

    def free_run(self, dtype):
        """Six iterations of the reference text on the DAMPED weights from the start state, in `dtype` (independent of the back end)."""
        def make():
            p = model(self.S, True)["p64" if dtype == torch.float64 else "p32"]
            pyr = self.pyr64 if dtype == torch.float64 else [f.float() for f in self.pyr64]
            c, v, _ = V.forward_window(pyr, self.coords.to(dtype), self.feat.to(dtype), self.vis.to(dtype), self.track_mask.to(dtype),
                                       self.maskb, p, 6, self.chunk)
            return c, v
        return self.cached(("free", dtype), make)


_cases = {}


def get_case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.fixture(scope="module", params=list(SHAPES))
def case(request):
    return get_case(request.param)


# ------------------------------------------------------------------------------------------
# stage 0: what the inputs are
# ------------------------------------------------------------------------------------------
def test_inputs_move_leave_the_frame_are_unnormalised_and_masked(case):
    c, S, N = case.coords, case.S, case.N
    step = (c[1:] - c[:-1]).abs()
    assert 0.05 < float(step.mean()) and float(step.max()) <= 1.0           # level-0 units per frame (x 4 = px)
    for side in ((c[..., 0] < 0).any(0), (c[..., 0] > HW[1] - 1).any(0), (c[..., 1] < 0).any(0), (c[..., 1] > HW[0] - 1).any(0)):
        assert 0.005 * N <= int(side.sum()) <= 0.05 * N                      # a few per cent of the tracks leave on each side
    assert int(((c == c.round()).all(-1)).sum()) >= 0.015 * S * N           # integer taps: weight exactly 0 / 1
    assert int((((c * 2) == (c * 2).round()) & (c != c.round())).all(-1).sum()) >= 0.01 * S * N
    norms = case.pyr[0].norm(dim=-1).flatten()
    q = torch.quantile(norms[:: max(1, norms.numel() // 100000)], torch.tensor([0.01, 0.99], device=dev()))
    assert float(q[1] / q[0]) > 5.0, "the pixels of an unnormalised map have a spread of norms"
    fn = case.feat.norm(dim=-1)
    assert 0.5 < float(fn[fn > 0].median() / norms.median()) < 2.0          # track_feat of the features' scale
    assert set(case.track_mask.unique().tolist()) == {0.0, 1.0} and 0.3 < float(case.track_mask.mean()) < 0.7
    assert float(case.vis.std()) > 0.5
    for l in range(1, 4):  # the pyramid the float64 stages read is the library's own; in float64 it agrees with pooling again
        ref = torch.nn.functional.avg_pool2d(case.pyr64[l - 1], 2, stride=2)
        assert float((case.pyr64[l] - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    splits = (N + 1023) // 1024
    per = ((N + splits - 1) // splits + 31) // 32 * 32                       # attention.hip: keys per split of attention_q64_kernel
    assert splits == {"full": 7, "full_masked": 7, "ragged": 5, "small": 1, "long": 2}[case.name]
    if case.name == "ragged":
        assert all(N % k for k in (32, 64, 256, 1024))
    if case.mask is None:
        return
    m = case.maskb
    whole = [s_ for s_ in range(splits) if not bool(m[s_ * per:(s_ + 1) * per].any())]
    assert whole == [2], "exactly one key split is masked as a whole"
    assert bool(m[per:2 * per].any()) and not bool(m[per:2 * per].all()) and bool(m[3 * per:4 * per].any()) and not bool(m[3 * per:4 * per].all())
    rest = torch.cat([m[:MASKED_RUN[0]], m[MASKED_RUN[1]:]]).float()
    assert 0.85 < float(rest.mean()) < 0.95                                   # ~10 % of the others
    assert float(case.feat[:, ~m].abs().max()) == 0.0 and bool((case.feat[:, m].abs().amax(dim=-1) > 0).all())


def test_shapes_reach_the_kernels_they_name(case, precision):
    """The library's launch recorder over one former call: the persistent split-half GEMMs run at every shape but `small` (and never
    on the exact-f32 back end), the masked virtual<-points attention and the time attention at each of the six depths."""
    from cotracker_amd import ops
    pw = case.pw(precision)

    def call():
        ops.update_former_ex(case.x(pw.split), pw.split, case.S, case.N, pw.former, case.mask)
        torch.cuda.synchronize()
    rows = recorded(call)[1]
    persistent = sorted(r for r in rows if r.startswith("gemm_sh_pp"))
    record(case.name, precision, "0_launches", persistent_gemms=persistent, attention={k: v for k, v in rows.items() if k.startswith("attention")})
    assert bool(persistent) == (precision == "f16x3" and case.name != "small"), rows
    assert rows["attention_v2p"] == 6 and rows["attention_p2v"] == 6 and rows["attention_time"] == 6, rows


# ------------------------------------------------------------------------------------------
# stage 1: positional embedding at the first frame's coordinates
# ------------------------------------------------------------------------------------------
def test_stage1_pos(case):
    with torch.no_grad():
        ref = V.pos(case.p64, case.coords[0])
    w = check(case.pos()[:, None], ref[:, None])
    record(case.name, None, "1_pos", **w2d(w))
    expect("stage 1, sample_features4d of pos_emb (frame = 0, column = channel)", w, BAR["pos"])


# ------------------------------------------------------------------------------------------
# stage 2: CorrBlock.corr + sample, all N x S x 196 outputs against the float64 volume
# ------------------------------------------------------------------------------------------
def test_stage2_corrblock_sample(case):
    w, bar = case.stage_errors("f32")["2_corrblock_sample"]
    masked = 0.0 if case.mask is None else float(case.fcorrs()[~case.maskb].abs().max())
    record(case.name, None, "2_corrblock_sample", bar=bar, scale=bar / BAR["corrblock"], masked_max=masked, **w2d(w))
    assert masked == 0.0, "masked points (zero track_feat) must give exactly zero correlations"
    expect("stage 2, ctk_corrblock_sample (column = 49 level + 7 x tap + y tap)", w, bar)


# ------------------------------------------------------------------------------------------
# stage 3: token assembly on the real fcorrs, by the rules of tests/test_gpu_v2_ops.py
# ------------------------------------------------------------------------------------------
def test_stage3_v2_assemble(case):
    from cotracker_amd import ops
    S, N = case.S, case.N
    x, pos = case.x().view(N, S, -1), case.pos()
    exact = torch.zeros_like(x)                                               # every column but sin / cos is ONE float32 addition
    exact[..., 0:2] = (case.coords - case.coords[0:1]).permute(1, 0, 2) + pos[:, None, 0:2]
    exact[..., 130:326] = case.fcorrs() + pos[:, None, 130:326]
    exact[..., 326:454] = case.feat.permute(1, 0, 2) + pos[:, None, 326:454]
    exact[..., 454] = case.track_mask.t() + pos[:, None, 454]
    exact[..., 455] = case.vis.t() + pos[:, None, 455]
    trig = torch.zeros(x.shape[-1], dtype=torch.bool, device=dev())
    trig[2:130] = True
    w, bar = case.stage_errors("f32")["3_v2_assemble_trig"]
    sh_same = same_bits(case.x(True), ops.split_rows(case.x()))
    record(case.name, None, "3_v2_assemble", sh_equals_split_of_f32=sh_same, **w2d(w))
    assert same_bits(x[..., ~trig], exact[..., ~trig]), "flows, fcorrs, track_feat, track_mask, vis (+ pos) and the padding: bit for bit"
    assert int(x[..., V.IN_DIM:].view(torch.int32).abs().max()) == 0
    expect("stage 3, ctk_v2_assemble, sin / cos columns (column = 2 + 64 axis + 2 k + (0 sin | 1 cos) - 2)", w, bar)
    assert sh_same, "SH ctk_v2_assemble is not the split of the f32 one"


# ------------------------------------------------------------------------------------------
# stage 4: the update former with the mask, after every depth
# ------------------------------------------------------------------------------------------
def test_stage4_update_former(case, precision):
    m = case.former(precision)
    by_depth = [check(case.delta(precision, d).view(case.N, case.S, -1)[..., :130], m["ref"][d - 1]) for d in range(1, 7)]
    pad = float(case.delta(precision).view(case.N, case.S, -1)[..., 130:].abs().max())
    record(case.name, precision, "4_update_former", bar=m["bar"], bar_is_3x_floor=m["bar"] != BAR["former"], float32_torch_floor=m["floor"],
           by_depth=[w[0] for w in by_depth], delta_max=float(m["ref"][-1].abs().max()), **w2d(by_depth[-1]))
    assert pad == 0.0
    for d, w in enumerate(by_depth, 1):  # the first wrong depth is named first; masked query rows are compared too
        expect(f"stage 4, update former after depth {d} of 6 (ctk_update_former_ex; column = dx, dy, 128 feature deltas)", w, m["bar"])
    assert case.stage_errors(precision)["4_update_former"][0] == by_depth[-1]


# ------------------------------------------------------------------------------------------
# stage 5: the state update -- ctk_v2_apply_delta, the track_feat_updater Linear, ctk_v2_vis_head
# ------------------------------------------------------------------------------------------
def test_stage5_apply_delta_updater_vis_head(case, precision):
    S, N, p = case.S, case.N, case.p64
    err = case.stage_errors(precision)
    step = case.delta(precision).view(N, S, -1)[..., :2].permute(1, 0, 2)
    coords_exact = same_bits(case.applied(precision)[0], case.coords + step)
    feat = case.updated(precision)
    with torch.no_grad():
        ref = V.vis_head(feat.double(), p)
        terms = (feat.double() * p["vis_predictor.0.weight"][0]).abs().sum(dim=-1)
    bound = 2.0 ** -23 * ref.abs() + 1e-9 * terms
    wv = check(nsc(case.vis_logits(precision).double() / bound), nsc(ref / bound))
    (wa, ba), (wu, bu) = err["5_v2_apply_delta"], err["5_updater"]
    record(case.name, precision, "5_state_update", coords_bit_equal=coords_exact, apply_delta_in_units_of_bound=w2d(wa), updater=w2d(wu),
           updater_bar=bu, vis_head_in_units_of_bound=w2d(wv), track_feat_max=float(feat.abs().max()))
    assert coords_exact, "coords after ctk_v2_apply_delta are not coords + delta[:, :2] bit for bit"
    expect("stage 5, ctk_v2_apply_delta, GroupNorm rows (in units of the bound of include/ctk.h)", wa, ba)
    expect("stage 5, track_feat_updater Linear + erf GELU + residual, in place (column = channel)", wu, bu)
    expect("stage 5, ctk_v2_vis_head (in units of one float32 ulp of the logit + 1e-9 sum |terms|)", wv, BAR["vis_head"])


# ------------------------------------------------------------------------------------------
# stage 6: one iteration through ctk_forward_window_v2(iters=1), from the HIP state after k = 0 .. 5 iterations
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(6))
def test_stage6_one_iteration_along_the_orbit(case, precision, k):
    states = case.orbit(precision)
    (c0, f0, _), (c1, f1, v1) = states[k], states[k + 1]
    with torch.no_grad():
        rc, rv, rf = V.forward_window(case.pyr64, c0, f0.double(), case.vis, case.track_mask, case.maskb, case.p64, 1, case.chunk)
    bar = case.former(precision)["bar"]
    w = {"coords": check(nsc(c1), nsc(rc)), "track_feat": check(nsc(f1), nsc(rf)), "vis_out": check(nsc(v1), nsc(rv))}
    bars = {"coords": bar, "track_feat": tol_for(precision, rf), "vis_out": BAR["vis_out"]}
    finite = all(bool(torch.isfinite(t_).all()) for t_ in (c1, f1, v1))
    record(case.name, precision, f"6_iteration_{k}", bars=bars, state_finite=finite, track_feat_max=float(f1.abs().max()),
           moved=float((c1 - c0).abs().max()), **{n: w2d(v) for n, v in w.items()})
    assert finite, "a value left the f16 range (ctk_forward_window_v2 has no range guard: this is its range_fallbacks)"
    for n, v in w.items():
        expect(f"stage 6, iteration {k} of the HIP orbit through ctk_forward_window_v2, {n} (level-0 units / features / logits)", v, bars[n])
    assert float((c1 - c0).abs().max()) > 1e-3  # the iteration moved the tracks


def test_stage6_window_graph_replay_is_bit_identical(precision):
    """At `full`: a captured V2WindowGraph replays the launches of the direct call (two iterations from the start state)."""
    from cotracker_amd import ops
    cs = get_case("full")
    pw = cs.pw(precision)
    win = ops.V2Window(cs.pyr, cs.coords.clone(), cs.feat.clone(), cs.vis, cs.track_mask, cs.mask, 2)
    ops.forward_window_v2(win, pw)
    torch.cuda.synchronize()
    direct = (win.keep[1].clone(), win.keep[2].clone(), win.vis_out.clone())
    gw = ops.V2Window(cs.pyr, cs.coords.clone(), cs.feat.clone(), cs.vis, cs.track_mask, cs.mask, 2)
    gr = ops.V2WindowGraph(gw, pw)
    gr.launch()
    torch.cuda.synchronize()
    record("full", precision, "6_graph_replay", nodes=int(gr.nodes))
    for a, b in zip((gw.keep[1], gw.keep[2], gw.vis_out), direct):
        assert same_bits(a, b)
    assert float((direct[0] - cs.coords).abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------
# stage 7: six iterations free-running, all points, on the damped weights
# ------------------------------------------------------------------------------------------
def test_stage7_six_iterations_damped(case, precision):
    from cotracker_amd import ops
    win = ops.V2Window(case.pyr, case.coords.clone(), case.feat.clone(), case.vis, case.track_mask, case.mask, 6)
    ops.forward_window_v2(win, case.pw(precision, damped=True))
    torch.cuda.synchronize()
    (rc, rv), (fc, fv) = case.free_run(torch.float64), case.free_run(torch.float32)
    floor = {"px": check(nsc(fc.double() * STRIDE), nsc(rc * STRIDE))[0], "logit": check(nsc(fv), nsc(rv))[0]}
    bars = {"px": max(BAR["px"], 3 * floor["px"]), "logit": max(BAR["logit"], 3 * floor["logit"])}   # test_gpu_scale.py, scale_v2_c2
    w = {"px": check(nsc(win.keep[1].double() * STRIDE), nsc(rc * STRIDE)), "logit": check(nsc(win.vis_out), nsc(rv))}
    record(case.name, precision, "7_six_iterations_damped", bars=bars, float32_torch_floor=floor,
           moved_px=float((rc - case.coords.double()).abs().max()) * STRIDE, **{n: w2d(v) for n, v in w.items()})
    expect("stage 7, six iterations on damped weights, coords (px at model resolution)", w["px"], bars["px"])
    expect("stage 7, six iterations on damped weights, visibility logit", w["logit"], bars["logit"])


# ------------------------------------------------------------------------------------------
# negative controls: faults planted in the float64 reference, never in a kernel.  Each must fail ITS stage and no other
# ------------------------------------------------------------------------------------------
FAULTS = {  # name -> (the fault, the stage it must fail)
    "dropped_tap_of_one_level": ({"drop_tap": (2, 17)}, "2_corrblock_sample"),
    "x_and_y_embeddings_swapped": ({"swap_xy": True}, "3_v2_assemble_trig"),
    "time_embedding_rows_exchanged": ({"swap_time": 3}, "4_update_former"),
    "key_mask_ignored_for_one_tile": ({"v2p_unmask": (1, 3, 1856, 1888)}, "4_update_former"),
    "masked_queries_left_unmasked": ({"p2v_unmask": 1}, "4_update_former"),
    "unbiased_groupnorm_variance": ({"unbiased": True}, "5_v2_apply_delta"),
    "tanh_gelu_in_the_updater": ({"tanh_gelu": True}, "5_updater"),
}
MUTATION_POINTS = 400  # the correlation stage of a mutation run looks at the first float64 chunk


@pytest.mark.parametrize("fault", list(FAULTS))
def test_mutation_fails_its_stage_and_no_other(fault, precision):
    cs = get_case("full_masked")
    planted, own = FAULTS[fault]
    clean = {k: ratio(*v) for k, v in cs.stage_errors(precision, None, MUTATION_POINTS).items()}
    got = {k: ratio(*v) for k, v in cs.stage_errors(precision, planted, MUTATION_POINTS).items()}
    record("full_masked", precision, "mutation_" + fault, fails_stage=own, ratio_to_bar=got[own], unmutated_ratio_to_bar=clean[own],
           other_stages_ratio_to_bar={k: v for k, v in got.items() if k != own})
    assert all(v <= 1.0 for v in clean.values()), clean
    for k, v in got.items():
        if k != own:
            assert v <= 1.0 and abs(v - clean[k]) <= 0.01, f"{fault} moved stage {k}: {clean[k]:.3f} -> {v:.3f} x its bar"
    if fault == "key_mask_ignored_for_one_tile":
        return check_key_tile(cs, precision, got[own], clean[own])
    assert got[own] > 1.0, f"{fault} moves stage {own} by {got[own]:.2f} x its bar only: the bar does not bite"


def check_key_tile(cs, precision, tile_ratio, clean_ratio):
    """One 32-key tile of 6400 keys in one head of one layer: as at the C3 shape (test_mutation_dropped_key_tile_of_one_head) the
    fault is held against the MEASURED error where it does not reach the bar, and a whole masked key split of that head must."""
    with torch.no_grad():
        ref = V.update_former(cs.x_ref(), cs.p64, cs.maskb, faults={"v2p_unmask": (1, 3, 1856, 2784)})
    bar = cs.former(precision)["bar"]
    split_ratio = check(cs.delta(precision).view(cs.N, cs.S, -1)[..., :130], ref)[0] / bar
    record("full_masked", precision, "mutation_key_mask_ignored_for_one_tile", whole_split_ratio_to_bar=split_ratio)
    assert tile_ratio >= 2 * clean_ratio, f"an unmasked 32-key tile moves stage 4 from {clean_ratio:.3f} to {tile_ratio:.3f} x its bar only"
    assert split_ratio > 1.0, f"a whole unmasked key split of one head moves stage 4 by {split_ratio:.2f} x its bar only"
