"""Every stage of one update window at FULL SIZE against float64, on every point (-m gpu).

The other GPU files compare the stages of the update iteration with an independent reference at S = 8, N = 12 only, where none of
the kernels of the headline step engage (the persistent split-half GEMMs and their tail, attention over key splits + merge, the
persistent time attention, the grid-stride heads, the point chunking of the correlation stage).  Here the reference is computed:
oracle/window_fp64.py in float64 ON THE GPU (torch ops only; pinned on the CPU against the unmodified reference's goldens by
tests/test_window_fp64_reference.py), at

  c3      S = 16, N = 6400   the headline window (and once more with ~10 % of the points masked: c3_masked)
  ragged  S = 16, N = 4099   N not a multiple of 32 / 64 / 256: ragged key tile, ragged last GEMM row block, tail cut elsewhere
  small   S = 8,  N = 300    below every persistent threshold

on a 96 x 128 level-0 pyramid of L2-normalised random features, fill_synthetic_(seed=0) weights, tracks that MOVE (smooth drift,
~2 % leave the frame on each side, some integer and half-integer coordinates) and random vis / conf logits.

Every stage is teacher-forced: the HIP stage and the float64 stage get the same input -- the HIP output of the stage before,
converted to double -- so each assertion measures ONE stage at that stage's own bar, over ALL rows (float64 volumes in point
chunks).  A failure names the stage and the worst entry as (track n, frame t, column).  Measured errors go to
$CTK_SESSION_OUT/window_stages_<id>_<precision>.json (default session_out/, as tools/gpu_session.sh; a copy of a run:
profiles/window_stages.json).

Tap POSITIONS follow the reference's float32 coordinate arithmetic on both sides (oracle/window_fp64._grid; pinned bit for bit by
test_tap_indices_bit_exact / test_sampler_math_host); the VALUES are float64.  Stages 1-2 do not depend on the Linear back end and
run once per shape; stages 3-8 run for both back ends (f16x3, f32)."""
import ctypes as C
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from ctk_support import dev  # noqa: E402
# stages 3-8 run on both Linear back ends: split-half MFMA (the default) and exact-f32 MFMA
from ctk_support import precision_param as precision  # noqa: E402,F401
from oracle import window_fp64 as W  # noqa: E402  (checker only)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, STRIDE, HW, SCALE_XY = (384, 512), 4, (96, 128), (128.0, 96.0)
SHAPES = {"c3": (16, 6400, False), "c3_masked": (16, 6400, True), "ragged": (16, 4099, False), "small": (8, 300, False)}
CUT_INSIDE_A_TILE = {"c3": 1000, "c3_masked": 1000, "ragged": 1000, "small": 70}  # points_per_chunk: rows per chunk % 256 != 0
F64_CHUNK = 800  # points per float64 volume (16 x 800 x 2401 doubles = 246 MB)
# the bars the project holds at S = 8, N = 12 (tests/test_gpu_parity.py), and the end-to-end bar
BAR = {"support": 1e-6, "volume": 3e-6, "corr_embed": 1e-5, "posenc": 1e-6, "former": 3e-5, "former_cap": 1e-4, "px": 1e-3,
       "logit": 1e-4}


# ------------------------------------------------------------------------------------------
# the one checker every comparison goes through
# ------------------------------------------------------------------------------------------
def check(ours, ref, n0=0):
    """ours, ref [n, S, C] -> (max |ours - ref|, track n0 + n, frame t, column); a non-finite entry counts as infinite."""
    assert ours.shape == ref.shape and ours.dim() == 3, (ours.shape, ref.shape)
    d = (ours.double() - ref.double()).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, math.inf))
    i = int(d.argmax())
    n, S, Cc = d.shape
    return float(d.reshape(-1)[i]), n0 + i // (S * Cc), (i // Cc) % S, i % Cc


def worse(a, b):
    return b if a is None or b[0] > a[0] else a


def expect(stage, w, bar):
    assert w[0] <= bar, f"{stage}: max |error| {w[0]:.3e} > bar {bar:.1e} at track n={w[1]}, frame t={w[2]}, column {w[3]}" + \
        (f", {w[4]}" if len(w) > 4 else "")


def tsn(x):
    """[S,N,...] (the state's layout) -> [N,S,C] (the checker's)."""
    return (x if x.dim() == 3 else x[..., None]).permute(1, 0, 2)


# ------------------------------------------------------------------------------------------
# measured numbers -> $CTK_SESSION_OUT/window_stages_<id>_<precision>.json (default session_out/)
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
        with open(os.path.join(out, f"window_stages_{name}_{prec}.json"), "w") as f:
            json.dump({"case": name, "S": S, "N": N, "masked": masked, "precision": prec, "bars": BAR,
                       "stages": {**rep[None], **rep[prec]}}, f, indent=1, sort_keys=True)


def w2d(w):
    return {"max": w[0], "track": w[1], "frame": w[2], "column": w[3]}


# ------------------------------------------------------------------------------------------
# model, inputs, and the HIP outputs of every stage (computed once per shape / back end)
# ------------------------------------------------------------------------------------------
_model = {}


def model():
    if not _model:
        from cotracker_amd.model import CoTrackerThreeOnline
        from cotracker_amd.weights import fill_synthetic_
        m = CoTrackerThreeOnline(stride=STRIDE, corr_radius=3, window_len=16).eval()
        fill_synthetic_(m, seed=0)
        m = m.to(dev())
        _model.update(m=m, p64=W.cast_params(m.state_dict(), dev(), torch.float64), p32=W.cast_params(m.state_dict(), dev(), torch.float32))
    return _model


def features(S, seed):
    """Level-0 features [S,96,128,128] channels-last, L2-normalised over channels."""
    g = torch.Generator().manual_seed(seed)
    f0 = torch.randn(S, HW[0], HW[1], 128, generator=g).to(dev())
    return (f0 / f0.norm(dim=-1, keepdim=True)).contiguous()


def make_tracks(S, N, seed):
    """Queries and a moving window state.  coords[t] = query + (t - query frame) * velocity + a slow sine, <= 0.6 level-0 units
    (2.4 px) per frame (1 unit for the integer tracks: posenc arguments stay below 8); tracks n % 50 == 0 / 1 / 2 / 3 start within half a unit of the left / right / top / bottom border and drift out
    (so their taps are clamped, then out of range); n % 50 == 4 keeps integer coordinates in every frame, n % 50 == 5 half-integer ones."""
    g = torch.Generator().manual_seed(seed)
    size = torch.tensor([HW[1] - 1.0, HW[0] - 1.0])
    qc = torch.rand(N, 2, generator=g) * size
    qf = torch.randint(0, S, (N,), generator=g)
    vel = torch.rand(N, 2, generator=g) - 0.5
    amp = torch.rand(N, 2, generator=g) * 0.2
    phase = torch.rand(N, 2, generator=g) * 2 * math.pi
    edge = torch.rand(N, generator=g) * 0.45
    k = torch.arange(N) % 50
    for side, axis, sign in ((0, 0, -1.0), (1, 0, 1.0), (2, 1, -1.0), (3, 1, 1.0)):
        sel = k == side
        qc[sel, axis] = edge[sel] if sign < 0 else size[axis] - edge[sel]
        vel[sel, axis] = sign * 0.5
    qc[k == 4] = qc[k == 4].round()
    vel[k == 4] = vel[k == 4].sign()
    qc[k == 5] = qc[k == 5].floor().clamp(max=HW[0] - 2.0) + 0.5
    vel[k == 5] = vel[k == 5].sign() * 0.5
    amp[(k == 4) | (k == 5)] = 0.0
    dt = (torch.arange(S)[:, None] - qf[None, :]).float()[..., None]                          # [S,N,1]
    coords = qc[None] + dt * vel[None] + amp[None] * (torch.sin(0.4 * dt + phase[None]) - torch.sin(phase[None]))
    vis, conf = torch.randn(S, N, generator=g), torch.randn(S, N, generator=g)
    return qc, qf, coords.contiguous(), vis, conf


class Case:
    def __init__(self, name):
        from cotracker_amd import ops
        self.name = name
        self.S, self.N, masked = SHAPES[name]
        S, N = self.S, self.N
        self.pyr = ops.build_pyramid(features(S, seed=100))
        self.pyr64 = [f.permute(0, 3, 1, 2).double().contiguous() for f in self.pyr]
        qc, qf, coords, vis, conf = make_tracks(S, N, seed=7)
        self.qc, self.qf = qc.to(dev()), qf.to(dev())
        self.coords, self.vis, self.conf = coords.to(dev()), vis.to(dev()), conf.to(dev())
        self.mask = None
        if masked:
            self.mask = (torch.rand(N, generator=torch.Generator().manual_seed(3)) > 0.1).to(torch.uint8).to(dev())
        # stage 1's HIP output, and what every later float64 stage starts from: the HIP support as doubles, masked tracks zeroed
        # (attention_mask acts on the support alone, cotracker3_online.py:493-496)
        self.sup = [ops.sample_support(self.pyr[l], self.qf.float(), (self.qc / 2 ** l).contiguous()) for l in range(4)]
        self.sup64 = self.sup64_of(self.sup, self.mask)
        self.chunk = min(N, F64_CHUNK)
        self._cache = {}

    @staticmethod
    def sup64_of(sup, mask):
        out = [s_.permute(1, 0, 2).double() for s_ in sup]
        return out if mask is None else [s_ * mask[None, :, None].double() for s_ in out]

    def state(self):
        return self.coords.clone(), self.vis.clone(), self.conf.clone()

    def window(self, state=None, iters=1, **kw):
        from cotracker_amd import ops
        c, v, f = state if state is not None else self.state()
        return ops.Window(self.pyr, self.sup, c, v, f, SCALE_XY, iters=iters, point_mask=self.mask, **kw)

    def cached(self, key, make):
        if key not in self._cache:
            with torch.no_grad():
                self._cache[key] = make()
        return self._cache[key]

    # ---- stages 2 + 3 (reference side): ONE pass over the float64 volumes -------------------------------------------------
    def corr_pass(self):
        """Compares the three HIP volumes with every float64 volume chunk as it goes by, and keeps the float64 corr_mlp output
        of those volumes: {"worst": {which: (err, n, t, col, level)}, "pad": .., "masked": .., "emb64": [S,N,1024]}."""
        def make():
            from cotracker_amd import _lib, ops
            S, N = self.S, self.N
            win = self.window()
            vols = {"f32": ops.corr_volume(win), "sh_v3": ops.corr_volume_sh(win)}
            with _lib.option(_lib.OPT_CORR_VERSION, 1):
                vols["sh_v1"] = ops.corr_volume_sh(win)
            torch.cuda.synchronize()
            res = {"worst": {k: None for k in vols}, "pad": {k: 0.0 for k in vols}, "masked": {k: 0.0 for k in vols}}

            def look(l, n0, n1, vol):
                ref = vol.permute(1, 0, 2)
                for k, v in vols.items():
                    rows = v[l, n0 * S:n1 * S]
                    full = (rows if k == "f32" else ops.unsplit(rows)).reshape(n1 - n0, S, _lib.CORR_LD)
                    res["worst"][k] = worse(res["worst"][k], check(full[..., :_lib.CORR_K], ref, n0) + (f"level {l}",))
                    res["pad"][k] = max(res["pad"][k], float(full[..., _lib.CORR_K:].abs().max()))
                    if self.mask is not None and bool((self.mask[n0:n1] == 0).any()):
                        res["masked"][k] = max(res["masked"][k], float(full[self.mask[n0:n1] == 0].abs().max()))

            res["emb64"] = W.corr_embeds(self.pyr64, self.sup64, self.coords, model()["p64"], self.chunk, on_volume=look)
            return res
        return self.cached("corr", make)

    # ---- HIP outputs per back end ----------------------------------------------------------------------------------------------
    def pw(self, precision):
        return model()["m"].packed(dev(), precision)

    def x_corr(self, precision):
        """ops.corr_embed at the default chunking: x [N*S,1120], columns < 1024 written."""
        def make():
            from cotracker_amd import ops
            x = ops.corr_embed(self.window(), self.pw(precision))
            torch.cuda.synchronize()
            return x
        return self.cached(("x_corr", precision), make)

    def x_full(self, precision):
        def make():
            from cotracker_amd import ops
            x = ops.assemble_tokens(self.window(), self.x_corr(precision).clone())
            torch.cuda.synchronize()
            return x
        return self.cached(("x_full", precision), make)

    def x_ref(self, precision):
        """The HIP x as the float64 former wants it: reference column order [vis, conf, corr, posenc], time embedding added
        (the library folds it into the per-frame bias rows of the input projection, ctk_model_weights.in_bias_t)."""
        x = self.x_full(precision).double().reshape(self.N, self.S, -1)
        xr = torch.cat([x[..., 1024:1026], x[..., 0:1024], x[..., 1026:1110]], dim=-1)
        return xr + W.time_embed(model()["p64"], self.S)

    def delta_hip(self, precision):
        def make():
            from cotracker_amd import ops
            d = ops.update_former(self.x_full(precision), self.S, self.N, self.pw(precision)).reshape(self.N, self.S, 4)
            torch.cuda.synchronize()
            return d
        return self.cached(("delta", precision), make)

    def former(self, precision):
        """Stage 5's measurement: the float64 former on the HIP x after every depth, the same in float32 torch (the noise
        floor), the HIP delta, and the bar that follows: 3e-5, or max(3e-5, 3 x floor) <= 1e-4 where 3e-5 does not hold."""
        def make():
            ref = W.update_former(self.x_ref(precision), model()["p64"], each_depth=True)
            f32 = W.update_former(self.x_ref(precision).float(), model()["p32"], each_depth=True)
            floor = [check(a, b) for a, b in zip(f32, ref)]
            w = check(self.delta_hip(precision), ref[-1])
            bar = BAR["former"] if w[0] <= BAR["former"] else min(BAR["former_cap"], max(BAR["former"], 3 * floor[-1][0]))
            return {"ref": ref, "floor": floor, "worst": w, "bar": bar}
        return self.cached(("former", precision), make)

    def free_run64(self):
        """Six float64 iterations from the float64 image of the start state (independent of the back end)."""
        return self.cached("free64", lambda: W.forward_window(self.pyr64, self.coords.double(), self.sup64, self.vis.double(),
                                                              self.conf.double(), model()["p64"], 6, RES, STRIDE, self.chunk))


_cases = {}


def get_case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.fixture(scope="module", params=list(SHAPES))
def case(request):
    return get_case(request.param)


def former_ex(cs, precision, depth):
    """ctk_update_former_ex on the CoTracker3 weights with `depth` layers: delta [N,S,4] after that many layers.  (Its heads run as
    a Linear with 64 zero-padded output columns, not through the fused heads kernel -- ops.update_former covers that one.)"""
    from cotracker_amd import _lib as L, ops
    pw, sd = cs.pw(precision), model()["p32"]
    st = pw.struct_for(cs.S)
    fw = L.FormerWeights()
    fw.depth, fw.in_dim, fw.in_ld, fw.out_dim, fw.out_ld = depth, L.X_DIM, L.X_LD, 4, 64
    fw.in_w, fw.in_p, fw.in_bias_t, fw.virtual_tokens = st.in_w, st.in_p, st.in_bias_t, st.virtual_tokens
    in_b = pw.in_b.contiguous()
    head_w, head_b = torch.zeros(64, L.HID, device=dev()), torch.zeros(64, device=dev())
    head_w[:4] = torch.cat([sd["updateformer.flow_head.weight"], sd["updateformer.vis_conf_head.weight"]])
    head_b[:4] = torch.cat([sd["updateformer.flow_head.bias"], sd["updateformer.vis_conf_head.bias"]])
    fw.in_b, fw.head_w, fw.head_p, fw.head_b = in_b.data_ptr(), head_w.data_ptr(), None, head_b.data_ptr()
    for blocks in ("time_blocks", "virtual2point", "virtual_self", "point2virtual"):
        setattr(fw, blocks, C.cast(getattr(st, blocks), C.POINTER(L.BlockWeights)))
    d = ops.update_former_ex(cs.x_full(precision), False, cs.S, cs.N, fw, None)
    torch.cuda.synchronize()  # (in_b / head_w / head_b stay alive until here)
    return d.reshape(cs.N, cs.S, 64)


# ------------------------------------------------------------------------------------------
# stage 0: what the inputs are
# ------------------------------------------------------------------------------------------
def test_inputs_move_leave_the_frame_and_hit_lattice_points(case):
    c = case.coords
    S, N = case.S, case.N
    step = (c[1:] - c[:-1]).abs()
    assert 0.05 < float(step.mean()) and float(step.max()) <= 1.0           # level-0 units per frame (x 4 = px)
    out = [(c[..., 0] < 0).any(0), (c[..., 0] > HW[1] - 1).any(0), (c[..., 1] < 0).any(0), (c[..., 1] > HW[0] - 1).any(0)]
    for side in out:
        assert 0.005 * N <= int(side.sum()) <= 0.05 * N                      # a few per cent of the tracks leave on each side
    assert int(((c == c.round()).all(-1)).sum()) >= 0.015 * S * N           # integer taps: weight exactly 0 / 1
    assert int((((c * 2) == (c * 2).round()) & (c != c.round())).all(-1).sum()) >= 0.01 * S * N
    # the pyramid the float64 stages read is the library's own (average pooling is pinned by test_normalize_and_pool); in float64
    # the pooled levels agree with pooling level 0 again
    for l in range(1, 4):
        ref = torch.nn.functional.avg_pool2d(case.pyr64[l - 1], 2, stride=2)
        assert float((case.pyr64[l] - ref).abs().max()) <= 1e-7


# ------------------------------------------------------------------------------------------
# stage 1: support features
# ------------------------------------------------------------------------------------------
def test_stage1_support(case):
    with torch.no_grad():
        ref = W.support(case.pyr64, case.qf, case.qc)
    worst = None
    for l in range(4):
        worst = worse(worst, check(case.sup[l], ref[l].permute(1, 0, 2)) + (f"level {l} (frame = support tap, column = channel)",))
    record(case.name, None, "1_support", **w2d(worst))
    expect("stage 1, sample_support", worst, BAR["support"])


# ------------------------------------------------------------------------------------------
# stage 2: correlation volume, three kernels, four levels
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["f32", "sh_v3", "sh_v1"])
def test_stage2_volume(case, which):
    res = case.corr_pass()
    record(case.name, None, "2_volume_" + which, pad_max=res["pad"][which], masked_max=res["masked"][which], **w2d(res["worst"][which]))
    assert res["pad"][which] == 0.0, "padding columns >= 2401 must be exactly 0"
    assert res["masked"][which] == 0.0, "masked tracks must give an exactly zero volume"
    expect(f"stage 2, correlation volume ({which})", res["worst"][which], BAR["volume"])


# ------------------------------------------------------------------------------------------
# stage 3: corr_embed
# ------------------------------------------------------------------------------------------
def test_stage3_corr_embed(case, precision):
    from cotracker_amd import ops
    S, N = case.S, case.N
    x = case.x_corr(precision)
    w = check(x[:, :1024].reshape(N, S, 1024), case.corr_pass()["emb64"].permute(1, 0, 2))
    record(case.name, precision, "3_corr_embed", **w2d(w))
    expect("stage 3, corr_embed (column = 256 * level + channel)", w, BAR["corr_embed"])
    win = case.window()
    win.args.points_per_chunk = CUT_INSIDE_A_TILE[case.name]
    assert (win.args.points_per_chunk * S) % 256 != 0 and win.args.points_per_chunk < N
    assert torch.equal(ops.corr_embed(win, case.pw(precision)), x), "chunking of the correlation stage changed x"


# ------------------------------------------------------------------------------------------
# stage 4: assemble_tokens, f32 and SH x
# ------------------------------------------------------------------------------------------
def test_stage4_assemble_tokens(case, precision):
    from cotracker_amd import _lib as L, ops
    S, N = case.S, case.N
    before, x = case.x_corr(precision), case.x_full(precision)
    with torch.no_grad():
        vc, pe = W.posenc_tokens(case.coords.double(), case.vis.double(), case.conf.double(), RES, STRIDE)
    xr = x.reshape(N, S, -1)
    assert torch.equal(xr[..., 1024:1026], vc.float()), "vis / conf columns must be copies"
    w = check(xr[..., 1026:1110], pe)
    assert float(x[:, 1110:].abs().max()) == 0.0 and torch.equal(x[:, :1024], before[:, :1024])
    # the SH form of the same call: the same values, split, and nothing else touched
    xs = ops.split_rows(before)
    untouched = xs[:, :32].clone()
    L.check(L.load().ctk_assemble_tokens(C.byref(case.window().args), xs.data_ptr(), 1, torch.cuda.current_stream().cuda_stream),
            "ctk_assemble_tokens")
    torch.cuda.synchronize()
    assert torch.equal(xs[:, :32], untouched), "SH columns < 1024 touched"
    full = ops.unsplit(xs).reshape(N, S, -1)
    w_sh = check(full[..., 1026:1110], pe)
    same = torch.equal(xs[:, 32:], ops.split_rows(x)[:, 32:])
    record(case.name, precision, "4_assemble_tokens", sh_posenc_max=w_sh[0], sh_equals_split_of_f32=same, **w2d(w))
    expect("stage 4, posenc (f32 x; column = posenc element)", w, BAR["posenc"])
    expect("stage 4, posenc (SH x)", w_sh, BAR["posenc"])
    assert float(full[..., 1110:].abs().max()) == 0.0
    assert same, "SH assemble_tokens is not the split of the f32 one"


# ------------------------------------------------------------------------------------------
# stage 5: update_former
# ------------------------------------------------------------------------------------------
def test_stage5_update_former(case, precision):
    m = case.former(precision)
    by_depth = []
    for d in (1, 2, 3):
        by_depth.append(check(former_ex(case, precision, d)[..., :4], m["ref"][d - 1]))
    record(case.name, precision, "5_update_former", bar=m["bar"], float32_torch_floor=[f[0] for f in m["floor"]],
           by_depth=[w[0] for w in by_depth], **w2d(m["worst"]))
    assert m["bar"] <= BAR["former_cap"]
    for d, w in enumerate(by_depth, 1):  # the first wrong depth is named first
        expect(f"stage 5, update former after depth {d} of 3 (ctk_update_former_ex; column = dx, dy, dvis, dconf)", w, m["bar"])
    expect("stage 5, update former (column = dx, dy, dvis, dconf)", m["worst"], m["bar"])


# ------------------------------------------------------------------------------------------
# stage 6: one iteration through the window call (fused heads + state update, overlap streams)
# ------------------------------------------------------------------------------------------
def compare_state(ours, ref, px_scale=1.0):
    """(coords, vis, conf) [S,N,..] of both sides -> {"coords": worst, "vis": worst, "conf": worst}; coords x px_scale."""
    out = {}
    for k, a, b in zip(("coords", "vis", "conf"), ours, ref):
        s = px_scale if k == "coords" else 1.0
        out[k] = check(tsn(a.double() * s), tsn(b * s))
    return out


def test_stage6_one_iteration(case, precision):
    from cotracker_amd import ops
    st = case.state()
    ops.forward_window(case.window(st, iters=1), case.pw(precision))
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = W.iterate((case.coords, case.vis, case.conf), case.pyr64, case.sup64, model()["p64"], RES, STRIDE, case.chunk)
    bar = case.former(precision)["bar"]
    w = compare_state(st, ref)
    record(case.name, precision, "6_one_iteration", bar=bar, **{k: w2d(v) for k, v in w.items()})
    for k, v in w.items():
        expect(f"stage 6, one iteration of forward_window, {k} (level-0 units / logits)", v, bar)
    assert float((st[0] - case.coords).abs().max()) > 1e-3  # the iteration moved the tracks


# ------------------------------------------------------------------------------------------
# stage 7: six iterations, free-running, every point
# ------------------------------------------------------------------------------------------
def test_stage7_six_iterations(case, precision):
    from cotracker_amd import ops
    st = case.state()
    ops.forward_window(case.window(st, iters=6), case.pw(precision))
    torch.cuda.synchronize()
    ref = case.free_run64()
    w = compare_state(st, ref, px_scale=float(STRIDE))
    moved = float((ref[0] - case.coords.double()).abs().max()) * STRIDE
    record(case.name, precision, "7_six_iterations", moved_px=moved, **{k: w2d(v) for k, v in w.items()})
    expect("stage 7, six iterations, coords (px at model resolution)", w["coords"], BAR["px"])
    expect("stage 7, six iterations, vis logit", w["vis"], BAR["logit"])
    expect("stage 7, six iterations, conf logit", w["conf"], BAR["logit"])


# ------------------------------------------------------------------------------------------
# stage 8: joint and shared calls at a size where the persistent kernels engage
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["joint", "shared"])
def test_stage8_joint_and_shared_calls(form, precision):
    """B = 2 windows of N = 3200 over two different videos (ops.forward_windows), and G = 2 query groups of 3200 over one video
    (shared=True): one iteration, every window against the float64 single-window iteration at stage 6's bar."""
    from cotracker_amd import ops
    cs = get_case("c3")
    S, N, h = cs.S, cs.N, cs.N // 2
    pw, p64 = cs.pw(precision), model()["p64"]
    halves = [slice(0, h), slice(h, N)]
    coords = torch.stack([cs.coords[:, s_] for s_ in halves]).contiguous()                 # [2,S,h,2]
    vis = torch.stack([cs.vis[:, s_] for s_ in halves]).contiguous()
    conf = torch.stack([cs.conf[:, s_] for s_ in halves]).contiguous()
    start = [(coords[g].clone(), vis[g].clone(), conf[g].clone()) for g in range(2)]
    if form == "shared":
        pyrs, pyrs64, sup = [cs.pyr, cs.pyr], [cs.pyr64, cs.pyr64], cs.sup                # support [2*h,49,128]: group g = rows g*h ..
        wins = ops.group_windows(cs.pyr, sup, coords, vis, conf, SCALE_XY, iters=1)
        sups = [[s_[g * h:(g + 1) * h] for s_ in sup] for g in range(2)]
    else:
        pyr_b = ops.build_pyramid(features(S, seed=200))
        pyrs = [cs.pyr, pyr_b]
        pyrs64 = [cs.pyr64, [f.permute(0, 3, 1, 2).double().contiguous() for f in pyr_b]]
        sups = [[s_[:h].contiguous() for s_ in cs.sup],
                [ops.sample_support(pyr_b[l], cs.qf[h:].float(), (cs.qc[h:] / 2 ** l).contiguous()) for l in range(4)]]
        wins = [ops.Window(pyrs[g], sups[g], coords[g], vis[g], conf[g], SCALE_XY, iters=1) for g in range(2)]
    ops.forward_windows(wins, pw, shared=(form == "shared"))
    torch.cuda.synchronize()
    bar = cs.former(precision)["bar"]
    worst = {}
    for g in range(2):
        with torch.no_grad():
            ref = W.iterate(start[g], pyrs64[g], Case.sup64_of(sups[g], None), p64, RES, STRIDE, F64_CHUNK)
        for k, v in compare_state((coords[g], vis[g], conf[g]), ref).items():
            worst[k] = worse(worst.get(k), (v[0], v[1] + g * h) + v[2:] + (f"window {g}",))
    record("c3", precision, "8_" + form, bar=bar, **{k: w2d(v) for k, v in worst.items()})
    for k, v in worst.items():
        expect(f"stage 8, {form} call of 2 x 3200 tracks, {k}", v, bar)


# ------------------------------------------------------------------------------------------
# negative controls: the checker sees a small fault where it is, and the bars bite
# ------------------------------------------------------------------------------------------
def test_checker_finds_a_planted_block_and_a_zeroed_volume_row():
    from cotracker_amd import _lib, ops
    cs = get_case("c3")
    S, N = cs.S, cs.N
    ref = cs.corr_pass()["emb64"].permute(1, 0, 2)
    bad = cs.x_corr("f16x3")[:, :1024].reshape(N, S, 1024).double().clone()
    n0, c0, bar = 4711, 600, BAR["corr_embed"]
    bad[n0, :, c0:c0 + 16] = ref[n0, :, c0:c0 + 16] + 4 * bar        # 16 rows (track 4711, every frame) x 16 columns
    bad[n0, 5, c0 + 7] = ref[n0, 5, c0 + 7] + 5 * bar                  # ... and its peak
    w = check(bad, ref)
    assert w[1:] == (n0, 5, c0 + 7) and abs(w[0] - 5 * bar) < 1e-9
    with pytest.raises(AssertionError, match=r"track n=4711, frame t=5, column 607"):
        expect("planted", w, bar)
    # stage 2: the volume rows of one track at one frame, zeroed
    n, t, l = 3333, 9, 1
    with torch.no_grad():
        vref = W.volume(cs.pyr64[l], cs.sup64[l][:, n:n + 1], cs.coords[:, n:n + 1] / 2 ** l).permute(1, 0, 2)
    win = ops.Window(cs.pyr, [s_[n:n + 1].contiguous() for s_ in cs.sup], cs.coords[:, n:n + 1].contiguous(), cs.vis[:, n:n + 1].contiguous(),
                     cs.conf[:, n:n + 1].contiguous(), SCALE_XY)
    vol = ops.unsplit(ops.corr_volume_sh(win)[l])[:, :_lib.CORR_K].reshape(1, S, _lib.CORR_K)
    assert check(vol, vref, n)[0] <= BAR["volume"]
    vol[0, t] = 0
    w = check(vol, vref, n)
    assert w[0] > 10 * BAR["volume"] and w[1:3] == (n, t)
    record("c3", None, "control_zeroed_volume_row", ratio_to_bar=w[0] / BAR["volume"])


def test_mutation_dropped_k_tile_of_one_fc2(precision):
    """The float64 reference without 32 of the 1536 reduction columns of ONE mlp.fc2 (points<-virtual block, layer 1)."""
    cs = get_case("c3")
    m = cs.former(precision)
    p = dict(model()["p64"])
    k = "updateformer.space_point2virtual_blocks.1.mlp.fc2.weight"
    p[k] = p[k].clone()
    p[k][:, 512:544] = 0
    with torch.no_grad():
        w = check(cs.delta_hip(precision), W.update_former(cs.x_ref(precision), p))
    record("c3", precision, "mutation_fc2_k_tile", ratio_to_bar=w[0] / m["bar"], bar=m["bar"])
    assert w[0] >= 10 * m["bar"], f"a dropped 32-column K tile of one fc2 moves stage 5 by {w[0] / m['bar']:.1f} x its bar only"


def test_mutation_dropped_key_tile_of_one_head(precision):
    """The float64 reference without 32 of the 6400 point keys in one head of ONE virtual<-points attention (head 3, keys 1830..1861).

    MEASURED (profiles/window_stages.json): this fault does NOT reach stage 5's bar.  64 virtual tracks average over 6400 keys and
    reach delta only through points<-virtual, so one 32-key tile moves delta by 0.1-0.4 x the bar (layer 2 .. layer 0), 512 keys by
    0.3-1.3 x, and half of all keys of one head by 1-5 x.  The smallest fault of this attention that the 3e-5 bar sees is therefore
    about 512 keys of one head in layer 0 or 1 -- e.g. one lost key split of v2p_splits(6400) = 7 -- and a single tile only shows
    against the MEASURED error (2.4e-6 split-half, 1.0e-6 exact f32), which is what this test asserts; the bar stays where it is."""
    cs = get_case("c3")
    m = cs.former(precision)
    ratios = {}
    for layer, width in ((0, 32), (1, 32), (0, 915)):
        with torch.no_grad():
            ref = W.update_former(cs.x_ref(precision), model()["p64"], faults={"v2p_keys": (layer, 3, 1830, 1830 + width)})
        ratios[f"layer{layer}_keys{width}"] = check(cs.delta_hip(precision), ref)[0] / m["bar"]
    record("c3", precision, "mutation_v2p_key_tile", ratio_to_bar=ratios, bar=m["bar"], unmutated_ratio_to_bar=m["worst"][0] / m["bar"])
    assert ratios["layer0_keys32"] * m["bar"] >= 2 * m["worst"][0] and ratios["layer1_keys32"] * m["bar"] >= 2 * m["worst"][0]
    assert ratios["layer0_keys915"] >= 2.0  # one key split of seven, lost: above the bar, but not by 10 x


def test_mutation_dropped_tap_of_one_level(precision):
    """The float64 reference without ONE of the 49 taps of the frame patch on ONE level (tap 17 of level 2)."""
    cs = get_case("c3")
    S, N = cs.S, cs.N
    n1 = 800  # the first float64 chunk is enough to see it
    seen = {}

    def drop(l, a, b, vol):
        if l != 2:
            return None
        vol = vol.clone()
        vol[..., 17 * 49:18 * 49] = 0
        seen["volume"] = check(ops_volume[:, :, :2401], vol.permute(1, 0, 2))
        return vol

    from cotracker_amd import ops
    sub = ops.Window(cs.pyr, [s_[:n1].contiguous() for s_ in cs.sup], cs.coords[:, :n1].contiguous(), cs.vis[:, :n1].contiguous(),
                     cs.conf[:, :n1].contiguous(), SCALE_XY)
    ops_volume = ops.unsplit(ops.corr_volume_sh(sub)[2]).reshape(n1, S, -1)
    with torch.no_grad():
        emb = W.corr_embeds(cs.pyr64, [s_[:, :n1] for s_ in cs.sup64], cs.coords[:, :n1], model()["p64"], n1, on_volume=drop)
    w = check(cs.x_corr(precision)[:n1 * S, :1024].reshape(n1, S, 1024), emb.permute(1, 0, 2))
    record("c3", precision, "mutation_dropped_tap", ratio_to_bar_corr_embed=w[0] / BAR["corr_embed"],
           ratio_to_bar_volume=seen["volume"][0] / BAR["volume"])
    assert seen["volume"][0] >= 10 * BAR["volume"]
    assert 512 <= w[3] < 768, "the fault is on level 2"
    assert w[0] >= 10 * BAR["corr_embed"], f"a dropped tap moves stage 3 by {w[0] / BAR['corr_embed']:.1f} x its bar only"
