"""Pin oracle/window_fp64.py -- the float64 reference of tests/test_gpu_window_stages.py -- on the CPU, in float32 and in
float64, against what the UNMODIFIED reference wrote (tests/golden/ops.npz, update_former.npz), at the bars
tests/test_oracle_golden.py holds the numpy oracle to.  Needs no GPU.

It also prints how far float64 and float32 of the same text are apart at every stage: the yardstick for the errors the GPU
stage tests measure ("stage parity at the C3 window shape")."""
import numpy as np
import pytest
import torch

from oracle import window_fp64 as W

DTYPES = [torch.float32, torch.float64]
BARS = {"support": 2e-6, "corr_volume": 2e-6, "corr_emb": 1e-5, "posenc": 1e-6, "uf_delta": 2e-5, "uf_y_full": 5e-5,
        "fw_coords_px": 1e-3, "fw_logit": 1e-4}
RES = (96, 128)  # model resolution of the ops.npz goldens (a 24 x 32 level-0 map at stride 4)


def params(dtype, window_len=8, seed=3, head_scale=None):
    from cotracker_amd.model import CoTrackerThreeOnline
    from cotracker_amd.weights import fill_synthetic_
    m = CoTrackerThreeOnline(stride=4, corr_radius=3, window_len=window_len, model_resolution=RES).eval()
    fill_synthetic_(m, seed=seed, **({} if head_scale is None else {"head_scale": head_scale}))
    return W.cast_params(m.state_dict(), "cpu", dtype)


def T(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def err(a, b):
    return float((a.double() - torch.from_numpy(np.asarray(b)).double()).abs().max())


def run_stages(g, dtype):
    """Every stage of the module on the golden inputs, in `dtype`: name -> tensor in the golden's layout (batch axis dropped)."""
    p = params(dtype)
    out = {}
    pyr = [T(g[f"fmaps{l}"][0], dtype) for l in range(4)]
    sup = W.support(pyr, T(g["queried_frames"][0], dtype), T(g["queried_coords"][0], dtype))
    coords = T(g["coords"][0], dtype)
    for l in range(4):
        out[f"support{l}"] = sup[l]
        gsup = T(g[f"support{l}"][0], dtype)  # the stages below start from the golden's support: one stage per comparison
        vol = W.volume(pyr[l], gsup, coords / 2 ** l)
        if l in (0, 3):
            out[f"corr_volume{l}"] = vol
        out[f"corr_emb{l}"] = W.corr_embed(T(g[f"corr_volume{l}"][0], dtype) if l in (0, 3) else vol, p)
    out["posenc_out"] = W.posenc(T(g["posenc_in"], dtype))
    out["uf_delta"] = W.update_former(T(g["uf_x"][0], dtype), p)
    S, N = coords.shape[:2]
    trace = []
    gsup = [T(g[f"support{l}"][0], dtype) for l in range(4)]
    W.forward_window(pyr, T(g["queried_coords"][0], dtype)[None].expand(S, N, 2), gsup, T(g["fw_vis_init"][0, ..., 0], dtype),
                     T(g["fw_conf_init"][0, ..., 0], dtype), p, iters=3, res=RES, chunk=5, trace=trace)
    for it, (c, v, f) in enumerate(trace):
        out[f"fw_coords{it}"], out[f"fw_vis{it}"], out[f"fw_conf{it}"] = c * 4.0, v, f
    return out


def posenc_golden_rounding(x):
    """What the float32 reference itself loses in posenc: it rounds the sine's argument x 2^k + pi/2 to float32 (half an ulp of an
    argument of up to 2^9 |x|), which float64 does not.  Per element of the golden, as an allowance for the float64 run only."""
    x = torch.from_numpy(x).double()
    xb = (x[..., None, :] * 2.0 ** torch.arange(10, dtype=torch.float64)[:, None]).reshape(*x.shape[:-1], -1)
    arg = torch.cat([xb, xb + 0.5 * torch.pi], dim=-1).abs()
    return torch.cat([torch.zeros_like(x), arg * 2.0 ** -23], dim=-1)


def bar_of(name):
    if name.startswith("fw_coords"):
        return BARS["fw_coords_px"]
    if name.startswith("fw_"):
        return BARS["fw_logit"]
    return BARS[name.rstrip("0123456789").replace("posenc_out", "posenc")]


@pytest.fixture(scope="module")
def stages(golden):
    torch.manual_seed(0)
    with torch.no_grad():
        return {dt: run_stages(golden("ops"), dt) for dt in DTYPES}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_every_stage_matches_the_reference_goldens(golden, stages, dtype):
    g = golden("ops")
    for name, ours in stages[dtype].items():
        if name == "posenc_out":
            d = (ours.double() - torch.from_numpy(g[name]).double()).abs()
            allow = posenc_golden_rounding(g["posenc_in"]) if dtype == torch.float64 else 0.0
            assert float((d - allow).max()) <= bar_of(name), f"posenc in {dtype}: {float(d.max()):.3e}"
            continue
        e = err(ours, g[name][0])
        assert e <= bar_of(name), f"{name} in {dtype}: {e:.3e} > {bar_of(name):.0e}"


def test_float64_and_float32_agree_to_the_same_bars(golden, stages):
    rows = []
    for name, a in stages[torch.float64].items():
        e = float((a - stages[torch.float32][name].double()).abs().max())
        rows.append(f"{name:14s} {e:.3e}  (bar {bar_of(name):.0e})")
        if name == "posenc_out":  # arguments of up to 2^9 |x| ~ 1e3 here: the float32 side rounds them (posenc_golden_rounding)
            e = float(((a - stages[torch.float32][name].double()).abs() - posenc_golden_rounding(golden("ops")["posenc_in"])).max())
        assert e <= bar_of(name), rows[-1]
    print("\nfloat64 vs float32 of oracle/window_fp64.py at S=8, N=12 (max abs):\n  " + "\n  ".join(rows))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_update_former_golden_with_large_heads(golden, dtype):
    """tests/golden/update_former.npz: the imported reference's EfficientUpdateFormer on weights whose heads are scaled by 50."""
    g = golden("update_former")
    p = params(dtype, window_len=16, seed=5, head_scale=50.0)
    with torch.no_grad():
        outs = W.update_former(T(g["x"][0], dtype), p, each_depth=True)
    assert err(outs[-1], g["y_full"][0]) <= BARS["uf_y_full"]
    assert len(outs) == 3 and err(outs[0], g["y_full"][0]) > 1e-2  # the per-depth deltas are different things


def test_planted_faults_change_the_reference(golden):
    """The two fault hooks of the module do what the negative controls of the GPU stage tests rely on."""
    g = golden("ops")
    p = params(torch.float64)
    x = T(g["uf_x"][0], torch.float64)
    with torch.no_grad():
        good = W.update_former(x, p)
        bad = W.update_former(x, p, faults={"v2p_keys": (1, 2, 0, 4)})
        assert float((good - bad).abs().max()) > 0
        seen = []
        pyr = [T(g[f"fmaps{l}"][0], torch.float64) for l in range(4)]
        sup = [T(g[f"support{l}"][0], torch.float64) for l in range(4)]
        emb = W.corr_embeds(pyr, sup, T(g["coords"][0], torch.float64), p, chunk=5, on_volume=lambda l, n0, n1, v: seen.append((l, n0, n1)))
    assert seen == [(l, n0, min(12, n0 + 5)) for l in range(4) for n0 in (0, 5, 10)]
    for l in range(4):
        assert err(emb[..., l * 256:(l + 1) * 256], g[f"corr_emb{l}"][0]) <= BARS["corr_emb"]
