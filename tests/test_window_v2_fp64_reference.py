"""Pin oracle/window_v2_fp64.py -- the float64 reference of tests/test_gpu_window_v2_stages.py -- on the CPU, in float32 and in
float64, against what the UNMODIFIED reference wrote (tests/golden/cotracker2.npz, corrblock.npz), at the bars
tests/test_oracle_golden.py holds the numpy oracle to.  Needs no GPU.

With head_scale = 1 the CoTracker2 map amplifies a rounding difference about 15-20 x per iteration, so only the float32 run is
compared free-running with the three-iteration golden.  In float64 (and in float32 again) every stage is pinned TEACHER-FORCED on
the per-iteration trace of the numpy oracle (O.forward_window_v2(..., trace=), itself pinned on the same goldens): iteration k is
fed the oracle's state after iteration k - 1, and each stage output is held to its stage bar.  The free-running float64-vs-float32
gap is printed per iteration: the yardstick DESIGN.md section 2 quotes ("stage parity of the CoTracker2 window")."""
import numpy as np
import pytest
import torch

from oracle import cotracker_oracle as O
from oracle import window_v2_fp64 as V

DTYPES = [torch.float32, torch.float64]
# by source: former / window bars of tests/test_oracle_golden.py (test_cotracker2_update_former_with_masks, test_cotracker2_forward_window),
# the CorrBlock bar of its test_corrblock_oracle; the stage bars of the teacher-forced run are the GPU stage file's
BARS = {"uf_delta": 3e-5, "cb_out": 2e-6, "fw_coords_px": 1e-3, "fw_logit": 3e-4,
        "x": 1e-6,          # x max(1, max |x|): sampled values and sin / cos, support / posenc bar of the C3 stage file
        "delta": 3e-5,      # the former bar
        "coords": 3e-5,     # coords + delta[:, :2] of a delta at the former bar
        "track_feat": 2e-5,  # tests/test_gpu_gemm_matrix.py::tol_for("f32", .), the exact-f32 Linear bound
        "vis": 1e-4}


def params(dtype):
    from cotracker_amd.model_v2 import CoTracker2
    from cotracker_amd.weights import fill_synthetic_
    m = CoTracker2(window_len=8, stride=4, model_resolution=(64, 96)).eval()
    fill_synthetic_(m, seed=6, head_scale=1.0)
    return V.cast_params(m.state_dict(), "cpu", dtype)


def T(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def err(a, b):
    return float((a.double() - torch.from_numpy(np.asarray(b)).double()).abs().max())


def window_inputs(g, dtype, coords_dtype=torch.float32):
    """forward_window's arguments from cotracker2.npz, batch axis dropped; track_feat masked as the model does (cotracker.py:346).
    The coordinates stay float32 unless asked otherwise: where a tap lands is part of what the reference computes (window_fp64._grid),
    and float32 coordinates are what the GPU stage tests hand the float64 text."""
    amask = g["fw_attention_mask"][0]
    assert (amask == amask[0:1]).all()
    return dict(pyr=V.pyramid(T(g["fw_fmaps"][0], dtype)), coords=T(g["fw_coords"][0], coords_dtype),
                track_feat=T(amask[..., None] * g["fw_track_feat"][0], dtype), vis=T(g["fw_vis"][0, ..., 0], dtype),
                track_mask=T(g["fw_track_mask"][0, ..., 0], dtype), mask=torch.from_numpy(amask[0]))


@pytest.fixture(scope="module")
def oracle_trace(golden):
    g = golden("cotracker2")
    p = {k: v.numpy() for k, v in params(torch.float32).items()}
    amask = g["fw_attention_mask"]
    trace = []
    c, v = O.forward_window_v2(g["fw_fmaps"], g["fw_coords"], amask[..., None] * g["fw_track_feat"], g["fw_vis"], g["fw_track_mask"],
                               amask, p, iters=3, trace=trace)
    assert np.abs(c * 4.0 - g["fw_out_coords"]).max() < BARS["fw_coords_px"] and np.abs(v - g["fw_out_vis"]).max() < BARS["fw_logit"]
    return trace, v


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_masked_former_matches_the_reference_golden(golden, dtype):
    g = golden("cotracker2")
    with torch.no_grad():
        outs = V.update_former(T(g["uf_x"][0], dtype), params(dtype), torch.from_numpy(g["uf_mask"]), each_depth=True)
    assert g["uf_mask"].shape == (8, 10) and not g["uf_mask"].all() and len(outs) == 6
    e = err(outs[-1], g["uf_delta"][0])
    print(f"\nmasked former in {dtype} vs cotracker2.npz: {e:.3e}")
    assert e <= BARS["uf_delta"]
    assert err(outs[0], g["uf_delta"][0]) > 1e-2  # the per-depth deltas are different things


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_corrblock_matches_the_reference_golden(golden, dtype):
    g = golden("corrblock")
    pyr = V.pyramid(T(g["cb_fmaps"][0], dtype))
    seen = []
    with torch.no_grad():
        out = V.corrblock(pyr, T(g["cb_targets"][0], dtype), T(g["cb_coords"][0], torch.float32), chunk=5,
                          on_volume=lambda l, n0, n1, v: seen.append((l, n0, n1, err(v, g[f"cb_corrs{l}"][0][:, n0:n1]))))
    assert [s_[:3] for s_ in seen] == [(l, n0, min(12, n0 + 5)) for l in range(4) for n0 in (0, 5, 10)]
    assert max(s_[3] for s_ in seen) <= BARS["cb_out"]                # the volumes themselves (cb_corrs*)
    e = err(out, g["cb_out"])
    print(f"\ncorrblock in {dtype} vs corrblock.npz: {e:.3e} at max |cb_out| = {float(np.abs(g['cb_out']).max()):.2f}")
    assert e <= BARS["cb_out"]


GOLDEN_THREADS = 8  # tests/golden/make_golden.py writes every golden under torch.set_num_threads(8)


def test_float32_window_matches_the_reference_golden_free_running(golden):
    """Three free-running float32 iterations reproduce the golden only in the golden's own reduction order: the map amplifies the
    rounding of a differently partitioned float32 GEMM like any other difference.  Measured here at 8 / 4 / 2 / 1 intra-op threads:
    3.1e-5 / 1.7e-4 / 8.0e-5 / 1.8e-4 px and 8.3e-5 / 5.2e-4 / 6.3e-4 / 4.3e-4 logit against the 3e-4 bar -- and an earlier test of
    the session may have left another count (tests/test_bench_contract.py runs a 2-thread benchmark in process).  So this test runs
    at the count the golden was written with and puts the session's back; the bars are test_oracle_golden's, unchanged."""
    g = golden("cotracker2")
    a = window_inputs(g, torch.float32)
    threads = torch.get_num_threads()
    torch.set_num_threads(GOLDEN_THREADS)
    try:
        with torch.no_grad():
            c, v, _ = V.forward_window(a["pyr"], a["coords"], a["track_feat"], a["vis"], a["track_mask"], a["mask"], params(torch.float32),
                                       3, chunk=4)
    finally:
        torch.set_num_threads(threads)
    ec, ev = err(c * 4.0, g["fw_out_coords"][0]), err(v, g["fw_out_vis"][0])
    print(f"\nfloat32 window, three free-running iterations vs cotracker2.npz: {ec:.3e} px, {ev:.3e} logit")
    assert ec <= BARS["fw_coords_px"] and ev <= BARS["fw_logit"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_every_stage_teacher_forced_on_the_oracle_trace(golden, oracle_trace, dtype):
    g = golden("cotracker2")
    trace, vis_out = oracle_trace
    a, p = window_inputs(g, dtype), params(dtype)
    rows, worst = [], {}
    with torch.no_grad():
        pos = V.pos(p, a["coords"][0])
        coords, feat = a["coords"], a["track_feat"]
        for k, tr in enumerate(trace):
            x_or, d_or = T(tr["x"], dtype), T(tr["delta"][0], dtype)
            x = V.tokens(coords, V.corrblock(a["pyr"], feat, coords, chunk=3), feat, a["track_mask"], a["vis"], pos, p)
            delta = V.update_former(x_or, p, a["mask"])
            new_coords, normed = V.apply_delta(coords, d_or, p)
            new_feat = V.updater(normed, feat, p)
            e = {"x": err(x, tr["x"]) / max(1.0, float(np.abs(tr["x"]).max())), "delta": err(delta, tr["delta"][0]),
                 "coords": err(new_coords, tr["coords"][0]), "track_feat": err(new_feat, tr["track_feat"][0])}
            rows.append(f"iteration {k}: " + ", ".join(f"{n} {v:.2e}" for n, v in e.items()))
            for n, v in e.items():
                worst[n] = max(worst.get(n, 0.0), v)
            coords, feat = T(tr["coords"][0], torch.float32), T(tr["track_feat"][0], dtype)       # the ORACLE's state feeds the next one
        worst["vis"] = err(V.vis_head(feat, p), vis_out[0])
    print(f"\nteacher-forced on the numpy oracle's trace, {dtype} (max abs; x relative to max(1, max |x|)):\n  " + "\n  ".join(rows) +
          f"\n  vis head {worst['vis']:.2e}")
    for n, v in worst.items():
        assert v <= BARS[n], f"{n} in {dtype}: {v:.3e} > {BARS[n]:.0e}"


def test_free_running_float64_vs_float32_gap_is_printed(golden):
    """Not a bar: what the map amplifies.  Only that one iteration stays a decade under the former bar is asserted."""
    g = golden("cotracker2")
    tr = {}
    with torch.no_grad():
        for dt in DTYPES:
            a, tr[dt] = window_inputs(g, dt, dt), []
            V.forward_window(a["pyr"], a["coords"], a["track_feat"], a["vis"], a["track_mask"], a["mask"], params(dt), 3, trace=tr[dt])
    p64 = params(torch.float64)
    rows = []
    for k in range(3):
        px = 4.0 * float((tr[torch.float64][k]["coords"] - tr[torch.float32][k]["coords"].double()).abs().max())
        lg = float((V.vis_head(tr[torch.float64][k]["track_feat"], p64) - V.vis_head(tr[torch.float32][k]["track_feat"].double(), p64)).abs().max())
        rows.append((px, lg))
    print("\nfloat64 vs float32 of oracle/window_v2_fp64.py, free-running at S=8, N=10, head_scale=1:\n  " +
          "\n  ".join(f"after {k + 1} iteration(s): {px:.2e} px, {lg:.2e} logit" for k, (px, lg) in enumerate(rows)))
    assert rows[0][0] <= 4 * 3e-6 and rows[0][1] <= 3e-5
    assert rows[2][0] > rows[0][0]  # it grows: a free-running comparison at head_scale = 1 measures the map, not the code


def test_planted_faults_change_the_reference(golden):
    """Every fault hook of the module does what the negative controls of the GPU stage tests rely on: it moves the output of its
    own stage, and the hooks that take a position only act there."""
    g = golden("cotracker2")
    a, p = window_inputs(g, torch.float64), params(torch.float64)
    N = a["coords"].shape[1]
    mask = a["mask"].clone()
    mask[[2, 7]] = False
    with torch.no_grad():
        pos = V.pos(p, a["coords"][0])
        fc = V.corrblock(a["pyr"], a["track_feat"], a["coords"])
        bad = V.corrblock(a["pyr"], a["track_feat"], a["coords"], faults={"drop_tap": (2, 17)})
        assert float((fc - bad).abs()[..., 2 * 49 + 17].max()) > 0 and float(bad[..., 2 * 49 + 17].abs().max()) == 0
        keep = torch.ones(196, dtype=torch.bool)
        keep[2 * 49 + 17] = False
        assert torch.equal(fc[..., keep], bad[..., keep])
        zero = V.corrblock(a["pyr"], a["track_feat"], a["coords"], on_volume=lambda l, n0, n1, v: v * 0 if l == 1 else None)
        assert float(zero[..., 49:98].abs().max()) == 0 and torch.equal(zero[..., :49], fc[..., :49])
        x = V.tokens(a["coords"], fc, a["track_feat"], a["track_mask"], a["vis"], pos, p)
        sw = V.tokens(a["coords"], fc, a["track_feat"], a["track_mask"], a["vis"], pos, p, faults={"swap_xy": True})
        assert float((x - sw)[..., 2:130].abs().max()) > 1e-3 and torch.equal(x[..., 130:], sw[..., 130:]) and torch.equal(x[..., :2], sw[..., :2])
        st = V.tokens(a["coords"], fc, a["track_feat"], a["track_mask"], a["vis"], pos, p, faults={"swap_time": 3})
        assert float((x - st)[:, 3:5].abs().max()) > 1e-3 and torch.equal(x[:, :3], st[:, :3]) and torch.equal(x[:, 5:], st[:, 5:])
        good = V.update_former(x, p, mask)
        assert float((good - V.update_former(x, p, None)).abs().max()) > 1e-4        # the mask matters at all
        for f in ({"v2p_unmask": (1, 2, 0, N)}, {"p2v_unmask": 4}):
            assert float((good - V.update_former(x, p, mask, faults=f)).abs().max()) > 1e-6, f
        assert torch.equal(good, V.update_former(x, p, mask, faults={"v2p_unmask": (1, 2, 3, 7)}))   # no masked key in 3..6: nothing changes
        c1, n1 = V.apply_delta(a["coords"], good, p)
        c2, n2 = V.apply_delta(a["coords"], good, p, faults={"unbiased": True})
        assert torch.equal(c1, c2) and float((n1 - n2).abs().max()) > 1e-3
        assert float((V.updater(n1, a["track_feat"], p) - V.updater(n1, a["track_feat"], p, faults={"tanh_gelu": True})).abs().max()) > 1e-5
