"""Pin the numpy oracle against outputs of the UNMODIFIED reference (tests/golden/*.npz,
made by tests/golden/make_golden.py with torch 2.10.0+rocm7.0 on CPU)."""
import numpy as np
import pytest

from oracle import cotracker_oracle as O
from cotracker_amd.weights import synthetic_tensor


def synth_params(shapes, seed):
    return {k: synthetic_tensor(k, s, seed).numpy() for k, s in shapes.items()}


def model_param_shapes(window_len=8):
    """Key set of the CoTracker3 update path without the encoder."""
    sh = {"corr_mlp.fc1.weight": (384, 2401), "corr_mlp.fc1.bias": (384,),
          "corr_mlp.fc2.weight": (256, 384), "corr_mlp.fc2.bias": (256,)}
    u = "updateformer."
    sh[u + "input_transform.weight"] = (384, 1110)
    sh[u + "input_transform.bias"] = (384,)
    sh[u + "flow_head.weight"] = (2, 384)
    sh[u + "flow_head.bias"] = (2,)
    sh[u + "vis_conf_head.weight"] = (2, 384)
    sh[u + "vis_conf_head.bias"] = (2,)
    sh[u + "virual_tracks"] = (1, 64, 1, 384)

    def attn(pfx):
        sh[pfx + "to_q.weight"] = (384, 384)
        sh[pfx + "to_q.bias"] = (384,)
        sh[pfx + "to_kv.weight"] = (768, 384)
        sh[pfx + "to_kv.bias"] = (768,)
        sh[pfx + "to_out.weight"] = (384, 384)
        sh[pfx + "to_out.bias"] = (384,)

    def mlp(pfx):
        sh[pfx + "fc1.weight"] = (1536, 384)
        sh[pfx + "fc1.bias"] = (1536,)
        sh[pfx + "fc2.weight"] = (384, 1536)
        sh[pfx + "fc2.bias"] = (384,)

    for i in range(3):
        for name in ("time_blocks", "space_virtual_blocks"):
            attn(f"{u}{name}.{i}.attn.")
            mlp(f"{u}{name}.{i}.mlp.")
        for name in ("space_point2virtual_blocks", "space_virtual2point_blocks"):
            sh[f"{u}{name}.{i}.norm_context.weight"] = (384,)
            sh[f"{u}{name}.{i}.norm_context.bias"] = (384,)
            attn(f"{u}{name}.{i}.cross_attn.")
            mlp(f"{u}{name}.{i}.mlp.")
    return sh


def oracle_params(seed, window_len=8):
    p = synth_params(model_param_shapes(window_len), seed)
    p["time_emb"] = O.sincos_time_embed(1110, window_len)
    return p


@pytest.mark.parametrize("tag", ["d1", "d1b", "d5"])
def test_sampler_bit_exact(golden, tag):
    g = golden("sampler")
    out = O.bilinear_sampler_5d(g[f"{tag}_input"], g[f"{tag}_coords"])
    assert np.array_equal(out, g[f"{tag}_output"])  # bit-exact incl. OOB and integer coords


def test_support_and_corr_volume(golden):
    g = golden("ops")
    for i in range(4):
        sup = O.get_track_feat(g[f"fmaps{i}"], g["queried_frames"],
                               (g["queried_coords"] / np.float32(2**i)).astype(np.float32))
        assert np.array_equal(sup, g[f"support{i}"])
    B, S, N, _ = g["coords"].shape
    for i in (0, 3):
        cf = O.get_correlation_feat(g[f"fmaps{i}"], (g["coords"].reshape(B * S, N, 2) / np.float32(2**i)))
        vol = O.corr_volume(cf, g[f"support{i}"])
        np.testing.assert_allclose(vol, g[f"corr_volume{i}"], atol=2e-6, rtol=0)


def test_corr_mlp_posenc_timeemb(golden):
    g = golden("ops")
    p = oracle_params(3)
    B, S, N, _ = g["coords"].shape
    for i in (0, 3):
        emb = O.mlp(g[f"corr_volume{i}"].reshape(B * S * N, -1), p, "corr_mlp.", O.gelu_erf)
        np.testing.assert_allclose(emb.reshape(B, S, N, -1), g[f"corr_emb{i}"], atol=5e-6, rtol=0)
    np.testing.assert_allclose(O.posenc(g["posenc_in"]), g["posenc_out"], atol=1e-6, rtol=0)
    np.testing.assert_allclose(p["time_emb"], g["time_emb"], atol=1e-6, rtol=0)
    for t in (5, 8, 12, 24):
        np.testing.assert_allclose(O.interpolate_time_embed(g["time_emb"], t), g[f"time_emb_interp{t}"],
                                   atol=1e-6, rtol=0)


def test_update_former(golden):
    g = golden("ops")
    p = oracle_params(3)
    d = O.update_former(g["uf_x"], p)
    np.testing.assert_allclose(d, g["uf_delta"], atol=2e-5, rtol=0)


def test_forward_window(golden):
    g = golden("ops")
    p = oracle_params(3)
    pyr = [g[f"fmaps{i}"] for i in range(4)]
    sup = [g[f"support{i}"] for i in range(4)]
    B, S, N, _ = g["coords"].shape
    cinit = np.broadcast_to(g["queried_coords"].reshape(B, 1, N, 2), (B, S, N, 2))
    trace = []
    O.forward_window(pyr, cinit, sup, g["fw_vis_init"], g["fw_conf_init"], p, iters=3,
                     model_resolution=(96, 128), trace=trace)
    for it in range(3):
        np.testing.assert_allclose(trace[it]["coords"] * 4.0, g[f"fw_coords{it}"], atol=2e-4, rtol=0)
        np.testing.assert_allclose(trace[it]["vis"][..., 0], g[f"fw_vis{it}"], atol=5e-5, rtol=0)
        np.testing.assert_allclose(trace[it]["conf"][..., 0], g[f"fw_conf{it}"], atol=5e-5, rtol=0)


def _pad_fmaps(fm, window_len, T):
    pad = (window_len - T % window_len) % window_len
    if pad:
        fm = np.concatenate([fm, np.repeat(fm[-1:], pad, axis=0)], axis=0)
    return fm


def logit(p):
    return np.log(p / (1 - p))


def test_model_online_sliding_and_streaming(golden):
    g = golden("model_online")
    p = oracle_params(1)
    fm = O.normalize_fmaps(g["on_fnet"][None])[0]
    T = fm.shape[0]
    c, v, f = O.model_forward_online(_pad_fmaps(fm, 8, T)[None], g["on_queries"], p, window_len=8, iters=4,
                                     model_resolution=(64, 96), T=T)
    np.testing.assert_allclose(c, g["on_coords"], atol=1e-3, rtol=0)
    np.testing.assert_allclose(logit(v), logit(g["on_vis"]), atol=1e-4, rtol=0)
    np.testing.assert_allclose(logit(f), logit(g["on_conf"]), atol=1e-4, rtol=0)
    # streaming (is_online=True) path
    st = O.OnlineState()
    for ind in range(0, T - 4, 4):
        chunk = fm[ind: ind + 8]
        cs, vs, fs = O.model_forward_online(chunk[None], g["on_queries"], p, window_len=8, iters=4,
                                            model_resolution=(64, 96), is_online=True, state=st)
    np.testing.assert_allclose(cs, g["on_stream_coords"], atol=1e-3, rtol=0)
    np.testing.assert_allclose(logit(vs), logit(g["on_stream_vis"]), atol=1e-4, rtol=0)
    np.testing.assert_allclose(logit(fs), logit(g["on_stream_conf"]), atol=1e-4, rtol=0)


def test_model_offline(golden):
    g = golden("model_offline")
    p = oracle_params(2)
    fm = O.normalize_fmaps(g["off_fnet"][None])
    c, v, f = O.model_forward_offline(fm, g["off_queries"], p, iters=4, model_resolution=(64, 96))
    np.testing.assert_allclose(c, g["off_coords"], atol=1e-3, rtol=0)
    np.testing.assert_allclose(logit(v), logit(g["off_vis"]), atol=1e-4, rtol=0)
    np.testing.assert_allclose(logit(f), logit(g["off_conf"]), atol=1e-4, rtol=0)


# ------------------------------------------------------------------------------------------
# CoTracker2's CorrBlock (blocks.py:284-362) and the 4-D bilinear_sampler under it
# ------------------------------------------------------------------------------------------
def test_sampler_4d_bit_exact(golden):
    g = golden("corrblock")
    for tag in "abc":
        out = O.bilinear_sampler_4d(g[f"s4_{tag}_input"], g[f"s4_{tag}_coords"])
        assert np.array_equal(out, g[f"s4_{tag}_output"]), tag


def test_corrblock_oracle(golden):
    g = golden("corrblock")
    pyr = O.corrblock_pyramid(g["cb_fmaps"])
    corrs = O.corrblock_corr(pyr, g["cb_targets"])
    for i in range(4):
        assert np.abs(corrs[i] - g[f"cb_corrs{i}"]).max() < 2e-6  # BLAS reduction order only
    # sampling the reference's own volumes is bit-exact (indices, weights, FMA blend order)
    out = O.corrblock_sample([g[f"cb_corrs{i}"] for i in range(4)], g["cb_coords"])
    assert np.array_equal(out, g["cb_out"])
    out = O.corrblock_sample(corrs, g["cb_coords"])
    assert np.abs(out - g["cb_out"]).max() < 2e-6


# ------------------------------------------------------------------------------------------
# CoTracker2: oracle vs goldens of the unmodified reference (tests/golden/cotracker2.npz)
# ------------------------------------------------------------------------------------------
def _v2_params():
    from cotracker_amd.model_v2 import CoTracker2
    from cotracker_amd.weights import fill_synthetic_
    m = CoTracker2(window_len=8, stride=4, model_resolution=(64, 96)).eval()
    fill_synthetic_(m, seed=6, head_scale=1.0)
    return {k: v.numpy() for k, v in m.state_dict().items() if not k.startswith("fnet.")}


def _logit(p):
    p = np.asarray(p, np.float64)
    return np.log(p / (1 - p))


def test_cotracker2_update_former_with_masks():
    g = np.load("tests/golden/cotracker2.npz")
    p = _v2_params()
    delta = O.update_former(g["uf_x"], p, depth=6, mask=g["uf_mask"])
    assert delta.shape == g["uf_delta"].shape == (1, 10, 8, 130)
    assert np.abs(delta - g["uf_delta"]).max() < 3e-5


def test_cotracker2_forward_window():
    g = np.load("tests/golden/cotracker2.npz")
    p = _v2_params()
    amask = g["fw_attention_mask"]
    c, v = O.forward_window_v2(g["fw_fmaps"], g["fw_coords"], amask[..., None] * g["fw_track_feat"], g["fw_vis"],
                               g["fw_track_mask"], amask, p, iters=3)
    assert np.abs(c * 4.0 - g["fw_out_coords"]).max() < 1e-3
    assert np.abs(v - g["fw_out_vis"]).max() < 3e-4  # logits of magnitude ~4 read off the 3x-updated track features


def test_cotracker2_model_sliding_and_streaming():
    g = np.load("tests/golden/cotracker2.npz")
    p = _v2_params()
    fm = g["fmaps"]                                   # [1,20,128,16,24] from the reference's fnet
    T = fm.shape[1]
    pad = (8 - T % 8) % 8
    fmp = np.concatenate([fm, np.repeat(fm[:, -1:], pad, axis=1)], axis=1)
    c, v = O.model_forward_v2(fmp, g["queries"], p, window_len=8, iters=1, T=T)  # goldens: 1 iteration per window
    assert np.abs(c - g["coords"]).max() < 1e-3
    assert np.abs(_logit(v) - _logit(g["vis"])).max() < 2e-4
    st = O.OnlineStateV2()
    for ind in range(0, T - 4, 4):
        cs, vs = O.model_forward_v2(fm[:, ind:ind + 8], g["queries"], p, window_len=8, iters=1, is_online=True, state=st)
    assert np.abs(cs - g["stream_coords"]).max() < 1e-3
    assert np.abs(_logit(vs) - _logit(g["stream_vis"])).max() < 2e-4


# ---- torch-CPU port (oracle/torch_port.py): the CPU baseline bench.py times -------------------------------
def test_torch_port_matches_reference_goldens(golden):
    """The port calls the same ATen kernels in the same order as the reference, so it reproduces the reference's
    model-level outputs (sliding windows incl. the carry-over logic, and the offline single window) to fp32 noise."""
    import torch
    from oracle import torch_port as TP
    from cotracker_amd.model import CoTrackerThreeOnline, CoTrackerThreeOffline
    from cotracker_amd.weights import fill_synthetic_

    def params(m):
        return m.fnet, {k: v for k, v in m.state_dict().items() if not k.startswith("fnet.")}

    def lg(p):
        p = torch.from_numpy(np.asarray(p)).double()
        return torch.log(p / (1 - p))

    g = golden("model_online")
    m = CoTrackerThreeOnline(stride=4, corr_radius=3, window_len=8, model_resolution=(64, 96)).eval()
    fill_synthetic_(m, seed=1)
    fnet, p = params(m)
    c, v, f = TP.model_forward(fnet, p, torch.from_numpy(g["on_video"]), torch.from_numpy(g["on_queries"]), iters=4, window_len=8)
    assert float((c - torch.from_numpy(g["on_coords"])).abs().max()) < 2e-4
    assert float((v.double() - lg(g["on_vis"])).abs().max()) < 1e-4
    assert float((f.double() - lg(g["on_conf"])).abs().max()) < 1e-4

    g = golden("model_offline")
    m = CoTrackerThreeOffline(stride=4, corr_radius=3, window_len=8, model_resolution=(64, 96)).eval()
    fill_synthetic_(m, seed=2)
    fnet, p = params(m)
    c, v, f = TP.model_forward(fnet, p, torch.from_numpy(g["off_video"]), torch.from_numpy(g["off_queries"]), iters=4, offline=True)
    assert float((c - torch.from_numpy(g["off_coords"])).abs().max()) < 2e-4
    assert float((v.double() - lg(g["off_vis"])).abs().max()) < 1e-4


# weights of the EfficientUpdateFormer in tests/golden/update_former.npz: cotracker_amd.weights.synthetic_tensor per state_dict
# entry, heads scaled up so that the output moves by far more than the tolerance when the space attention is switched off
UPDATE_FORMER_WEIGHTS = dict(seed=5, head_scale=50.0)


def test_update_former_add_space_attn_false_matches_reference(golden):
    """EfficientUpdateFormer.forward(add_space_attn=False) (cotracker.py:496-502): the oracle against what the imported reference
    returned for the same input and weights (tests/golden/update_former.npz, tests/golden/make_golden_reference.py)."""
    from cotracker_amd.model import CoTrackerThreeOnline
    from cotracker_amd.weights import synthetic_tensor
    from oracle import cotracker_oracle as O
    g = golden("update_former")
    x, y, y_full = g["x"], g["y"], g["y_full"]
    # the reference's key set and shapes (tests/test_boundary_vs_reference.py) for input_dim=1110, hidden 384, 3 + 3 blocks, 64 virtual tracks
    shapes = CoTrackerThreeOnline(stride=4, corr_radius=3, window_len=16, model_resolution=(64, 96)).updateformer.state_dict()
    p = {"updateformer." + k: synthetic_tensor("updateformer." + k, v.shape, **UPDATE_FORMER_WEIGHTS).numpy() for k, v in shapes.items()}
    assert np.abs(O.update_former(x, p, add_space_attn=False) - y).max() < 5e-5
    assert np.abs(O.update_former(x, p) - y_full).max() < 5e-5
    assert np.abs(y - y_full).max() > 1e-2
