"""corr_mlp.fc2 folded into the input projection, the algebra (no GPU): for random float64 weights the folded weight and bias of
cotracker_amd.model (fold_input_weights, input_bias_rows) reproduce

    input_transform(cat(vis, conf, fc2(h1_0), .., fc2(h1_3), posenc) + e_t)

on the xf column order [h1_0 | h1_1 | h1_2 | h1_3 | vis, conf, posenc, zero padding] to 1e-12 relative -- at the trained window
length and with an interpolated time embedding (S != trained length)."""
import pytest
import torch
import torch.nn.functional as F

from cotracker_amd import _lib as L
from cotracker_amd.model import fold_input_weights, input_bias_rows, interpolate_time_embed

TRAINED = 16


def random_weights(seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)  # noqa: E731
    return {"in_w": r(L.HID, L.X_DIM) / 30, "in_b": r(L.HID), "fc2_w": r(256, L.HID) / 20, "fc2_b": r(256),
            "time_emb": r(1, TRAINED, L.X_DIM)}


@pytest.mark.parametrize("S", [TRAINED, 8, 23])
def test_folded_projection_equals_the_unfolded_formulas(S):
    p = random_weights(S)
    g = torch.Generator().manual_seed(100 + S)
    N = 5
    h1 = torch.randn(L.LEVELS, N, S, L.HID, generator=g, dtype=torch.float64)   # GELU(fc1(volume_l)): any values
    vis_conf = torch.randn(N, S, 2, generator=g, dtype=torch.float64)
    pe = torch.randn(N, S, 84, generator=g, dtype=torch.float64)
    te = interpolate_time_embed(p["time_emb"], S)                               # [S,1110], reference column order
    assert te.shape == (S, L.X_DIM)
    # the unfolded formulas (cotracker3_online.py:205-247 + cotracker.py:484)
    emb = torch.cat([F.linear(h1[l], p["fc2_w"], p["fc2_b"]) for l in range(L.LEVELS)], dim=-1)
    ref = F.linear(torch.cat([vis_conf, emb, pe], dim=-1) + te, p["in_w"], p["in_b"])
    # the folded ones
    wf, extra = fold_input_weights(p["in_w"], p["fc2_w"], p["fc2_b"])
    assert wf.shape == (L.HID, L.XF_LD) and wf.dtype == torch.float64 and extra.shape == (L.HID,)
    assert L.XF_SMALL == L.LEVELS * L.HID and L.XF_DIM == L.XF_SMALL + 86 and L.XF_LD % 32 == 0
    assert float(wf[:, L.XF_DIM:].abs().max()) == 0.0, "padding columns of the folded weight must be zero"
    xf = torch.zeros(N, S, L.XF_LD, dtype=torch.float64)
    for l in range(L.LEVELS):
        xf[..., L.HID * l:L.HID * (l + 1)] = h1[l]
    xf[..., L.XF_SMALL:L.XF_SMALL + 2] = vis_conf
    xf[..., L.XF_SMALL + 2:L.XF_SMALL + 86] = pe
    xf[..., L.XF_DIM:] = 7.0  # what the padding columns hold must not matter
    rows = input_bias_rows(te, p["in_w"], p["in_b"], extra)                     # [S,384], indexed by frame
    got = xf @ wf.t() + rows[None]
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"S={S}: folded vs unfolded, max relative error {err:.3e}")
    assert err <= 1e-12
    # the unfolded bias rows are the same function without the extra term
    plain = input_bias_rows(te, p["in_w"], p["in_b"])
    assert torch.equal(rows, plain + extra)
    assert float((plain - (te @ p["in_w"].t() + p["in_b"])).abs().max()) == 0.0
