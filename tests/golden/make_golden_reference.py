"""Fixtures of the CPU tests that pin this package on the UNMODIFIED reference without importing it at test time.

Needs a checkout of facebookresearch/co-tracker (no test imports it):

    COTRACKER_REFERENCE=<checkout> python tests/golden/make_golden_reference.py

Writes, next to this file,
  reference_boundary.json  state_dict keys / shapes / dtypes, attributes and signatures of every model, predictor, builder and
                           hub entry point (tests/test_boundary_vs_reference.py)
  reference_buffers.npz    the deterministic time_emb / pos_emb buffers of those models (a seeded sample above 65 536 elements)
  edge_cases.npz           the reference's outputs on the edge-case inputs (tests/test_edge_cases_vs_reference.py)
  tapvid_metrics.npz       compute_tapvid_metrics and get_points_on_a_grid on the inputs of tests/test_evaluation.py
  update_former.npz        EfficientUpdateFormer with and without space attention (tests/test_oracle_golden.py)
  bilinear_sampler.npz     model_utils.bilinear_sampler on the inputs of tests/test_sampler_math_host.py
The inputs and the case tables live in the test modules; this script imports them from there, so both sides see the same ones.
Weights are not stored: both sides regenerate them with cotracker_amd.weights (name + shape keyed).
"""
import importlib
import importlib.util
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ["COTRACKER_REFERENCE"]  # a checkout of facebookresearch/co-tracker
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

from cotracker_amd.synthetic import synthetic_video  # noqa: E402
from cotracker_amd.weights import fill_synthetic_, synthetic_tensor  # noqa: E402

META = dict(torch_version=torch.__version__, reference="facebookresearch/co-tracker@2025-03-04")


def save(name, **arrs):
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()}
    out["meta"] = np.array(str(META))
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB")


def gen_boundary():
    import test_boundary_vs_reference as TB
    mods = dict(
        build=importlib.import_module("cotracker.models.build_cotracker"),
        predictor=importlib.import_module("cotracker.predictor"),
        online=importlib.import_module("cotracker.models.core.cotracker.cotracker3_online"),
        offline=importlib.import_module("cotracker.models.core.cotracker.cotracker3_offline"),
        v2=importlib.import_module("cotracker.models.core.cotracker.cotracker"),
    )
    spec = importlib.util.spec_from_file_location("ref_hubconf", os.path.join(REF, "hubconf.py"))
    hub = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hub)
    doc, buffers = {"meta": META, "models": {}}, {}
    for key, cls, _, kw in TB.CASES:
        R = getattr(mods[key], cls)
        r = R(**TB.common_kwargs(kw))
        sd = r.state_dict()
        name = TB.case_id(key, kw)
        doc["models"][name] = {
            "state_dict": [[k, list(v.shape), str(v.dtype)] for k, v in sd.items()],
            "attrs": {a: getattr(r, a) for a in TB.ATTRS},
            "ctor": TB.sig(TB.ctor_sig_of(R)), "forward": TB.sig(R.forward),
            "init_video_online_processing": TB.sig(R.init_video_online_processing) if key != "offline" else None,
        }
        for k in TB.BUFFERS:
            if k in sd:
                buffers[f"{name}/{k}"] = sd[k].flatten()[TB.buffer_sample(sd[k].numel())]
    P = mods["predictor"]
    doc["predictors"] = {n: {"ctor": TB.sig(getattr(P, n).__init__), "forward": TB.sig(getattr(P, n).forward)}
                         for n in ("CoTrackerPredictor", "CoTrackerOnlinePredictor")}
    doc["build_cotracker"] = TB.sig(mods["build"].build_cotracker)
    doc["_compute_sparse_tracks"] = TB.sig(P.CoTrackerPredictor._compute_sparse_tracks)
    doc["_compute_dense_tracks"] = TB.sig(P.CoTrackerPredictor._compute_dense_tracks)
    doc["hub"] = {n: TB.sig(f) for n, f in vars(hub).items()
                  if inspect.isfunction(f) and n.startswith("cotracker") and f.__module__ == "ref_hubconf"}
    # the seam of SURVEY 8b: what the reference's predictor reads off its model
    p = P.CoTrackerPredictor(checkpoint=None, offline=True, window_len=60)
    doc["predictor_seam"] = {"interp_shape": list(p.interp_shape), "support_grid_size": p.support_grid_size}
    with open(os.path.join(HERE, "reference_boundary.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    save("reference_buffers.npz", **buffers)


@torch.no_grad()
def gen_edge_cases():
    from cotracker.models.core.cotracker.cotracker3_offline import CoTrackerThreeOffline as RefOff
    from cotracker.models.core.cotracker.cotracker3_online import CoTrackerThreeOnline as RefOn
    from test_edge_cases_vs_reference import CASES
    out = {}
    for case, (H, W, T, offline, q) in sorted(CASES.items()):
        torch.manual_seed(0)
        ref = (RefOff if offline else RefOn)(stride=4, corr_radius=3, window_len=8, model_resolution=(H, W)).eval()
        fill_synthetic_(ref, seed=7)
        c, v, f, _ = ref(synthetic_video(T, H, W, seed=11), torch.tensor([q]), iters=4)
        assert torch.isfinite(c).all()
        out[case + "_coords"], out[case + "_vis"], out[case + "_conf"] = c, v, f
    save("edge_cases.npz", **out)


def gen_tapvid():
    from cotracker.evaluation.core.eval_utils import compute_tapvid_metrics
    from cotracker.models.core.model_utils import get_points_on_a_grid
    import test_evaluation as TE
    out = {}
    for mode in TE.MODES:
        for i, args in enumerate(TE.metric_inputs()):
            for k, v in compute_tapvid_metrics(*args, mode).items():
                out[f"{mode}/{i}/{k}"] = v
    for i, (size, extent, center) in enumerate(TE.GRIDS):
        out[f"grid/{i}"] = get_points_on_a_grid(size, extent, center)
    save("tapvid_metrics.npz", **out)


@torch.no_grad()
def gen_update_former():
    from cotracker.models.core.cotracker.cotracker import EfficientUpdateFormer
    import test_oracle_golden as TO
    f = EfficientUpdateFormer(space_depth=3, time_depth=3, input_dim=1110, hidden_size=384, output_dim=4, mlp_ratio=4.0,
                              num_virtual_tracks=64, add_space_attn=True, linear_layer_for_vis_conf=True).eval()
    for k, t in f.state_dict().items():
        t.copy_(synthetic_tensor("updateformer." + k, t.shape, **TO.UPDATE_FORMER_WEIGHTS))
    x = torch.randn(1, 5, 8, 1110, generator=torch.Generator().manual_seed(0))
    save("update_former.npz", x=x, y=f(x, add_space_attn=False), y_full=f(x))


def gen_bilinear_sampler():
    from cotracker.models.core.model_utils import bilinear_sampler
    import test_sampler_math_host as TS
    out = {}
    for name, (inp, c, align, pad) in TS.restated_oracle_cases().items():
        out[name + "/input"], out[name + "/coords"] = inp, c
        out[name + "/out"] = bilinear_sampler(inp, c.clone(), align, pad)
    save("bilinear_sampler.npz", **out)


if __name__ == "__main__":
    gen_boundary()
    gen_edge_cases()
    gen_tapvid()
    gen_update_former()
    gen_bilinear_sampler()
