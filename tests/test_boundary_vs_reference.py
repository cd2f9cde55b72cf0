"""Drop-in boundary proof against the reference (CPU).  The reference's side -- state_dict key sets, shapes, dtypes, signatures,
deterministic buffers -- is stored in tests/golden/reference_boundary.json / reference_buffers.npz, written from the imported,
unmodified reference by tests/golden/make_golden_reference.py.  For every model the reference's ``build_cotracker`` can return,
ours must
  * expose the identical ``state_dict`` key set with identical shapes and dtypes,
  * accept the reference's own state_dict with ``load_state_dict(strict=True)`` (and vice versa),
  * have identical ``__init__`` / ``forward`` signatures (names, order, defaults),
and the predictors / hub entry points must have the reference's signatures.
"""
import importlib
import inspect
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ATTRS = ("model_resolution", "window_len", "stride")
BUFFERS = ("time_emb", "pos_emb")


@pytest.fixture(scope="module")
def ref():
    with open(os.path.join(GOLDEN, "reference_boundary.json")) as f:
        return json.load(f)


def sig(fn):
    """A signature as JSON holds it: [name, kind, repr(default)] per parameter."""
    return [[p.name, int(p.kind), repr(p.default)] for p in inspect.signature(fn).parameters.values()]


def ctor_sig_of(cls):
    """The constructor a caller sees: CoTrackerThreeOnline.__init__(self, **args) just forwards to its base
    (cotracker3_online.py:160-161), so walk the MRO to the first __init__ that names its parameters."""
    for c in cls.__mro__:
        init = c.__dict__.get("__init__")
        if init is None:
            continue
        if any(p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD and p.name != "self" for p in inspect.signature(init).parameters.values()):
            return init
    return cls.__init__


def common_kwargs(kw):
    return dict(stride=4, model_resolution=(384, 512), **kw)


def case_id(key, kw):
    return key + "".join(f",{k}={v}" for k, v in sorted(kw.items()))


def buffer_sample(numel, limit=65536):
    """Indices of the buffer elements the fixture stores: all of them up to `limit`, a fixed seeded sample above."""
    return np.arange(numel) if numel <= limit else np.sort(np.random.RandomState(0).choice(numel, limit, replace=False))


CASES = [  # (reference module key, class name, ours, kwargs)
    ("online", "CoTrackerThreeOnline", "cotracker_amd.model", dict(window_len=16)),
    ("offline", "CoTrackerThreeOffline", "cotracker_amd.model", dict(window_len=60)),
    ("v2", "CoTracker2", "cotracker_amd.model_v2", dict(window_len=8)),
    # round 4: the two constructor variants that only change the PARAMETER SET (same kernels) -- cotracker3_online.py:43-53
    ("online", "CoTrackerThreeOnline", "cotracker_amd.model", dict(window_len=16, linear_layer_for_vis_conf=False)),
    ("offline", "CoTrackerThreeOffline", "cotracker_amd.model", dict(window_len=60, add_space_attn=False)),
    ("online", "CoTrackerThreeOnline", "cotracker_amd.model", dict(window_len=16, add_space_attn=False, linear_layer_for_vis_conf=False)),
]


@pytest.mark.parametrize("key,cls,ours_mod,kw", CASES)
def test_state_dict_and_signatures_match_reference(ref, key, cls, ours_mod, kw):
    R = ref["models"][case_id(key, kw)]
    O = getattr(importlib.import_module(ours_mod), cls)
    o = O(**common_kwargs(kw))
    rs = {k: torch.zeros(shape, dtype=getattr(torch, dtype.split(".")[1])) for k, shape, dtype in R["state_dict"]}
    os_ = o.state_dict()
    assert set(rs.keys()) == set(os_.keys())
    for k in rs:
        assert rs[k].shape == os_[k].shape and rs[k].dtype == os_[k].dtype, k
    if not any(k in kw for k in ("add_space_attn", "linear_layer_for_vis_conf")):
        assert len(rs) == (321 if key == "v2" else 188)
    if kw.get("add_space_attn") is False:
        assert not any(".space_" in k for k in os_)
    if kw.get("linear_layer_for_vis_conf") is False:
        assert os_["updateformer.flow_head.weight"].shape == (4, 384) and not any("vis_conf_head" in k for k in os_)
    # deterministic buffers carry the same values (sin/cos tables built independently)
    buffers = np.load(os.path.join(GOLDEN, "reference_buffers.npz"), allow_pickle=False)
    for k in BUFFERS:
        if k in rs:
            ours = os_[k].flatten()[buffer_sample(os_[k].numel())]
            assert torch.allclose(torch.from_numpy(buffers[f"{case_id(key, kw)}/{k}"]), ours, atol=1e-6), k
    # checkpoints travel both ways: a state_dict with the reference's keys, shapes and dtypes loads strictly into ours, and the
    # equal key sets and shapes asserted above are what a strict load of ours into the reference checks
    assert o.load_state_dict(rs, strict=True) is not None
    # signatures: constructor and forward
    assert R["ctor"] == sig(ctor_sig_of(O))
    assert R["forward"] == sig(O.forward)
    for attr in ATTRS:
        v = getattr(o, attr)
        assert R["attrs"][attr] == (list(v) if isinstance(v, tuple) else v)
    if key != "offline":
        assert R["init_video_online_processing"] == sig(O.init_video_online_processing)


def test_predictor_and_builder_signatures(ref):
    from cotracker_amd import predictor as P
    from cotracker_amd import build_cotracker as B
    for name in ("CoTrackerPredictor", "CoTrackerOnlinePredictor"):
        R, O = ref["predictors"][name], getattr(P, name)
        assert R["ctor"] == sig(O.__init__), name
        assert R["forward"] == sig(O.forward), name
    assert ref["build_cotracker"] == sig(B.build_cotracker)
    assert ref["_compute_sparse_tracks"] == sig(P.CoTrackerPredictor._compute_sparse_tracks)
    assert ref["_compute_dense_tracks"] == sig(P.CoTrackerPredictor._compute_dense_tracks)


def test_hub_entry_points(ref):
    spec = importlib.util.spec_from_file_location("our_hubconf", os.path.join(os.path.dirname(os.path.dirname(__file__)), "hubconf.py"))
    ours = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ours)
    assert len(ref["hub"]) == 6
    for n in ref["hub"]:
        assert hasattr(ours, n), n
        assert ref["hub"][n] == sig(getattr(ours, n)), n


def test_predictor_accepts_a_reference_checkpoint_and_fails_loudly_off_gpu(ref):
    """The seam of SURVEY §8b: the reference's CoTrackerPredictor reads interp_shape and support_grid_size off itself and calls
    .model; ours holds the same values, its model takes a state_dict with the reference's keys, and off-GPU it raises."""
    from cotracker_amd.predictor import CoTrackerPredictor
    p = CoTrackerPredictor(checkpoint=None, offline=True, window_len=60)
    R = ref["models"][case_id("offline", dict(window_len=60))]
    p.model.load_state_dict({k: torch.zeros(shape) for k, shape, _ in R["state_dict"]}, strict=True)
    assert list(p.interp_shape) == ref["predictor_seam"]["interp_shape"] == list(p.model.model_resolution)
    assert p.support_grid_size == ref["predictor_seam"]["support_grid_size"]
    with pytest.raises(RuntimeError, match="MI355X GPU only"):  # product path fails loudly off-GPU: no CPU fallback
        p(torch.zeros(1, 4, 3, 64, 64), grid_size=2)
