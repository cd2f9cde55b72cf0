"""Seed points on corners, the part that needs no GPU: ctk_seed_points is declared, bound and exported without an ABI bump, the new
struct's ctypes mirror has the compiler's layout, every refusal comes back before any launch, and the predictors refuse what they
must and keep their defaults."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import pytest
import torch

from ctk_support import ROOT, header_layout, lib  # noqa: F401

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
POINTERS = ("frame", "seeds")


def test_declared_bound_exported_and_abi(lib):
    from cotracker_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "ctk.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    name = "ctk_seed_points"
    assert re.search(r"\bint %s\(" % name, header)
    assert name in L.SYMBOLS and hasattr(lib, name)
    assert any(ln.split()[-1] == name and " T " in ln for ln in nm.splitlines())
    assert lib.ctk_abi_version() == L.ABI_VERSION == 9  # additive
    assert int(header_layout()["sizeof"]["ctk_stream_args"]) == C.sizeof(L.StreamArgs) == 200  # no existing struct grew
    assert C.sizeof(L.StreamHealth.Args) == 136
    assert name in header.split("#define CTK_ABI_VERSION")[0]  # the ABI history names the addition
    makefile = open(os.path.join(ROOT, "co-tracker_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bseed\.hip\b", makefile, re.M) and re.search(r"^NOFMA = .*\bseed\b", makefile, re.M)
    assert re.search(r"^HDRS = .*\bseed_math\.h\b", makefile, re.M)


def test_seed_args_mirror_matches_the_compiler():
    """sizeof and every offsetof of ctk_seed_args, from a C program compiled against include/ctk.h."""
    from cotracker_amd import _lib as L
    fields = [f[0] for f in L.Seed.Args._fields_]
    lines = ['printf("S %zu\\n", sizeof(ctk_seed_args));']
    lines += [f'printf("F {f} %zu\\n", offsetof(ctk_seed_args, {f}));' for f in fields]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "seed_layout.c"), os.path.join(d, "seed_layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "ctk.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert int(out[0].split()[1]) == C.sizeof(L.Seed.Args)
    got = {ln.split()[1]: int(ln.split()[2]) for ln in out[1:]}
    assert got == {f: getattr(L.Seed.Args, f).offset for f in fields}
    assert len(got) == 17
    # the header declares the fields in the mirror's order and no others
    body = re.search(r"typedef struct ctk_seed_args \{(.*?)\} ctk_seed_args;", open(os.path.join(ROOT, "include", "ctk.h")).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert declared == fields


def seed_args(**kw):
    """A ctk_seed_args that passes every check: an 8 x 12 grid over a 64 x 96 picture."""
    from cotracker_amd import _lib as L
    a = L.Seed.Args()
    a.h, a.w, a.radius, a.margin, a.inset, a.min_score = 64, 96, 3, 4, 1, 1
    a.x_lo, a.x_hi, a.y_lo, a.y_hi, a.gh, a.gw, a.inv_cw, a.inv_ch, a.reserved = 0.0, 95.0, 0.0, 63.0, 8, 12, 12 / 95, 8 / 63, 0
    for n in POINTERS:
        setattr(a, n, 4096)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_seed_refuses_before_any_launch(lib):
    """Every refusal is an E_* code (a launch on a machine without a GPU would be a hipError_t > 0)."""
    seed = lambda a: lib.ctk_seed_points(None if a is None else C.byref(a), None)  # noqa: E731
    nan, inf = float("nan"), float("inf")
    assert seed(None) == E_NULL
    for f in POINTERS:
        assert seed(seed_args(**{f: None})) == E_NULL, f
    for field, values in (("h", (0, -1, 32769)), ("w", (0, -1, 32769)), ("radius", (0, -1, 8, 100)), ("margin", (-1, -100)), ("inset", (-1,)),
                          ("min_score", (-1, -(2 ** 31))), ("gh", (0, -1, 5462)), ("gw", (0, -1, 8193)),
                          ("x_lo", (nan, inf, -inf, 95.0, 96.0)), ("x_hi", (nan, inf, -inf, 0.0, -1.0)),
                          ("y_lo", (nan, inf, -inf, 63.0, 64.0)), ("y_hi", (nan, inf, -inf, 0.0, -1.0)), ("inv_cw", (nan, inf, 0.0, -0.1)),
                          ("inv_ch", (nan, inf, 0.0, -0.1)), ("reserved", (1, -1))):
        for v in values:
            assert seed(seed_args(**{field: v})) == E_SHAPE, (field, v)
    assert seed(seed_args(gh=256, gw=257)) == E_SHAPE  # 65792 cells
    assert seed(seed_args(gh=65536, gw=65536)) == E_SHAPE  # (the product does not wrap)
    for f in POINTERS:
        assert seed(seed_args(**{f: 4098})) == E_ALIGN, f
    # what the rules admit reaches the pointer check: the refusal is then the NULL one
    for kw in (dict(gh=256, gw=256), dict(gh=65536, gw=1), dict(h=1, w=1), dict(h=32768, w=32768), dict(radius=1), dict(radius=7),
               dict(margin=0, inset=0, min_score=0), dict(margin=2 ** 31 - 1, inset=2 ** 31 - 1, min_score=2 ** 31 - 1),
               dict(x_lo=-2.5, x_hi=97.5), dict(inv_cw=1e30)):
        assert seed(seed_args(seeds=None, **kw)) == E_NULL, kw


def test_ops_seed_points_signature():
    from cotracker_amd import ops
    sig = inspect.signature(ops.seed_points)
    assert list(sig.parameters)[:7] == ["frame", "grid", "bounds", "radius", "margin", "inset", "min_score"]
    assert [sig.parameters[n].default for n in ("bounds", "radius", "margin", "inset", "min_score")] == [None, 3, None, 0, 1]
    with pytest.raises(ValueError, match="device tensor"):
        ops.seed_points(torch.zeros(3, 8, 8), (2, 2))  # a host tensor: refused, no fall-back


def test_predictor_refusals_and_defaults():
    from cotracker_amd.predictor import CoTrackerOnlinePredictor, CoTrackerPredictor
    # the forward signatures are the reference's: the new switches are attributes
    assert list(inspect.signature(CoTrackerOnlinePredictor.forward).parameters) == ["self", "video_chunk", "is_first_step", "queries", "grid_size",
                                                                                     "grid_query_frame", "add_support_grid"]
    assert list(inspect.signature(CoTrackerPredictor.forward).parameters) == ["self", "video", "queries", "segm_mask", "grid_size",
                                                                               "grid_query_frame", "backward_tracking"]
    rep = inspect.signature(CoTrackerOnlinePredictor.replenish).parameters
    assert [rep[n].default for n in ("seeds", "min_score", "skip_flat")] == ["centre", 1, False]
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=8)
    off = CoTrackerPredictor(checkpoint=None, window_len=8)
    assert p.grid_seeds == "grid" and off.grid_seeds == "grid"
    # an unknown `seeds` is refused before anything else is looked at, a stream or not
    for bad in ("corner", "center", None, 3):
        with pytest.raises(ValueError, match="seeds must be"):
            p.replenish(2, seeds=bad)
    with pytest.raises(ValueError, match="min_score"):
        p.replenish(2, seeds="corners", min_score=-1)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.replenish(2, seeds="corners")
    p.spare_points = 2
    p(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, queries=torch.zeros(1, 3, 3))
    with pytest.raises(RuntimeError, match="no stream is running"):  # after the first step: no window has been tracked
        p.replenish(2, seeds="corners")
    # first-step grids: the chunk must hold the frame the seeds are taken on
    p.grid_seeds = "corners"
    for frame in (1, 5, -1):
        with pytest.raises(ValueError, match="grid_query_frame"):
            p(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, grid_size=4, grid_query_frame=frame)
    off.grid_seeds = "corners"
    with pytest.raises(ValueError, match="grid_query_frame"):
        off(torch.zeros(1, 3, 3, 32, 48), grid_size=4, grid_query_frame=3)
    for x in (p, off):
        x.grid_seeds = "lattice"
    with pytest.raises(ValueError, match="grid_seeds must be"):
        p(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, grid_size=4)
    with pytest.raises(ValueError, match="grid_seeds must be"):
        off(torch.zeros(1, 3, 3, 32, 48), grid_size=4)
    # a request with queries never looks at the switch's frame rule
    p.grid_seeds = "corners"
    assert p(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, queries=torch.zeros(1, 3, 3), grid_query_frame=7) == (None, None)
    p2 = CoTrackerOnlinePredictor(checkpoint=None, v2=True, window_len=8)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.replenish(2, seeds="corners")
    p2.grid_seeds = "corners"
    with pytest.raises(NotImplementedError, match="v2"):
        p2(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, grid_size=4)
