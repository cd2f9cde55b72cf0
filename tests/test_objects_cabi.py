"""Fit objects, the part that needs no GPU: ctk_fit_objects and its workspace query are declared, bound and exported without an ABI
bump, the new struct's ctypes mirror has the compiler's layout, every refusal comes back before any launch, and the Python layers have
the signatures and defaults the callers rely on."""
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
NAMES = ("ctk_fit_objects", "ctk_fit_objects_workspace_bytes")


def test_declared_bound_exported_and_abi(lib):
    from cotracker_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "ctk.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header)
        assert name in L.SYMBOLS and hasattr(lib, name)
        assert any(ln.split()[-1] == name and " T " in ln for ln in nm.splitlines())
        assert name in header.split("#define CTK_ABI_VERSION")[0]  # the ABI history names the addition
    assert lib.ctk_abi_version() == L.ABI_VERSION == 9  # additive
    assert int(header_layout()["sizeof"]["ctk_stream_args"]) == C.sizeof(L.StreamArgs) == 200  # no existing struct grew
    assert C.sizeof(L.Motion.Args) == 128 and C.sizeof(L.Field.Args) == 152 and C.sizeof(L.Draw.Args) == 216
    section = header.split("fit objects: which points move together")[1].split("Op A")[0]
    assert not re.search(r"#define CTK_\w+\s+-?\d+", section)  # no new error code; the two constants live with the rules
    assert (L.Objects.OBJECTS_MAX, L.Objects.NONE) == (16, 127) and "127 (CTK_OBJECT_NONE" in section
    math_h = open(os.path.join(ROOT, "co-tracker_amd", "csrc", "objects_math.h")).read()
    assert re.search(r"#define CTK_OBJECTS_MAX 16\b", math_h) and re.search(r"#define CTK_OBJECT_NONE 127\b", math_h)
    makefile = open(os.path.join(ROOT, "co-tracker_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bobjects\.hip\b", makefile, re.M) and re.search(r"^NOFMA = .*\bobjects\b", makefile, re.M)
    assert re.search(r"^HDRS = .*\bobjects_math\.h\b", makefile, re.M) and re.search(r"^HDRS = .*\bmotion_device\.h\b", makefile, re.M)
    assert re.search(r"^HDRS = .*\bfit_device\.h\b", makefile, re.M)  # what the six fit kernels share
    # the release library carries no CTK_* string literal
    blob = open(L.LIB_PATH, "rb").read()
    assert not re.findall(rb"CTK_OBJECT\w*", blob)


def test_objects_args_mirror_matches_the_compiler():
    """sizeof and every offsetof of ctk_fit_objects_args, from a C program compiled against include/ctk.h."""
    from cotracker_amd import _lib as L
    fields = [f[0] for f in L.Objects.Args._fields_]
    lines = ['printf("S %zu\\n", sizeof(ctk_fit_objects_args));']
    lines += [f'printf("F {f} %zu\\n", offsetof(ctk_fit_objects_args, {f}));' for f in fields]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "objects_layout.c"), os.path.join(d, "objects_layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "ctk.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert int(out[0].split()[1]) == C.sizeof(L.Objects.Args) == 176
    got = {ln.split()[1]: int(ln.split()[2]) for ln in out[1:]}
    assert got == {f: getattr(L.Objects.Args, f).offset for f in fields}
    assert len(got) == 32
    # the header declares the fields in the mirror's order and no others
    body = re.search(r"typedef struct ctk_fit_objects_args \{(.*?)\} ctk_fit_objects_args;", open(os.path.join(ROOT, "include", "ctk.h")).read(),
                     re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert declared == fields


POINTERS = ("hist_coords", "visible", "hist_vis", "hist_conf", "first_row", "labels", "motion", "label", "stats", "box")


def objects_args(**kw):
    """A ctk_fit_objects_args that passes every check: 3 frames out of a ring of 8 rows, the lag form, labels mode."""
    from cotracker_amd import _lib as L
    a = L.Objects.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.F, a.to, a.lag, a.anchor_frame = 2, 5, 4, 8, 6, 3, -1, 2, 0
    a.L, a.min_points, a.model, a.K, a.seed = 4, 8, 1, 128, 7
    a.tol, a.min_base, a.sx, a.sy, a.thresh, a.reserved = 2.0, 16.0, 1.37, 0.81, 0.6, 0
    for n in POINTERS:
        setattr(a, n, 4096)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


ANCHOR = dict(lag=0, anchor_coords=4096, anchor_visible=4096, anchor_frame=3)


def test_objects_refuses_before_any_launch(lib):
    """Every refusal is an E_* code (a launch on a machine without a GPU would be a hipError_t > 0)."""
    def fit(a, ws=None, nbytes=0):
        return lib.ctk_fit_objects(None if a is None else C.byref(a), ws, nbytes, None)

    def query(a):
        n = C.c_size_t(99)
        return lib.ctk_fit_objects_workspace_bytes(None if a is None else C.byref(a), C.byref(n))
    nan, inf = float("nan"), float("inf")
    assert fit(None) == E_NULL and query(None) == E_NULL
    assert lib.ctk_fit_objects_workspace_bytes(C.byref(objects_args()), None) == E_NULL
    for f in ("hist_coords", "motion", "label", "stats", "box"):
        assert fit(objects_args(**{f: None})) == E_NULL, f
    assert fit(objects_args(visible=None, hist_vis=None)) == E_NULL and fit(objects_args(visible=None, hist_conf=None)) == E_NULL
    assert fit(objects_args(**{**ANCHOR, "anchor_visible": None})) == E_NULL and fit(objects_args(**{**ANCHOR, "anchor_coords": None})) == E_NULL
    # ctk_fit_motion's refusals for the shared fields, and the two new ones
    shape = (("G", (0, -1, 65536)), ("N", (0, -1, 3)), ("N_out", (0, -1, 6)), ("R", (0, -1, 4)), ("F", (0, -1, 7, 65536)),
             ("f0", (-1, -100, 2 ** 30 - 2)), ("lag", (0, -1, -2, 6, 1000)), ("model", (-1, 2, 7)), ("K", (0, -1, 4097)),
             ("tol", (nan, 0.0, -1.0, 1 / 32, 256.04, inf, 1e30)), ("min_base", (nan, -0.001, 8192.5, inf)),
             ("sx", (0.0, -1.0, nan, inf)), ("sy", (0.0, -1.0, nan, inf)), ("reserved", (1, -1)),
             ("L", (0, -1, 17, 1000)), ("min_points", (0, -1, 8193)))
    for field, values in shape:
        for v in values:
            assert fit(objects_args(**{field: v})) == E_SHAPE, (field, v)
            assert query(objects_args(**{field: v})) == E_SHAPE, (field, v)
    assert fit(objects_args(N=9000, N_out=8193)) == E_SHAPE and query(objects_args(N=9000, N_out=8192)) == 0    # N_out > 8192
    assert fit(objects_args(F=7, lag=2, R=8)) == E_SHAPE and query(objects_args(F=6, lag=2, R=8, f0=4)) == 0    # F + lag > R
    assert query(objects_args(f0=2 ** 30 - 3, F=3)) == 0 and fit(objects_args(f0=2 ** 30 - 2, F=3)) == E_SHAPE  # f0 + F > 2^30
    assert fit(objects_args(G=8193, N=8192, N_out=1)) == E_SHAPE and fit(objects_args(G=65535, N=65535, N_out=1)) == E_SHAPE  # G * N > 2^26
    assert fit(objects_args(visible=None, thresh=nan)) == E_SHAPE and query(objects_args(visible=None, thresh=nan)) == E_SHAPE
    assert fit(objects_args(thresh=nan, motion=None)) == E_NULL
    # ctk_track_field's refusals for the source form: exactly one of the three, and rows of a ring that would alias
    for kw in (dict(lag=0), dict(to=3), dict(to=-2, lag=0), dict(to=2 ** 30 + 1, lag=0), dict(lag=2 ** 30 + 1), dict(ANCHOR, lag=2),
               dict(ANCHOR, to=3), dict(ANCHOR, anchor_frame=-1), dict(ANCHOR, anchor_frame=2 ** 30 + 1), dict(ANCHOR, F=9, f0=0),
               dict(to=0, lag=0, f0=6, F=3), dict(to=14, lag=0, f0=6, F=3)):
        assert fit(objects_args(**kw)) == E_SHAPE, kw
        assert query(objects_args(**kw)) == E_SHAPE, kw
    for kw in (dict(to=1, lag=0, f0=6, F=3), dict(to=13, lag=0, f0=6, F=3), dict(to=7, lag=0), dict(ANCHOR), dict(ANCHOR, F=8, f0=0),
               dict(ANCHOR, anchor_frame=2 ** 30)):
        assert query(objects_args(**kw)) == 0, kw
    # the one-launch form keeps everything in LDS: the query answers 0 and no workspace is too small for it
    n = C.c_size_t(99)
    assert lib.ctk_fit_objects_workspace_bytes(C.byref(objects_args()), C.byref(n)) == 0 and n.value == 0
    assert fit(objects_args(hist_coords=4100)) == E_ALIGN and fit(objects_args(**{**ANCHOR, "anchor_coords": 4100})) == E_ALIGN
    for f in ("motion", "stats", "box"):
        assert fit(objects_args(**{f: 4098})) == E_ALIGN, f
    # what the rules admit reaches the pointer check: the refusal is then the NULL one; labels and label need no alignment
    for kw in (dict(lag=1, F=7), dict(lag=5, F=3), dict(model=0), dict(K=1), dict(K=4096), dict(tol=1 / 16), dict(tol=256.0), dict(min_base=0.0),
               dict(min_base=8192.0), dict(N_out=5), dict(f0=0), dict(f0=1, lag=5), dict(N=8192, N_out=8192), dict(G=65535, N=1024, N_out=1),
               dict(first_row=None), dict(visible=None), dict(seed=2 ** 32 - 1), dict(sx=1e-30, sy=1e30), dict(L=1), dict(L=16),
               dict(min_points=1), dict(min_points=8192), dict(labels=None), dict(labels=4097, label=4099), dict(ANCHOR)):
        assert fit(objects_args(stats=None, **kw)) == E_NULL, kw
        assert query(objects_args(stats=None, **kw)) == 0, kw  # the query looks at no pointer of the struct but the anchor's


def test_python_layers_signatures_and_refusals():
    from cotracker_amd import model, ops
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    sig = inspect.signature(ops.fit_objects)
    assert list(sig.parameters) == ["tracks", "visible", "labels", "objects", "lag", "to", "anchor", "model", "tol", "hypotheses", "min_base",
                                    "min_points", "seed", "scale", "frames", "first_row"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[2:]] == [None, 4, 1, None, None, "similarity", 2.0, 128, 16.0, 8, 0, (1, 1),
                                                                             None, None]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[2:])
    ssig = inspect.signature(CoTrackerOnlinePredictor.split_objects)
    assert list(ssig.parameters)[:5] == ["self", "frame", "lag", "objects", "group"]
    assert [ssig.parameters[n].default for n in ("frame", "lag", "objects", "group", "min_points", "seed")] == [None, 8, 4, 0, 8, 0]
    lsig = inspect.signature(CoTrackerOnlinePredictor.label_objects)
    assert list(lsig.parameters) == ["self", "boxes", "frame", "group"] and [lsig.parameters[n].default for n in ("frame", "group")] == [None, 0]
    fsig = inspect.signature(CoTrackerOnlinePredictor.follow)
    assert list(fsig.parameters) == ["self", "objects", "n", "first_frame", "model", "tol", "hypotheses", "min_base", "min_points", "seed"]
    assert [fsig.parameters[n].default for n in list(fsig.parameters)[2:]] == [None, None, "similarity", 2.0, 128, 16.0, 8, 0]
    assert hasattr(ops.StreamGroups, "objects") and hasattr(model.CoTrackerThreeOnline, "stream_objects") and ops.OBJECT_NONE == 127
    for doc in (ops.fit_objects.__doc__, CoTrackerOnlinePredictor.split_objects.__doc__):  # what split's round order is
        doc = " ".join(doc.split())
        assert "most inliers first" in doc and "NOT stable from pair to pair" in doc
    # host tensors are refused: no fall-back
    with pytest.raises(ValueError, match="device tensor"):
        ops.fit_objects(torch.zeros(2, 3, 2), torch.zeros(2, 3, dtype=torch.bool))
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=8)
    calls = (lambda x: x.split_objects(), lambda x: x.label_objects([[0, 0, 10, 10]]), lambda x: x.follow(None))
    for call in calls:
        with pytest.raises(RuntimeError, match="no stream is running"):
            call(p)
    p(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, queries=torch.zeros(1, 3, 3))
    for call in calls:
        with pytest.raises(RuntimeError, match="no stream is running"):  # after the first step: no window has been tracked
            call(p)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.model.stream_objects(0, 1)
    p2 = CoTrackerOnlinePredictor(checkpoint=None, v2=True, window_len=8)
    for call in calls:
        with pytest.raises(NotImplementedError, match="v2"):
            call(p2)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.model.stream_objects(0, 1)
