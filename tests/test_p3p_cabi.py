"""Fit p3p, the part that needs no GPU: ctk_fit_p3p and its workspace query are declared, bound and exported without an ABI bump, the new
struct's ctypes mirror has the compiler's layout and is ctk_fit_resection_args without seed_pose, every refusal comes back before any
launch and is ctk_fit_resection's for the fields both structs have, and the Python layers have the signatures, defaults and stated
limits the callers rely on."""
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
NAMES = ("ctk_fit_p3p", "ctk_fit_p3p_workspace_bytes")


def test_declared_bound_exported_and_abi(lib):
    from cotracker_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "ctk.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    history = header.split("#define CTK_ABI_VERSION")[0]
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header)
        assert name in L.SYMBOLS and hasattr(lib, name)
        assert any(ln.split()[-1] == name and " T " in ln for ln in nm.splitlines())
        assert any(e.startswith("v9, additive") and name in e for e in re.split(r"\n \*   (?=v\d)", history))  # the ABI history names the addition
    assert lib.ctk_abi_version() == L.ABI_VERSION == 9  # additive
    assert re.search(r"#define CTK_ABI_VERSION 9\b", header)
    assert int(header_layout()["sizeof"]["ctk_stream_args"]) == C.sizeof(L.StreamArgs) == 200  # no existing struct grew
    assert C.sizeof(L.Epipolar.Args) == 168 and C.sizeof(L.Pose.Args) == 176 and C.sizeof(L.Resection.Args) == 192
    section = header.split("fit p3p: the camera's pose against")[1].split("fit structure: points added")[0]
    assert not re.search(r"#define CTK_\w+\s+-?\d+", section)  # no new error code; the constants live with the rules
    for limit in ("Known limits", "ONE root per triple", "nearest the structure's own distances", "was not tried", "unit is the structure's",
                  "stay tracked", "pinhole", "lens distortion", "no bundle adjustment"):
        assert limit in section, limit
    for rule in ("4096", "only read", "2^61", "8 x 8", "(I | 0)", "bits 0 /", "bit 3", "bit 2", "lowest k on ties", "no seed", "Six Newton rounds",
                 "collinear or repeated", "0 .. hypotheses", "the first three of the four"):
        assert rule in section, rule
    # resection's known limits keep their words and point here
    old = header.split("fit resection: the camera's pose against")[1].split("typedef struct ctk_fit_resection_args")[0]
    assert "no minimal P3P solver" in old and "ctk_fit_p3p" in old
    csrc = os.path.join(ROOT, "co-tracker_amd", "csrc")
    math_h = open(os.path.join(csrc, "p3p_math.h")).read()
    assert re.search(r"#define CTK_P3P_ROUNDS 6\b", math_h) and L.P3p.ROUNDS == 6
    for limit in ("Known limit", "one root per triple", "was not tried", "0.99 / 0.98 / 0.97 / 0.95"):
        assert limit in math_h, limit
    body = math_h.split("#pragma once")[1]
    assert '#include "resection_math.h"' in body and "structure_math.h" not in body
    for reused in ("ctk_pose_ray", "ctk_pose_rsqrt", "ctk_pose_polar", "ctk_pose_valid", "ctk_pose_cross", "ctk_pose_dot", "ctk_resection_eye"):
        assert reused in body, reused
    # the rules take no library root and no trigonometry, and restate nothing of resection's
    assert not re.search(r"(?<![\w])(sqrtf?|sinf?|cosf?|tanf?|atan2?f?|acosf?|asinf?)\s*\(", body)
    assert not re.search(r"CTK_MM_HD \w+ ctk_(resection|pose|plane)_", body)
    kernel = open(os.path.join(csrc, "p3p.hip")).read().split("namespace {")[1]
    assert "atomic" not in kernel and "sqrt" not in kernel and "asm" not in kernel
    for reused in ("ctk_p3p_candidate", "ctk_plane_sample", "ctk_resection_apply", "ctk_resection_entry", "ctk_resection_terms",
                   "ctk_resection_update", "ctk_resection_better", "ctk_resection_point", "fit_gather", "fit_block_sums", "fit_launch"):
        assert reused in kernel, reused
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS = .*\bp3p\.hip\b", makefile, re.M) and re.search(r"^NOFMA = .*\bp3p\b", makefile, re.M)
    assert re.search(r"^HDRS = .*\bp3p_math\.h\b", makefile, re.M)
    blob = open(L.LIB_PATH, "rb").read()  # the release library carries no CTK_* string literal
    assert not re.findall(rb"CTK_P3P\w*", blob)


def test_mirror_matches_the_compiler():
    from cotracker_amd import _lib as L
    cls, struct = L.P3p.Args, "ctk_fit_p3p_args"
    fields = [f[0] for f in cls._fields_]
    lines = [f'printf("S %zu\\n", sizeof({struct}));'] + [f'printf("F {f} %zu\\n", offsetof({struct}, {f}));' for f in fields]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p3p_layout.c"), os.path.join(d, "p3p_layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "ctk.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    got_size, got = int(out[0].split()[1]), {ln.split()[1]: int(ln.split()[2]) for ln in out[1:]}
    assert got_size == C.sizeof(cls) == 184
    assert got == {f: getattr(cls, f).offset for f in fields} and len(got) == 33
    # the header declares the fields in the mirror's order and no others
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), open(os.path.join(ROOT, "include", "ctk.h")).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert declared == fields
    # ctk_fit_resection_args without seed_pose: the same fields of the same types in the same order
    assert list(cls._fields_) == [f for f in L.Resection.Args._fields_ if f[0] != "seed_pose"]


POINTERS = ("hist_coords", "visible", "hist_vis", "hist_conf", "first_row", "structure", "valid", "pose", "label", "error", "stats")


def make_args(cls, **kw):
    """An args struct of `cls` (P3p.Args or Resection.Args) that passes every check: 3 frames out of a ring of 8 rows, the lag form."""
    a = cls()
    a.G, a.N, a.N_out, a.R, a.f0, a.F, a.to, a.lag, a.anchor_frame = 2, 5, 4, 8, 6, 3, -1, 2, 0
    a.min_points, a.hypotheses, a.seed = 16, 256, 7
    a.fx, a.fy, a.cx, a.cy = 1000.0, 990.0, 960.0, 540.0
    a.sx, a.sy, a.thresh, a.tol = 1.37, 0.81, 0.6, 2.0
    for n in POINTERS + (("seed_pose",) if hasattr(a, "seed_pose") else ()):
        setattr(a, n, 4096)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def p3p_args(**kw):
    from cotracker_amd import _lib as L
    return make_args(L.P3p.Args, **kw)


ANCHOR = dict(lag=0, anchor_coords=4096, anchor_visible=4096, anchor_frame=3)


def test_fit_refuses_before_any_launch(lib):
    """Every refusal is an E_* code (a launch on a machine without a GPU would be a hipError_t > 0), and it is the code
    ctk_fit_resection answers for the same fields."""
    from cotracker_amd import _lib as L

    def fit(a, ws=None, nbytes=0):
        return lib.ctk_fit_p3p(None if a is None else C.byref(a), ws, nbytes, None)

    def query(a):
        n = C.c_size_t(99)
        return lib.ctk_fit_p3p_workspace_bytes(None if a is None else C.byref(a), C.byref(n))

    def both(expect, **kw):
        """The refusal of ctk_fit_p3p, and ctk_fit_resection's for the same fields."""
        assert fit(p3p_args(**kw)) == expect, kw
        assert lib.ctk_fit_resection(C.byref(make_args(L.Resection.Args, **kw)), None, 0, None) == expect, kw
    nan, inf = float("nan"), float("inf")
    assert fit(None) == E_NULL and query(None) == E_NULL
    assert lib.ctk_fit_p3p_workspace_bytes(C.byref(p3p_args()), None) == E_NULL
    for f in ("hist_coords", "structure", "valid", "pose", "label", "error", "stats"):
        both(E_NULL, **{f: None})
    both(E_NULL, visible=None, hist_vis=None), both(E_NULL, visible=None, hist_conf=None)
    both(E_NULL, **{**ANCHOR, "anchor_visible": None}), both(E_NULL, **{**ANCHOR, "anchor_coords": None})
    shape = (("G", (0, -1, 65536)), ("N", (0, -1, 3)), ("N_out", (0, -1, 6)), ("R", (0, -1, 4)), ("F", (0, -1, 7, 65536)),
             ("f0", (-1, -100, 2 ** 30 - 2)), ("lag", (0, -1, -2, 6, 1000)),
             ("sx", (0.0, -1.0, nan, inf)), ("sy", (0.0, -1.0, nan, inf)),
             ("min_points", (0, -1, 1, 5, 8193)), ("hypotheses", (0, -1, 1025, 4096)), ("tol", (0.0, -0.0, -1.0, nan, inf, -inf)),
             ("fx", (0.0, -1.0, -0.0, nan, inf, -inf)), ("fy", (0.0, -1000.0, nan, inf, -inf)), ("cx", (nan, inf, -inf)), ("cy", (nan, inf, -inf)))
    for field, values in shape:
        for v in values:
            both(E_SHAPE, **{field: v})
            assert query(p3p_args(**{field: v})) == E_SHAPE, (field, v)
    assert fit(p3p_args(N=9000, N_out=8193)) == E_SHAPE and query(p3p_args(N=9000, N_out=8192)) == 0    # N_out > 8192
    assert fit(p3p_args(F=7, lag=2, R=8)) == E_SHAPE and query(p3p_args(F=6, lag=2, R=8, f0=4)) == 0    # F + lag > R
    assert query(p3p_args(f0=2 ** 30 - 3, F=3)) == 0 and fit(p3p_args(f0=2 ** 30 - 2, F=3)) == E_SHAPE  # f0 + F > 2^30
    assert fit(p3p_args(G=8193, N=8192, N_out=1)) == E_SHAPE and fit(p3p_args(G=65535, N=65535, N_out=1)) == E_SHAPE
    assert fit(p3p_args(visible=None, thresh=nan)) == E_SHAPE and query(p3p_args(visible=None, thresh=nan)) == E_SHAPE
    assert fit(p3p_args(thresh=nan, pose=None)) == E_NULL
    # the source form: exactly one of the three, and rows of a ring that would alias
    for kw in (dict(lag=0), dict(to=3), dict(to=-2, lag=0), dict(to=2 ** 30 + 1, lag=0), dict(lag=2 ** 30 + 1), dict(ANCHOR, lag=2),
               dict(ANCHOR, to=3), dict(ANCHOR, anchor_frame=-1), dict(ANCHOR, anchor_frame=2 ** 30 + 1), dict(ANCHOR, F=9, f0=0),
               dict(to=0, lag=0, f0=6, F=3), dict(to=14, lag=0, f0=6, F=3)):
        both(E_SHAPE, **kw)
        assert query(p3p_args(**kw)) == E_SHAPE, kw
    for kw in (dict(to=1, lag=0, f0=6, F=3), dict(to=13, lag=0, f0=6, F=3), dict(to=7, lag=0), dict(ANCHOR), dict(ANCHOR, F=8, f0=0),
               dict(ANCHOR, anchor_frame=2 ** 30)):
        assert query(p3p_args(**kw)) == 0, kw
    # the one-launch form keeps everything in LDS and registers: the query answers 0, and reads no pointer of the struct
    n = C.c_size_t(99)
    assert lib.ctk_fit_p3p_workspace_bytes(C.byref(p3p_args()), C.byref(n)) == 0 and n.value == 0
    n = C.c_size_t(99)
    assert lib.ctk_fit_p3p_workspace_bytes(C.byref(p3p_args(N=8192, N_out=8192, hypotheses=1024)), C.byref(n)) == 0 and n.value == 0
    both(E_ALIGN, hist_coords=4100), both(E_ALIGN, **{**ANCHOR, "anchor_coords": 4100})
    for f in ("structure", "pose", "error", "stats"):
        both(E_ALIGN, **{f: 4098})
    # what the rules admit reaches the pointer check: the refusal is then the NULL one; valid and label need no alignment
    for kw in (dict(lag=1, F=7), dict(lag=5, F=3), dict(N_out=5), dict(f0=0), dict(f0=1, lag=5), dict(N=8192, N_out=8192),
               dict(G=65535, N=1024, N_out=1), dict(first_row=None), dict(visible=None), dict(sx=1e-30, sy=1e30), dict(min_points=6),
               dict(min_points=8192), dict(hypotheses=1), dict(hypotheses=1024), dict(tol=1e-30), dict(tol=3e38), dict(seed=2 ** 32 - 1),
               dict(valid=4097, label=4099), dict(ANCHOR), dict(fx=1e-30, fy=3e38), dict(cx=-3e38, cy=3e38), dict(cx=0.0, cy=-0.0)):
        both(E_NULL, stats=None, **kw)
        assert query(p3p_args(stats=None, **kw)) == 0, kw  # the query looks at no pointer of the struct but the anchor's


def test_python_layers_signatures_and_refusals():
    from cotracker_amd import model, model_v2, ops
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    sig = inspect.signature(ops.fit_p3p)
    assert list(sig.parameters) == ["tracks", "visible", "intrinsics", "structure", "valid", "lag", "to", "anchor", "tol", "hypotheses",
                                    "min_points", "seed", "first_row", "scale", "out"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[5:]] == [1, None, None, 2.0, 256, 16, 0, None, (1, 1), None]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[5:])
    assert all(sig.parameters[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in list(sig.parameters)[:5])
    # fit_resection without seed_pose, and fit_resection itself as it was
    rsig = inspect.signature(ops.fit_resection)
    assert [n for n in rsig.parameters if n != "seed_pose"] == list(sig.parameters)
    assert [rsig.parameters[n].default for n in sig.parameters] == [sig.parameters[n].default for n in sig.parameters]
    gsig, old = inspect.signature(ops.StreamGroups.p3p), inspect.signature(ops.StreamGroups.resection)
    assert list(gsig.parameters)[:6] == ["self", "f0", "F", "intrinsics", "structure", "valid"]
    assert list(gsig.parameters) == [n for n in old.parameters if n != "seed_pose"]
    assert [gsig.parameters[n].default for n in ("lag", "to", "anchor", "thresh", "tol", "hypotheses", "min_points", "seed", "group", "out")] == \
        [1, None, None, 0.6, 2.0, 256, 16, 0, None, None]
    msig = inspect.signature(model.CoTrackerThreeOnline.stream_p3p)
    assert list(msig.parameters)[:6] == ["self", "f0", "F", "intrinsics", "structure", "valid"]
    assert hasattr(model_v2, "__file__") and "stream_p3p" in open(model_v2.__file__).read()
    psig = inspect.signature(CoTrackerOnlinePredictor.resect)
    assert list(psig.parameters) == ["self", "structure", "n", "first_frame", "tol", "hypotheses", "min_points", "seed"]
    assert [psig.parameters[n].default for n in list(psig.parameters)[2:]] == [None, None, 2.0, 256, 16, 0]
    lsig = inspect.signature(CoTrackerOnlinePredictor.localize)  # localize() and its signature do not change
    assert list(lsig.parameters) == ["self", "structure", "n", "first_frame", "tol", "hypotheses", "min_points", "seed", "epipolar_tol",
                                     "epipolar_hypotheses", "min_base"]
    assert [lsig.parameters[n].default for n in list(lsig.parameters)[2:]] == [None, None, 2.0, 256, 16, 0, 1.0, 512, 16.0]
    for doc in (CoTrackerOnlinePredictor.resect.__doc__, ops.fit_p3p.__doc__):
        for limit in ("one root per triple", "nearest", "pinhole", "distortion", "bundle"):
            assert limit in doc, limit
    assert "ONE\n        launch" in CoTrackerOnlinePredictor.resect.__doc__ or "ONE launch" in CoTrackerOnlinePredictor.resect.__doc__
    assert "no minimal P3P solver" in CoTrackerOnlinePredictor.localize.__doc__ and "resect()" in CoTrackerOnlinePredictor.localize.__doc__
    assert "no minimal solver" in ops.fit_resection.__doc__ and "fit_p3p" in ops.fit_resection.__doc__
    # host tensors are refused: no fall-back
    cam = (100.0, 100.0, 24.0, 16.0)
    with pytest.raises(ValueError, match="device tensor"):
        ops.fit_p3p(torch.zeros(2, 9, 2), torch.zeros(2, 9, dtype=torch.bool), cam, torch.zeros(9, 3), torch.zeros(9, dtype=torch.int8))
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=8)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.resect(None)
    p(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, queries=torch.zeros(1, 3, 3))
    with pytest.raises(RuntimeError, match="no stream is running"):  # after the first step: no window has been tracked
        p.resect(None)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.model.stream_p3p(0, 1, cam, None, None)
    p2 = CoTrackerOnlinePredictor(checkpoint=None, v2=True, window_len=8)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.resect(None)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.model.stream_p3p(0, 1, cam, None, None)
