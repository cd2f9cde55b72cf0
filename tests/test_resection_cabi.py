"""Fit resection, the part that needs no GPU: ctk_fit_resection and its workspace query are declared, bound and exported without an ABI
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
NAMES = ("ctk_fit_resection", "ctk_fit_resection_workspace_bytes")


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
    assert re.search(r"#define CTK_ABI_VERSION 9\b", header)
    assert int(header_layout()["sizeof"]["ctk_stream_args"]) == C.sizeof(L.StreamArgs) == 200  # no existing struct grew
    assert C.sizeof(L.Epipolar.Args) == 168 and C.sizeof(L.Pose.Args) == 176
    section = header.split("fit resection: the camera's pose against")[1].split("Op A")[0]
    assert not re.search(r"#define CTK_\w+\s+-?\d+", section)  # no new error code; the constants live with the rules
    for limit in ("Known limits", "unit is the structure's", "stay tracked", "no minimal P3P solver", "pinhole", "lens distortion",
                  "No bundle adjustment"):
        assert limit in section, limit
    for rule in ("4096", "only read", "2^61", "8 x 8", "(I | 0)", "bits 0 / 1 / 4", "bit 3", "bit 2", "no float", "lowest k on ties"):
        assert rule in section, rule
    csrc = os.path.join(ROOT, "co-tracker_amd", "csrc")
    math_h = open(os.path.join(csrc, "resection_math.h")).read()
    for name, value in (("LIST_MAX", 4096), ("MIN_POINTS", 6), ("HYPOTHESES_MAX", 1024), ("ROUNDS", 3)):
        assert re.search(r"#define CTK_RESECTION_%s %d\b" % (name, value), math_h), name
        assert getattr(L.Resection, name) == value
    assert "2^61" in math_h  # the bound of the int64 sums is stated
    body = math_h.split("#pragma once")[1]
    for inc in ("pose_math.h", "epipolar_math.h", "plane_math.h", "motion_math.h"):
        assert '#include "%s"' % inc in body
    # the rules take no library root and no trigonometry
    assert not re.search(r"(?<![\w])(sqrtf?|sinf?|cosf?|tanf?|atan2?f?|acosf?|asinf?)\s*\(", body) and "ctk_pose_polar" in body
    kernel = open(os.path.join(csrc, "resection.hip")).read().split("namespace {")[1]
    assert "atomic" not in kernel and "sqrt" not in kernel and "asm" not in kernel
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS = .*\bresection\.hip\b", makefile, re.M) and re.search(r"^NOFMA = .*\bresection\b", makefile, re.M)
    assert re.search(r"^HDRS = .*\bresection_math\.h\b", makefile, re.M)
    blob = open(L.LIB_PATH, "rb").read()  # the release library carries no CTK_* string literal
    assert not re.findall(rb"CTK_RESECTION\w*", blob)


def test_mirror_matches_the_compiler():
    from cotracker_amd import _lib as L
    cls, struct = L.Resection.Args, "ctk_fit_resection_args"
    fields = [f[0] for f in cls._fields_]
    lines = [f'printf("S %zu\\n", sizeof({struct}));'] + [f'printf("F {f} %zu\\n", offsetof({struct}, {f}));' for f in fields]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "resection_layout.c"), os.path.join(d, "resection_layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "ctk.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    got_size, got = int(out[0].split()[1]), {ln.split()[1]: int(ln.split()[2]) for ln in out[1:]}
    assert got_size == C.sizeof(cls) == 192
    assert got == {f: getattr(cls, f).offset for f in fields} and len(got) == 34
    # the header declares the fields in the mirror's order and no others
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), open(os.path.join(ROOT, "include", "ctk.h")).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert declared == fields
    # ctk_fit_pose_args' source fields and camera; the structure, the seed and the fit instead of the matrix, the mask and the depths
    pose = [f[0] for f in L.Pose.Args._fields_]
    assert [f for f in pose if f not in fields] == ["reserved", "mask", "fundamental", "depth"]
    assert [f for f in fields if f not in pose] == ["hypotheses", "seed", "tol", "structure", "valid", "seed_pose", "error"]


POINTERS = ("hist_coords", "visible", "hist_vis", "hist_conf", "first_row", "structure", "valid", "seed_pose", "pose", "label", "error", "stats")


def res_args(**kw):
    """A ctk_fit_resection_args that passes every check: 3 frames out of a ring of 8 rows, the lag form."""
    from cotracker_amd import _lib as L
    a = L.Resection.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.F, a.to, a.lag, a.anchor_frame = 2, 5, 4, 8, 6, 3, -1, 2, 0
    a.min_points, a.hypotheses, a.seed = 16, 256, 7
    a.fx, a.fy, a.cx, a.cy = 1000.0, 990.0, 960.0, 540.0
    a.sx, a.sy, a.thresh, a.tol = 1.37, 0.81, 0.6, 2.0
    for n in POINTERS:
        setattr(a, n, 4096)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


ANCHOR = dict(lag=0, anchor_coords=4096, anchor_visible=4096, anchor_frame=3)


def test_fit_refuses_before_any_launch(lib):
    """Every refusal is an E_* code (a launch on a machine without a GPU would be a hipError_t > 0)."""
    def fit(a, ws=None, nbytes=0):
        return lib.ctk_fit_resection(None if a is None else C.byref(a), ws, nbytes, None)

    def query(a):
        n = C.c_size_t(99)
        return lib.ctk_fit_resection_workspace_bytes(None if a is None else C.byref(a), C.byref(n))
    nan, inf = float("nan"), float("inf")
    assert fit(None) == E_NULL and query(None) == E_NULL
    assert lib.ctk_fit_resection_workspace_bytes(C.byref(res_args()), None) == E_NULL
    for f in ("hist_coords", "structure", "valid", "seed_pose", "pose", "label", "error", "stats"):
        assert fit(res_args(**{f: None})) == E_NULL, f
    assert fit(res_args(visible=None, hist_vis=None)) == E_NULL and fit(res_args(visible=None, hist_conf=None)) == E_NULL
    assert fit(res_args(**{**ANCHOR, "anchor_visible": None})) == E_NULL
    assert fit(res_args(**{**ANCHOR, "anchor_coords": None})) == E_NULL
    # ctk_fit_pose's refusals for the shared fields, min_points from 6 on, the hypotheses, the tolerance and the camera
    shape = (("G", (0, -1, 65536)), ("N", (0, -1, 3)), ("N_out", (0, -1, 6)), ("R", (0, -1, 4)), ("F", (0, -1, 7, 65536)),
             ("f0", (-1, -100, 2 ** 30 - 2)), ("lag", (0, -1, -2, 6, 1000)),
             ("sx", (0.0, -1.0, nan, inf)), ("sy", (0.0, -1.0, nan, inf)),
             ("min_points", (0, -1, 1, 5, 8193)), ("hypotheses", (0, -1, 1025, 4096)), ("tol", (0.0, -0.0, -1.0, nan, inf, -inf)),
             ("fx", (0.0, -1.0, -0.0, nan, inf, -inf)), ("fy", (0.0, -1000.0, nan, inf, -inf)), ("cx", (nan, inf, -inf)), ("cy", (nan, inf, -inf)))
    for field, values in shape:
        for v in values:
            assert fit(res_args(**{field: v})) == E_SHAPE, (field, v)
            assert query(res_args(**{field: v})) == E_SHAPE, (field, v)
    assert fit(res_args(N=9000, N_out=8193)) == E_SHAPE and query(res_args(N=9000, N_out=8192)) == 0    # N_out > 8192
    assert fit(res_args(F=7, lag=2, R=8)) == E_SHAPE and query(res_args(F=6, lag=2, R=8, f0=4)) == 0    # F + lag > R
    assert query(res_args(f0=2 ** 30 - 3, F=3)) == 0 and fit(res_args(f0=2 ** 30 - 2, F=3)) == E_SHAPE  # f0 + F > 2^30
    assert fit(res_args(G=8193, N=8192, N_out=1)) == E_SHAPE and fit(res_args(G=65535, N=65535, N_out=1)) == E_SHAPE
    assert fit(res_args(visible=None, thresh=nan)) == E_SHAPE and query(res_args(visible=None, thresh=nan)) == E_SHAPE
    assert fit(res_args(thresh=nan, pose=None)) == E_NULL
    # the source form: exactly one of the three, and rows of a ring that would alias
    for kw in (dict(lag=0), dict(to=3), dict(to=-2, lag=0), dict(to=2 ** 30 + 1, lag=0), dict(lag=2 ** 30 + 1), dict(ANCHOR, lag=2),
               dict(ANCHOR, to=3), dict(ANCHOR, anchor_frame=-1), dict(ANCHOR, anchor_frame=2 ** 30 + 1), dict(ANCHOR, F=9, f0=0),
               dict(to=0, lag=0, f0=6, F=3), dict(to=14, lag=0, f0=6, F=3)):
        assert fit(res_args(**kw)) == E_SHAPE, kw
        assert query(res_args(**kw)) == E_SHAPE, kw
    for kw in (dict(to=1, lag=0, f0=6, F=3), dict(to=13, lag=0, f0=6, F=3), dict(to=7, lag=0), dict(ANCHOR), dict(ANCHOR, F=8, f0=0),
               dict(ANCHOR, anchor_frame=2 ** 30)):
        assert query(res_args(**kw)) == 0, kw
    # the one-launch form keeps everything in LDS: the query answers 0, and reads no pointer of the struct (none of them is mapped)
    n = C.c_size_t(99)
    assert lib.ctk_fit_resection_workspace_bytes(C.byref(res_args()), C.byref(n)) == 0 and n.value == 0
    n = C.c_size_t(99)
    assert lib.ctk_fit_resection_workspace_bytes(C.byref(res_args(N=8192, N_out=8192, hypotheses=1024)), C.byref(n)) == 0 and n.value == 0
    assert fit(res_args(hist_coords=4100)) == E_ALIGN and fit(res_args(**{**ANCHOR, "anchor_coords": 4100})) == E_ALIGN
    for f in ("structure", "seed_pose", "pose", "error", "stats"):
        assert fit(res_args(**{f: 4098})) == E_ALIGN, f
    # what the rules admit reaches the pointer check: the refusal is then the NULL one; valid and label need no alignment
    for kw in (dict(lag=1, F=7), dict(lag=5, F=3), dict(N_out=5), dict(f0=0), dict(f0=1, lag=5), dict(N=8192, N_out=8192),
               dict(G=65535, N=1024, N_out=1), dict(first_row=None), dict(visible=None), dict(sx=1e-30, sy=1e30), dict(min_points=6),
               dict(min_points=8192), dict(hypotheses=1), dict(hypotheses=1024), dict(tol=1e-30), dict(tol=3e38), dict(seed=2 ** 32 - 1),
               dict(valid=4097, label=4099), dict(ANCHOR), dict(fx=1e-30, fy=3e38), dict(cx=-3e38, cy=3e38), dict(cx=0.0, cy=-0.0)):
        assert fit(res_args(stats=None, **kw)) == E_NULL, kw
        assert query(res_args(stats=None, **kw)) == 0, kw  # the query looks at no pointer of the struct but the anchor's


def test_python_layers_signatures_and_refusals():
    from cotracker_amd import model, ops
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    sig = inspect.signature(ops.fit_resection)
    assert list(sig.parameters) == ["tracks", "visible", "intrinsics", "structure", "valid", "seed_pose", "lag", "to", "anchor", "tol",
                                    "hypotheses", "min_points", "seed", "first_row", "scale", "out"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[6:]] == [1, None, None, 2.0, 256, 16, 0, None, (1, 1), None]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[6:])
    assert all(sig.parameters[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in list(sig.parameters)[:6])
    ssig = inspect.signature(ops.structure_from_pose)
    assert list(ssig.parameters) == ["tracks_row", "intrinsics", "depth", "label", "max_depth", "scale"]
    assert ssig.parameters["max_depth"].default == 64.0 and ssig.parameters["scale"].default == (1, 1)
    assert ops.Structure.__slots__ == ("points", "valid", "anchor", "intrinsics")
    rsig = inspect.signature(CoTrackerOnlinePredictor.reconstruct)
    assert list(rsig.parameters) == ["self", "intrinsics", "frame", "lag", "max_depth", "group", "tol", "hypotheses", "min_base", "min_points",
                                     "seed", "mask"]
    assert [rsig.parameters[n].default for n in list(rsig.parameters)[2:]] == [None, 8, 64.0, 0, 1.0, 512, 16.0, 16, 0, None]
    lsig = inspect.signature(CoTrackerOnlinePredictor.localize)
    assert list(lsig.parameters)[:8] == ["self", "structure", "n", "first_frame", "tol", "hypotheses", "min_points", "seed"]
    assert [lsig.parameters[n].default for n in list(lsig.parameters)[2:8]] == [None, None, 2.0, 256, 16, 0]
    for doc in (CoTrackerOnlinePredictor.reconstruct.__doc__, CoTrackerOnlinePredictor.localize.__doc__):
        for limit in ("baseline", "replenish()", "triangulating new points", "not built", "pinhole", "distortion", "bundle"):
            assert limit in doc, limit
    gsig = inspect.signature(ops.StreamGroups.resection)
    assert list(gsig.parameters)[:7] == ["self", "f0", "F", "intrinsics", "structure", "valid", "seed_pose"]
    assert [gsig.parameters[n].default for n in ("lag", "to", "anchor", "thresh", "tol", "hypotheses", "min_points", "seed", "group", "out")] == \
        [1, None, None, 0.6, 2.0, 256, 16, 0, None, None]
    msig = inspect.signature(model.CoTrackerThreeOnline.stream_resection)
    assert list(msig.parameters)[:7] == ["self", "f0", "F", "intrinsics", "structure", "valid", "seed_pose"]
    # the existing readers keep their defaults
    psig = inspect.signature(CoTrackerOnlinePredictor.pose)
    assert [psig.parameters[n].default for n in list(psig.parameters)[2:]] == [None, None, 8, 1.0, 512, 16.0, 16, 0, None, 0]
    # structure_from_pose is elementwise torch and runs anywhere
    row = torch.tensor([[100.0, 50.0], [10.0, 20.0], [30.0, 40.0], [1.0, 2.0]])
    depth = torch.tensor([[2.0, 4.0], [1.0, -1.0], [float("nan"), 1.0], [3.0, 65.0]])
    pts, ok = ops.structure_from_pose(row, (100.0, 50.0, 50.0, 25.0), depth, torch.tensor([1, 1, 1, 1], dtype=torch.int8), scale=(1.0, 2.0))
    assert ok.tolist() == [1, 0, 0, 0] and ok.dtype == torch.int8 and pts[0].tolist() == [2.0, 6.0, 4.0] and (pts[1:] == 0).all()
    pts, ok = ops.structure_from_pose(row, (100.0, 50.0, 50.0, 25.0), depth, torch.tensor([0, 1, 1, 1], dtype=torch.int8), max_depth=65.0)
    assert ok.tolist() == [0, 0, 0, 1]
    # host tensors are refused: no fall-back
    cam = (100.0, 100.0, 24.0, 16.0)
    with pytest.raises(ValueError, match="device tensor"):
        ops.fit_resection(torch.zeros(2, 9, 2), torch.zeros(2, 9, dtype=torch.bool), cam, torch.zeros(9, 3), torch.zeros(9, dtype=torch.int8),
                          torch.zeros(2, 3, 4))
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=8)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.reconstruct(cam)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.localize(None)
    p(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, queries=torch.zeros(1, 3, 3))
    with pytest.raises(RuntimeError, match="no stream is running"):  # after the first step: no window has been tracked
        p.reconstruct(cam)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.model.stream_resection(0, 1, cam, None, None, None)
    p2 = CoTrackerOnlinePredictor(checkpoint=None, v2=True, window_len=8)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.reconstruct(cam)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.localize(None)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.model.stream_resection(0, 1, cam, None, None, None)
