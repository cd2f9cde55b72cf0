"""Fit pose, the part that needs no GPU: ctk_fit_pose and its workspace query are declared, bound and exported without an ABI bump,
the new struct's ctypes mirror has the compiler's layout, every refusal comes back before any launch, and the Python layers have the
signatures and defaults the callers rely on."""
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
NAMES = ("ctk_fit_pose", "ctk_fit_pose_workspace_bytes")


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
    assert C.sizeof(L.Motion.Args) == 128 and C.sizeof(L.Planes.Args) == 176 and C.sizeof(L.Epipolar.Args) == 168
    section = header.split("fit pose: how the camera turned")[1].split("Op A")[0]
    assert not re.search(r"#define CTK_\w+\s+-?\d+", section)  # no new error code; the constants live with the rules
    for limit in ("Known limits", "scale is unknown", "depths are in baselines", "changes from frame to frame", "pinhole", "lens distortion",
                  "No parallax means no pose", "stats[1] / stats[0]", "ctk_fit_planes", "no bundle adjustment"):
        assert limit in section, limit
    for rule in ("Horn 1990", "0x7FC00000", "only read", "2^61", "8 x 8", "cheirality", "rsqrt", "(I | 0)"):
        assert rule in section, rule
    csrc = os.path.join(ROOT, "co-tracker_amd", "csrc")
    math_h = open(os.path.join(csrc, "pose_math.h")).read()
    assert re.search(r"#define CTK_POSE_MIN_POINTS 8\b", math_h) and re.search(r"#define CTK_POSE_SUMS 28\b", math_h)
    assert re.search(r"#define CTK_POSE_ROUNDS 2\b", math_h) and "2^61" in math_h  # the bound of the int64 sums is stated
    assert (L.Pose.MIN_POINTS, L.Pose.SUMS, L.Pose.ROUNDS) == (8, 28, 2)
    body = math_h.split("#pragma once")[1]
    for inc in ("epipolar_math.h", "plane_math.h", "motion_math.h"):
        assert '#include "%s"' % inc in body
    assert not re.search(r"(?<![\w])sqrtf?\s*\(", body) and "ctk_pose_rsqrt" in body  # the rules take no library square root
    kernel = open(os.path.join(csrc, "pose.hip")).read()
    assert "atomic" not in kernel.split("namespace {")[1] and "sqrt" not in kernel.split("namespace {")[1]
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS = .*\bpose\.hip\b", makefile, re.M) and re.search(r"^NOFMA = .*\bpose\b", makefile, re.M)
    assert re.search(r"^HDRS = .*\bpose_math\.h\b", makefile, re.M)
    blob = open(L.LIB_PATH, "rb").read()  # the release library carries no CTK_* string literal
    assert not re.findall(rb"CTK_POSE\w*", blob)


def test_mirror_matches_the_compiler():
    from cotracker_amd import _lib as L
    cls, struct = L.Pose.Args, "ctk_fit_pose_args"
    fields = [f[0] for f in cls._fields_]
    lines = [f'printf("S %zu\\n", sizeof({struct}));'] + [f'printf("F {f} %zu\\n", offsetof({struct}, {f}));' for f in fields]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "pose_layout.c"), os.path.join(d, "pose_layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "ctk.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    got_size, got = int(out[0].split()[1]), {ln.split()[1]: int(ln.split()[2]) for ln in out[1:]}
    assert got_size == C.sizeof(cls) == 176
    assert got == {f: getattr(cls, f).offset for f in fields} and len(got) == 31
    # the header declares the fields in the mirror's order and no others
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), open(os.path.join(ROOT, "include", "ctk.h")).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert declared == fields
    # ctk_fit_epipolar_args without K, seed, tol, min_base and error, with the camera; fundamental and label stay, as inputs
    epi = [f[0] for f in L.Epipolar.Args._fields_]
    assert [f for f in epi if f not in fields] == ["K", "seed", "tol", "min_base", "error"]
    assert [f for f in fields if f not in epi] == ["fx", "fy", "cx", "cy", "pose", "depth"]


POINTERS = ("hist_coords", "visible", "hist_vis", "hist_conf", "first_row", "mask", "fundamental", "label", "pose", "depth", "stats")


def pose_args(**kw):
    """A ctk_fit_pose_args that passes every check: 3 frames out of a ring of 8 rows, the lag form, a mask."""
    from cotracker_amd import _lib as L
    a = L.Pose.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.F, a.to, a.lag, a.anchor_frame = 2, 5, 4, 8, 6, 3, -1, 2, 0
    a.min_points = 16
    a.fx, a.fy, a.cx, a.cy = 1000.0, 990.0, 960.0, 540.0
    a.sx, a.sy, a.thresh, a.reserved = 1.37, 0.81, 0.6, 0
    for n in POINTERS:
        setattr(a, n, 4096)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


ANCHOR = dict(lag=0, anchor_coords=4096, anchor_visible=4096, anchor_frame=3)


def test_fit_refuses_before_any_launch(lib):
    """Every refusal is an E_* code (a launch on a machine without a GPU would be a hipError_t > 0)."""
    def fit(a, ws=None, nbytes=0):
        return lib.ctk_fit_pose(None if a is None else C.byref(a), ws, nbytes, None)

    def query(a):
        n = C.c_size_t(99)
        return lib.ctk_fit_pose_workspace_bytes(None if a is None else C.byref(a), C.byref(n))
    nan, inf = float("nan"), float("inf")
    assert fit(None) == E_NULL and query(None) == E_NULL
    assert lib.ctk_fit_pose_workspace_bytes(C.byref(pose_args()), None) == E_NULL
    for f in ("hist_coords", "fundamental", "label", "pose", "depth", "stats"):
        assert fit(pose_args(**{f: None})) == E_NULL, f
    assert fit(pose_args(visible=None, hist_vis=None)) == E_NULL and fit(pose_args(visible=None, hist_conf=None)) == E_NULL
    assert fit(pose_args(**{**ANCHOR, "anchor_visible": None})) == E_NULL
    assert fit(pose_args(**{**ANCHOR, "anchor_coords": None})) == E_NULL
    # ctk_fit_epipolar's refusals for the shared fields, min_points from 8 on, and the camera
    shape = (("G", (0, -1, 65536)), ("N", (0, -1, 3)), ("N_out", (0, -1, 6)), ("R", (0, -1, 4)), ("F", (0, -1, 7, 65536)),
             ("f0", (-1, -100, 2 ** 30 - 2)), ("lag", (0, -1, -2, 6, 1000)),
             ("sx", (0.0, -1.0, nan, inf)), ("sy", (0.0, -1.0, nan, inf)), ("reserved", (1, -1)),
             ("min_points", (0, -1, 1, 7, 8193)),
             ("fx", (0.0, -1.0, -0.0, nan, inf, -inf)), ("fy", (0.0, -1000.0, nan, inf, -inf)), ("cx", (nan, inf, -inf)), ("cy", (nan, inf, -inf)))
    for field, values in shape:
        for v in values:
            assert fit(pose_args(**{field: v})) == E_SHAPE, (field, v)
            assert query(pose_args(**{field: v})) == E_SHAPE, (field, v)
    assert fit(pose_args(N=9000, N_out=8193)) == E_SHAPE and query(pose_args(N=9000, N_out=8192)) == 0    # N_out > 8192
    assert fit(pose_args(F=7, lag=2, R=8)) == E_SHAPE and query(pose_args(F=6, lag=2, R=8, f0=4)) == 0    # F + lag > R
    assert query(pose_args(f0=2 ** 30 - 3, F=3)) == 0 and fit(pose_args(f0=2 ** 30 - 2, F=3)) == E_SHAPE  # f0 + F > 2^30
    assert fit(pose_args(G=8193, N=8192, N_out=1)) == E_SHAPE and fit(pose_args(G=65535, N=65535, N_out=1)) == E_SHAPE
    assert fit(pose_args(visible=None, thresh=nan)) == E_SHAPE and query(pose_args(visible=None, thresh=nan)) == E_SHAPE
    assert fit(pose_args(thresh=nan, pose=None)) == E_NULL
    # the source form: exactly one of the three, and rows of a ring that would alias
    for kw in (dict(lag=0), dict(to=3), dict(to=-2, lag=0), dict(to=2 ** 30 + 1, lag=0), dict(lag=2 ** 30 + 1), dict(ANCHOR, lag=2),
               dict(ANCHOR, to=3), dict(ANCHOR, anchor_frame=-1), dict(ANCHOR, anchor_frame=2 ** 30 + 1), dict(ANCHOR, F=9, f0=0),
               dict(to=0, lag=0, f0=6, F=3), dict(to=14, lag=0, f0=6, F=3)):
        assert fit(pose_args(**kw)) == E_SHAPE, kw
        assert query(pose_args(**kw)) == E_SHAPE, kw
    for kw in (dict(to=1, lag=0, f0=6, F=3), dict(to=13, lag=0, f0=6, F=3), dict(to=7, lag=0), dict(ANCHOR), dict(ANCHOR, F=8, f0=0),
               dict(ANCHOR, anchor_frame=2 ** 30)):
        assert query(pose_args(**kw)) == 0, kw
    n = C.c_size_t(99)  # the one-launch form keeps everything in LDS: the query answers 0
    assert lib.ctk_fit_pose_workspace_bytes(C.byref(pose_args()), C.byref(n)) == 0 and n.value == 0
    assert lib.ctk_fit_pose_workspace_bytes(C.byref(pose_args(N=8192, N_out=8192)), C.byref(n)) == 0 and n.value == 0
    assert fit(pose_args(hist_coords=4100)) == E_ALIGN and fit(pose_args(**{**ANCHOR, "anchor_coords": 4100})) == E_ALIGN
    for f in ("fundamental", "pose", "depth", "stats"):
        assert fit(pose_args(**{f: 4098})) == E_ALIGN, f
    # what the rules admit reaches the pointer check: the refusal is then the NULL one; mask and label need no alignment
    for kw in (dict(lag=1, F=7), dict(lag=5, F=3), dict(N_out=5), dict(f0=0), dict(f0=1, lag=5), dict(N=8192, N_out=8192),
               dict(G=65535, N=1024, N_out=1), dict(first_row=None), dict(visible=None), dict(sx=1e-30, sy=1e30), dict(min_points=8),
               dict(min_points=8192), dict(mask=None), dict(mask=4097, label=4099), dict(ANCHOR), dict(fx=1e-30, fy=3e38),
               dict(cx=-3e38, cy=3e38), dict(cx=0.0, cy=-0.0)):
        assert fit(pose_args(stats=None, **kw)) == E_NULL, kw
        assert query(pose_args(stats=None, **kw)) == 0, kw  # the query looks at no pointer of the struct but the anchor's


def test_python_layers_signatures_and_refusals():
    from cotracker_amd import model, ops
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    sig = inspect.signature(ops.fit_pose)
    assert list(sig.parameters) == ["tracks", "visible", "intrinsics", "fundamental", "label", "mask", "lag", "to", "anchor", "min_points",
                                    "first_row", "scale", "out"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[5:]] == [None, 1, None, None, 8, None, (1, 1), None]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[5:])
    assert all(sig.parameters[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in list(sig.parameters)[:5])
    psig = inspect.signature(CoTrackerOnlinePredictor.pose)
    assert list(psig.parameters) == ["self", "intrinsics", "n", "first_frame", "lag", "tol", "hypotheses", "min_base", "min_points", "seed",
                                     "mask", "group"]
    assert [psig.parameters[n].default for n in list(psig.parameters)[2:]] == [None, None, 8, 1.0, 512, 16.0, 16, 0, None, 0]
    assert psig.parameters["intrinsics"].default is inspect.Parameter.empty
    gsig = inspect.signature(ops.StreamGroups.pose)
    assert list(gsig.parameters)[:6] == ["self", "f0", "F", "intrinsics", "fundamental", "label"]
    assert [gsig.parameters[n].default for n in ("mask", "lag", "to", "anchor", "thresh", "min_points", "group", "out")] == \
        [None, 1, None, None, 0.6, 8, None, None]
    msig = inspect.signature(model.CoTrackerThreeOnline.stream_pose)
    assert list(msig.parameters)[:6] == ["self", "f0", "F", "intrinsics", "fundamental", "label"]
    # the existing readers keep their defaults
    esig = inspect.signature(CoTrackerOnlinePredictor.epipolar)
    assert [esig.parameters[n].default for n in list(esig.parameters)[1:]] == [None, None, 8, 1.0, 512, 16.0, 16, 0, None, 0]
    # host tensors are refused: no fall-back
    cam = (100.0, 100.0, 24.0, 16.0)
    with pytest.raises(ValueError, match="device tensor"):
        ops.fit_pose(torch.zeros(2, 9, 2), torch.zeros(2, 9, dtype=torch.bool), cam, torch.zeros(1, 2, 3, 3),
                     torch.zeros(1, 2, 9, dtype=torch.int8))
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=8)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.pose(cam)
    p(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, queries=torch.zeros(1, 3, 3))
    with pytest.raises(RuntimeError, match="no stream is running"):  # after the first step: no window has been tracked
        p.pose(cam)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.model.stream_pose(0, 1, cam, None, None)
    p2 = CoTrackerOnlinePredictor(checkpoint=None, v2=True, window_len=8)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.pose(cam)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.model.stream_pose(0, 1, cam, None, None)
