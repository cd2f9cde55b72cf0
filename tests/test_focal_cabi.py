"""Fit focal, the part that needs no GPU: ctk_fit_focal and its workspace query are declared, bound and exported without an ABI bump, the
new struct's ctypes mirror has the compiler's layout, every refusal comes back before any launch and is ctk_fit_pose's for the fields
both structs have, and the Python layers have the signatures, defaults and stated limits the callers rely on."""
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
NAMES = ("ctk_fit_focal", "ctk_fit_focal_workspace_bytes")
LIMITS = ("Square pixels", "principal point is assumed", "must TURN", "no zoom", "No distortion estimate")


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
    assert C.sizeof(L.Epipolar.Args) == 168 and C.sizeof(L.Pose.Args) == 176 and C.sizeof(L.P3p.Args) == 184
    section = header.split("fit focal: the focal length the camera had")[1].split("fit structure: points added")[0]
    assert not re.search(r"#define CTK_\w+\s+-?\d+", section)  # no new error code; the constants live with the rules
    for limit in ("Known limits",) + LIMITS + ("finer sweep",):
        assert limit in section, limit
    for rule in ("read only", "2^61", "2^32", "lowest index on ties", "curve_in", "bit 0", "bit 1", "bit 2", "65535", "one plain store",
                 "Two launches", "8-byte aligned", "answers 0"):
        assert rule in section, rule
    csrc = os.path.join(ROOT, "co-tracker_amd", "csrc")
    math_h = open(os.path.join(csrc, "focal_math.h")).read()
    for define, value in (("CTK_FOCAL_K_MAX 256", L.Focal.K_MAX), ("CTK_FOCAL_FRAMES_MAX 65535", L.Focal.FRAMES_MAX),
                          ("CTK_FOCAL_BIT_END 1", L.Focal.BIT_END), ("CTK_FOCAL_BIT_FLAT 2", L.Focal.BIT_FLAT),
                          ("CTK_FOCAL_BIT_CANDIDATE 4", L.Focal.BIT_CANDIDATE)):
        assert re.search(r"#define %s\b" % define, math_h) and int(define.split()[1]) == value
    assert "CTK_FOCAL_ONE 4294967296.0" in math_h and L.Focal.ONE == 2 ** 32
    body = math_h.split("#pragma once")[1]
    assert '#include "pose_math.h"' in body
    for reused in ("ctk_pose_essential", "ctk_pose_entry", "CtkPoseCam"):
        assert reused in body, reused
    # the rules take no library root, logarithm or power, and restate nothing of pose's
    assert not re.search(r"(?<![\w])(sqrtf?|logf?|log2f?|powf?|expf?|sinf?|cosf?)\s*\(", body)
    assert not re.search(r"CTK_MM_HD \w+ ctk_(pose|plane|epi)_", body)
    kernel = open(os.path.join(csrc, "focal.hip")).read().split("namespace {")[1]
    assert "atomic" not in kernel and "sqrt" not in kernel and "asm" not in kernel
    for reused in ("ctk_pose_essential", "ctk_pose_decompose", "ctk_pose_depths", "ctk_pose_front", "ctk_pose_choose", "ctk_pose_entry",
                   "ctk_pose_terms", "ctk_pose_update", "CTK_POSE_ROUNDS", "CTK_POSE_SOLVE_DOUBLES", "ctk_focal_term", "ctk_focal_choose",
                   "fit_gather", "fit_stage", "motion_wave_sum", "fit_check_source", "fit_null_source", "fit_align_source"):
        assert reused in kernel, reused
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS = .*\bfocal\.hip\b", makefile, re.M) and re.search(r"^NOFMA = .*\bfocal\b", makefile, re.M)
    assert re.search(r"^HDRS = .*\bfocal_math\.h\b", makefile, re.M)
    blob = open(L.LIB_PATH, "rb").read()  # the release library carries no CTK_* string literal
    assert not re.findall(rb"CTK_FOCAL\w*", blob)


def test_mirror_matches_the_compiler():
    from cotracker_amd import _lib as L
    cls, struct = L.Focal.Args, "ctk_fit_focal_args"
    fields = [f[0] for f in cls._fields_]
    lines = [f'printf("S %zu\\n", sizeof({struct}));'] + [f'printf("F {f} %zu\\n", offsetof({struct}, {f}));' for f in fields]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "focal_layout.c"), os.path.join(d, "focal_layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "ctk.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    got_size, got = int(out[0].split()[1]), {ln.split()[1]: int(ln.split()[2]) for ln in out[1:]}
    assert got_size == C.sizeof(cls) == 208
    assert got == {f: getattr(cls, f).offset for f in fields} and len(got) == 36
    # the header declares the fields in the mirror's order and no others
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), open(os.path.join(ROOT, "include", "ctk.h")).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert declared == fields
    # ctk_fit_pose_args' source fields, fundamental, label, mask, min_points, cx, cy: the same names and types
    pose = dict(L.Pose.Args._fields_)
    shared = [f for f in cls._fields_ if f[0] in pose]
    assert [f[0] for f in shared] == [n for n, _ in L.Pose.Args._fields_ if n not in ("fx", "fy", "pose", "depth")]
    assert all(pose[n] is ty for n, ty in shared)


POINTERS = ("hist_coords", "visible", "hist_vis", "hist_conf", "first_row", "mask", "fundamental", "label", "stats")
SHARED = ("G", "N", "N_out", "R", "f0", "F", "to", "lag", "anchor_frame", "min_points", "cx", "cy", "sx", "sy", "thresh", "reserved",
          "anchor_coords", "anchor_visible") + POINTERS


def make_args(cls, **kw):
    """An args struct of `cls` (Focal.Args or Pose.Args) that passes every check: 3 frames out of a ring of 8 rows, the lag form.  A
    keyword that the struct does not have is left out."""
    a = cls()
    a.G, a.N, a.N_out, a.R, a.f0, a.F, a.to, a.lag, a.anchor_frame = 2, 5, 4, 8, 6, 3, -1, 2, 0
    a.min_points, a.cx, a.cy, a.sx, a.sy, a.thresh, a.reserved = 16, 960.0, 540.0, 1.37, 0.81, 0.6, 0
    own = ("focals", "focal", "curve", "cost") if hasattr(a, "focals") else ("pose", "depth")
    for n in POINTERS + own:
        setattr(a, n, 4096)
    if hasattr(a, "focals"):
        a.K, a.min_frames, a.tol, a.contrast = 64, 1, 1.0, 1.5
    else:
        a.fx, a.fy = 1000.0, 1000.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def focal_args(**kw):
    from cotracker_amd import _lib as L
    return make_args(L.Focal.Args, **kw)


ANCHOR = dict(lag=0, anchor_coords=4096, anchor_visible=4096, anchor_frame=3)


def test_fit_refuses_before_any_launch(lib):
    """Every refusal is an E_* code (a launch on a machine without a GPU would be a hipError_t > 0), and it is the code ctk_fit_pose
    answers for the fields both structs have."""
    from cotracker_amd import _lib as L

    def fit(a, ws=None, nbytes=0):
        return lib.ctk_fit_focal(None if a is None else C.byref(a), ws, nbytes, None)

    def query(a):
        n = C.c_size_t(99)
        return lib.ctk_fit_focal_workspace_bytes(None if a is None else C.byref(a), C.byref(n))

    def both(expect, **kw):
        """The refusal of ctk_fit_focal, and ctk_fit_pose's for the same fields."""
        assert fit(focal_args(**kw)) == expect, kw
        assert all(k in SHARED for k in kw), kw
        assert lib.ctk_fit_pose(C.byref(make_args(L.Pose.Args, **kw)), None, 0, None) == expect, kw
    nan, inf = float("nan"), float("inf")
    assert fit(None) == E_NULL and query(None) == E_NULL
    assert lib.ctk_fit_focal_workspace_bytes(C.byref(focal_args()), None) == E_NULL
    for f in ("hist_coords", "fundamental", "label", "stats"):
        both(E_NULL, **{f: None})
    for f in ("focals", "focal", "curve", "cost"):
        assert fit(focal_args(**{f: None})) == E_NULL, f
    both(E_NULL, visible=None, hist_vis=None), both(E_NULL, visible=None, hist_conf=None)
    both(E_NULL, **{**ANCHOR, "anchor_visible": None}), both(E_NULL, **{**ANCHOR, "anchor_coords": None})
    shape = (("G", (0, -1, 65536)), ("N", (0, -1, 3)), ("N_out", (0, -1, 6)), ("R", (0, -1, 4)), ("F", (0, -1, 7, 65536)),
             ("f0", (-1, -100, 2 ** 30 - 2)), ("lag", (0, -1, -2, 6, 1000)), ("reserved", (1, -1)),
             ("sx", (0.0, -1.0, nan, inf)), ("sy", (0.0, -1.0, nan, inf)),
             ("min_points", (0, -1, 1, 7, 8193)), ("cx", (nan, inf, -inf)), ("cy", (nan, inf, -inf)))
    for field, values in shape:
        for v in values:
            both(E_SHAPE, **{field: v})
            assert query(focal_args(**{field: v})) == E_SHAPE, (field, v)
    own = (("K", (0, -1, 257, 4096)), ("min_frames", (0, -1)), ("tol", (0.0, -0.0, -1.0, nan, inf, -inf)),
           ("contrast", (0.0, 0.999, -2.0, nan, inf, -inf)))
    for field, values in own:
        for v in values:
            assert fit(focal_args(**{field: v})) == E_SHAPE and query(focal_args(**{field: v})) == E_SHAPE, (field, v)
    assert fit(focal_args(N=9000, N_out=8193)) == E_SHAPE and query(focal_args(N=9000, N_out=8192)) == 0    # N_out > 8192
    assert fit(focal_args(F=7, lag=2, R=8)) == E_SHAPE and query(focal_args(F=6, lag=2, R=8, f0=4)) == 0    # F + lag > R
    assert query(focal_args(f0=2 ** 30 - 3, F=3)) == 0 and fit(focal_args(f0=2 ** 30 - 2, F=3)) == E_SHAPE  # f0 + F > 2^30
    assert query(focal_args(R=65536, F=65535, lag=1, f0=1)) == 0 and query(focal_args(R=2 ** 17, F=65536, lag=1, f0=1)) == E_SHAPE  # the frame bound
    assert fit(focal_args(visible=None, thresh=nan)) == E_SHAPE and query(focal_args(visible=None, thresh=nan)) == E_SHAPE
    assert fit(focal_args(thresh=nan, cost=None)) == E_NULL
    # the source form: exactly one of the three, and rows of a ring that would alias
    for kw in (dict(lag=0), dict(to=3), dict(to=-2, lag=0), dict(to=2 ** 30 + 1, lag=0), dict(lag=2 ** 30 + 1), dict(ANCHOR, lag=2),
               dict(ANCHOR, to=3), dict(ANCHOR, anchor_frame=-1), dict(ANCHOR, anchor_frame=2 ** 30 + 1), dict(ANCHOR, F=9, f0=0),
               dict(to=0, lag=0, f0=6, F=3), dict(to=14, lag=0, f0=6, F=3)):
        both(E_SHAPE, **kw)
        assert query(focal_args(**kw)) == E_SHAPE, kw
    for kw in (dict(to=1, lag=0, f0=6, F=3), dict(to=13, lag=0, f0=6, F=3), dict(to=7, lag=0), dict(ANCHOR), dict(ANCHOR, F=8, f0=0),
               dict(ANCHOR, anchor_frame=2 ** 30)):
        assert query(focal_args(**kw)) == 0, kw
    # everything lives in LDS and in `cost`: the query answers 0, and reads no pointer of the struct
    n = C.c_size_t(99)
    assert lib.ctk_fit_focal_workspace_bytes(C.byref(focal_args(N=8192, N_out=8192, K=256)), C.byref(n)) == 0 and n.value == 0
    both(E_ALIGN, hist_coords=4100), both(E_ALIGN, **{**ANCHOR, "anchor_coords": 4100})
    for f in ("fundamental", "stats"):
        both(E_ALIGN, **{f: 4098})
    for f, v in (("focals", 4098), ("focal", 4098), ("curve_in", 4100), ("curve", 4100), ("cost", 4100)):
        assert fit(focal_args(**{f: v})) == E_ALIGN, f
    # what the rules admit reaches the pointer check: the refusal is then the NULL one; label and mask need no alignment
    for kw in (dict(lag=1, F=7), dict(lag=5, F=3), dict(N_out=5), dict(f0=0), dict(f0=1, lag=5), dict(N=8192, N_out=8192),
               dict(G=65535, N=1024, N_out=1), dict(first_row=None), dict(visible=None), dict(mask=None), dict(sx=1e-30, sy=1e30),
               dict(min_points=8), dict(min_points=8192), dict(label=4097, mask=4099), dict(ANCHOR), dict(cx=-3e38, cy=3e38),
               dict(cx=0.0, cy=-0.0)):
        both(E_NULL, stats=None, **kw)
        assert query(focal_args(stats=None, **kw)) == 0, kw  # the query looks at no pointer of the struct but the anchor's
    for kw in (dict(K=1), dict(K=256), dict(min_frames=2 ** 31 - 1), dict(tol=1e-30), dict(tol=3e38), dict(contrast=1.0), dict(contrast=3e38),
               dict(curve_in=None), dict(curve_in=4104)):
        assert fit(focal_args(stats=None, **kw)) == E_NULL and query(focal_args(stats=None, **kw)) == 0, kw


def test_python_layers_signatures_and_refusals():
    from cotracker_amd import model, model_v2, ops
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    sig = inspect.signature(ops.fit_focal)
    assert list(sig.parameters) == ["tracks", "visible", "fundamental", "label", "focals", "size", "candidates", "span", "principal", "mask",
                                    "lag", "to", "anchor", "tol", "min_points", "min_frames", "contrast", "curve", "first_row", "scale", "out"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[4:]] == [None, None, 64, (0.25, 4.0), None, None, 1, None, None, 1.0, 16, 1,
                                                                             1.5, None, None, (1, 1), None]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[4:])
    assert all(sig.parameters[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in list(sig.parameters)[:4])
    assert "focal" in ops._FITS and ops._FITS["focal"].entry == "ctk_fit_focal" and len(ops._FITS) == 10
    gsig, old = inspect.signature(ops.StreamGroups.focal), inspect.signature(ops.StreamGroups.pose)
    assert list(gsig.parameters)[:5] == ["self", "f0", "F", "fundamental", "label"]
    for n in ("mask", "lag", "to", "anchor", "N_out", "scale", "thresh", "first_row", "group", "out"):  # pose's source keywords, alike
        assert gsig.parameters[n].default == old.parameters[n].default and gsig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY, n
    assert [gsig.parameters[n].default for n in ("focals", "size", "candidates", "span", "principal", "tol", "min_points", "min_frames",
                                                 "contrast", "curve")] == [None, None, 64, (0.25, 4.0), None, 1.0, 16, 1, 1.5, None]
    msig = inspect.signature(model.CoTrackerThreeOnline.stream_focal)
    assert list(msig.parameters)[:5] == ["self", "f0", "F", "fundamental", "label"]
    assert "stream_focal" in open(model_v2.__file__).read()
    psig = inspect.signature(CoTrackerOnlinePredictor.calibrate)
    assert list(psig.parameters) == ["self", "n", "first_frame", "lag", "candidates", "span", "focals", "principal", "tol", "hypotheses",
                                     "min_base", "min_points", "min_frames", "contrast", "seed", "mask", "group", "state"]
    assert [psig.parameters[n].default for n in list(psig.parameters)[1:]] == [None, None, 8, 64, (0.25, 4.0), None, None, 1.0, 512, 16.0, 16, 1,
                                                                               1.5, 0, None, 0, None]
    isig = inspect.signature(CoTrackerOnlinePredictor.intrinsics)
    assert list(isig.parameters) == ["self", "focal", "principal"] and isig.parameters["principal"].default is None
    posig = inspect.signature(CoTrackerOnlinePredictor.pose)  # pose() and its signature do not change
    assert list(posig.parameters) == ["self", "intrinsics", "n", "first_frame", "lag", "tol", "hypotheses", "min_base", "min_points", "seed",
                                      "mask", "group"]
    for doc in (CoTrackerOnlinePredictor.calibrate.__doc__, ops.fit_focal.__doc__):
        for limit in ("quare pixels", "assumed", "must turn", "zoom", "no distortion estimate"):
            assert limit in doc, limit
    assert "three launches, no wait" in CoTrackerOnlinePredictor.calibrate.__doc__
    assert "one device-to-host copy" in CoTrackerOnlinePredictor.intrinsics.__doc__.replace("THE one", "one")
    assert "calibrate()" in CoTrackerOnlinePredictor.pose.__doc__ and "calibrate()" in CoTrackerOnlinePredictor.reconstruct.__doc__
    # the candidates as the restatement makes them, and the refusals that need no device
    import focal_reference as FR
    for bad in (dict(candidates=0), dict(candidates=257), dict(span=(0.0, 1.0)), dict(span=(2.0, 1.0)), dict(span=(1.0, float("inf")))):
        with pytest.raises(ValueError):
            ops.focal_candidates((1080, 1920), "cpu", **bad)
    assert FR.candidates(1920, K=64)[0] == 480.0 and FR.candidates(1920, K=64)[-1] == 7680.0 and len(FR.candidates(1920, K=1)) == 1
    # host tensors are refused: no fall-back
    with pytest.raises(ValueError, match="device tensor"):
        ops.fit_focal(torch.zeros(2, 9, 2), torch.zeros(2, 9, dtype=torch.bool), torch.zeros(1, 2, 3, 3), torch.zeros(1, 2, 9, dtype=torch.int8),
                      size=(10, 10))
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=8)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.calibrate()
    with pytest.raises(RuntimeError, match="no stream has been started"):
        p.intrinsics(500.0)
    assert p.intrinsics(500.0, (10.0, 20.0)) == (500.0, 500.0, 10.0, 20.0)
    for zero in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="no fit yet"):
            p.intrinsics(zero, (10.0, 20.0))
    p(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, queries=torch.zeros(1, 3, 3))
    with pytest.raises(RuntimeError, match="no stream is running"):  # after the first step: no window has been tracked
        p.calibrate()
    assert p.intrinsics(500.0) == (500.0, 500.0, 23.5, 15.5)  # the picture centre
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.model.stream_focal(0, 1, None, None)
    p2 = CoTrackerOnlinePredictor(checkpoint=None, v2=True, window_len=8)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.calibrate()
    with pytest.raises(NotImplementedError, match="v2"):
        p2.model.stream_focal(0, 1, None, None)
