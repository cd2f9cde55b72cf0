"""Fit structure, the part that needs no GPU: ctk_fit_structure and its workspace query are declared, bound and exported without an ABI
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
NAMES = ("ctk_fit_structure", "ctk_fit_structure_workspace_bytes")


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
    assert C.sizeof(L.Resection.Args) == 192 and C.sizeof(L.Pose.Args) == 176
    section = header.split("fit structure: points added to a 3-D structure")[1].split("Op A")[0]
    assert not re.search(r"#define CTK_\w+\s+-?\d+", section)  # no new error code; the constants live with the rules
    for limit in ("Known limits", "visible on the frame", "once per restatement", "No bundle adjustment", "first counted view", "not robust",
                  "pinhole", "lens distortion"):
        assert limit in section, limit
    for rule in ("only read", "one division", "g = 4, 2, 1", "2 counted >= m", "bit 3", "bits 0 / 1 / 2", "bit 4", "bit 5", "bit 6",
                 "No atomics", "ascending order", "one plain store", "R_k R_o"):
        assert rule in section, rule
    assert "nothing adds points to it" not in header and "ctk_fit_structure (below) adds points to it" in header
    csrc = os.path.join(ROOT, "co-tracker_amd", "csrc")
    math_h = open(os.path.join(csrc, "structure_math.h")).read()
    for name, value in (("VIEWS_MAX", 256), ("POINTS_MAX", 8192), ("MIN_VIEWS", 2), ("ROUNDS", 3), ("BIT_ROUND1", 1), ("BIT_ROUND2", 2),
                        ("BIT_ROUND3", 4), ("BIT_NO_START", 8), ("BIT_NO_PARALLAX", 16), ("BIT_INTO", 32), ("BIT_MINORITY", 64)):
        assert re.search(r"#define CTK_STRUCTURE_%s %d\b" % (name, value), math_h), name
        assert getattr(L.Structure3D, name) == value
    assert "no fixed-point sums are needed" in math_h and "ASCENDING view order" in math_h  # why plain double sums are deterministic here
    body = math_h.split("#pragma once")[1]
    assert '#include "resection_math.h"' in body
    for reused in ("ctk_motion_quant", "ctk_pose_ray", "ctk_pose_dot", "ctk_pose_cross", "ctk_pose_polar", "ctk_pose_valid",
                   "ctk_resection_apply", "ctk_resection_error", "ctk_resection_within", "ctk_resection_tol2", "ctk_resection_finite32"):
        assert reused in math_h and not re.search(r"CTK_MM_HD \w+ %s\(" % reused, body), reused  # reused, not restated
    # the rules take no library root and no trigonometry
    assert not re.search(r"(?<![\w])(sqrtf?|sinf?|cosf?|tanf?|atan2?f?|acosf?|asinf?)\s*\(", body)
    kernel = open(os.path.join(csrc, "structure.hip")).read().split("namespace {")[1]
    assert "atomic" not in kernel and "sqrt" not in kernel and "asm" not in kernel and kernel.count("__syncthreads()") == 1
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS = .*\bstructure\.hip\b", makefile, re.M) and re.search(r"^NOFMA = .*\bstructure\b", makefile, re.M)
    assert re.search(r"^HDRS = .*\bstructure_math\.h\b", makefile, re.M)
    blob = open(L.LIB_PATH, "rb").read()  # the release library carries no CTK_* string literal
    assert not re.findall(rb"CTK_STRUCTURE\w*", blob)


def test_mirror_matches_the_compiler():
    from cotracker_amd import _lib as L
    cls, struct = L.Structure3D.Args, "ctk_fit_structure_args"
    fields = [f[0] for f in cls._fields_]
    lines = [f'printf("S %zu\\n", sizeof({struct}));'] + [f'printf("F {f} %zu\\n", offsetof({struct}, {f}));' for f in fields]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "structure_layout.c"), os.path.join(d, "structure_layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "ctk.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    got_size, got = int(out[0].split()[1]), {ln.split()[1]: int(ln.split()[2]) for ln in out[1:]}
    assert got_size == C.sizeof(cls) == 200
    assert got == {f: getattr(cls, f).offset for f in fields} and len(got) == 35
    # the header declares the fields in the mirror's order and no others
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), open(os.path.join(ROOT, "include", "ctk.h")).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert declared == fields
    # the history, the camera and the tolerance of ctk_fit_resection_args; the views, the old structure and the origin instead of its source
    # forms, its seed and its pose
    res = [f[0] for f in L.Resection.Args._fields_]
    assert [f for f in res if f not in fields] == ["to", "lag", "anchor_frame", "min_points", "hypotheses", "seed", "anchor_coords", "anchor_visible",
                                                   "structure", "valid", "seed_pose"]
    assert [f for f in fields if f not in res] == ["into", "source_frame", "min_views", "refine", "min_sin2", "reserved", "pose_stats",
                                                   "structure_in", "valid_in", "origin_in", "points", "origin_out"]
    # nested: the census of module-level mirrors does not grow
    assert not isinstance(L.Structure3D, type(C.Structure)) and issubclass(L.Structure3D.Args, C.Structure)


POINTERS = ("hist_coords", "visible", "hist_vis", "hist_conf", "first_row", "pose", "pose_stats", "structure_in", "valid_in", "origin_in",
            "points", "label", "error", "stats", "origin_out")


def st_args(**kw):
    """A ctk_fit_structure_args that passes every check: 3 views out of a ring of 8 rows, the old structure carried into the last."""
    from cotracker_amd import _lib as L
    a = L.Structure3D.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.F, a.into, a.source_frame, a.min_views, a.refine = 2, 5, 4, 8, 6, 3, 2, 4, 3, 0
    a.fx, a.fy, a.cx, a.cy = 1000.0, 990.0, 960.0, 540.0
    a.sx, a.sy, a.thresh, a.tol, a.min_sin2 = 1.37, 0.81, 0.6, 2.0, 3.0e-4
    for n in POINTERS:
        setattr(a, n, 4096)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_fit_refuses_before_any_launch(lib):
    """Every refusal is an E_* code (a launch on a machine without a GPU would be a hipError_t > 0)."""
    def fit(a, ws=None, nbytes=0):
        return lib.ctk_fit_structure(None if a is None else C.byref(a), ws, nbytes, None)

    def query(a):
        n = C.c_size_t(99)
        return lib.ctk_fit_structure_workspace_bytes(None if a is None else C.byref(a), C.byref(n))
    nan, inf = float("nan"), float("inf")
    assert fit(None) == E_NULL and query(None) == E_NULL
    assert lib.ctk_fit_structure_workspace_bytes(C.byref(st_args()), None) == E_NULL
    for f in ("hist_coords", "pose", "points", "label", "error", "stats"):
        assert fit(st_args(**{f: None})) == E_NULL, f
    assert fit(st_args(visible=None, hist_vis=None)) == E_NULL and fit(st_args(visible=None, hist_conf=None)) == E_NULL
    assert fit(st_args(structure_in=None)) == E_NULL and fit(st_args(valid_in=None)) == E_NULL  # one without the other
    shape = (("G", (0, -1, 65536)), ("N", (0, -1, 3)), ("N_out", (0, -1, 6)), ("R", (0, -1, 2)), ("F", (0, -1, 9, 257, 65536)),
             ("f0", (-1, -100, 2 ** 30 - 2)), ("into", (-2, 3, 256, -100)), ("source_frame", (-1, 2 ** 30 + 1)),
             ("min_views", (0, -1, 1, 257)), ("refine", (-1, 2)), ("tol", (0.0, -0.0, -1.0, nan, inf, -inf)),
             ("min_sin2", (0.0, -0.0, -1.0, 1.0000001, 2.0, nan, inf, -inf)),
             ("sx", (0.0, -1.0, nan, inf)), ("sy", (0.0, -1.0, nan, inf)),
             ("fx", (0.0, -1.0, -0.0, nan, inf, -inf)), ("fy", (0.0, -1000.0, nan, inf, -inf)), ("cx", (nan, inf, -inf)), ("cy", (nan, inf, -inf)))
    for field, values in shape:
        for v in values:
            assert fit(st_args(**{field: v})) == E_SHAPE, (field, v)
            assert query(st_args(**{field: v})) == E_SHAPE, (field, v)
    assert fit(st_args(N=9000, N_out=8193)) == E_SHAPE and query(st_args(N=9000, N_out=8192)) == 0  # N_out > 8192
    assert fit(st_args(R=300, F=257)) == E_SHAPE and query(st_args(R=300, F=256)) == 0  # more than 256 views
    assert query(st_args(f0=2 ** 30 - 3, F=3)) == 0 and fit(st_args(f0=2 ** 30 - 2, F=3)) == E_SHAPE  # f0 + F > 2^30
    assert fit(st_args(G=8193, N=8192, N_out=1)) == E_SHAPE
    assert fit(st_args(visible=None, thresh=nan)) == E_SHAPE and query(st_args(visible=None, thresh=nan)) == E_SHAPE
    assert fit(st_args(thresh=nan, pose=None)) == E_NULL
    # every slot is one thread's: the query answers 0, and reads no pointer of the struct (none of them is mapped)
    n = C.c_size_t(99)
    assert lib.ctk_fit_structure_workspace_bytes(C.byref(st_args(N=8192, N_out=8192, R=256, F=256)), C.byref(n)) == 0 and n.value == 0
    assert fit(st_args(hist_coords=4100)) == E_ALIGN
    for f in ("hist_vis", "hist_conf", "first_row", "pose", "pose_stats", "structure_in", "origin_in", "points", "error", "stats", "origin_out"):
        assert fit(st_args(**{f: 4098})) == E_ALIGN, f
    # what the rules admit reaches the pointer check: the refusal is then the NULL one; the byte tensors need no alignment
    for kw in (dict(F=8, f0=0), dict(F=1, into=0), dict(into=-1), dict(into=0), dict(N_out=5), dict(f0=0), dict(N=8192, N_out=8192),
               dict(G=65535, N=1024, N_out=1), dict(first_row=None), dict(visible=None), dict(pose_stats=None), dict(origin_in=None),
               dict(origin_out=None), dict(structure_in=None, valid_in=None), dict(sx=1e-30, sy=1e30), dict(min_views=2),
               dict(min_views=256), dict(refine=1), dict(tol=1e-30), dict(tol=3e38), dict(min_sin2=1.0), dict(min_sin2=1e-38),
               dict(source_frame=0), dict(source_frame=2 ** 30), dict(visible=4097, valid_in=4099, label=4097),
               dict(fx=1e-30, fy=3e38), dict(cx=-3e38, cy=3e38)):
        assert fit(st_args(stats=None, **kw)) == E_NULL, kw
        assert query(st_args(stats=None, **kw)) == 0, kw


def test_python_layers_signatures_and_refusals():
    from cotracker_amd import model, ops
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    sig = inspect.signature(ops.fit_structure)
    assert list(sig.parameters) == ["tracks", "visible", "intrinsics", "pose", "pose_stats", "structure", "valid", "source_frame", "origin",
                                    "into", "tol", "min_views", "min_parallax", "refine", "first_row", "scale", "out"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[4:]] == [None, None, None, 0, None, None, 2.0, 3, 1.0, False, None, (1, 1),
                                                                            None]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[4:])
    assert all(sig.parameters[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in list(sig.parameters)[:4])
    esig = inspect.signature(CoTrackerOnlinePredictor.extend)
    assert list(esig.parameters) == ["self", "structure", "frame", "n", "first_frame", "tol", "min_views", "min_parallax", "refine", "poses",
                                     "localize_kw"]
    assert [esig.parameters[n].default for n in list(esig.parameters)[2:10]] == [None, None, None, 2.0, 3, 1.0, False, None]
    for limit in ("visible on the keyframe", "once per keyframe", "no bundle adjustment", "first counted view", "pinhole", "FIVE launches",
                  "valid is all zero"):
        assert limit in CoTrackerOnlinePredictor.extend.__doc__, limit
    for doc in (CoTrackerOnlinePredictor.reconstruct.__doc__, CoTrackerOnlinePredictor.localize.__doc__):
        assert "extend()" in doc and "is the next step" not in doc
    gsig = inspect.signature(ops.StreamGroups.structure)
    assert list(gsig.parameters)[:5] == ["self", "f0", "F", "intrinsics", "pose"]
    assert [gsig.parameters[n].default for n in ("pose_stats", "structure", "valid", "source_frame", "origin", "into", "thresh", "tol",
                                                 "min_views", "min_parallax", "refine", "group", "out")] == \
        [None, None, None, 0, None, None, 0.6, 2.0, 3, 1.0, False, None, None]
    assert list(inspect.signature(model.CoTrackerThreeOnline.stream_structure).parameters)[:5] == ["self", "f0", "F", "intrinsics", "pose"]
    # ops.Structure: four positional fields as before, the origin as an optional fifth
    s4 = ops.Structure(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int8), None, (1, 2, 3, 4))
    assert s4.origin is None and s4.intrinsics == (1.0, 2.0, 3.0, 4.0) and ops.Structure.__slots__ == ("points", "valid", "anchor", "intrinsics")
    assert not hasattr(s4, "__dict__")
    s5 = ops.Structure(s4.points, s4.valid, None, (1, 2, 3, 4), torch.eye(3, 4))
    assert torch.equal(s5.origin, torch.eye(3, 4))
    # compose_pose is elementwise torch and runs anywhere: (R R_o | R t_o + t)
    g = torch.Generator().manual_seed(0)
    pose, origin = torch.randn(5, 3, 4, generator=g, dtype=torch.float64), torch.randn(3, 4, generator=g, dtype=torch.float64)
    got = ops.compose_pose(pose, origin)
    X = torch.randn(3, generator=g, dtype=torch.float64)
    assert torch.allclose(got[..., :3] @ X + got[..., 3], pose[..., :3] @ (origin[:, :3] @ X + origin[:, 3]) + pose[..., 3], atol=1e-12)
    assert ops.compose_pose(pose, None) is pose and tuple(got.shape) == (5, 3, 4)
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=8)
    assert p.world_pose(s4, pose) is pose and torch.equal(p.world_pose(s5, pose.float()), ops.compose_pose(pose.float(), s5.origin))
    with pytest.raises(ValueError, match="ops.Structure"):
        p.world_pose(None, pose)
    # min_parallax in degrees becomes the float32 of sin^2 on the host
    assert ops.min_sin2_of(90.0) == 1.0 and abs(ops.min_sin2_of(1.0) - 3.0458649e-4) < 1e-10
    for bad in (0.0, -1.0, 91.0, float("nan"), 1e-30):
        with pytest.raises(ValueError):
            ops.min_sin2_of(bad)
    # host tensors are refused: no fall-back
    cam = (100.0, 100.0, 24.0, 16.0)
    with pytest.raises(ValueError, match="device tensor"):
        ops.fit_structure(torch.zeros(2, 9, 2), torch.zeros(2, 9, dtype=torch.bool), cam, torch.zeros(2, 3, 4))
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.extend(None)
    p(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, queries=torch.zeros(1, 3, 3))
    with pytest.raises(RuntimeError, match="no stream is running"):  # after the first step: no window has been tracked
        p.extend(s4)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.model.stream_structure(0, 1, cam, None)
    p2 = CoTrackerOnlinePredictor(checkpoint=None, v2=True, window_len=8)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.extend(s4)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.model.stream_structure(0, 1, cam, None)
