"""Lens, the part that needs no GPU: ctk_lens_frames and ctk_lens_points are declared, bound and exported without an ABI bump, the new
structs' ctypes mirrors have the compiler's layout, every refusal comes back before any launch, and the Python layers have the
signatures, defaults and refusals the callers rely on."""
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
NAMES = ("ctk_lens_frames", "ctk_lens_points")
ACTION = ((1000.0, 1000.0, 959.5, 539.5), (-0.28, 0.09, 1e-3, -8e-4, -0.013))


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
    lay = header_layout()
    assert int(lay["sizeof"]["ctk_stream_args"]) == C.sizeof(L.StreamArgs) == 200  # no existing struct grew
    assert C.sizeof(L.Warp.Args) == 88 and C.sizeof(L.Planes.WarpArgs) == 96 and C.sizeof(L.Motion.Args) == 128
    assert C.sizeof(L.Epipolar.Args) == 168 and C.sizeof(L.Pose.Args) == 176 and C.sizeof(L.Resection.Args) == 192
    # the mirrored constants, as the one layout program reads them from the header
    assert lay["constants"]["CTK_LENS_TO_IDEAL"] == L.LENS_TO_IDEAL == 0 and lay["constants"]["CTK_LENS_TO_SENSOR"] == L.LENS_TO_SENSOR == 1
    assert lay["constants"]["CTK_LENS_ROUNDS"] == L.LENS_ROUNDS == 8
    # the section stands with the resamplers, in front of the fits whose sections admit no #define
    assert header.index("---- warp frames") < header.index("---- lens:") < header.index("---- track field") < header.index("---- Op A")
    section = header.split("---- lens:")[1].split("---- track field")[0]
    assert not re.search(r"#define CTK_E_\w+\s+-?\d+", section)  # no new error code
    for rule in ("Brown-Conrady", "(k1, k2, p1, p2, k3)", "CTK_LENS_ROUNDS = 8", "always all of them", "idet = 1 / det", "0x7FC00000", "label -1",
                 "llrint", "X >> 8", "X & 255", "bit for bit", "far less than 1/512", "[1, 1e6]", "<= 32768", "<= 64", "never counts as the identity",
                 "fill[c] under either border", "must not overlap", "dst == src with equal strides", "capture-safe", "no atomics", "Known limits",
                 "CTK_E_NULL", "CTK_E_SHAPE", "CTK_E_ALIGN"):
        assert rule in section, rule
    # the fits say where a lens is corrected, and still say everything they said
    for title in ("fit epipolar: one fundamental", "fit pose: how the camera turned", "fit resection: the camera's pose", "fit structure: points added"):
        fit = header.split(title)[1].split("typedef struct")[0]
        assert "ctk_lens_frames / ctk_lens_points correct a lens in front of" in fit and "lens distortion" in fit and "Known limits" in fit, title
    csrc = os.path.join(ROOT, "co-tracker_amd", "csrc")
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS = .*\blens\.hip\b", makefile, re.M) and re.search(r"^NOFMA = .*\blens\b", makefile, re.M)
    assert re.search(r"^HDRS = .*\blens_math\.h\b", makefile, re.M)
    math_h = open(os.path.join(csrc, "lens_math.h")).read()
    assert '#include "warp_math.h"' in math_h and "ctk_warp_blend(int" not in math_h and "ctk_warp_clamp(int" not in math_h  # reused, not restated
    kernel = open(os.path.join(csrc, "lens.hip")).read()
    assert '#include "lens_math.h"' in kernel and "ctk_warp_blend(" in kernel and "ctk_warp_clamp(" in kernel  # reused, not restated
    assert "atomic" not in kernel.split("namespace {")[1] and "__shared__" not in kernel and "hipStreamSynchronize" not in kernel
    blob = open(L.LIB_PATH, "rb").read()
    assert not re.findall(rb"CTK_LENS\w*", blob)
    assert "CTK_OPT_COUNT = 7" in header and L.OPT_COUNT == 7  # two kernels, not an option


CAMERA_FIELDS = ["sensor", "ideal", "k", "reserved"]
FRAMES_FIELDS = ["F", "H", "W", "Ho", "Wo", "layout", "border", "direction", "tol", "reserved", "fill", "src_frame_stride", "src_row_stride",
                 "dst_frame_stride", "dst_row_stride", "lens", "src", "dst"]
POINTS_FIELDS = ["G", "F", "N", "direction", "tol", "reserved", "src_group_stride", "src_frame_stride", "dst_group_stride", "dst_frame_stride",
                 "lens", "src", "dst", "label"]


@pytest.mark.parametrize("cname,holder,size,order", [("ctk_lens", "Camera", 112, CAMERA_FIELDS), ("ctk_lens_frames_args", "FramesArgs", 208, FRAMES_FIELDS),
                                                     ("ctk_lens_points_args", "PointsArgs", 192, POINTS_FIELDS)])
def test_args_mirrors_match_the_compiler(cname, holder, size, order):
    """sizeof and every offsetof of the three new structs, from a C program compiled against include/ctk.h."""
    from cotracker_amd import _lib as L
    cls = getattr(L.Lens, holder)
    fields = [f[0] for f in cls._fields_]
    assert fields == order
    lines = [f'printf("S %zu\\n", sizeof({cname}));']
    lines += [f'printf("F {f} %zu\\n", offsetof({cname}, {f}));' for f in fields]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "lens_layout.c"), os.path.join(d, "lens_layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "ctk.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert int(out[0].split()[1]) == C.sizeof(cls) == size
    got = {ln.split()[1]: int(ln.split()[2]) for ln in out[1:]}
    assert got == {f: getattr(cls, f).offset for f in fields} and len(got) == len(order)
    # the header declares the fields in the mirror's order and no others
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), open(os.path.join(ROOT, "include", "ctk.h")).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert declared == fields


BASE = 1 << 20


def set_lens(cam, intrinsics=ACTION[0], k=ACTION[1], ideal=None):
    for i in range(4):
        cam.sensor[i], cam.ideal[i] = intrinsics[i], (intrinsics if ideal is None else ideal)[i]
    for i in range(5):
        cam.k[i] = k[i]
    cam.reserved = 0.0


def frames_args(**kw):
    """A ctk_lens_frames_args that passes every check: 3 HWC pictures of 20 x 30 with padded rows into pictures of 24 x 34, dst well
    behind src."""
    from cotracker_amd import _lib as L
    a = L.Lens.FramesArgs()
    a.F, a.H, a.W, a.Ho, a.Wo, a.layout, a.border, a.direction, a.tol, a.reserved = 3, 20, 30, 24, 34, 0, 0, 0, 0.01, 0
    a.src_frame_stride, a.src_row_stride, a.dst_frame_stride, a.dst_row_stride = 2000, 96, 2600, 104
    a.src, a.dst = BASE, 2 * BASE
    set_lens(a.lens)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def points_args(**kw):
    from cotracker_amd import _lib as L
    a = L.Lens.PointsArgs()
    a.G, a.F, a.N, a.direction, a.tol, a.reserved = 2, 3, 10, 0, 0.01, 0
    a.src_group_stride, a.src_frame_stride, a.dst_group_stride, a.dst_frame_stride = 80, 24, 60, 20
    a.src, a.dst, a.label = BASE, 2 * BASE, 3 * BASE
    set_lens(a.lens)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def bad_lenses():
    """(what is wrong, a function that spoils the camera of an args struct)."""
    nan, inf = float("nan"), float("inf")
    out = []
    for field, idx, values in (("sensor", 0, (0.999, 1e6 + 1, nan, inf, -1000.0)), ("sensor", 1, (0.0, nan)), ("ideal", 0, (0.5, inf)),
                               ("ideal", 1, (2e6, nan)), ("sensor", 2, (32768.5, nan, -inf)), ("sensor", 3, (-32769.0,)),
                               ("ideal", 2, (40000.0,)), ("ideal", 3, (nan,)), ("k", 0, (64.001, nan)), ("k", 1, (-65.0,)), ("k", 2, (inf,)),
                               ("k", 3, (-inf,)), ("k", 4, (100.0, nan))):
        for v in values:
            out.append(((field, idx, v), lambda cam, field=field, idx=idx, v=v: getattr(cam, field).__setitem__(idx, v)))
    for v in (1.0, -1.0, nan, 5e-324):
        out.append((("reserved", v), lambda cam, v=v: setattr(cam, "reserved", v)))
    return out


def test_lens_frames_refuses_before_any_launch(lib):
    """Every refusal is an E_* code (a launch on a machine without a GPU would be a hipError_t > 0)."""
    def run(a):
        return lib.ctk_lens_frames(None if a is None else C.byref(a), None)
    nan, inf = float("nan"), float("inf")
    assert run(None) == E_NULL
    for f in ("src", "dst"):
        assert run(frames_args(**{f: None})) == E_NULL, f
    shape = (("F", (0, -1, 65536)), ("H", (0, -1, 32769)), ("W", (0, -1, 32769)), ("Ho", (0, -1, 32769)), ("Wo", (0, -1, 32769)),
             ("layout", (-1, 2)), ("border", (-1, 2, 7)), ("direction", (-1, 2)), ("reserved", (1, -1)), ("tol", (0.0, -0.01, nan, inf, -inf)),
             ("src_row_stride", (89, 0, -96, 2 ** 40 + 1)), ("dst_row_stride", (101, 0, -104, 2 ** 40 + 1)),
             ("src_frame_stride", (1919, 0, -1, 2 ** 40 + 1)), ("dst_frame_stride", (2495, 0, -1, 2 ** 40 + 1)))
    for field, values in shape:
        for v in values:
            assert run(frames_args(**{field: v})) == E_SHAPE, (field, v)
    for what, spoil in bad_lenses():
        a = frames_args()
        spoil(a.lens)
        assert run(a) == E_SHAPE, what  # refused, never taken for the identity
    # planar: a row is W elements, a frame 3 H rows
    assert run(frames_args(layout=1, src_row_stride=29)) == E_SHAPE and run(frames_args(layout=1, src_row_stride=32, src_frame_stride=1919)) == E_SHAPE
    assert run(frames_args(layout=1, dst_row_stride=33)) == E_SHAPE and run(frames_args(layout=1, dst_row_stride=36, dst_frame_stride=2591)) == E_SHAPE
    # overlapping byte ranges: src covers 2 * 2000 + 19 * 96 + 90 = 5914 bytes, dst 2 * 2600 + 23 * 104 + 102 = 7694
    for dst in (BASE, BASE + 1, BASE + 5913, BASE - 7693, BASE - 1):
        assert run(frames_args(dst=dst)) == E_SHAPE, dst
    # a NULL pointer is named before a shape
    assert run(frames_args(F=0, src=None)) == E_NULL
    # (every refusal of this entry point is CTK_E_SHAPE and a struct that passes would launch: what the rules ADMIT -- F = 65535, 1 x 1
    # pictures, byte-aligned and back-to-back buffers -- is shown by tests/test_gpu_lens.py, on memory that exists)


def test_lens_points_refuses_before_any_launch(lib):
    def run(a):
        return lib.ctk_lens_points(None if a is None else C.byref(a), None)
    nan, inf = float("nan"), float("inf")
    assert run(None) == E_NULL
    for f in ("src", "dst"):
        assert run(points_args(**{f: None})) == E_NULL, f
    shape = (("G", (0, -1, 65536)), ("F", (0, -1, 65536)), ("N", (0, -1, 2 ** 20 + 1)), ("direction", (-1, 2)), ("reserved", (1, -1)),
             ("tol", (0.0, -1.0, nan, inf)), ("src_frame_stride", (19, 0, -24, 2 ** 40 + 2)), ("dst_frame_stride", (18, 0, 2 ** 40 + 2)),
             ("src_group_stride", (71, 70, 0, -80, 2 ** 40 + 2)), ("dst_group_stride", (58, 0, 2 ** 40 + 2)))
    for field, values in shape:
        for v in values:
            assert run(points_args(**{field: v})) == E_SHAPE, (field, v)
    for what, spoil in bad_lenses():
        a = points_args()
        spoil(a.lens)
        assert run(a) == E_SHAPE, what
    # overlap: src covers 4 * (80 + 2 * 24 + 20) = 592 bytes, dst 4 * (60 + 2 * 20 + 20) = 480, label 60
    for dst in (BASE, BASE + 8, BASE + 584, BASE - 472):  # dst == src with OTHER strides is an overlap like any other
        assert run(points_args(dst=dst)) == E_SHAPE, dst
    for label in (BASE, BASE + 591, BASE - 59, 2 * BASE + 479, 2 * BASE - 1):
        assert run(points_args(label=label)) == E_SHAPE, label
    # alignment: positions are 8-byte loads and stores; the shape is named first
    for kw in (dict(src=BASE + 4), dict(dst=2 * BASE + 4), dict(src=BASE + 1), dict(src_frame_stride=25), dict(dst_frame_stride=21, dst_group_stride=64),
               dict(src_group_stride=81), dict(dst_group_stride=61)):
        assert run(points_args(**kw)) == E_ALIGN, kw
    assert run(points_args(G=0, src=BASE + 4)) == E_SHAPE and run(points_args(G=0, src=None)) == E_NULL
    # what the rules admit reaches the alignment check: in place with equal strides, back to back, no label, either direction
    # (`odd`: the side whose strides are then made odd -- the last check of all --, the one whose growing end meets nothing)
    for kw in (dict(dst=BASE, dst_group_stride=80, dst_frame_stride=24, odd="both"), dict(dst=BASE + 592), dict(dst=BASE - 480, odd="src"),
               dict(label=None), dict(direction=1), dict(G=65535, F=1, src_group_stride=24, dst_group_stride=20, dst=1 << 40, label=None),
               dict(G=1, F=1, N=2 ** 20, src_frame_stride=2 ** 21, src_group_stride=2 ** 21, dst_frame_stride=2 ** 21, dst_group_stride=2 ** 21,
                    dst=1 << 40, label=None), dict(label=BASE + 592), dict(label=BASE - 60)):
        odd = kw.pop("odd", "dst")
        a = points_args(**kw)
        for side in ("src", "dst"):
            if odd in (side, "both"):  # (the group stride stays >= F frame strides)
                setattr(a, side + "_frame_stride", getattr(a, side + "_frame_stride") + 1)
                setattr(a, side + "_group_stride", getattr(a, side + "_group_stride") + 4)
        assert run(a) == E_ALIGN, kw


def test_python_layers_signatures_and_refusals():
    from cotracker_amd import ops
    from cotracker_amd.predictor import CoTrackerOnlinePredictor

    def check(fn, names, positional, defaults):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == names
        assert [sig.parameters[n].default for n in names[positional:]] == defaults
        return sig
    check(ops.Lens.__init__, ["self", "intrinsics", "coefficients", "ideal"], 3, [None])
    sig = check(ops.lens_frames, ["frames", "lens", "to", "size", "out", "border", "fill", "tol", "layout"], 2,
                ["ideal", None, None, "fill", (0, 0, 0), 0.01, None])
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[2:])
    sig = check(ops.lens_points, ["tracks", "lens", "to", "out", "labels", "tol"], 2, ["ideal", None, False, 0.01])
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[2:])
    check(CoTrackerOnlinePredictor.undistort, ["self", "frames", "out", "border", "fill"], 2, [None, "fill", (0, 0, 0)])
    check(CoTrackerOnlinePredictor.to_sensor, ["self", "tracks", "labels"], 2, [False])
    assert isinstance(CoTrackerOnlinePredictor.lens, property) and "forward() does not read `lens`" in CoTrackerOnlinePredictor.lens.__doc__
    for word in ("fit_epipolar", "fit_pose", "fit_resection", "fit_structure", "lens.ideal"):
        assert word in ops.lens_points.__doc__, word
    # no keyword was added to a reader: the lens reaches the predictor through the property and the two methods only
    for name in ("epipolar", "split_scene", "pose", "reconstruct", "localize", "extend", "push_frames", "forward", "draw", "overlay"):
        assert "lens" not in inspect.signature(getattr(CoTrackerOnlinePredictor, name)).parameters, name
        if name in ("epipolar", "pose", "reconstruct", "localize", "extend"):
            assert "ctk_lens_frames" in getattr(CoTrackerOnlinePredictor, name).__doc__ and "pinhole" in getattr(CoTrackerOnlinePredictor, name).__doc__
    # Lens: tuples of floats, validated, never the identity by default
    lens = ops.Lens(*ACTION)
    assert lens.intrinsics == ACTION[0] and lens.coefficients == ACTION[1] and lens.ideal == ACTION[0]
    assert all(isinstance(v, tuple) for v in (lens.intrinsics, lens.coefficients, lens.ideal))
    assert ops.Lens(ACTION[0], ACTION[1], ideal=(900, 900, 700, 400)).ideal == (900.0, 900.0, 700.0, 400.0)
    nan = float("nan")
    for bad in (((0.5, 1000, 0, 0), ACTION[1], None), ((1000, nan, 0, 0), ACTION[1], None), ((1000, 1000, 4e4, 0), ACTION[1], None),
                (ACTION[0], (65.0, 0, 0, 0, 0), None), (ACTION[0], (0, 0, 0, 0, nan), None), (ACTION[0], ACTION[1], (2e6, 1000, 0, 0)),
                (ACTION[0], (0, 0, 0, 0), None), ((1000, 1000, 0), ACTION[1], None), (torch.ones(4), ACTION[1], None)):
        with pytest.raises(ValueError, match="Lens"):
            ops.Lens(*bad)
    # host tensors are refused: no fall-back
    with pytest.raises(ValueError, match="device tensor"):
        ops.lens_frames(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), lens)
    with pytest.raises(ValueError, match="device tensor"):
        ops.lens_points(torch.zeros(2, 5, 2), lens)


def test_predictor_lens_property_and_push_path():
    from cotracker_amd import ops
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    lens = ops.Lens((40.0, 40.0, 23.5, 15.5), ACTION[1])
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=8)
    assert p.lens is None
    with pytest.raises(RuntimeError, match="no lens"):
        p.undistort(torch.zeros(1, 32, 48, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no lens"):
        p.to_sensor(torch.zeros(1, 4, 2))
    with pytest.raises(ValueError, match="ops.Lens"):
        p.lens = (1000.0, 1000.0, 0.0, 0.0)
    # lens=None leaves push_frames on its old path: _ingest gets the caller's own frames, and nothing of the lens runs
    p(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, queries=torch.zeros(1, 3, 3))
    seen = []
    p._ingest = lambda src, dst, layout: seen.append((src, layout))
    p._undistorted = lambda *a: pytest.fail("the lens path ran without a lens")
    frames = torch.zeros(2, 32, 48, 3, dtype=torch.uint8)
    assert p.push_frames(frames) == (None, None)
    assert len(seen) == 1 and seen[0][0].data_ptr() == frames.data_ptr() and seen[0][1] == "hwc" and p._lens_buf is None
    # with a lens: float32 frames are refused before anything is touched; uint8 frames go through the resampler, then _ingest
    p.lens = lens
    assert p.lens is lens
    with pytest.raises(ValueError, match="uint8"):
        p.push_frames(torch.zeros(2, 32, 48, 3))
    marker = torch.ones(2, 32, 48, 3, dtype=torch.uint8)
    p._undistorted = lambda f, layout: marker
    p.push_frames(frames)
    assert len(seen) == 2 and seen[1][0].data_ptr() == marker.data_ptr()
    # while a pushed stream has tracked a window and is not closed the property cannot change; before and after it can
    p._push_tracked = True
    with pytest.raises(RuntimeError, match="pushed stream is running"):
        p.lens = None
    with pytest.raises(RuntimeError, match="pushed stream is running"):
        p.lens = lens
    p._push_closed = True
    p.lens = None
    assert p.lens is None
    p._push_reset()
    p.lens = lens
    assert p.lens is lens
