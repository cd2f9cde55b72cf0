"""Fit planes / warp planes, the part that needs no GPU: ctk_fit_planes, its workspace query and ctk_warp_planes are declared, bound and
exported without an ABI bump, the two new structs' ctypes mirrors have the compiler's layout, every refusal comes back before any
launch, and the Python layers have the signatures and defaults the callers rely on."""
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
NAMES = ("ctk_fit_planes", "ctk_fit_planes_workspace_bytes", "ctk_warp_planes")


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
    assert C.sizeof(L.Motion.Args) == 128 and C.sizeof(L.Field.Args) == 152 and C.sizeof(L.Objects.Args) == 176
    assert C.sizeof(L.Field.WarpArgs) == 104 and C.sizeof(L.Warp.Args) == 88
    section = header.split("fit planes / warp planes: planar surfaces")[1].split("Op A")[0]
    assert not re.search(r"#define CTK_\w+\s+-?\d+", section)  # no new error code; the constants live with the rules
    assert (L.Planes.PLANES_MAX, L.Planes.NONE, L.Planes.BORDER_KEEP) == (16, 127, 2)
    assert "CTK_WARP_KEEP = 2" in section and "CTK_PLANES_MAX" in section and "Known limits" in section
    math_h = open(os.path.join(ROOT, "co-tracker_amd", "csrc", "plane_math.h")).read()
    assert re.search(r"#define CTK_PLANES_MAX 16\b", math_h) and re.search(r"#define CTK_WARP_KEEP 2\b", math_h)
    makefile = open(os.path.join(ROOT, "co-tracker_amd", "csrc", "Makefile")).read()
    for unit in ("planes", "warp_planes"):
        assert re.search(r"^SRCS = .*\b%s\.hip\b" % unit, makefile, re.M) and re.search(r"^NOFMA = .*\b%s\b" % unit, makefile, re.M)
    assert re.search(r"^HDRS = .*\bplane_math\.h\b", makefile, re.M)
    blob = open(L.LIB_PATH, "rb").read()  # the release library carries no CTK_* string literal
    assert not re.findall(rb"CTK_PLANE\w*", blob) and not re.findall(rb"CTK_WARP\w*", blob)


def layout_of(struct, fields):
    """sizeof and every offsetof of a struct of include/ctk.h, from a C program compiled against it -> (size, {field: offset})."""
    lines = [f'printf("S %zu\\n", sizeof({struct}));'] + [f'printf("F {f} %zu\\n", offsetof({struct}, {f}));' for f in fields]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "planes_layout.c"), os.path.join(d, "planes_layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "ctk.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    return int(out[0].split()[1]), {ln.split()[1]: int(ln.split()[2]) for ln in out[1:]}


@pytest.mark.parametrize("struct,mirror,size,count", (("ctk_fit_planes_args", "Args", 176, 32), ("ctk_warp_planes_args", "WarpArgs", 96, 17)))
def test_mirrors_match_the_compiler(struct, mirror, size, count):
    from cotracker_amd import _lib as L
    cls = getattr(L.Planes, mirror)
    fields = [f[0] for f in cls._fields_]
    got_size, got = layout_of(struct, fields)
    assert got_size == C.sizeof(cls) == size
    assert got == {f: getattr(cls, f).offset for f in fields} and len(got) == count
    # the header declares the fields in the mirror's order and no others
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), open(os.path.join(ROOT, "include", "ctk.h")).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert declared == fields


POINTERS = ("hist_coords", "visible", "hist_vis", "hist_conf", "first_row", "labels", "homography", "label", "stats", "box")


def planes_args(**kw):
    """A ctk_fit_planes_args that passes every check: 3 frames out of a ring of 8 rows, the lag form, four labelled planes."""
    from cotracker_amd import _lib as L
    a = L.Planes.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.F, a.to, a.lag, a.anchor_frame = 2, 5, 4, 8, 6, 3, -1, 2, 0
    a.L, a.min_points, a.inverse, a.K, a.seed = 4, 8, 0, 128, 7
    a.tol, a.min_base, a.sx, a.sy, a.thresh, a.reserved = 2.0, 16.0, 1.37, 0.81, 0.6, 0
    for n in POINTERS:
        setattr(a, n, 4096)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


ANCHOR = dict(lag=0, anchor_coords=4096, anchor_visible=4096, anchor_frame=3)


def test_fit_refuses_before_any_launch(lib):
    """Every refusal is an E_* code (a launch on a machine without a GPU would be a hipError_t > 0)."""
    def fit(a, ws=None, nbytes=0):
        return lib.ctk_fit_planes(None if a is None else C.byref(a), ws, nbytes, None)

    def query(a):
        n = C.c_size_t(99)
        return lib.ctk_fit_planes_workspace_bytes(None if a is None else C.byref(a), C.byref(n))
    nan, inf = float("nan"), float("inf")
    assert fit(None) == E_NULL and query(None) == E_NULL
    assert lib.ctk_fit_planes_workspace_bytes(C.byref(planes_args()), None) == E_NULL
    for f in ("hist_coords", "homography", "label", "stats", "box"):
        assert fit(planes_args(**{f: None})) == E_NULL, f
    assert fit(planes_args(visible=None, hist_vis=None)) == E_NULL and fit(planes_args(visible=None, hist_conf=None)) == E_NULL
    assert fit(planes_args(**{**ANCHOR, "anchor_visible": None})) == E_NULL and fit(planes_args(**{**ANCHOR, "anchor_coords": None})) == E_NULL
    # ctk_fit_objects' refusals for the shared fields (there is no model), and the two new ones
    shape = (("G", (0, -1, 65536)), ("N", (0, -1, 3)), ("N_out", (0, -1, 6)), ("R", (0, -1, 4)), ("F", (0, -1, 7, 65536)),
             ("f0", (-1, -100, 2 ** 30 - 2)), ("lag", (0, -1, -2, 6, 1000)), ("K", (0, -1, 4097)),
             ("tol", (nan, 0.0, -1.0, 1 / 32, 256.04, inf, 1e30)), ("min_base", (nan, -0.001, 8192.5, inf)),
             ("sx", (0.0, -1.0, nan, inf)), ("sy", (0.0, -1.0, nan, inf)), ("reserved", (1, -1)),
             ("L", (0, -1, 17, 1000)), ("min_points", (0, -1, 8193)), ("inverse", (-1, 2, 7)))
    for field, values in shape:
        for v in values:
            assert fit(planes_args(**{field: v})) == E_SHAPE, (field, v)
            assert query(planes_args(**{field: v})) == E_SHAPE, (field, v)
    for L_ in (2, 4, 16):  # without labels there is one list
        assert fit(planes_args(labels=None, L=L_)) == E_SHAPE and query(planes_args(labels=None, L=L_)) == E_SHAPE
    assert query(planes_args(labels=None, L=1)) == 0
    assert fit(planes_args(N=9000, N_out=8193)) == E_SHAPE and query(planes_args(N=9000, N_out=8192)) == 0    # N_out > 8192
    assert fit(planes_args(F=7, lag=2, R=8)) == E_SHAPE and query(planes_args(F=6, lag=2, R=8, f0=4)) == 0    # F + lag > R
    assert query(planes_args(f0=2 ** 30 - 3, F=3)) == 0 and fit(planes_args(f0=2 ** 30 - 2, F=3)) == E_SHAPE  # f0 + F > 2^30
    assert fit(planes_args(G=8193, N=8192, N_out=1)) == E_SHAPE and fit(planes_args(G=65535, N=65535, N_out=1)) == E_SHAPE  # G * N > 2^26
    assert fit(planes_args(visible=None, thresh=nan)) == E_SHAPE and query(planes_args(visible=None, thresh=nan)) == E_SHAPE
    assert fit(planes_args(thresh=nan, homography=None)) == E_NULL
    # the source form: exactly one of the three, and rows of a ring that would alias
    for kw in (dict(lag=0), dict(to=3), dict(to=-2, lag=0), dict(to=2 ** 30 + 1, lag=0), dict(lag=2 ** 30 + 1), dict(ANCHOR, lag=2),
               dict(ANCHOR, to=3), dict(ANCHOR, anchor_frame=-1), dict(ANCHOR, anchor_frame=2 ** 30 + 1), dict(ANCHOR, F=9, f0=0),
               dict(to=0, lag=0, f0=6, F=3), dict(to=14, lag=0, f0=6, F=3)):
        assert fit(planes_args(**kw)) == E_SHAPE, kw
        assert query(planes_args(**kw)) == E_SHAPE, kw
    for kw in (dict(to=1, lag=0, f0=6, F=3), dict(to=13, lag=0, f0=6, F=3), dict(to=7, lag=0), dict(ANCHOR), dict(ANCHOR, F=8, f0=0),
               dict(ANCHOR, anchor_frame=2 ** 30)):
        assert query(planes_args(**kw)) == 0, kw
    n = C.c_size_t(99)  # the one-launch form keeps everything in LDS: the query answers 0
    assert lib.ctk_fit_planes_workspace_bytes(C.byref(planes_args()), C.byref(n)) == 0 and n.value == 0
    assert fit(planes_args(hist_coords=4100)) == E_ALIGN and fit(planes_args(**{**ANCHOR, "anchor_coords": 4100})) == E_ALIGN
    for f in ("homography", "stats", "box"):
        assert fit(planes_args(**{f: 4098})) == E_ALIGN, f
    # what the rules admit reaches the pointer check: the refusal is then the NULL one; labels and label need no alignment
    for kw in (dict(lag=1, F=7), dict(lag=5, F=3), dict(inverse=1), dict(K=1), dict(K=4096), dict(tol=1 / 16), dict(tol=256.0), dict(min_base=0.0),
               dict(min_base=8192.0), dict(N_out=5), dict(f0=0), dict(f0=1, lag=5), dict(N=8192, N_out=8192), dict(G=65535, N=1024, N_out=1),
               dict(first_row=None), dict(visible=None), dict(seed=2 ** 32 - 1), dict(sx=1e-30, sy=1e30), dict(L=1), dict(L=16),
               dict(min_points=1), dict(min_points=8192), dict(labels=None, L=1), dict(labels=4097, label=4099), dict(ANCHOR)):
        assert fit(planes_args(stats=None, **kw)) == E_NULL, kw
        assert query(planes_args(stats=None, **kw)) == 0, kw  # the query looks at no pointer of the struct but the anchor's and labels


def warp_args(**kw):
    """A ctk_warp_planes_args that passes every check but the launch: 2 pictures of 6 x 10 from sources of 5 x 7, HWC, padded rows."""
    from cotracker_amd import _lib as L
    a = L.Planes.WarpArgs()
    a.F, a.H, a.W, a.Hs, a.Ws, a.C, a.layout, a.border, a.reserved = 2, 6, 10, 5, 7, 3, 0, 0, 0
    a.src_frame_stride, a.src_row_stride, a.dst_frame_stride, a.dst_row_stride = 5 * 24, 24, 6 * 32, 32
    a.matrices, a.src, a.dst = 4096, 8192, 65536
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_warp_refuses_before_any_launch(lib):
    def warp(a):
        return lib.ctk_warp_planes(None if a is None else C.byref(a), None)
    assert warp(None) == E_NULL
    for f in ("matrices", "src", "dst"):
        assert warp(warp_args(**{f: None})) == E_NULL, f
    side = 32768
    shape = (("F", (0, -1, 65536)), ("H", (0, -1, side + 1)), ("W", (0, -1, side + 1)), ("Hs", (0, -1, side + 1)), ("Ws", (0, -1, side + 1)),
             ("C", (0, 2, 4)), ("layout", (-1, 2)), ("border", (-1, 3)), ("reserved", (1, -1)),
             ("src_row_stride", (20, 0, -24, 2 ** 40 + 1)), ("dst_row_stride", (29, 0, 2 ** 40 + 1)),
             ("src_frame_stride", (5 * 24 - 1, -1, 2 ** 40 + 1)), ("dst_frame_stride", (6 * 32 - 1, 0, 2 ** 40 + 1)))
    for field, values in shape:
        for v in values:
            assert warp(warp_args(**{field: v})) == E_SHAPE, (field, v)
    assert warp(warp_args(matrices=4098)) == E_ALIGN
    # overlapping byte ranges: the picture never overlaps the frames it is drawn into
    assert warp(warp_args(src=65536 + 100)) == E_SHAPE and warp(warp_args(src=65536 - 200)) == E_SHAPE
    assert warp(warp_args(src=65536 + 2 * 6 * 32, matrices=None)) == E_NULL  # right behind the destination: no overlap
    # planar: a frame holds C H rows
    assert warp(warp_args(layout=1, src_row_stride=8, dst_row_stride=12, src_frame_stride=3 * 5 * 8 - 1, dst_frame_stride=3 * 6 * 12)) == E_SHAPE
    assert warp(warp_args(layout=1, src_row_stride=8, dst_row_stride=12, src_frame_stride=3 * 5 * 8, dst_frame_stride=3 * 6 * 12 - 1)) == E_SHAPE
    # what the rules admit reaches the pointer check
    for kw in (dict(border=1), dict(border=2), dict(src_frame_stride=0), dict(C=1, src_row_stride=7, dst_row_stride=10, src_frame_stride=35,
                                                                             dst_frame_stride=60),
               dict(layout=1, src_row_stride=8, dst_row_stride=12, src_frame_stride=3 * 5 * 8, dst_frame_stride=3 * 6 * 12),
               dict(H=side, W=1, dst_row_stride=3, dst_frame_stride=3 * side, dst=1 << 30), dict(F=65535, src_frame_stride=0, dst=1 << 30)):
        assert warp(warp_args(matrices=None, **kw)) == E_NULL, kw


def test_python_layers_signatures_and_refusals():
    from cotracker_amd import model, ops
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    sig = inspect.signature(ops.fit_planes)
    assert list(sig.parameters) == ["tracks", "visible", "labels", "planes", "lag", "to", "anchor", "inverse", "tol", "hypotheses", "min_base",
                                    "min_points", "seed", "scale", "frames", "first_row"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[2:]] == [None, 1, 1, None, None, False, 2.0, 128, 16.0, 8, 0, (1, 1), None,
                                                                             None]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[2:])
    wsig = inspect.signature(ops.warp_planes)
    assert list(wsig.parameters) == ["src", "matrices", "size", "out", "border", "fill", "layout"]
    assert [wsig.parameters[n].default for n in list(wsig.parameters)[2:]] == [None, None, "fill", (0, 0, 0), None]
    assert all(wsig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(wsig.parameters)[2:])
    assert list(inspect.signature(ops.quad_matrix).parameters) == ["corners", "size"]
    csig = inspect.signature(ops.quad_constant)  # the device constant, kept per quad: what overlay() and rectify() multiply with
    assert list(csig.parameters) == ["corners", "size", "device", "inverse"] and csig.parameters["inverse"].kind is inspect.Parameter.KEYWORD_ONLY
    fsig = inspect.signature(CoTrackerOnlinePredictor.follow_planes)
    assert list(fsig.parameters) == ["self", "objects", "n", "first_frame", "inverse", "tol", "hypotheses", "min_base", "min_points", "seed"]
    assert [fsig.parameters[n].default for n in list(fsig.parameters)[2:]] == [None, None, False, 2.0, 128, 16.0, 8, 0]
    osig = inspect.signature(CoTrackerOnlinePredictor.overlay)
    assert list(osig.parameters) == ["self", "frames", "picture", "corners", "objects", "index", "first_frame"]
    assert [osig.parameters[n].default for n in ("index", "first_frame")] == [0, None]
    rsig = inspect.signature(CoTrackerOnlinePredictor.rectify)
    assert list(rsig.parameters) == ["self", "frames", "corners", "objects", "index", "size", "first_frame", "border", "fill", "out"]
    assert [rsig.parameters[n].default for n in ("index", "first_frame", "border", "fill", "out")] == [0, None, "fill", (0, 0, 0), None]
    assert hasattr(ops.StreamGroups, "planes") and hasattr(model.CoTrackerThreeOnline, "stream_planes")
    assert callable(ops.overlay) and callable(ops.rectify) and ops.PLANE_BORDERS == {"fill": 0, "edge": 1, "keep": 2}
    # quad_matrix: host float64, the picture's corner pixels land on the corners
    corners = [[10.0, 20.0], [110.0, 25.0], [100.0, 90.0], [5.0, 80.0]]
    q = ops.quad_matrix(corners, (30, 40))
    assert q.dtype == torch.float64 and tuple(q.shape) == (3, 3) and not q.is_cuda and float(q[2, 2]) == 1.0
    pic = torch.tensor([[0.0, 0.0, 1.0], [39.0, 0.0, 1.0], [39.0, 29.0, 1.0], [0.0, 29.0, 1.0]], dtype=torch.float64)
    img = pic @ q.T
    assert torch.allclose(img[:, :2] / img[:, 2:], torch.tensor(corners, dtype=torch.float64), atol=1e-9)
    for bad in ([[0, 0], [1, 1], [2, 2], [5, 0]], [[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 0], [1, 1], [float("nan"), 1]]):
        with pytest.raises(ValueError):
            ops.quad_matrix(bad, (30, 40))
    # host tensors are refused: no fall-back
    with pytest.raises(ValueError, match="device tensor"):
        ops.fit_planes(torch.zeros(2, 5, 2), torch.zeros(2, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match="device tensor"):
        ops.warp_planes(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.eye(3)[None])
    with pytest.raises(ValueError, match="device tensor"):
        ops.overlay(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(2, 2, 3, dtype=torch.uint8), corners, torch.zeros(2, 5, 2),
                    torch.zeros(2, 5, dtype=torch.bool), src_frame=0)
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=8)
    calls = (lambda x: x.follow_planes(None), lambda x: x.overlay(None, None, None, None), lambda x: x.rectify(None, None, None))
    for call in calls:
        with pytest.raises(RuntimeError, match="no stream is running"):
            call(p)
    p(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, queries=torch.zeros(1, 3, 3))
    for call in calls:
        with pytest.raises(RuntimeError, match="no stream is running"):  # after the first step: no window has been tracked
            call(p)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.model.stream_planes(0, 1)
    p2 = CoTrackerOnlinePredictor(checkpoint=None, v2=True, window_len=8)
    for call in calls:
        with pytest.raises(NotImplementedError, match="v2"):
            call(p2)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.model.stream_planes(0, 1)
