"""Track field, the part that needs no GPU: ctk_track_field, its workspace query and ctk_warp_field are declared, bound and exported
without an ABI bump, the new structs' ctypes mirrors have the compiler's layout, every refusal include/ctk.h lists comes back before
any launch, the workspace query is consistent, and the Python layers have the signatures and defaults the callers rely on."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import pytest
import torch

import field_reference as R
from ctk_support import ROOT, lib  # noqa: F401

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
NAMES = ("ctk_track_field", "ctk_track_field_workspace_bytes", "ctk_warp_field")


def test_declared_bound_exported_and_abi(lib):
    from cotracker_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "ctk.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    history = header.split("#define CTK_ABI_VERSION")[0]
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header)
        assert name in L.SYMBOLS and hasattr(lib, name)
        assert any(ln.split()[-1] == name and " T " in ln for ln in nm.splitlines())
    assert any(e.startswith("v9, additive") and "ctk_track_field" in e and "ctk_warp_field" in e for e in re.split(r"\n \*   (?=v\d)", history))
    assert lib.ctk_abi_version() == L.ABI_VERSION == 9  # additive
    assert C.sizeof(L.StreamArgs) == 200 and C.sizeof(L.Draw.Args) == 216 and C.sizeof(L.Motion.Args) == 128 and C.sizeof(L.Warp.Args) == 88
    assert header.index("---- warp frames") < header.index("---- track field") < header.index("---- Op A")
    section = header.split("---- track field")[1].split("---- Op A")[0]
    assert not re.search(r"#define CTK_\w+\s+-?\d+", section)  # no new error code, no new constant: the borders are ctk_warp_frames'
    for word in ("Known limits", "zeroth order", "0.6 pixel", "3.2 pixels"):
        assert word in section
    makefile = open(os.path.join(ROOT, "co-tracker_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bfield\.hip\b", makefile, re.M) and re.search(r"^NOFMA = .*\bfield\b", makefile, re.M)
    assert re.search(r"^HDRS = .*\bfield_math\.h\b", makefile, re.M)
    blob = open(L.LIB_PATH, "rb").read()
    assert not re.findall(rb"CTK_FIELD\w*", blob)
    assert "CTK_OPT_COUNT = 7" in header and L.OPT_COUNT == 7  # kernels, not options
    assert (L.Field.POINTS_MAX, L.Field.CS_MIN, L.Field.CS_MAX, L.Field.RADIUS_MAX, L.Field.NO_LEVEL) == (8192, 2, 6, 4, R.NO_LEVEL)
    math_h = open(os.path.join(ROOT, "co-tracker_amd", "csrc", "field_math.h")).read()
    for name, value in (("POINTS_MAX", 8192), ("CS_MIN", 2), ("CS_MAX", 6), ("RADIUS_MAX", 4), ("NO_LEVEL", 255)):
        assert re.search(r"#define CTK_FIELD_%s %d\b" % (name, value), math_h)
    # the rules are reused, not restated
    assert '#include "motion_math.h"' in math_h and '#include "warp_math.h"' in math_h
    for reused in ("ctk_motion_quant(", "ctk_warp_blend", "ctk_warp_clamp"):
        assert reused in math_h and not re.search(r"CTK_FM_HD \w+ %s" % re.escape(reused.rstrip("(")), math_h)


TRACK_FIELDS = ["G", "N", "N_out", "R", "f0", "F", "H", "W", "cs", "radius", "to", "lag", "anchor_frame", "sx", "sy", "thresh", "reserved",
                "hist_coords", "visible", "hist_vis", "hist_conf", "first_row", "anchor_coords", "anchor_visible", "field", "level", "stats"]
WARP_FIELDS = ["F", "H", "W", "C", "layout", "border", "cs", "reserved", "fill", "src_frame_stride", "src_row_stride", "dst_frame_stride",
               "dst_row_stride", "field", "src", "dst", "flow"]


@pytest.mark.parametrize("cname,holder,size,order", [("ctk_track_field_args", "Args", 152, TRACK_FIELDS),
                                                     ("ctk_warp_field_args", "WarpArgs", 104, WARP_FIELDS)])
def test_args_mirrors_match_the_compiler(cname, holder, size, order):
    """sizeof and every offsetof of the two new structs, from a C program compiled against include/ctk.h."""
    from cotracker_amd import _lib as L
    cls = getattr(L.Field, holder)
    fields = [f[0] for f in cls._fields_]
    assert fields == order
    lines = [f'printf("S %zu\\n", sizeof({cname}));']
    lines += [f'printf("F {f} %zu\\n", offsetof({cname}, {f}));' for f in fields]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "field_layout.c"), os.path.join(d, "field_layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "ctk.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert int(out[0].split()[1]) == C.sizeof(cls) == size
    got = {ln.split()[1]: int(ln.split()[2]) for ln in out[1:]}
    assert got == {f: getattr(cls, f).offset for f in fields} and len(got) == len(order)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), open(os.path.join(ROOT, "include", "ctk.h")).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert declared == fields


BASE = 1 << 20


def track_args(**kw):
    """A ctk_track_field_args that passes every check: 2 groups of 40 points on a ring of 16 rows, 4 frames against the frame before."""
    from cotracker_amd import _lib as L
    a = L.Field.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.F, a.H, a.W, a.cs, a.radius = 2, 40, 30, 16, 20, 4, 45, 70, 4, 2
    a.to, a.lag, a.anchor_frame, a.sx, a.sy, a.thresh, a.reserved = -1, 1, 0, 1.0, 1.5, 0.6, 0
    a.hist_coords, a.visible, a.hist_vis, a.hist_conf, a.first_row = 4096, None, 8192, 12288, 16384
    a.anchor_coords, a.anchor_visible, a.field, a.level, a.stats = None, None, 20480, 24576, 28672
    for k, v in kw.items():
        setattr(a, k, v)
    return a


ANCHOR = dict(lag=0, anchor_coords=32768, anchor_visible=36864, anchor_frame=3)
WS = 1 << 21


def test_track_field_refuses_before_any_launch(lib):
    """Every refusal is an E_* code (a launch on a machine without a GPU would be a hipError_t > 0)."""
    def run(a, ws=BASE, nbytes=WS):
        return lib.ctk_track_field(None if a is None else C.byref(a), ws, nbytes, None)

    def query(a):
        n = C.c_size_t(0)
        return lib.ctk_track_field_workspace_bytes(C.byref(a), C.byref(n)), n.value
    nan, inf = float("nan"), float("inf")
    assert run(None) == E_NULL and lib.ctk_track_field_workspace_bytes(None, C.byref(C.c_size_t(0))) == E_NULL
    assert lib.ctk_track_field_workspace_bytes(C.byref(track_args()), None) == E_NULL
    for f in ("hist_coords", "field", "level", "stats", "hist_vis", "hist_conf"):
        assert run(track_args(**{f: None})) == E_NULL, f
    assert run(track_args(), ws=None) == E_NULL
    assert run(track_args(**dict(ANCHOR, anchor_visible=None))) == E_NULL and run(track_args(**dict(ANCHOR, anchor_coords=None))) == E_NULL
    shape = (("G", (0, -1, 65536)), ("N", (0, -1, 29)), ("N_out", (0, -1, 41)), ("R", (0, -1, 4)), ("F", (0, -1, 16, 65536)),
             ("f0", (-1, 2 ** 30 - 3)), ("H", (0, -1, 32769)), ("W", (0, -1, 32769)), ("cs", (1, 7, -1)), ("radius", (0, 5, -1)),
             ("to", (-2, 0, 5)), ("lag", (0, 13, -13, 2 ** 30 + 1)), ("sx", (0.0, -1.0, nan, inf)), ("sy", (0.0, -2.0, nan, inf)),
             ("thresh", (nan,)), ("reserved", (1, -1)))
    for field, values in shape:
        for v in values:
            assert run(track_args(**{field: v})) == E_SHAPE, (field, v)
            assert query(track_args(**{field: v}))[0] == E_SHAPE, (field, v)
    assert run(track_args(N=8193, N_out=8193, G=1)) == E_SHAPE and run(track_args(G=65535, N=2 ** 11)) == E_SHAPE  # N_out, G * N
    # the "to" forms: exactly one; rows of a ring must not alias
    assert run(track_args(**dict(ANCHOR, lag=1))) == E_SHAPE and run(track_args(**dict(ANCHOR, to=3))) == E_SHAPE
    assert run(track_args(**dict(ANCHOR, anchor_frame=-1))) == E_SHAPE and run(track_args(**dict(ANCHOR, anchor_frame=2 ** 30 + 1))) == E_SHAPE
    assert run(track_args(**dict(ANCHOR, F=17))) == E_SHAPE
    assert run(track_args(lag=0, to=7)) == E_SHAPE  # frames 7 .. 23: 17 rows of a ring of 16
    assert run(track_args(lag=0, to=36)) == E_SHAPE and run(track_args(lag=0, to=2 ** 30 + 1)) == E_SHAPE
    # a NULL pointer is named before a shape, a shape before the workspace, the workspace before the alignment
    assert run(track_args(G=0, field=None)) == E_NULL and run(track_args(G=0, hist_coords=4100)) == E_SHAPE
    rc, need = query(track_args())
    gh, gw = R.grid(45, 4), R.grid(70, 4)
    nodes = sum(h * w for h, w in ((4, 6), (2, 3), (1, 2), (1, 1)))
    assert (gh, gw) == (4, 6) and rc == 0 and need == 2 * 4 * nodes * 24
    assert run(track_args(hist_coords=4100), nbytes=need - 1) == E_SHAPE and run(track_args(hist_coords=4100), nbytes=need) == E_ALIGN
    for kw in (dict(hist_coords=4100), dict(field=20484), dict(stats=28674), dict(ANCHOR, anchor_coords=32772)):
        assert run(track_args(**kw)) == E_ALIGN, kw
    assert run(track_args(), ws=BASE + 4) == E_ALIGN
    # what the rules admit reaches the alignment check; the query answers for them
    for kw in (dict(lag=12), dict(lag=-12), dict(lag=0, to=8), dict(lag=0, to=23), dict(lag=0, to=35), dict(ANCHOR), dict(ANCHOR, F=16),
               dict(ANCHOR, anchor_frame=2 ** 30), dict(visible=40960, hist_vis=None, hist_conf=None, thresh=nan), dict(first_row=None),
               dict(cs=2, radius=1), dict(cs=6, radius=4), dict(N_out=40), dict(f0=0, lag=3), dict(H=1, W=1)):
        assert run(track_args(stats=28674, **kw)) == E_ALIGN, kw
        assert query(track_args(**kw))[0] == 0, kw
    # the workspace query: 24 bytes per node of every level, per group and frame
    for (H, W, cs), levels in (((1, 1, 2), ((2, 2), (1, 1))), ((67, 130, 3), ((10, 18), (5, 9), (3, 5), (2, 3), (1, 2), (1, 1))),
                               ((1080, 1920, 4), ((69, 121), (35, 61), (18, 31), (9, 16), (5, 8), (3, 4), (2, 2), (1, 1)))):
        rc, need = query(track_args(H=H, W=W, cs=cs, G=3, F=5))
        assert rc == 0 and need == 3 * 5 * 24 * sum(h * w for h, w in levels), (H, W, cs)


def warp_args(**kw):
    """A ctk_warp_field_args that passes every check: 3 HWC pictures of 20 x 30 with padded rows, dst well behind src, and a flow."""
    from cotracker_amd import _lib as L
    a = L.Field.WarpArgs()
    a.F, a.H, a.W, a.C, a.layout, a.border, a.cs, a.reserved = 3, 20, 30, 3, 0, 0, 3, 0
    a.src_frame_stride, a.src_row_stride, a.dst_frame_stride, a.dst_row_stride = 2000, 96, 2100, 100
    a.field, a.src, a.dst, a.flow = 4096, BASE, 2 * BASE, 3 * BASE
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_warp_field_refuses_before_any_launch(lib):
    def warp(a):
        return lib.ctk_warp_field(None if a is None else C.byref(a), None)
    assert warp(None) == E_NULL and warp(warp_args(field=None)) == E_NULL
    assert warp(warp_args(dst=None, flow=None)) == E_NULL and warp(warp_args(src=None)) == E_NULL
    shape = (("F", (0, -1, 65536)), ("H", (0, -1, 32769)), ("W", (0, -1, 32769)), ("C", (0, 2, 4, -1)), ("layout", (-1, 2)),
             ("border", (-1, 2, 7)), ("cs", (1, 7, -1)), ("reserved", (1, -1)), ("src_row_stride", (89, 0, -96, 2 ** 40 + 1)),
             ("dst_row_stride", (89, 0, -100, 2 ** 40 + 1)), ("src_frame_stride", (1919, 1, -1, 2 ** 40 + 1)),
             ("dst_frame_stride", (1999, 0, -1, 2 ** 40 + 1)))
    for field, values in shape:
        for v in values:
            assert warp(warp_args(**{field: v})) == E_SHAPE, (field, v)
    # planar: a row is W elements, a frame 3 H rows; one channel: a row is W elements, a frame H rows
    assert warp(warp_args(layout=1, src_row_stride=29)) == E_SHAPE and warp(warp_args(layout=1, src_row_stride=32, src_frame_stride=1919)) == E_SHAPE
    assert warp(warp_args(C=1, src_row_stride=29)) == E_SHAPE and warp(warp_args(C=1, src_row_stride=32, src_frame_stride=639)) == E_SHAPE
    # overlapping byte ranges: src covers 2 * 2000 + 19 * 96 + 90 = 5914 bytes, dst 2 * 2100 + 19 * 100 + 90 = 6190
    for dst in (BASE, BASE + 1, BASE + 5913, BASE - 6189, BASE - 1):
        assert warp(warp_args(dst=dst)) == E_SHAPE, dst
    for dst in (BASE + 5914, BASE - 6190):  # back to back is no overlap: the refusal is then the alignment one
        assert warp(warp_args(dst=dst, field=4100)) == E_ALIGN, dst
    assert warp(warp_args(field=4100)) == E_ALIGN and warp(warp_args(flow=3 * BASE + 4)) == E_ALIGN
    assert warp(warp_args(F=0, field=None)) == E_NULL and warp(warp_args(F=0, field=4100)) == E_SHAPE
    # what the rules admit reaches the alignment check: the flow alone (no stride is looked at), one source for all pictures, ...
    for kw in (dict(dst=None, src=None, src_row_stride=0, dst_row_stride=-5), dict(flow=None), dict(src_frame_stride=0), dict(border=1),
               dict(layout=1, H=6), dict(C=1, src_row_stride=30, dst_row_stride=30, src_frame_stride=600, dst_frame_stride=600),
               dict(C=1, layout=1), dict(cs=2), dict(cs=6), dict(dst=2 * BASE + 1),
               dict(F=65535, src_frame_stride=1920, dst_frame_stride=2000, dst=1 << 30, flow=1 << 40)):
        assert warp(warp_args(field=4100, **kw)) == E_ALIGN, kw


def test_python_layers_signatures_and_refusals():
    from cotracker_amd import model, ops
    from cotracker_amd.predictor import CoTrackerOnlinePredictor

    def check(fn, names, positional, defaults):
        sig = inspect.signature(fn)
        assert list(sig.parameters)[:len(names)] == names
        assert [sig.parameters[n].default for n in names[positional:]] == defaults
        assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in list(sig.parameters.values())[positional:])
        return sig
    check(ops.track_field, ["tracks", "visible", "size", "cell", "radius", "to", "lag", "anchor", "scale", "N_out"], 3,
          [16, 2, None, None, None, (1.0, 1.0), None])
    assert inspect.signature(ops.track_field).parameters["size"].default is inspect.Parameter.empty
    check(ops.warp_field, ["src", "field", "cell", "border", "fill", "out", "flow"], 3, ["fill", (0, 0, 0), None, False])
    assert inspect.signature(ops.warp_field).parameters["cell"].default is inspect.Parameter.empty
    check(ops.propagate, ["picture", "tracks", "visible", "src_frame", "frames"], 4, [None])
    check(ops.dense_flow, ["tracks", "visible", "size", "lag"], 3, [1])
    sig = inspect.signature(ops.StreamGroups.field)
    assert list(sig.parameters)[:3] == ["self", "f0", "F"] and all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in list(sig.parameters.values())[3:])
    assert list(inspect.signature(CoTrackerOnlinePredictor.pin).parameters) == ["self", "frame", "group"]
    sig = inspect.signature(CoTrackerOnlinePredictor.propagate)
    assert list(sig.parameters) == ["self", "picture", "anchor_or_frame", "first_frame", "n", "cell", "radius", "border", "fill", "out", "group"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [None, None, 16, 2, "fill", (0, 0, 0), None, 0]
    sig = inspect.signature(CoTrackerOnlinePredictor.dense_flow)
    assert list(sig.parameters)[:4] == ["self", "n", "first_frame", "lag"] and sig.parameters["lag"].default == 1
    assert hasattr(model.CoTrackerThreeOnline, "stream_field")
    for word in ("zeroth order", "untouched", "four launches"):
        assert word in CoTrackerOnlinePredictor.propagate.__doc__
    assert ops.field_grid((1080, 1920), 16) == (69, 121) == (R.grid(1080, 4), R.grid(1920, 4)) and ops.field_grid((1, 1), 4) == (2, 2)
    for cell in (0, 2, 3, 12, 128):
        with pytest.raises(ValueError, match="power of two"):
            ops.field_grid((8, 8), cell)
    # host tensors are refused: no fall-back
    with pytest.raises(ValueError, match="device tensor"):
        ops.track_field(torch.zeros(2, 3, 2), torch.zeros(2, 3, dtype=torch.uint8), size=(8, 8), lag=1)
    with pytest.raises(ValueError, match="device tensor"):
        ops.warp_field(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 2, 2, 2, dtype=torch.int32), cell=16)
    with pytest.raises(ValueError, match="device tensor"):
        ops.propagate(torch.zeros(8, 8, dtype=torch.uint8), torch.zeros(2, 3, 2), torch.zeros(2, 3, dtype=torch.uint8), src_frame=0)
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=8)
    mask = torch.zeros(32, 48, dtype=torch.uint8)
    for call in (lambda: p.pin(), lambda: p.propagate(mask, 0), lambda: p.dense_flow()):
        with pytest.raises(RuntimeError, match="no stream is running"):
            call()
    p(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, queries=torch.zeros(1, 3, 3))
    for call in (lambda: p.pin(), lambda: p.propagate(mask, 0), lambda: p.dense_flow(), lambda: p.model.stream_field(0, 1, size=(32, 48), lag=1)):
        with pytest.raises(RuntimeError, match="no stream is running"):  # after the first step: no window has been tracked
            call()
    p2 = CoTrackerOnlinePredictor(checkpoint=None, v2=True, window_len=8)
    for call in (lambda: p2.pin(), lambda: p2.propagate(mask, 0), lambda: p2.dense_flow(), lambda: p2.model.stream_field(0, 1, size=(32, 48), lag=1)):
        with pytest.raises(NotImplementedError, match="v2"):
            call()
