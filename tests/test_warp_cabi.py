"""Warp frames, the part that needs no GPU: ctk_warp_frames and ctk_smooth_path are declared, bound and exported without an ABI bump,
the new structs' ctypes mirrors have the compiler's layout, every refusal comes back before any launch, and the Python layers have the
signatures and defaults the callers rely on."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from ctk_support import ROOT, header_layout, lib  # noqa: F401

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
NAMES = ("ctk_warp_frames", "ctk_smooth_path")


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
    assert int(header_layout()["sizeof"]["ctk_stream_args"]) == C.sizeof(L.StreamArgs) == 200  # no existing struct grew
    assert C.sizeof(L.Draw.Args) == 216 and C.sizeof(L.Motion.Args) == 128
    section = header.split("---- warp frames")[1]
    assert section.index("Op A") < section.index("Op C")  # the section stands before "Op A"
    assert header.index("---- fit motion") < header.index("---- warp frames") < header.index("---- Op A")
    assert not re.search(r"#define CTK_E_\w+\s+-?\d+", section.split("Op A")[0])  # no new error code
    assert (L.Warp.BORDER_FILL, L.Warp.BORDER_EDGE) == (0, 1)
    assert re.search(r"#define CTK_WARP_FILL 0\b", header) and re.search(r"#define CTK_WARP_EDGE 1\b", header)
    makefile = open(os.path.join(ROOT, "co-tracker_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bwarp\.hip\b", makefile, re.M) and re.search(r"^NOFMA = .*\bwarp\b", makefile, re.M)
    assert re.search(r"^HDRS = .*\bwarp_math\.h\b", makefile, re.M)
    # the release library carries no CTK_* string literal
    blob = open(L.LIB_PATH, "rb").read()
    assert not re.findall(rb"CTK_WARP\w*", blob) and not re.findall(rb"CTK_E_\w+", blob)
    assert "CTK_OPT_COUNT = 7" in header and L.OPT_COUNT == 7  # one kernel, not an option


WARP_FIELDS = ["F", "H", "W", "layout", "border", "reserved", "fill", "src_frame_stride", "src_row_stride", "dst_frame_stride",
               "dst_row_stride", "matrices", "src", "dst"]
PATH_FIELDS = ["G", "F", "alpha", "reserved", "motion", "post", "state", "warp"]


@pytest.mark.parametrize("cname,holder,size,order", [("ctk_warp_args", "Args", 88, WARP_FIELDS), ("ctk_smooth_path_args", "PathArgs", 48, PATH_FIELDS)])
def test_args_mirrors_match_the_compiler(cname, holder, size, order):
    """sizeof and every offsetof of the two new structs, from a C program compiled against include/ctk.h."""
    from cotracker_amd import _lib as L
    cls = getattr(L.Warp, holder)
    fields = [f[0] for f in cls._fields_]
    assert fields == order
    lines = [f'printf("S %zu\\n", sizeof({cname}));']
    lines += [f'printf("F {f} %zu\\n", offsetof({cname}, {f}));' for f in fields]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "warp_layout.c"), os.path.join(d, "warp_layout")
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


def warp_args(**kw):
    """A ctk_warp_args that passes every check: 3 HWC pictures of 20 x 30 with padded rows, dst well behind src."""
    from cotracker_amd import _lib as L
    a = L.Warp.Args()
    a.F, a.H, a.W, a.layout, a.border, a.reserved = 3, 20, 30, 0, 0, 0
    a.src_frame_stride, a.src_row_stride, a.dst_frame_stride, a.dst_row_stride = 2000, 96, 2100, 100
    a.matrices, a.src, a.dst = 4096, BASE, 2 * BASE
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def path_args(**kw):
    from cotracker_amd import _lib as L
    a = L.Warp.PathArgs()
    a.G, a.F, a.alpha, a.reserved = 2, 5, 0.1, 0
    a.motion, a.post, a.state, a.warp = 4096, 8192, 12288, 16384
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_warp_frames_refuses_before_any_launch(lib):
    """Every refusal is an E_* code (a launch on a machine without a GPU would be a hipError_t > 0)."""
    def warp(a):
        return lib.ctk_warp_frames(None if a is None else C.byref(a), None)
    assert warp(None) == E_NULL
    for f in ("matrices", "src", "dst"):
        assert warp(warp_args(**{f: None})) == E_NULL, f
    shape = (("F", (0, -1, 65536)), ("H", (0, -1, 32769)), ("W", (0, -1, 32769)), ("layout", (-1, 2)), ("border", (-1, 2, 7)),
             ("reserved", (1, -1)), ("src_row_stride", (89, 0, -96, 2 ** 40 + 1)), ("dst_row_stride", (89, 0, -100, 2 ** 40 + 1)),
             ("src_frame_stride", (1919, 0, -1, 2 ** 40 + 1)), ("dst_frame_stride", (1999, 0, -1, 2 ** 40 + 1)))
    for field, values in shape:
        for v in values:
            assert warp(warp_args(**{field: v})) == E_SHAPE, (field, v)
    # planar: a row is W elements, a frame 3 H rows
    assert warp(warp_args(layout=1, src_row_stride=29)) == E_SHAPE and warp(warp_args(layout=1, src_row_stride=32, src_frame_stride=1919)) == E_SHAPE
    assert warp(warp_args(layout=1, src_row_stride=32, src_frame_stride=1920, dst=None)) == E_NULL
    # overlapping byte ranges: src covers 2 * 2000 + 19 * 96 + 90 = 5914 bytes, dst 2 * 2100 + 19 * 100 + 90 = 6190
    for dst in (BASE, BASE + 1, BASE + 5913, BASE - 6189, BASE - 1):
        assert warp(warp_args(dst=dst)) == E_SHAPE, dst
    for dst in (BASE + 5914, BASE - 6190):  # back to back is no overlap: the refusal is then the alignment one
        assert warp(warp_args(dst=dst, matrices=4098)) == E_ALIGN, dst
    assert warp(warp_args(matrices=4097)) == E_ALIGN and warp(warp_args(matrices=4098)) == E_ALIGN
    # a NULL pointer is named before a shape, a shape before the alignment
    assert warp(warp_args(F=0, src=None)) == E_NULL and warp(warp_args(F=0, matrices=4097)) == E_SHAPE
    # what the rules admit reaches the alignment check
    for kw in (dict(F=65535, src_frame_stride=1920, dst_frame_stride=2000, dst=1 << 30), dict(F=1, src_frame_stride=1920, H=20),
               dict(border=1), dict(layout=1, H=6), dict(src_row_stride=90, dst_row_stride=90), dict(dst=2 * BASE + 1),
               dict(H=32768, W=1, src_row_stride=3, dst_row_stride=3, src_frame_stride=3 * 32768, dst_frame_stride=3 * 32768, F=2, dst=1 << 30),
               dict(src_row_stride=2 ** 40, src_frame_stride=2 ** 40, dst_row_stride=2 ** 40, dst_frame_stride=2 ** 40, H=1, F=1, dst=1 << 50)):
        assert warp(warp_args(matrices=4098, **kw)) == E_ALIGN, kw


def test_smooth_path_refuses_before_any_launch(lib):
    def path(a):
        return lib.ctk_smooth_path(None if a is None else C.byref(a), None)
    nan, inf = float("nan"), float("inf")
    assert path(None) == E_NULL
    for f in ("motion", "state", "warp"):
        assert path(path_args(**{f: None})) == E_NULL, f
    for field, values in (("G", (0, -1, 65536)), ("F", (0, -1, 65536)), ("alpha", (nan, -0.001, 1.001, inf, -inf)), ("reserved", (1, -1))):
        for v in values:
            assert path(path_args(**{field: v})) == E_SHAPE, (field, v)
    assert path(path_args(state=12292)) == E_ALIGN and path(path_args(state=12289)) == E_ALIGN
    assert path(path_args(motion=4098)) == E_ALIGN and path(path_args(warp=16385)) == E_ALIGN
    assert path(path_args(post=8193)) == E_ALIGN and path(path_args(post=8194)) == E_ALIGN  # (post is optional, but a float pointer)
    assert path(path_args(G=0, motion=None)) == E_NULL and path(path_args(G=0, state=12292)) == E_SHAPE
    # what the rules admit reaches the alignment check: post is optional, alpha may be 0 or 1
    for kw in (dict(post=None), dict(alpha=0.0), dict(alpha=1.0), dict(G=65535, F=65535), dict(G=1, F=1)):
        assert path(path_args(state=12292, **kw)) == E_ALIGN, kw


def test_python_layers_signatures_and_refusals():
    from cotracker_amd import model, ops
    from cotracker_amd.predictor import CoTrackerOnlinePredictor

    def check(fn, names, positional, defaults):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == names
        assert [sig.parameters[n].default for n in names[positional:]] == defaults
        return sig
    sig = check(ops.warp_frames, ["frames", "matrices", "out", "border", "fill", "layout"], 2, [None, "fill", (0, 0, 0), None])
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[2:])
    sig = check(ops.smooth_path, ["motion", "state", "alpha", "post", "out"], 1, [None, 0.1, None, None])
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[2:])
    assert list(inspect.signature(ops.zoom_matrix).parameters) == ["H", "W", "zoom"]
    sig = check(ops.stabilize, ["frames", "tracks", "visible", "alpha", "zoom", "border", "fill", "out", "state", "model", "tol", "hypotheses",
                                "min_base", "seed"], 3, [0.1, 1.0, "fill", (0, 0, 0), None, None, "similarity", 2.0, 128, 16.0, 0])
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[3:])
    sig = inspect.signature(ops.StreamGroups.stabilize)
    assert list(sig.parameters)[:5] == ["self", "frames", "f0", "group", "reset"]
    assert sig.parameters["group"].default == 0 and sig.parameters["reset"].default is False
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in list(sig.parameters.values())[3:])
    check(CoTrackerOnlinePredictor.stabilize, ["self", "frames", "first_frame", "alpha", "zoom", "border", "fill", "out", "group", "reset", "model",
                                               "tol", "hypotheses", "min_base", "seed"], 2,
          [None, 0.1, 1.0, "fill", (0, 0, 0), None, 0, False, "similarity", 2.0, 128, 16.0, 0])
    for word in ("draw()", "inverse(warp)", "untouched"):
        assert word in CoTrackerOnlinePredictor.stabilize.__doc__
    assert hasattr(model.CoTrackerThreeOnline, "stream_stabilize")
    # zoom_matrix: float32, a scale by 1 / zoom about the picture centre
    z = ops.zoom_matrix(48, 64, 1.25)
    assert z.dtype == torch.float32 and tuple(z.shape) == (2, 3) and z[0, 0] == z[1, 1] == torch.tensor(0.8) and z[0, 1] == z[1, 0] == 0
    assert torch.allclose(z.double() @ torch.tensor([31.5, 23.5, 1.0], dtype=torch.float64), torch.tensor([31.5, 23.5], dtype=torch.float64), atol=1e-5)
    assert torch.equal(ops.zoom_matrix(48, 64, 1.0), torch.tensor([[1.0, 0, 0], [0, 1.0, 0]]))
    import warp_reference as R
    for H, W, zoom in ((48, 64, 1.25), (1080, 1920, 1.1), (37, 53, 0.9)):  # the restatement's zoom is the one the tests compare with
        assert torch.equal(ops.zoom_matrix(H, W, zoom), torch.from_numpy(R.zoom_matrix(H, W, zoom)))
    assert np.array_equal(R.zoom_matrix(48, 64, 1.0), R.IDENTITY.reshape(2, 3))
    with pytest.raises(ValueError, match="zoom"):
        ops.zoom_matrix(48, 64, 0.0)
    # host tensors are refused: no fall-back
    with pytest.raises(ValueError, match="device tensor"):
        ops.warp_frames(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 2, 3))
    with pytest.raises(ValueError, match="device tensor"):
        ops.smooth_path(torch.zeros(2, 2, 3))
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=8)
    frames = torch.zeros(1, 32, 48, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.stabilize(frames)
    p(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, queries=torch.zeros(1, 3, 3))
    with pytest.raises(RuntimeError, match="no stream is running"):  # after the first step: no window has been tracked
        p.stabilize(frames)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.model.stream_stabilize(frames, 0)
    p2 = CoTrackerOnlinePredictor(checkpoint=None, v2=True, window_len=8)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.stabilize(frames)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.model.stream_stabilize(frames, 0)
