"""Draw tracks, the part that needs no GPU: ctk_draw_tracks and its workspace query are declared, bound and exported without an ABI
bump, the new struct's ctypes mirror has the compiler's layout, every refusal comes back before any launch, and the Python layers
have the signatures and defaults the callers rely on."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import pytest
import torch

import draw_reference as R
from ctk_support import ROOT, header_layout, lib  # noqa: F401

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
NAMES = ("ctk_draw_tracks", "ctk_draw_tracks_workspace_bytes")


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
    assert C.sizeof(L.Seed.Args) == 80 and C.sizeof(L.StreamHealth.Args) == 136
    assert not re.search(r"#define CTK_E_\w+\s+-?\d+", header.split("draw tracks")[1].split("Op A")[0])  # no new error code
    makefile = open(os.path.join(ROOT, "co-tracker_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bdraw\.hip\b", makefile, re.M) and re.search(r"^NOFMA = .*\bdraw\b", makefile, re.M)
    assert re.search(r"^HDRS = .*\bdraw_math\.h\b", makefile, re.M)
    # the release library carries no CTK_* string literal
    blob = open(L.LIB_PATH, "rb").read()
    assert not re.findall(rb"CTK_DRAW\w*", blob) and not re.findall(rb"CTK_E_\w+", blob)


def test_draw_args_mirror_matches_the_compiler():
    """sizeof and every offsetof of ctk_draw_args, from a C program compiled against include/ctk.h."""
    from cotracker_amd import _lib as L
    fields = [f[0] for f in L.Draw.Args._fields_]
    lines = ['printf("S %zu\\n", sizeof(ctk_draw_args));', 'printf("A %zu\\n", sizeof(((ctk_draw_args*)0)->alpha));']
    lines += [f'printf("F {f} %zu\\n", offsetof(ctk_draw_args, {f}));' for f in fields]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "draw_layout.c"), os.path.join(d, "draw_layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "ctk.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert int(out[0].split()[1]) == C.sizeof(L.Draw.Args)
    assert int(out[1].split()[1]) == C.sizeof(L.Draw.Args().alpha) == 65
    got = {ln.split()[1]: int(ln.split()[2]) for ln in out[2:]}
    assert got == {f: getattr(L.Draw.Args, f).offset for f in fields}
    assert len(got) == 28
    # the header declares the fields in the mirror's order and no others
    body = re.search(r"typedef struct ctk_draw_args \{(.*?)\} ctk_draw_args;", open(os.path.join(ROOT, "include", "ctk.h")).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert declared == fields


POINTERS = ("hist_coords", "visible", "hist_vis", "hist_conf", "first_row", "colors", "src", "dst")


def draw_args(**kw):
    """A ctk_draw_args that passes every check: 3 pictures of 37 x 53 pixels, channels-last, out of a ring of 8 rows."""
    from cotracker_amd import _lib as L
    a = L.Draw.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.F, a.trail, a.radius, a.half_width, a.max_jump = 2, 5, 4, 8, 6, 3, 3, 4, 1, 256
    a.sx, a.sy, a.thresh, a.layout, a.H, a.W, a.reserved = 1.37, 0.81, 0.6, 0, 37, 53, 0
    a.row_stride, a.frame_stride = 53 * 3 + 5, (53 * 3 + 5) * 37
    for n in POINTERS:
        setattr(a, n, 4096)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def need(lib, a):
    n = C.c_size_t(0)
    assert lib.ctk_draw_tracks_workspace_bytes(C.byref(a), C.byref(n)) == 0
    return n.value


def test_draw_refuses_before_any_launch(lib):
    """Every refusal is an E_* code (a launch on a machine without a GPU would be a hipError_t > 0)."""
    big = 1 << 40

    def draw(a, ws=4096, nbytes=big):
        return lib.ctk_draw_tracks(None if a is None else C.byref(a), ws, nbytes, None)

    def query(a):
        n = C.c_size_t(0)
        return lib.ctk_draw_tracks_workspace_bytes(None if a is None else C.byref(a), C.byref(n))
    nan = float("nan")
    assert draw(None) == E_NULL and query(None) == E_NULL
    assert lib.ctk_draw_tracks_workspace_bytes(C.byref(draw_args()), None) == E_NULL
    for f in ("hist_coords", "colors", "dst"):
        assert draw(draw_args(**{f: None})) == E_NULL, f
    assert draw(draw_args(), ws=None) == E_NULL
    # exactly one form of visibility: `visible` wins when it is given, the logits are needed when it is not
    assert draw(draw_args(visible=None, hist_vis=None)) == E_NULL and draw(draw_args(visible=None, hist_conf=None)) == E_NULL
    shape = (("G", (0, -1, 65536)), ("N", (0, -1, 3)), ("N_out", (0, -1, 6)), ("R", (0, -1, 5)), ("F", (0, -1, 6, 65536)),
             ("f0", (-1, -100, 2 ** 30 - 2)), ("trail", (-1, 6, 65, 1000)), ("radius", (0, -1, 33)), ("half_width", (-1, 17)),
             ("max_jump", (0, -1, 4096)), ("layout", (-1, 2)), ("H", (0, -1, 32769)), ("W", (0, -1, 32769)), ("reserved", (1, -1)),
             ("row_stride", (53 * 3 - 1, 0, -4, (1 << 40) + 1)), ("frame_stride", ((53 * 3 + 5) * 37 - 1, 0, -1, (1 << 40) + 1)))
    for field, values in shape:
        for v in values:
            assert draw(draw_args(**{field: v})) == E_SHAPE, (field, v)
            assert query(draw_args(**{field: v})) == E_SHAPE, (field, v)
    # (what is admitted is asked of the query, which never launches)
    assert draw(draw_args(F=5, trail=4, R=8)) == E_SHAPE and query(draw_args(F=4, trail=4, R=8, f0=4)) == 0  # F + trail > R
    assert query(draw_args(f0=2 ** 30 - 3, F=3)) == 0 and draw(draw_args(f0=2 ** 30 - 2, F=3)) == E_SHAPE   # f0 + F > 2^30
    assert draw(draw_args(G=8193, N=8192, N_out=1)) == E_SHAPE and draw(draw_args(G=65535, N=65535, N_out=1)) == E_SHAPE  # G * N > 2^26
    # planar: a row is W elements, a frame 3 H rows
    assert draw(draw_args(layout=1, row_stride=52)) == E_SHAPE and draw(draw_args(layout=1, row_stride=53, frame_stride=53 * 37 * 3 - 1)) == E_SHAPE
    assert query(draw_args(layout=1, row_stride=53, frame_stride=53 * 37 * 3)) == 0
    # a NaN threshold matters with logits only
    assert draw(draw_args(visible=None, thresh=nan)) == E_SHAPE and query(draw_args(visible=None, thresh=nan)) == E_SHAPE
    assert draw(draw_args(thresh=nan, dst=None)) == E_NULL
    # a workspace smaller than the query answers
    a = draw_args()
    assert need(lib, a) == 3 * (3 + 1) * 2 * 4 * 24
    assert draw(a, nbytes=need(lib, a) - 1) == E_SHAPE and draw(a, nbytes=0) == E_SHAPE
    assert draw(a, ws=4100) == E_ALIGN and draw(draw_args(hist_coords=4100)) == E_ALIGN
    # what the rules admit reaches the pointer check: the refusal is then the NULL one
    for kw in (dict(trail=0, F=8), dict(trail=5, F=3), dict(trail=64, R=100, F=36), dict(radius=1), dict(radius=32), dict(half_width=0),
               dict(half_width=16), dict(max_jump=1), dict(max_jump=4095), dict(H=1, W=1, row_stride=3, frame_stride=3),
               dict(H=32768, W=32768, row_stride=3 * 32768, frame_stride=3 * 32768 * 32768), dict(N_out=5), dict(f0=0), dict(sx=nan, sy=nan),
               dict(G=65535, N=1024, N_out=1), dict(src=None), dict(first_row=None), dict(visible=None)):
        assert draw(draw_args(dst=None, **kw)) == E_NULL, kw
        assert query(draw_args(dst=None, **kw)) == 0, kw  # the query looks at no pointer of the struct


def test_python_layers_signatures_and_refusals():
    from cotracker_amd import model, ops
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    sig = inspect.signature(ops.draw_tracks)
    assert list(sig.parameters) == ["frames", "tracks", "visible", "colors", "trail", "radius", "half_width", "alpha", "max_jump", "first_frame",
                                    "scale", "first_row", "out", "layout"]
    assert [sig.parameters[n].default for n in ("colors", "trail", "radius", "half_width", "alpha", "max_jump", "first_frame", "scale",
                                                "first_row", "out", "layout")] == [None, 0, 4, 1, None, 256, 0, (1.0, 1.0), None, None, None]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[4:])
    psig = inspect.signature(CoTrackerOnlinePredictor.draw)
    assert list(psig.parameters) == ["self", "frames", "first_frame", "trail", "radius", "half_width", "colors", "out", "group"]
    assert [psig.parameters[n].default for n in list(psig.parameters)[2:]] == [None, 8, 4, 1, None, None, None]
    assert hasattr(ops.StreamGroups, "draw") and hasattr(model.CoTrackerThreeOnline, "stream_draw")
    # the default fade: the reference's quadratic one, in integers
    for L_ in (0, 1, 3, 8, 64):
        a = ops.default_alpha(L_)
        assert a == R.default_alpha(L_)[:L_ + 1].tolist() and a[0] == 255 and all(x >= y for x, y in zip(a, a[1:]))
    assert ops.default_alpha(3) == [255, 143, 63, 15]
    # the default colours: an integer ramp over y, red at the top, blue at the bottom, ends exact
    y = torch.tensor([[0.0, 10.0, 20.0, 30.0, 40.0, float("nan")], [5.0, 5.0, 5.0, 5.0, 5.0, 5.0]])
    c = ops.rainbow_colors(y)
    assert c.dtype == torch.uint8 and c.shape == (2, 6, 3)
    assert c[0].tolist() == [[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 0]]
    assert c[1].tolist() == [[255, 0, 0]] * 6  # (one height: the start of the ramp)
    ramp = ops.rainbow_colors(torch.arange(1021.0))
    assert len({tuple(v) for v in ramp.tolist()}) == 1021 and bool((ramp.max(dim=1).values == 255).all())
    # host tensors are refused: no fall-back
    with pytest.raises(ValueError, match="device tensor"):
        ops.draw_tracks(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 3, 2), torch.zeros(2, 3, dtype=torch.bool))
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=8)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.draw(torch.zeros(1, 32, 48, 3, dtype=torch.uint8))
    p(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, queries=torch.zeros(1, 3, 3))
    with pytest.raises(RuntimeError, match="no stream is running"):  # after the first step: no window has been tracked
        p.draw(torch.zeros(1, 32, 48, 3, dtype=torch.uint8))
    p2 = CoTrackerOnlinePredictor(checkpoint=None, v2=True, window_len=8)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.draw(torch.zeros(1, 32, 48, 3, dtype=torch.uint8))
    with pytest.raises(NotImplementedError, match="v2"):
        p2.model.stream_draw(None, 0, None)
