"""Endless streams, the part that needs no GPU: the ring forms of the four stream entry points and ctk_stream_emit are declared,
bound and exported without an ABI bump, the new struct's ctypes mirror has the compiler's layout, every refusal comes back before
any launch, and the host switches (model.stream_history_frames, predictor.history_frames, ops.StreamGroups.frame_rows) behave."""
import copy
import ctypes as C
import os
import pickle
import re
import subprocess
import tempfile

import pytest
import torch

from ctk_support import ROOT, header_layout, lib  # noqa: F401

E_NULL, E_SHAPE = -1, -2
NEW = ("ctk_stream_begin_ring", "ctk_stream_support_ring", "ctk_stream_commit_ring", "ctk_stream_assign_ring", "ctk_stream_emit")


def test_declared_bound_exported_and_abi(lib):
    from cotracker_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "ctk.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in L.SYMBOLS and hasattr(lib, name), name
        assert any(ln.split()[-1] == name and " T " in ln for ln in nm.splitlines()), name
    assert lib.ctk_abi_version() == L.ABI_VERSION == 9  # additive
    assert int(header_layout()["sizeof"]["ctk_stream_args"]) == C.sizeof(L.StreamArgs) == 200  # the struct did not grow
    assert "ctk_stream_emit" in header.split("#define CTK_ABI_VERSION")[0]  # the ABI history names the addition


def test_emit_args_mirror_matches_the_compiler():
    """sizeof and every offsetof of ctk_stream_emit_args, from a C program compiled against include/ctk.h."""
    from cotracker_amd import _lib as L
    fields = [f[0] for f in L.StreamEmit.Args._fields_]
    lines = ['printf("S %zu\\n", sizeof(ctk_stream_emit_args));']
    lines += [f'printf("F {f} %zu\\n", offsetof(ctk_stream_emit_args, {f}));' for f in fields]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "emit_layout.c"), os.path.join(d, "emit_layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "ctk.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert int(out[0].split()[1]) == C.sizeof(L.StreamEmit.Args)
    got = {ln.split()[1]: int(ln.split()[2]) for ln in out[1:]}
    assert got == {f: getattr(L.StreamEmit.Args, f).offset for f in fields}
    assert len(got) == 18


def stream_args(**kw):
    """A ctk_stream_args on a ring of 8 rows that passes every check at a frame far beyond the ring."""
    from cotracker_amd import _lib as L
    a = L.StreamArgs()
    a.G, a.N, a.S, a.step, a.ind, a.T_valid, a.T_cap, a.stride = 3, 10, 8, 4, 4000, 8, 8, 4.0
    for n in ("queries", "hist_coords", "hist_vis", "hist_conf", "coords", "vis", "conf", "point_mask"):
        setattr(a, n, 4096)
    for l in range(L.LEVELS):
        a.H[l], a.W[l], a.fmaps[l], a.support[l] = 16 >> l, 24 >> l, 4096, 4096
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def ring_calls(lib):
    return {"begin": lambda a: lib.ctk_stream_begin_ring(None if a is None else C.byref(a), None),
            "support": lambda a: lib.ctk_stream_support_ring(None if a is None else C.byref(a), None),
            "commit": lambda a: lib.ctk_stream_commit_ring(None if a is None else C.byref(a), None),
            "assign": lambda a: lib.ctk_stream_assign_ring(None if a is None else C.byref(a), 4096, 4096, 5, None)}


def test_ring_forms_refuse_before_any_launch(lib):
    """Every refusal is an E_* code (a launch on a machine without a GPU would be a hipError_t > 0)."""
    calls = ring_calls(lib)
    for name, call in calls.items():
        assert call(None) == E_NULL, name
        # the capacity rule of a ring is R >= S: a T_cap below ind + S is no refusal, a T_cap below S is
        assert call(stream_args(T_cap=7)) == E_SHAPE, name
        assert call(stream_args(T_cap=0)) == E_SHAPE, name
        for field, values in (("G", (0, -1, 65536)), ("N", (0, -3)), ("S", (0, -8)), ("step", (0, -4, 8, 9)), ("ind", (-4, 2, 4001, 2 ** 30)),
                              ("stride", (0.0, -4.0, float("nan"), float("inf")))):
            for v in values:
                assert call(stream_args(**{field: v})) == E_SHAPE, (name, field, v)
        # t rides on a grid axis: a window longer than 65535 frames is refused, not launched (the ring is large enough for it)
        assert call(stream_args(S=65536, step=32768, ind=0, T_cap=65536, N=1, T_valid=8)) == E_SHAPE, name
    assert calls["begin"](stream_args(S=65534, step=32767, ind=0, T_cap=65534, N=1, queries=None)) == E_NULL  # (admitted up to the NULL check)
    # the linear forms still refuse what the ring admits
    assert lib.ctk_stream_begin(C.byref(stream_args()), None) == E_SHAPE
    assert lib.ctk_stream_commit(C.byref(stream_args()), None) == E_SHAPE
    reads = {"begin": ("queries", "hist_coords", "hist_vis", "hist_conf", "coords", "vis", "conf", "point_mask"),
             "support": ("queries",), "commit": ("hist_coords", "hist_vis", "hist_conf", "coords", "vis", "conf"),
             "assign": ("queries", "hist_coords", "hist_vis", "hist_conf")}
    for name, fields in reads.items():
        for f in fields:
            assert calls[name](stream_args(**{f: None})) == E_NULL, (name, f)
    for l in range(4):
        for name in ("support", "assign"):
            a = stream_args()
            a.support[l] = None
            assert calls[name](a) == E_NULL, (name, l)
        a = stream_args()
        a.fmaps[l] = None
        assert calls["support"](a) == E_NULL
        a = stream_args()
        a.H[l] = 0
        assert calls["support"](a) == E_SHAPE
        a = stream_args()
        a.support[l] = 4096 + 8
        assert calls["assign"](a) == E_SHAPE
    for T_valid in (0, -1, 9):
        assert calls["commit"](stream_args(T_valid=T_valid)) == E_SHAPE
    a = stream_args()
    assert lib.ctk_stream_assign_ring(C.byref(a), None, 4096, 5, None) == E_NULL
    assert lib.ctk_stream_assign_ring(C.byref(a), 4096, None, 5, None) == E_NULL
    for M in (0, -1, 31, 2 ** 31 - 1):  # G*N = 30
        assert lib.ctk_stream_assign_ring(C.byref(a), 4096, 4096, M, None) == E_SHAPE, M


def emit_args(**kw):
    from cotracker_amd import _lib as L
    a = L.StreamEmit.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.f1, a.sx, a.sy, a.thresh, a.reserved = 3, 10, 7, 16, 1000, 1016, 1.0, 1.0, 0.6, 0
    for n in ("hist_coords", "hist_vis", "hist_conf", "first_row", "tracks", "vis_logit", "conf_logit", "visible"):
        setattr(a, n, 4096)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_emit_refuses_before_any_launch(lib):
    emit = lambda a: lib.ctk_stream_emit(None if a is None else C.byref(a), None)  # noqa: E731
    assert emit(None) == E_NULL
    for f in ("hist_coords", "tracks", "hist_vis", "hist_conf"):
        assert emit(emit_args(**{f: None})) == E_NULL, f
    assert emit(emit_args(visible=None)) == E_NULL  # first_row without visible
    for field, values in (("G", (0, -1, 65536)), ("N", (0, -1, 2 ** 30)), ("N_out", (0, -1, 11)), ("R", (0, -1, 15)), ("f0", (-1, 999, 1016, 2000)),
                          ("f1", (1000, 999, 1017, 2 ** 30 + 1)), ("thresh", (float("nan"),)), ("reserved", (1, -1))):
        for v in values:
            assert emit(emit_args(**{field: v})) == E_SHAPE, (field, v)
    assert emit(emit_args(R=70000, f0=0, f1=65536)) == E_SHAPE  # frames ride on a grid axis


def test_frame_rows_of_ring_and_linear_history():
    """ops.StreamGroups.frame_rows (the rows the range guard saves and restores) needs no device."""
    from cotracker_amd import ops

    class Fake:
        ring_rows = None
    assert ops.StreamGroups.frame_rows(Fake(), 24, 28) == [slice(24, 28)]
    Fake.ring_rows = 11
    for f0, f1 in ((0, 4), (8, 11), (9, 13), (44, 48), (40, 44), (20, 31), (33, 33)):
        rows = [r for s_ in ops.StreamGroups.frame_rows(Fake(), f0, f1) for r in range(s_.start, s_.stop)]
        assert rows == [f % 11 for f in range(f0, f1)], (f0, f1)
    with pytest.raises(ValueError, match="ring_rows"):
        ops.StreamGroups(torch.zeros(1, 2, 3), 8, 4, 4.0, [(16, 24)] * 4, ring_rows=7)


def test_model_and_predictor_switches():
    from cotracker_amd.build_cotracker import build_cotracker
    from cotracker_amd.model import CoTrackerThreeOnline
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    m = CoTrackerThreeOnline(window_len=8, model_resolution=(64, 96))
    assert m.stream_history_frames is None and m.stream_window_start is None and copy.deepcopy(m).stream_history_frames is None
    for bad in (7, 0, -8, 8.0, "8", True):
        with pytest.raises(ValueError, match="window_len"):
            m.stream_history_frames = bad
    assert m.stream_history_frames is None
    m.stream_history_frames = 8
    m.stream_history_frames = 19
    assert copy.deepcopy(m).stream_history_frames == 19 and pickle.loads(pickle.dumps(m)).stream_history_frames == 19
    assert m.stream_slots is False and m.stream_groups is False  # independent switches
    m.stream_history_frames = None
    assert m.stream_history_frames is None
    v2 = build_cotracker(None, v2=True, window_len=8)
    assert v2.stream_history_frames is None
    with pytest.raises(NotImplementedError, match="stream_history_frames"):
        v2.stream_history_frames = 16
    v2.stream_history_frames = None
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=8)
    assert p.history_frames is None and p.window_start is None
    with pytest.raises(RuntimeError, match="history_frames"):
        p.recent(4)
    p2 = CoTrackerOnlinePredictor(checkpoint=None, v2=True, window_len=8)
    p2.history_frames = 16
    with pytest.raises(NotImplementedError, match="history_frames"):
        p2(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, queries=torch.zeros(1, 3, 3))
    p.history_frames = 4
    with pytest.raises(ValueError, match="window_len"):
        p(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, queries=torch.zeros(1, 3, 3))


def test_frame_limit_is_checked_on_the_host():
    """Frames are float32 in the query table: the window that would pass 2^24 is refused by a host comparison."""
    from cotracker_amd.model import CoTrackerThreeOnline
    m = CoTrackerThreeOnline(window_len=8, model_resolution=(64, 96))
    assert m.FRAME_LIMIT == 2 ** 24 and float(torch.tensor(2.0 ** 24 - 1)) == 2 ** 24 - 1
    m._check_frame_limit(2 ** 24 - 8)  # frames up to 2^24 - 1: exact
    with pytest.raises(RuntimeError, match="2\\^24"):
        m._check_frame_limit(2 ** 24 - 4)
