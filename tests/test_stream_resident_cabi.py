"""The resident slot assign, the part that needs no GPU: ctk_stream_assign_resident and its ring form are declared, bound and
exported without an ABI bump, every refusal comes back before a launch, and the host layers refuse what they must without a
device (the frame rule of the resident form: trunc(frame) >= ind - step, ind the first frame of the next call's window)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from ctk_support import ROOT, header_layout, lib  # noqa: F401

E_NULL, E_SHAPE = -1, -2
NEW = ("ctk_stream_assign_resident", "ctk_stream_assign_resident_ring")


def good_args(ring=False):
    """A ctk_stream_args that passes every check of the resident assign (the pointers are never dereferenced on the host).  `ind` is
    the first frame of the NEXT call's window; ring: 15 rows, far beyond them."""
    from cotracker_amd import _lib as L
    a = L.StreamArgs()
    a.G, a.N, a.S, a.step, a.ind, a.T_valid, a.T_cap, a.stride = 3, 10, 8, 4, (4000 if ring else 12), 0, (15 if ring else 32), 4.0
    for n in ("queries", "hist_coords", "hist_vis", "hist_conf"):
        setattr(a, n, 4096)
    for l in range(L.LEVELS):
        a.support[l], a.fmaps[l], a.H[l], a.W[l] = 4096, 8192, 16 >> l, 24 >> l
    return a


def call(lib, ring, a, slots=4096, newq=4096, M=5, rows=12):
    ref = None if a is None else C.byref(a)
    if ring:
        return lib.ctk_stream_assign_resident_ring(ref, slots, newq, M, None)
    return lib.ctk_stream_assign_resident(ref, slots, newq, M, rows, None)


def test_binding_export_and_abi(lib):
    from cotracker_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "ctk.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in L.SYMBOLS and hasattr(lib, name), name
        assert re.search(rf"\bint {name}\(", header), name
        assert any(ln.split()[-1] == name and " T " in ln for ln in nm.splitlines()), name
    assert L.SYMBOLS[NEW[0]][1] == L.SYMBOLS["ctk_stream_assign"][1] and L.SYMBOLS[NEW[1]][1] == L.SYMBOLS["ctk_stream_assign_ring"][1]
    assert lib.ctk_abi_version() == L.ABI_VERSION == 9  # additive
    assert int(header_layout()["sizeof"]["ctk_stream_args"]) == C.sizeof(L.StreamArgs) == 200  # the struct did not grow
    assert "ctk_stream_assign_resident" in header.split("#define CTK_ABI_VERSION")[0]  # the ABI history names the addition


@pytest.mark.parametrize("ring", [False, True], ids=["linear", "ring"])
def test_argument_validation_without_gpu(lib, ring):
    """Every refusal comes back before any launch (this machine may have no GPU at all: a launch would be a hipError_t > 0)."""
    assert call(lib, ring, None) == E_NULL
    assert call(lib, ring, good_args(ring), slots=None) == E_NULL
    assert call(lib, ring, good_args(ring), newq=None) == E_NULL
    for n in ("queries", "hist_coords", "hist_vis", "hist_conf"):
        a = good_args(ring)
        setattr(a, n, None)
        assert call(lib, ring, a) == E_NULL, n
    for l in range(4):
        for field in ("support", "fmaps"):
            a = good_args(ring)
            getattr(a, field)[l] = None
            assert call(lib, ring, a) == E_NULL, (field, l)
        a = good_args(ring)
        a.support[l] = 4096 + 8  # the accumulators are cleared with 16-byte stores
        assert call(lib, ring, a) == E_SHAPE, l
        for field in ("H", "W"):
            for v in (0, -3):
                a = good_args(ring)
                getattr(a, field)[l] = v
                assert call(lib, ring, a) == E_SHAPE, (field, l, v)
    a = good_args(ring)
    a.ind = 0  # no window has been tracked: nothing is resident
    assert call(lib, ring, a) == E_SHAPE
    a.ind = a.step  # the first admissible one
    assert a.ind + a.S <= a.T_cap or ring
    for M in (0, -1, 31, 2 ** 31 - 1):  # G*N = 30
        assert call(lib, ring, good_args(ring), M=M) == E_SHAPE, M
    if not ring:
        for rows in (-1, 33, 2 ** 31 - 1):  # T_cap = 32
            assert call(lib, ring, good_args(), rows=rows) == E_SHAPE, rows
        a = good_args()
        a.T_cap = a.ind + a.S - 1  # the carry rows [ind, ind + S - step) and the window behind them must fit
        assert call(lib, ring, a, rows=0) == E_SHAPE
    # what check_common refuses
    cap = (7, 0, -1)
    for field, values in (("G", (0, -1)), ("N", (0, -3)), ("S", (0, -8)), ("step", (0, -4, 8, 9)), ("ind", (-4, 2, 5, 13)),
                          ("T_cap", cap), ("stride", (0.0, -4.0, float("nan"), float("inf")))):
        for v in values:
            a = good_args(ring)
            setattr(a, field, v)
            assert call(lib, ring, a, rows=0) == E_SHAPE, (field, v)
    if ring:  # the ring's own limits: g rides on a grid axis, ind + S stays inside the 32-bit frame arithmetic
        a = good_args(True)
        a.G = 65536
        assert call(lib, True, a) == E_SHAPE
        a = good_args(True)
        a.ind = 2 ** 30
        assert call(lib, True, a) == E_SHAPE


def test_host_layers_refuse_without_a_device():
    from cotracker_amd import ops
    from cotracker_amd.build_cotracker import build_cotracker
    from cotracker_amd.model import CoTrackerThreeOnline
    from cotracker_amd.predictor import CoTrackerOnlinePredictor

    class Fake:
        G, N, S, step, T_cap, committed, next_ind, closed, ring_rows = 2, 5, 8, 4, 32, 16, 12, False, None
        queries = torch.zeros(10, 3)
    ok = torch.tensor([[9.0, 1.0, 2.0]])
    with pytest.raises(ValueError, match=r"\[8, 16\)"):  # the message names the resident frames
        ops.StreamGroups.assign(Fake(), [1], torch.tensor([[7.9, 0.0, 0.0]]), resident=True)
    for f in (7.99, 4.0, 0.0, -0.5):  # truncated toward zero, like the kernels' (long) cast
        with pytest.raises(ValueError, match=r"\[8, 16\)"):
            ops.StreamGroups.assign(Fake(), [1, 2], torch.tensor([[12.0, 0.0, 0.0], [f, 0.0, 0.0]]), resident=True)
    with pytest.raises(ValueError, match="left the stream"):  # the caller's rule still applies when given
        ops.StreamGroups.assign(Fake(), [1], ok, min_frame=10, resident=True)
    with pytest.raises(ValueError, match="not finite"):
        ops.StreamGroups.assign(Fake(), [1], torch.tensor([[float("nan"), 0.0, 0.0]]), resident=True)
    with pytest.raises(ValueError, match="twice"):
        ops.StreamGroups.assign(Fake(), [3, 3], ok.expand(2, 3), resident=True)
    closed = Fake()
    closed.closed = True
    with pytest.raises(RuntimeError, match="ended the stream"):
        ops.StreamGroups.assign(closed, [1], ok, resident=True)
    early = Fake()
    early.next_ind = 0
    with pytest.raises(RuntimeError, match="tracked window"):
        ops.StreamGroups.assign(early, [1], ok, resident=True)
    assert ops.StreamGroups.resident_frames.fget(Fake()) == (8, 16) and ops.StreamGroups.resident_frames.fget(early) is None

    m = CoTrackerThreeOnline(window_len=8, model_resolution=(64, 96))
    m.stream_slots = True
    m.init_video_online_processing()
    with pytest.raises(RuntimeError, match="no stream is running"):
        m.stream_assign([0], ok, resident=True)
    with pytest.raises(RuntimeError, match="no stream is running"):
        m.stream_resident_frames
    v2 = build_cotracker(None, v2=True, window_len=8)
    with pytest.raises(NotImplementedError, match="stream_assign"):
        v2.stream_assign([0], ok, resident=True)
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=8)
    with pytest.raises(RuntimeError):
        p.resident_frames
    import inspect
    assert inspect.signature(p.add_queries).parameters["resident"].default is False
    assert inspect.signature(m.stream_assign).parameters["resident"].default is False
