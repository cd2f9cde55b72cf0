"""Slots of a running stream, the part that needs no GPU: ctk_stream_assign is bound and exported without an ABI bump, validates
its arguments before touching the device, the host switch `stream_slots` behaves like the other opt-in attributes, and the frame
rule of an assign (frame >= ind + step, ind the first frame of the next call's window) admits exactly the frames that one later
call samples and begins from their query."""
import copy
import ctypes as C
import pickle
import subprocess

import numpy as np
import pytest
import torch

from ctk_support import header_layout, lib  # noqa: F401

E_NULL, E_SHAPE = -1, -2


def good_args():
    """A ctk_stream_args that passes every check (the pointers are never dereferenced on the host)."""
    from cotracker_amd import _lib as L
    a = L.StreamArgs()
    a.G, a.N, a.S, a.step, a.ind, a.T_valid, a.T_cap, a.stride = 3, 10, 8, 4, 0, 0, 32, 4.0
    for n in ("queries", "hist_coords", "hist_vis", "hist_conf"):
        setattr(a, n, 4096)
    for l in range(L.LEVELS):
        a.support[l] = 4096
    return a


def assign(lib, a, slots=4096, newq=4096, M=5, rows=12):
    return lib.ctk_stream_assign(None if a is None else C.byref(a), slots, newq, M, rows, None)


def test_binding_export_and_abi(lib):
    from cotracker_amd import _lib as L
    assert "ctk_stream_assign" in L.SYMBOLS and hasattr(lib, "ctk_stream_assign")
    assert lib.ctk_abi_version() == L.ABI_VERSION == 9  # additive
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(ln.split()[-1] == "ctk_stream_assign" and " T " in ln for ln in nm.splitlines())
    lay = header_layout()
    size, empty, as_long = lay["sizeof"]["ctk_stream_args"], lay["constants"]["CTK_STREAM_EMPTY_FRAME"], lay["as_long"]["CTK_STREAM_EMPTY_FRAME"]
    assert int(size) == C.sizeof(L.StreamArgs) == 200  # the struct did not grow
    assert float(empty) == L.STREAM_EMPTY_FRAME == 2.0 ** 30 and int(as_long) == 2 ** 30


def test_argument_validation_without_gpu(lib):
    """Every refusal comes back before any launch (this machine may have no GPU at all: a launch would be a hipError_t > 0)."""
    assert assign(lib, None) == E_NULL
    assert assign(lib, good_args(), slots=None) == E_NULL
    assert assign(lib, good_args(), newq=None) == E_NULL
    for n in ("queries", "hist_coords", "hist_vis", "hist_conf"):
        a = good_args()
        setattr(a, n, None)
        assert assign(lib, a) == E_NULL, n
    for l in range(4):
        a = good_args()
        a.support[l] = None
        assert assign(lib, a) == E_NULL, l
        a = good_args()
        a.support[l] = 4096 + 8  # the accumulators are cleared with 16-byte stores
        assert assign(lib, a) == E_SHAPE, l
    for M in (0, -1, 31, 2 ** 31 - 1):  # G*N = 30
        assert assign(lib, good_args(), M=M) == E_SHAPE, M
    for rows in (-1, 33, 2 ** 31 - 1):  # T_cap = 32
        assert assign(lib, good_args(), rows=rows) == E_SHAPE, rows
    # what check_common refuses for the three step calls
    for field, values in (("G", (0, -1)), ("N", (0, -3)), ("S", (0, -8)), ("step", (0, -4, 8, 9)), ("ind", (-4, 2, 5)),
                          ("T_cap", (7, 0, -1)), ("stride", (0.0, -4.0, float("nan"), float("inf")))):
        for v in values:
            a = good_args()
            setattr(a, field, v)
            assert assign(lib, a, rows=0) == E_SHAPE, (field, v)


def test_host_switch():
    from cotracker_amd.build_cotracker import build_cotracker
    from cotracker_amd.model import CoTrackerThreeOnline
    m = CoTrackerThreeOnline(window_len=8, model_resolution=(64, 96))
    assert m.stream_slots is False and copy.deepcopy(m).stream_slots is False
    with pytest.raises(RuntimeError, match="stream_slots is off"):
        m.stream_assign([0], torch.tensor([[8.0, 1.0, 1.0]]))
    with pytest.raises(RuntimeError, match="stream_slots is off"):
        m.stream_release([0])
    m.stream_slots = True
    assert copy.deepcopy(m).stream_slots is True and pickle.loads(pickle.dumps(m)).stream_slots is True
    assert m.stream_groups is False  # an independent switch
    m.init_video_online_processing()
    with pytest.raises(RuntimeError, match="no stream is running"):
        m.stream_assign([0], torch.tensor([[8.0, 1.0, 1.0]]))
    with pytest.raises(RuntimeError, match="no stream is running"):
        m.stream_occupied
    v2 = build_cotracker(None, v2=True, window_len=8)
    assert v2.stream_slots is False
    with pytest.raises(NotImplementedError, match="stream_slots"):
        v2.stream_slots = True
    v2.stream_slots = False
    assert v2.stream_slots is False


def test_predictor_keeps_the_reference_signature_and_refuses_spare_points_on_v2():
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=8)
    assert p.spare_points == 0 and p.model.stream_slots is False
    p2 = CoTrackerOnlinePredictor(checkpoint=None, v2=True, window_len=8)
    p2.spare_points = 4
    with pytest.raises(NotImplementedError, match="spare_points"):
        p2._with_spare(torch.zeros(1, 3, 3))


def test_empty_frame_is_exact_and_beyond_every_window():
    from cotracker_amd import ops
    e = ops.EMPTY_FRAME
    assert float(np.float32(e)) == e == 2.0 ** 30 and np.isfinite(np.float32(e))
    t = torch.tensor([e], dtype=torch.float32)
    assert int(t.long()) == 2 ** 30 and int(np.float32(e)) == 2 ** 30
    # never below ind + S, never inside [left, right): for every ind a float32 frame number expresses exactly (< 2^24) -- and
    # any S a window has
    for S in (2, 8, 16, 64, 4096):
        for ind in (0, S // 2, 1000 * (S // 2), (2 ** 24 // max(S // 2, 1)) * (S // 2)):
            assert not int(t.long()) < ind + S
            left, right = (0 if ind == 0 else ind + S // 2), ind + S
            assert not (left <= int(t.long()) < right)
            assert not (ind > 0 and int(t.long()) < ind + S - S // 2)  # begin: never carried over, starts from its (0, 0)


@pytest.mark.parametrize("S,step", [(8, 4), (16, 8)])
def test_frame_rule_admits_exactly_the_frames_one_later_call_samples(S, step):
    """An assign before the call at `ind` admits trunc(f) >= ind + step.  Per element, against the [left, right) ranges of the
    calls that follow (tests/test_stream_groups_cabi.py: the ranges partition the frames): an admitted frame is sampled by exactly
    one later call, and in that call -- and every call before it -- begin takes the point from its query (no carry-over of a
    previous occupant's history); a refused frame is sampled by no later call."""
    calls = [k * step for k in range(14)]
    for k_assign in range(1, 8):
        ind = calls[k_assign]  # model.online_ind when the assign happens: the first frame of the next call's window
        left_rule = ind + step
        for f in np.arange(0, calls[-1] + S, 0.5, dtype=np.float32):
            qf = int(torch.tensor([f]).long())
            admitted = qf >= left_rule
            hits, begins_from_query = [], True
            for later in calls[k_assign:]:
                left, right = (0 if later == 0 else later + step), later + S
                sampled = left <= qf < right
                if sampled:
                    hits.append(later)
                carried = later > 0 and qf < later + S - step  # begin_rule: history rows instead of the query
                if not hits or sampled:
                    begins_from_query &= not carried
            if admitted:
                assert len(hits) == 1 and begins_from_query, (ind, float(f), hits)
                assert int(qf < hits[0] + S) == 1  # point_mask goes up in the call that samples it
            else:
                assert hits == [], (ind, float(f), hits)


def test_host_checks_of_assign_need_no_device():
    """ops.StreamGroups.assign refuses on the host before anything is enqueued (a stand-in object: no device memory)."""
    from cotracker_amd import ops

    class Fake:
        G, N, T_cap, committed, next_ind = 2, 5, 32, 12, 8
        queries = torch.zeros(10, 3)
    ok = torch.tensor([[20.0, 1.0, 2.0]])
    for slots, q, kw, msg in (([], ok, {}, "non-empty"), ([0.5], ok, {}, "non-empty"), ([10], ok, {}, "outside"), ([-1], ok, {}, "outside"),
                              ([3, 3], ok.expand(2, 3), {}, "twice"), ([1], ok.expand(2, 3), {}, r"\[1,3\]"),
                              ([1], torch.zeros(1, 2), {}, r"\[1,3\]"), ([1], ok, {"rows": 33}, "rows"), ([1], ok, {"rows": -1}, "rows"),
                              ([1], torch.tensor([[float("nan"), 0.0, 0.0]]), {}, "not finite"),
                              ([1], torch.tensor([[float("inf"), 0.0, 0.0]]), {}, "not finite"),
                              ([1], torch.tensor([[11.9, 0.0, 0.0]]), {"min_frame": 12}, "left the stream")):
        with pytest.raises(ValueError, match=msg):
            ops.StreamGroups.assign(Fake(), slots, q, **kw)
