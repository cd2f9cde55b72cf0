"""Query groups over one video (ctk_window_batch.flags = CTK_BATCH_SHARED_FMAPS, model(video[1], queries[G])): everything that can
be checked without a GPU -- the flag in header / binding / library, struct sizes against the C compiler, argument validation
before any HIP call, the workspace saving, the host-side switches."""
import ctypes as C
import os
import re

import pytest

from ctk_support import ROOT, header_layout, lib  # noqa: F401

S, N = 16, 100
BASE = 1 << 20  # fake device addresses: validation never dereferences them


def _groups(B, flags=None, mask=False):
    """B query groups laid out as the flag demands: the same fmaps, state / support / mask one group behind the other."""
    from cotracker_amd import _lib as L
    arr = (L.WindowArgs * B)()
    for b, a in enumerate(arr):
        a.S, a.N, a.iters = S, N, 6
        a.scale_x, a.scale_y = 128.0, 96.0
        for l in range(L.LEVELS):
            a.H[l], a.W[l] = 96 >> l, 128 >> l
            a.fmaps[l] = BASE * (1 + l)
            a.support[l] = BASE * (8 + l) + b * N * 49 * 128 * 4
        a.coords = BASE * 16 + b * S * N * 2 * 4
        a.vis = BASE * 17 + b * S * N * 4
        a.conf = BASE * 18 + b * S * N * 4
        a.point_mask = BASE * 19 + b * N if mask else None
    return arr, L.WindowBatch(B, L.BATCH_SHARED_FMAPS if flags is None else flags, C.cast(arr, C.POINTER(L.WindowArgs)))


def test_flag_in_header_binding_and_library(lib):
    from cotracker_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "ctk.h")).read()
    m = re.search(r"#define CTK_BATCH_SHARED_FMAPS (\d+)\b", header)
    assert m and int(m.group(1)) == L.BATCH_SHARED_FMAPS == 1
    assert re.search(r"int32_t flags;\s*/\* 0 or CTK_BATCH_SHARED_FMAPS", header)
    assert [f[0] for f in L.WindowBatch._fields_] == ["B", "flags", "videos"]
    for name in ("ctk_corr_embed_batch_workspace_bytes", "ctk_corr_embed_batch"):
        assert re.search(rf"\bint {name}\(", header) and name in L.SYMBOLS and getattr(lib, name) is not None
    assert lib.ctk_abi_version() == 9 and re.search(r"#define CTK_ABI_VERSION 9\b", header)  # additive
    # the struct keeps its size and the flag sits where `reserved` sat
    lay = header_layout()
    out = [lay["sizeof"]["ctk_window_batch"], lay["offsetof"]["ctk_window_batch"]["flags"], lay["offsetof"]["ctk_window_batch"]["videos"],
           lay["constants"]["CTK_BATCH_SHARED_FMAPS"]]
    assert out == [16, 4, 8, 1]
    assert C.sizeof(L.WindowBatch) == 16 and L.WindowBatch.flags.offset == 4 and L.WindowBatch.videos.offset == 8


def test_shared_batch_validation_without_gpu(lib):
    """A malformed query-group batch is refused before any HIP call (without a GPU a HIP call would return a positive
    hipError_t instead)."""
    n = C.c_size_t(0)
    q = lib.ctk_forward_window_batch_workspace_bytes
    arr, b = _groups(4)
    assert q(C.byref(b), C.byref(n)) == 0 and n.value > 0
    arr, b = _groups(4, mask=True)
    assert q(C.byref(b), C.byref(n)) == 0
    for bad in (2, 3, 4, 1 << 16, -1):  # unknown flag bits
        arr, b = _groups(2, flags=bad)
        assert q(C.byref(b), C.byref(n)) == -2, bad

    def refused(mutate, code, mask=False, B=3):
        arr, b = _groups(B, mask=mask)
        mutate(arr[B - 1])
        rc = [q(C.byref(b), C.byref(n)), lib.ctk_corr_embed_batch_workspace_bytes(C.byref(b), C.byref(n)),
              lib.ctk_forward_window_batch(C.byref(b), None, None, 0, None)]
        h = C.c_void_p()
        rc.append(lib.ctk_window_batch_graph_create(C.byref(b), None, None, 0, C.byref(h)))
        rc.append(lib.ctk_corr_embed_batch(C.byref(b), None, None, None, 0, None))
        return rc == [code] * 5 and not h.value

    assert refused(lambda a: a.fmaps.__setitem__(2, BASE * 3 + 512), -2)           # a group with its own pyramid level
    assert refused(lambda a: setattr(a, "coords", a.coords + 8), -2)               # groups not equally strided
    assert refused(lambda a: setattr(a, "vis", a.vis - 4), -2)
    assert refused(lambda a: setattr(a, "conf", BASE * 40), -2)
    assert refused(lambda a: a.support.__setitem__(0, a.support[0] + 49 * 128 * 4), -2)
    assert refused(lambda a: setattr(a, "point_mask", a.point_mask + 1), -2, mask=True)
    assert refused(lambda a: setattr(a, "coords", None), -1)
    assert refused(lambda a: a.support.__setitem__(3, None), -1)
    assert refused(lambda a: setattr(a, "N", N + 1), -2)                           # (the joint-batch rules still hold)
    # the same three windows are a legal UNSHARED batch whatever their pointers are
    arr, b = _groups(3, flags=0)
    arr[2].coords += 8
    assert q(C.byref(b), C.byref(n)) == 0


def test_shared_workspace_is_smaller(lib):
    q = lib.ctk_forward_window_batch_workspace_bytes
    sizes = {}
    for B in (1, 4):
        for flags in (0, 1):
            arr, b = _groups(B, flags=flags)
            n = C.c_size_t(0)
            assert q(C.byref(b), C.byref(n)) == 0
            sizes[B, flags] = n.value
    assert sizes[1, 1] == sizes[1, 0]
    pyramid = sum(S * (96 >> l) * (128 >> l) * 128 * 4 for l in range(4))  # one split-half copy: the bytes of the f32 pyramid
    assert sizes[4, 0] - sizes[4, 1] == 3 * pyramid
    one = C.c_size_t(0)
    assert lib.ctk_forward_window_workspace_bytes(C.byref(arr[0]), C.byref(one)) == 0 and sizes[1, 1] == one.value
    # corr_embed on its own: B == 1 is the single window's workspace, shared saves the same three copies
    ce = {}
    for flags in (0, 1):
        arr, b = _groups(4, flags=flags)
        n = C.c_size_t(0)
        assert lib.ctk_corr_embed_batch_workspace_bytes(C.byref(b), C.byref(n)) == 0
        ce[flags] = n.value
    assert ce[0] - ce[1] == 3 * pyramid


def test_host_switches():
    """The two consumers opt in through attributes set after construction; the defaults are today's calls."""
    from cotracker_amd.build_cotracker import build_cotracker
    from cotracker_amd.evaluation import EvaluationPredictor
    from cotracker_amd.model import CoTrackerThreeOffline
    from cotracker_amd.predictor import CoTrackerPredictor
    ev = EvaluationPredictor(CoTrackerThreeOffline(window_len=8))
    assert ev.query_group == 1 and CoTrackerPredictor.dense_chunks_per_call == 1
    ev.query_group = 4
    assert ev.query_group == 4 and EvaluationPredictor.query_group == 1
    v2 = build_cotracker(None, v2=True, window_len=8)
    with pytest.raises(NotImplementedError):  # query groups on a CoTracker2 model run on the loop only
        v2.batch_mode = "joint"
