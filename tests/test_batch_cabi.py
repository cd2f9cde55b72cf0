"""Joint batch mode (ctk_forward_window_batch, batch_mode = "joint"): everything that can be checked without a GPU --
the new symbols, struct sizes against the C compiler, argument validation before any HIP call, the host-side switches."""
import ctypes as C
import os
import re

import pytest

from ctk_support import ROOT, header_layout, lib  # noqa: F401

NEW_SYMBOLS = ("ctk_forward_window_batch_workspace_bytes", "ctk_forward_window_batch", "ctk_window_batch_graph_create",
               "ctk_attention_ex")


def _batch(B, S=16, N=100, iters=6):
    from cotracker_amd import _lib as L
    arr = (L.WindowArgs * max(B, 1))()
    for a in arr:
        a.S, a.N, a.iters = S, N, iters
        a.scale_x, a.scale_y = 128.0, 96.0
        for l in range(L.LEVELS):
            a.H[l], a.W[l] = 96 >> l, 128 >> l
    return arr, L.WindowBatch(B, 0, C.cast(arr, C.POINTER(L.WindowArgs)))


def test_new_symbols_are_declared_bound_and_exported(lib):
    from cotracker_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "ctk.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in L.SYMBOLS
        assert getattr(lib, name) is not None
    assert re.search(r"#define CTK_MAX_BATCH 16\b", header) and L.MAX_BATCH == 16
    assert lib.ctk_abi_version() == 9  # additive: no existing struct or symbol changed


def test_batch_struct_sizes_match_header():
    from cotracker_amd import _lib as L
    pairs = {"ctk_window_batch": L.WindowBatch, "ctk_attn_batch2": L.AttnBatch2, "ctk_attn_args": L.AttnArgs,
             "ctk_window_args": L.WindowArgs}
    out = header_layout()["sizeof"]
    for n, cls in pairs.items():
        assert C.sizeof(cls) == int(out[n]), (n, C.sizeof(cls), out[n])
    assert C.sizeof(L.WindowBatch) == 16 and C.sizeof(L.AttnBatch2) == 48


def test_batch_argument_validation_without_gpu(lib):
    """Every malformed batch is refused with the right code before any HIP call (without a GPU a HIP call would return a
    positive hipError_t instead)."""
    n = C.c_size_t(0)
    q = lib.ctk_forward_window_batch_workspace_bytes
    assert q(None, C.byref(n)) == -1
    arr, b = _batch(2)
    assert q(C.byref(b), None) == -1
    assert q(C.byref(b), C.byref(n)) == 0 and n.value > 0
    two = n.value
    for bad in (0, -1, 17):
        b.B = bad
        assert q(C.byref(b), C.byref(n)) == -2, bad
    b.B = 16
    assert q(C.byref(b.__class__(16, 0, None)), C.byref(n)) == -1  # NULL videos
    # B == 1 needs exactly the single window's workspace
    arr1, b1 = _batch(1)
    one = C.c_size_t(0)
    assert q(C.byref(b1), C.byref(n)) == 0
    assert lib.ctk_forward_window_workspace_bytes(C.byref(arr1[0]), C.byref(one)) == 0 and one.value == n.value
    assert one.value < two <= 2 * one.value

    def refused(mutate, code):
        arr, b = _batch(3)
        mutate(arr[2])
        return q(C.byref(b), C.byref(n)) == code

    assert refused(lambda a: setattr(a, "N", 101), -2)
    assert refused(lambda a: setattr(a, "S", 8), -2)
    assert refused(lambda a: setattr(a, "iters", 4), -2)
    assert refused(lambda a: setattr(a, "flags", 1), -2)
    assert refused(lambda a: setattr(a, "flags", 2), -2)          # unknown bit in one video
    assert refused(lambda a: setattr(a, "scale_x", 64.0), -2)
    assert refused(lambda a: a.H.__setitem__(1, 47), -2)
    assert refused(lambda a: setattr(a, "point_mask", 256), -1)   # mask given for one video only

    # the run and capture entry points validate the same way, before the weights, the workspace or the device are touched
    arr, b = _batch(2)
    h = C.c_void_p()
    assert lib.ctk_forward_window_batch(None, None, None, 0, None) == -1
    assert lib.ctk_forward_window_batch(C.byref(b), None, None, 0, None) == -1          # weights NULL
    assert lib.ctk_window_batch_graph_create(C.byref(b), None, None, 0, C.byref(h)) == -1 and not h.value
    assert lib.ctk_window_batch_graph_create(C.byref(b), None, None, 0, None) == -1
    arr[1].N = 7
    assert lib.ctk_forward_window_batch(C.byref(b), None, None, 0, None) == -2          # shape first
    assert lib.ctk_window_batch_graph_create(C.byref(b), None, None, 0, C.byref(h)) == -2 and not h.value
    b.B = 17
    assert lib.ctk_forward_window_batch(C.byref(b), None, None, 0, None) == -2


def test_attention_ex_argument_validation_without_gpu(lib):
    from cotracker_amd import _lib as L
    a, b2 = L.AttnArgs(), L.AttnBatch2()
    assert lib.ctk_attention_ex(None, None, None) == -1
    assert lib.ctk_attention_ex(C.byref(a), C.byref(b2), None) == -1  # NULL operands
    a.q = a.k = a.v = a.out = 256
    a.q_ld = a.kv_ld = a.o_ld = 384
    a.nbatch, a.n1, a.n2 = 6, 64, 64
    b2.inner = 4  # 6 batches are not a whole number of groups of 4
    assert lib.ctk_attention_ex(C.byref(a), C.byref(b2), None) == -2


def test_batch_mode_attribute():
    from cotracker_amd.build_cotracker import build_cotracker
    from cotracker_amd.model import CoTrackerThreeOffline, CoTrackerThreeOnline
    for cls in (CoTrackerThreeOnline, CoTrackerThreeOffline):
        m = cls(window_len=8)
        assert m.batch_mode == "loop"
        m.batch_mode = "joint"
        assert m.batch_mode == "joint"
        for bad in ("Joint", "", None, 1, "stack"):
            with pytest.raises(ValueError, match="batch_mode"):
                m.batch_mode = bad
        assert m.batch_mode == "joint"
        import copy
        assert copy.deepcopy(m).batch_mode == "joint"
    v2 = build_cotracker(None, v2=True, window_len=8)
    assert v2.batch_mode == "loop"
    v2.batch_mode = "loop"
    with pytest.raises(NotImplementedError, match='batch_mode="joint" on a v2 model'):
        v2.batch_mode = "joint"
    with pytest.raises(ValueError):
        v2.batch_mode = "stack"
    assert v2.batch_mode == "loop"


def test_option_values_cover_the_table(lib):
    """The graph cache key of the host models carries the whole option table (a captured graph bakes the options in)."""
    from cotracker_amd import _lib as L
    base = L.option_values()
    assert len(base) == L.OPT_COUNT == 7
    with L.option(L.OPT_CORR_VERSION, 1):
        assert L.option_values() != base and L.option_values()[L.OPT_CORR_VERSION] == 1
    assert L.option_values() == base
