"""Streaming query groups, the part that needs no GPU: the three stream entry points of include/ctk.h (ctk_stream_begin /
ctk_stream_support / ctk_stream_commit) validate their arguments before touching the device, ctk_stream_args has the size the C
compiler gives it, the host switch `stream_groups` behaves like the other opt-in attributes, and the index rules the kernels
implement (per point and window row) are the reference's tensor expressions (cotracker3_online.py:411-414, 457-484, 498-510)."""
import copy
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

from ctk_support import header_layout, lib  # noqa: F401

E_NULL, E_SHAPE = -1, -2


def good_args():
    """A ctk_stream_args that passes every check (the pointers are never dereferenced on the host)."""
    from cotracker_amd import _lib as L
    a = L.StreamArgs()
    a.G, a.N, a.S, a.step, a.ind, a.T_valid, a.T_cap, a.stride = 3, 10, 8, 4, 4, 8, 32, 4.0
    for n in ("queries", "hist_coords", "hist_vis", "hist_conf", "coords", "vis", "conf", "point_mask", "nonfinite"):
        setattr(a, n, 4096)
    for l in range(L.LEVELS):
        a.H[l], a.W[l], a.fmaps[l], a.support[l] = 16 >> l, 24 >> l, 4096, 4096
    return a


def test_binding_has_the_stream_entry_points(lib):
    from cotracker_amd import _lib as L
    for name in ("ctk_stream_begin", "ctk_stream_support", "ctk_stream_commit"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert lib.ctk_abi_version() == 9  # additive


def test_struct_size_matches_the_header():
    from cotracker_amd import _lib as L
    lay = header_layout()
    size, (o_stride, o_h, o_flag) = lay["sizeof"]["ctk_stream_args"], (lay["offsetof"]["ctk_stream_args"][f] for f in ("stride", "H", "nonfinite"))
    assert C.sizeof(L.StreamArgs) == size == 200
    assert (L.StreamArgs.stride.offset, L.StreamArgs.H.offset, L.StreamArgs.nonfinite.offset) == (o_stride, o_h, o_flag)


@pytest.mark.parametrize("entry", ["ctk_stream_begin", "ctk_stream_support", "ctk_stream_commit"])
def test_argument_validation_without_gpu(lib, entry):
    """Every refusal comes back before any launch (this machine may have no GPU at all: a launch would be a hipError_t > 0)."""
    fn = getattr(lib, entry)
    assert fn(None, None) == E_NULL
    for field, values in (("G", (0, -1)), ("N", (0, -3)), ("S", (0, -8)), ("step", (0, -4, 8, 9)), ("ind", (-4, 2, 5)),
                          ("T_cap", (11, 0, -1)), ("stride", (0.0, -4.0, float("nan"), float("inf")))):
        for v in values:
            a = good_args()
            setattr(a, field, v)
            assert fn(C.byref(a), None) == E_SHAPE, (entry, field, v)
    a = good_args()
    a.ind, a.T_cap = 28, 35  # T_cap < ind + S
    assert fn(C.byref(a), None) == E_SHAPE
    used = {"ctk_stream_begin": ("queries", "hist_coords", "hist_vis", "hist_conf", "coords", "vis", "conf", "point_mask"),
            "ctk_stream_support": ("queries",),
            "ctk_stream_commit": ("hist_coords", "hist_vis", "hist_conf", "coords", "vis", "conf")}[entry]
    for n in used:
        a = good_args()
        setattr(a, n, None)
        assert fn(C.byref(a), None) == E_NULL, (entry, n)


def test_support_and_commit_specific_validation(lib):
    for l in range(4):
        for field in ("fmaps", "support"):
            a = good_args()
            getattr(a, field)[l] = None
            assert lib.ctk_stream_support(C.byref(a), None) == E_NULL
        for field in ("H", "W"):
            a = good_args()
            getattr(a, field)[l] = 0
            assert lib.ctk_stream_support(C.byref(a), None) == E_SHAPE
    for t in (0, -1, 9):
        a = good_args()
        a.T_valid = t
        assert lib.ctk_stream_commit(C.byref(a), None) == E_SHAPE


def test_host_switch():
    from cotracker_amd.build_cotracker import build_cotracker
    from cotracker_amd.model import CoTrackerThreeOnline
    m = CoTrackerThreeOnline(window_len=8, model_resolution=(64, 96))
    assert m.stream_groups is False
    assert copy.deepcopy(m).stream_groups is False
    m.stream_groups = True
    assert copy.deepcopy(m).stream_groups is True and pickle.loads(pickle.dumps(m)).stream_groups is True
    v2 = build_cotracker(None, v2=True, window_len=8)
    assert v2.stream_groups is False
    with pytest.raises(NotImplementedError, match="stream_groups"):
        v2.stream_groups = True
    v2.stream_groups = False
    assert v2.stream_groups is False


# ----------------------------------------------------------------------------------------------------------------------
# the index rules of the kernels (restated per element in numpy) against the reference's tensor expressions (torch, CPU)
# ----------------------------------------------------------------------------------------------------------------------
def begin_rule(queries, hist, ind, S, step, stride):
    """What stream_begin_kernel writes: per (t, n).  hist = (coords [T,N,2], vis [T,N], conf [T,N])."""
    N = queries.shape[0]
    ov = S - step
    inv = np.float32(1.0) / np.float32(stride)
    coords, vis, conf = np.zeros((S, N, 2), np.float32), np.zeros((S, N), np.float32), np.zeros((S, N), np.float32)
    mask = np.zeros(N, np.uint8)
    for n in range(N):
        qf = int(queries[n, 0])
        mask[n] = qf < ind + S
        for t in range(S):
            if ind > 0 and qf < ind + ov:
                row = ind + min(t, ov - 1)
                coords[t, n], vis[t, n], conf[t, n] = hist[0][row, n] * inv, hist[1][row, n], hist[2][row, n]
            else:
                coords[t, n] = queries[n, 1:3] * inv
    return coords, vis, conf, mask


def begin_reference(queries, hist, ind, S, step, stride):
    """cotracker3_online.py:333-336, 442-445, 457-484 on one query set."""
    q = torch.from_numpy(queries)
    qframes, qcoords = q[:, 0].long(), q[:, 1:3] / stride
    N = q.shape[0]
    coords_init = qcoords[None].expand(S, N, 2)
    vis_init, conf_init = torch.zeros(S, N), torch.zeros(S, N)
    if ind > 0:
        overlap = S - step
        copy_over = (qframes < ind + overlap)[None, :]
        c, v, f = (torch.from_numpy(h)[ind:ind + overlap] for h in hist)
        c = torch.cat([c / stride, (c / stride)[-1:].expand(step, -1, -1)], dim=0)
        v = torch.cat([v, v[-1:].expand(step, -1)], dim=0)
        f = torch.cat([f, f[-1:].expand(step, -1)], dim=0)
        coords_init = torch.where(copy_over[..., None], c, coords_init)
        vis_init, conf_init = torch.where(copy_over, v, vis_init), torch.where(copy_over, f, conf_init)
    return coords_init.numpy(), vis_init.numpy(), conf_init.numpy(), (qframes < ind + S).to(torch.uint8).numpy()


def edge_queries(r, ind, S, step, n_random=40):
    """Random query frames plus the edges: frame 0, exactly ind + S - step, ind + S - 1, ind + S, and their neighbours."""
    frames = [0, ind + S - step - 1, ind + S - step, ind + S - 1, ind + S, ind + S + 1, max(ind - 1, 0), ind, ind + step - 1,
              ind + step] + list(r.randint(0, ind + 2 * S, size=n_random))
    q = np.zeros((len(frames), 3), np.float32)
    q[:, 0] = frames
    q[:, 1:] = r.uniform(0, 90, size=(len(frames), 2))
    return q


@pytest.mark.parametrize("S,step", [(8, 4), (16, 8), (6, 3)])
def test_begin_rule_is_the_reference_expression(S, step):
    r = np.random.RandomState(S)
    for ind in (0, step, 3 * step):
        q = edge_queries(r, ind, S, step)
        N, T = q.shape[0], ind + S
        hist = (r.standard_normal((T, N, 2)).astype(np.float32) * 50, r.standard_normal((T, N)).astype(np.float32),
                r.standard_normal((T, N)).astype(np.float32))
        for got, ref in zip(begin_rule(q, hist, ind, S, step, 4), begin_reference(q, hist, ind, S, step, 4)):
            assert np.array_equal(got, ref), (ind, np.abs(got.astype(np.float64) - ref).max())


@pytest.mark.parametrize("S,step", [(8, 4), (16, 8)])
def test_support_ranges_partition_the_query_frames(S, step):
    """The kernel samples a point when left <= qframe < right (left = 0 at ind == 0, else ind + step; right = ind + S): the
    reference's sample mask (:411-414).  Over a stream the ranges are disjoint and cover every frame once."""
    hits = np.zeros(10 * step + S, int)
    for ind in range(0, 10 * step, step):
        left, right = (0 if ind == 0 else ind + step), ind + S
        qframes = torch.arange(hits.size)
        ref = ((qframes >= left) & (qframes < right)).numpy()  # the reference expression
        mine = np.array([left <= int(f) < right for f in range(hits.size)])
        assert np.array_equal(ref, mine)
        hits += mine
    assert (hits[:9 * step + S] == 1).all()


@pytest.mark.parametrize("T_valid", [8, 5, 4, 1])
def test_commit_rule_is_the_reference_write_back(T_valid):
    """History rows ind .. ind+T_valid-1 = (coords * stride, vis, conf)[:T_valid]; the history a stream returns has ind + T rows
    (cotracker3_online.py:349-360 pads by min(step, T - step) rows, :498-510 writes the window back) -- T_valid < S: a short last
    chunk."""
    import torch.nn.functional as F
    S, step, N, ind, stride = 8, 4, 7, 8, 4
    r = np.random.RandomState(T_valid)
    prev = torch.from_numpy(r.standard_normal((ind - step + S, N, 2)).astype(np.float32))  # what the previous call left
    coords = torch.from_numpy(r.standard_normal((S, N, 2)).astype(np.float32))
    ref = F.pad(prev, (0, 0, 0, 0, 0, min(step, T_valid - step)))
    ref[ind:ind + S] = (coords * float(stride))[:T_valid]
    cap = torch.zeros(32, N, 2)
    cap[:prev.shape[0]] = prev
    for t in range(T_valid):  # the kernel's rule, per row
        cap[ind + t] = coords[t] * np.float32(stride)
    assert ref.shape[0] == ind + T_valid
    assert torch.equal(cap[:ind + T_valid], ref)
