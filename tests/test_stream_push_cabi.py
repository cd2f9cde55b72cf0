"""Pushing new frames into a live stream, the part that needs no GPU: ctk_ingest_frames is bound and exported without an ABI bump,
its argument struct has one size on both sides of the binding, every refusal comes back before the device is touched, and the host
bookkeeping of CoTrackerOnlinePredictor.push_frames -- which pushes trigger a tracking step, what `final` flushes, that a stream is
fed one way -- is driven with a stand-in model."""
import copy
import ctypes as C
import os
import pickle
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from ctk_support import ROOT, header_layout, lib  # noqa: F401

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3


def good_args(**kw):
    """A ctk_ingest_args that passes every check (the pointers are never dereferenced on the host)."""
    from cotracker_amd import _lib as L
    a = L.IngestArgs()
    a.src, a.dst = 4096, 8192
    a.dtype, a.layout = L.INGEST_U8, L.INGEST_HWC
    a.F, a.H, a.W, a.h, a.w = 8, 1080, 1920, 384, 512
    a.row_stride, a.frame_stride = 1920 * 3, 1080 * 1920 * 3
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def ingest(lib, a):
    return lib.ctk_ingest_frames(None if a is None else C.byref(a), None)


def test_binding_export_and_abi(lib):
    from cotracker_amd import _lib as L
    assert "ctk_ingest_frames" in L.SYMBOLS and hasattr(lib, "ctk_ingest_frames")
    assert lib.ctk_abi_version() == L.ABI_VERSION == 9  # additive
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(ln.split()[-1] == "ctk_ingest_frames" and " T " in ln for ln in nm.splitlines())
    header = open(os.path.join(ROOT, "include", "ctk.h")).read()
    assert re.search(r"int ctk_ingest_frames\(const ctk_ingest_args\* a, void\* stream\);", header)
    assert "predictor.py:288-290" in header  # the reference lines the entry point replaces
    lay = header_layout()
    size, (o_fs, o_rs, o_dst) = lay["sizeof"]["ctk_ingest_args"], (lay["offsetof"]["ctk_ingest_args"][f] for f in ("frame_stride", "row_stride", "dst"))
    u8, f32, hwc, chw = (lay["constants"][n] for n in ("CTK_INGEST_U8", "CTK_INGEST_F32", "CTK_INGEST_HWC", "CTK_INGEST_CHW"))
    assert size == C.sizeof(L.IngestArgs)
    assert (o_fs, o_rs, o_dst) == (L.IngestArgs.frame_stride.offset, L.IngestArgs.row_stride.offset, L.IngestArgs.dst.offset)
    assert (u8, f32, hwc, chw) == (L.INGEST_U8, L.INGEST_F32, L.INGEST_HWC, L.INGEST_CHW)
    assert C.sizeof(L.StreamArgs) == 200  # the stream struct did not change


def test_argument_validation_without_gpu(lib):
    """Every refusal comes back before any launch (this machine may have no GPU at all: a launch would be a hipError_t > 0)."""
    from cotracker_amd import _lib as L
    assert ingest(lib, None) == E_NULL
    assert ingest(lib, good_args(src=None)) == E_NULL
    assert ingest(lib, good_args(dst=None)) == E_NULL
    for field in ("F", "H", "W", "h", "w"):
        for v in (0, -1, -(2 ** 31)):
            assert ingest(lib, good_args(**{field: v})) == E_SHAPE, (field, v)
    assert ingest(lib, good_args(F=65536, frame_stride=1080 * 1920 * 3)) == E_SHAPE
    for field in ("H", "W", "h", "w"):
        assert ingest(lib, good_args(**{field: 32769}, row_stride=2 ** 30, frame_stride=2 ** 39)) == E_SHAPE, field
    for v in (-1, 2, 7):
        assert ingest(lib, good_args(dtype=v)) == E_SHAPE, v
        assert ingest(lib, good_args(layout=v)) == E_SHAPE, v
    # strides smaller than a row or a frame, in elements: channels-last rows hold 3 W elements, planar rows W, planar frames 3 H rows
    assert ingest(lib, good_args(row_stride=1920 * 3 - 1)) == E_SHAPE
    assert ingest(lib, good_args(row_stride=0)) == E_SHAPE
    assert ingest(lib, good_args(row_stride=-5760)) == E_SHAPE
    assert ingest(lib, good_args(frame_stride=1080 * 1920 * 3 - 1)) == E_SHAPE
    assert ingest(lib, good_args(frame_stride=0)) == E_SHAPE
    assert ingest(lib, good_args(row_stride=6000, frame_stride=1080 * 6000 - 1)) == E_SHAPE
    assert ingest(lib, good_args(layout=L.INGEST_CHW, row_stride=1919, frame_stride=3 * 1080 * 1920)) == E_SHAPE
    assert ingest(lib, good_args(layout=L.INGEST_CHW, row_stride=1920, frame_stride=3 * 1080 * 1920 - 1)) == E_SHAPE
    # the rows of a w % 4 == 0 destination are stored as 16-byte vectors; any other width as single floats
    assert ingest(lib, good_args(dst=8192 + 4)) == E_ALIGN
    assert ingest(lib, good_args(dst=8192 + 8)) == E_ALIGN
    assert ingest(lib, good_args(dst=8192 + 2, w=511)) == E_ALIGN
    assert ingest(lib, good_args(dtype=L.INGEST_F32, src=4096 + 2)) == E_ALIGN


def test_ops_front_end_refuses_on_the_host():
    from cotracker_amd import ops
    out = torch.empty(2, 3, 8, 12)
    with pytest.raises(ValueError, match="device tensor"):
        ops.ingest_frames(torch.zeros(2, 16, 24, 3, dtype=torch.uint8), out)


# ---- the host bookkeeping of push_frames, with a stand-in model -----------------------------------------------------------------
class StandIn(torch.nn.Module):
    """Records what stream_push is handed; returns a history of as many rows as forward would."""
    window_len, model_resolution, stride = 8, (16, 24), 4

    def __init__(self):
        super().__init__()
        self.calls, self.ind, self.feed = [], 0, None

    def init_video_online_processing(self):
        self.ind, self.feed = 0, None

    def stream_push(self, frames, queries, iters=4, add_space_attn=True, final=False):
        if self.feed == "forward":
            raise RuntimeError("this stream is fed through forward")
        self.feed = "push"
        S, n = self.window_len, frames.shape[0]
        T = n if self.ind == 0 else S // 2 + n
        self.calls.append((self.ind, n, bool(final), int(iters), frames.clone()))
        G, N = queries.shape[:2]
        rows = self.ind + T
        self.ind += S // 2
        return torch.zeros(G, rows, N, 2), torch.ones(G, rows, N), torch.ones(G, rows, N), None


@pytest.fixture
def pred():
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=8)
    p.model = StandIn()
    p.interp_shape, p.step = p.model.model_resolution, 4
    # the resize on the host: the values ops.ingest_frames computes on the device
    p._ingest = lambda src, dst, layout: dst.copy_(F.interpolate((src.permute(0, 3, 1, 2) if layout == "hwc" else src).float(),
                                                                 tuple(dst.shape[2:]), mode="bilinear", align_corners=True))
    return p


def start(p, H=40, W=60, N=5):
    p(torch.zeros(1, 1, 3, H, W), is_first_step=True, queries=torch.rand(1, N, 3))  # a one-frame dummy of the right H, W does
    p.model.calls.clear()


def video(n, H=40, W=60, seed=0):
    return torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def resized(v):
    return F.interpolate(v.permute(0, 3, 1, 2).float(), (16, 24), mode="bilinear", align_corners=True)


def test_which_pushes_trigger_a_step(pred):
    start(pred)
    v = video(30)
    steps = []
    for i in range(30):
        tracks, vis = pred.push_frames(v[i])  # one frame [H,W,3] at a time
        steps.append(tracks is not None)
        if tracks is not None:
            k = len(pred.model.calls) - 1
            assert tracks.shape == (1, 4 * k + 8, 5, 2) and vis.shape == (1, 4 * k + 8, 5) and vis.dtype == torch.bool
    # the k-th step runs as soon as frames < k*step + S have arrived: after frames 7, 11, 15, ...
    assert [i for i, s in enumerate(steps) if s] == [7, 11, 15, 19, 23, 27]
    r = resized(v)
    for k, (ind, n, final, iters, frames) in enumerate(pred.model.calls):
        assert (ind, n, final, iters) == (4 * k, 8 if k == 0 else 4, False, 6)
        assert torch.equal(frames, r[:8] if k == 0 else r[4 * k + 4:4 * k + 8])  # the NEW frames only, each resized once


@pytest.mark.parametrize("sizes", [[30], [3] * 10, [8, 4, 4, 14], [5, 1, 2, 9, 13], [7, 1, 3, 1, 18]])
def test_any_partition_runs_the_same_steps(pred, sizes):
    v = video(30, seed=1)
    start(pred)
    i, last = 0, None
    for n in sizes:
        out = pred.push_frames(v[i:i + n])
        done_before, i = (i - 8) // 4 + 1 if i >= 8 else 0, i + n
        done = (i - 8) // 4 + 1 if i >= 8 else 0
        assert (out[0] is None) == (done == done_before)  # a push that completes no window returns (None, None)
        last = out if out[0] is not None else last
    assert [(c[0], c[1]) for c in pred.model.calls] == [(0, 8)] + [(4 * k, 4) for k in range(1, 6)]
    assert last[0].shape[1] == 28  # several windows in one push: the last result
    r = resized(v)
    assert torch.equal(torch.cat([c[4] for c in pred.model.calls]), r[:28])
    assert pred._push_fill == 2


def test_final(pred):
    v = video(40, seed=2)
    # r leftover frames are flushed as the closing chunk
    start(pred)
    assert pred.push_frames(v[:12])[0].shape[1] == 12
    tracks, _ = pred.push_frames(v[12:15], final=True)
    assert [(c[0], c[1], c[2]) for c in pred.model.calls] == [(0, 8, False), (4, 4, False), (8, 3, True)]
    assert tracks.shape[1] == 8 + 4 + 3
    with pytest.raises(RuntimeError, match="ended this stream"):
        pred.push_frames(v[15])
    # 0 leftover: nothing more to track, the last window's result (or nothing), and the stream is closed all the same
    start(pred)
    tracks, _ = pred.push_frames(v[:12], final=True)
    assert [(c[0], c[1], c[2]) for c in pred.model.calls] == [(0, 8, False), (4, 4, False)] and tracks.shape[1] == 12
    with pytest.raises(RuntimeError, match="ended this stream"):
        pred.push_frames(v[12])
    start(pred)
    pred.push_frames(v[:12])
    assert pred.push_frames(v[:0], final=True) == (None, None)
    # `step` leftover frames can only wait before the first window: a video shorter than one window
    start(pred)
    assert pred.push_frames(v[:4]) == (None, None)
    tracks, _ = pred.push_frames(v[:0], final=True)
    assert [(c[0], c[1], c[2]) for c in pred.model.calls] == [(0, 4, True)] and tracks.shape[1] == 4
    # the next first step opens a new stream on the same buffer
    buf = pred._push_buf
    start(pred)
    assert pred.push_frames(v[:8])[0].shape[1] == 8 and pred._push_buf is buf


def test_input_forms(pred):
    start(pred, H=40, W=60)
    v = video(8, seed=3)
    forms = [v, v.float(), v.permute(0, 3, 1, 2).contiguous(), v.permute(0, 3, 1, 2).float()]
    seen = []
    for f_ in forms:
        start(pred)
        pred.push_frames(f_)
        seen.append(pred.model.calls[0][4])
    assert all(torch.equal(s_, seen[0]) for s_ in seen[1:])
    start(pred)
    for bad in (v[:, :39], v[..., :2], v.long(), v[0, 0], torch.zeros(2, 1, 40, 60, 3)):
        with pytest.raises(ValueError):
            pred.push_frames(bad)
    with pytest.raises(ValueError, match="layout"):
        pred.push_frames(v, layout="nhwc")
    with pytest.raises(ValueError):
        pred.push_frames(v, layout="chw")
    # H == 3 (or W == 3): both readings fit a [n,3,3,3] tensor, layout= decides
    start(pred, H=3, W=3)
    sq = torch.randint(0, 256, (8, 3, 3, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="layout"):
        pred.push_frames(sq)
    pred.push_frames(sq, layout="hwc")
    a = pred.model.calls[0][4]
    start(pred, H=3, W=3)
    pred.push_frames(sq.permute(0, 3, 1, 2).contiguous(), layout="chw")
    assert torch.equal(a, pred.model.calls[0][4])


def test_no_first_step_and_support_grid(pred):
    with pytest.raises(RuntimeError, match="first step"):
        pred.push_frames(video(1))
    pred(torch.zeros(1, 1, 3, 40, 60), is_first_step=True, queries=torch.rand(1, 5, 3), add_support_grid=True)
    assert pred.queries.shape[1] == 5 + 36
    tracks, vis = pred.push_frames(video(8), add_support_grid=True)
    assert tracks.shape == (1, 8, 5, 2) and vis.shape == (1, 8, 5)


def test_mixing_forward_and_push_raises():
    """On the model: one stream is fed one way, until init_video_online_processing()."""
    from cotracker_amd.model import CoTrackerThreeOnline
    m = CoTrackerThreeOnline(window_len=8, model_resolution=(64, 96))
    m.init_video_online_processing()
    assert m._feed is None
    m._fed("forward")
    with pytest.raises(RuntimeError, match="fed through forward"):
        m.stream_push(torch.zeros(8, 3, 64, 96), torch.zeros(1, 4, 3))
    m.init_video_online_processing()
    m._fed("push")
    with pytest.raises(RuntimeError, match="fed through stream_push"):
        m._fed("forward")
    m.init_video_online_processing()
    assert m._feed is None
    # refused before anything is marked: wrong frame counts, a host tensor
    with pytest.raises(RuntimeError, match="MI355X GPU only"):
        m.stream_push(torch.zeros(8, 3, 64, 96), torch.zeros(1, 4, 3))
    with pytest.raises(ValueError, match="float32"):
        m.stream_push(torch.zeros(8, 3, 64, 96, dtype=torch.uint8), torch.zeros(1, 4, 3))
    assert m._feed is None
    # copies and pickles carry the bookkeeping and start a fresh stream cleanly
    m._fed("push")
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert c._feed == "push" and c._gstream is None
        c.init_video_online_processing()
        assert c._feed is None


def test_forward_marks_the_stream_before_it_needs_a_device():
    from cotracker_amd.model import CoTrackerThreeOnline
    m = CoTrackerThreeOnline(window_len=8, model_resolution=(64, 96))
    m.init_video_online_processing()
    m._fed("push")
    with pytest.raises(RuntimeError):  # (a host video is refused first, with its own RuntimeError: either way nothing runs)
        m(torch.zeros(1, 8, 3, 64, 96), torch.zeros(1, 4, 3), is_online=True)


def test_v2_raises():
    from cotracker_amd.build_cotracker import build_cotracker
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    v2 = build_cotracker(None, v2=True, window_len=8)
    with pytest.raises(NotImplementedError, match="stream_push"):
        v2.stream_push(torch.zeros(8, 3, 64, 96), torch.zeros(1, 4, 3))
    p2 = CoTrackerOnlinePredictor(checkpoint=None, v2=True, window_len=8)
    p2(torch.zeros(1, 1, 3, 40, 60), is_first_step=True, queries=torch.rand(1, 5, 3))
    with pytest.raises(NotImplementedError, match="push_frames"):
        p2.push_frames(video(1))
