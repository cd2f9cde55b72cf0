"""The resident slot assign (-m gpu): ops.StreamGroups.assign(resident=True) and the kernel behind it (csrc/stream.hip:
ctk_stream_assign_resident / _ring), model.stream_assign(resident=True), CoTrackerOnlinePredictor.add_queries(resident=True).

Between two calls the pyramid of the window just tracked, frames [ind - STEP, ind - STEP + S), is still on the device (ind: the first
frame of the next call's window).  A query on one of those frames gets its support patch sampled from it at once and (x, y) in the
history rows the next begin carries over, so the next window starts it as a fresh point.  Every comparison is exact (bits): against
the existing operators (ops.sample_support, index expressions), against a stream that was given the query up front (its
accumulator rows), and against a twin stream whose slot was assigned the plain way and then patched by hand with torch writes."""
import copy
import functools
import warnings

import pytest
import torch

import ctk_support
from ctk_support import HW, S, STEP, STRIDE, bits, chunks, dev, maxdiff, run_stream, stream_inputs

pytestmark = pytest.mark.gpu

OV = S - STEP
RING = S + STEP + 3  # 15 rows: the carry rows of ind = 12 are 12, 13, 14, 0
_models = {}
small_model = functools.partial(ctk_support.small_model, _models, batch_mode="loop", hip_graph=False, range_guard=True, stream_groups=True,
                                stream_slots=True, online_feature_cache=False, stream_range_check="deferred")
fresh_copy = functools.partial(ctk_support.copy_without_stream_state, stream_slots=True)


def empty_row():
    from cotracker_amd import ops
    return torch.tensor([ops.EMPTY_FRAME, 0.0, 0.0], device=dev())


def buffers(gs):
    return [gs.queries, *gs.support, *gs.hist, gs.coords, gs.vis, gs.conf, gs.mask, *gs.pyr, gs.nonfinite]


def is_resident(newq, ind):
    qf = newq[:, 0].long()
    return (qf >= ind - STEP) & (qf < ind + OV)


def sampled_support(gs, newq, ind, l):
    """What the resident assign leaves in support[l] for the rows of newq (all of them resident): the existing operator on the
    resident pyramid, at the truncated frame's row, position (x, y) / stride / 2^l as the model forms it."""
    from cotracker_amd import ops
    z = (newq[:, 0].long() - (ind - STEP)).float().contiguous()
    return 0.0 + ops.sample_support(gs.pyr[l], z, ((newq[:, 1:3] / STRIDE) / 2 ** l).contiguous())


def library_calls(monkeypatch):
    """-> a list that grows by the name of every entry point of the library called from now on (for the rest of the test)."""
    from cotracker_amd import _lib as L
    lib, seen = L.load(), []
    for name in L.SYMBOLS:
        if name != "ctk_error_string":
            def counted(*a, _fn=getattr(lib, name), _name=name):
                seen.append(_name)
                return _fn(*a)
            monkeypatch.setattr(lib, name, counted)
    return seen


# ----------------------------------------------------------------------------------------------------------------------
# 1. the kernel against existing operators and index expressions; every other byte of every buffer stays
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring,ind,rows", [(None, 4, None), (None, 12, 5), (RING, 12, None)], ids=["linear-4", "linear-12-rows5", "ring15-12"])
def test_kernel_against_existing_operators(monkeypatch, ring, ind, rows):
    from cotracker_amd import ops
    G, N = 3, 11
    g = torch.Generator().manual_seed(23 + ind)
    sizes = [(HW[0] // STRIDE >> l, HW[1] // STRIDE >> l) for l in range(4)]
    gs = ops.StreamGroups(torch.zeros(G, N, 3, device=dev()), S, STEP, STRIDE, sizes, ring_rows=ring)
    for t in buffers(gs):  # random bytes everywhere (NaN patterns included: compared as integers) ...
        raw = torch.randint(0, 256, (t.numel() * t.element_size(),), generator=g, dtype=torch.uint8).to(dev())
        t.view(torch.uint8).reshape(-1).copy_(raw)
    for p_ in gs.pyr:  # ... but a finite pyramid: it is sampled
        p_.copy_(torch.randn(p_.shape, generator=g).to(dev()))
    gs.next_ind, gs.committed = ind, ind + OV  # the books after the call at ind - STEP
    e = ops.EMPTY_FRAME
    newq = torch.tensor([[ind - STEP, 33.3, 20.7],        # the pyramid's first frame, interior
                         [ind - 1.0, 40.0, 24.0],         # integer position
                         [float(ind), 12.5, 8.5],         # half-integer
                         [ind + OV - 1.0, 95.0, 63.0],    # the pyramid's last frame, on the far border
                         [ind + 1.5, -7.3, -2.0],         # a fractional frame (truncated), outside the picture on the low side
                         [ind + 2.0, 120.0, 80.5],        # outside on the high side
                         [float(ind + OV), 50.0, 30.0],   # the first frame that is not resident: the plain assign
                         [ind + OV + 9.0, 10.0, 10.0],    # further ahead
                         [e, 0.0, 0.0]], device=dev())    # an empty slot
    M = newq.shape[0]
    res = is_resident(newq, ind)
    assert res.tolist() == [True] * 6 + [False] * 3
    slots = torch.tensor([21, 5, 32, 0, 16, 10, 27, 11, 22])  # every group, first and last slot of a group, in no order
    want = [t.clone() for t in buffers(gs)]
    ptrs = [t.data_ptr() for t in buffers(gs)]
    serial = gs.serial
    calls = library_calls(monkeypatch)
    gs.assign(slots, newq, rows=rows, resident=True)
    torch.cuda.synchronize()
    assert calls == ["ctk_stream_assign_resident" + ("_ring" if ring is not None else "")]  # ONE entry point, which launches once
    sd = slots.to(dev())
    want[0][sd] = newq
    for l in range(4):
        want[1 + l][sd] = 0.0
        want[1 + l][sd[res]] = sampled_support(gs, newq[res], ind, l)
        assert bool(want[1 + l][sd[res]].abs().sum(dim=(1, 2)).gt(0).all())
    nrows = gs.T_cap if ring is not None else (gs.committed if rows is None else rows)
    carry = [f % gs.T_cap for f in range(ind, ind + OV)] if ring is not None else list(range(ind, ind + OV))
    if ring is not None:
        assert carry == [12, 13, 14, 0]
    for h_ in want[5:8]:
        h_[sd // N, :nrows, sd % N] = 0.0
    for s_, row in zip(sd[res].tolist(), newq[res]):
        for r_ in carry:
            want[5][s_ // N, r_, s_ % N] = row[1:3]
            want[6][s_ // N, r_, s_ % N] = 0.0
            want[7][s_ // N, r_, s_ % N] = 0.0
    for k, (got, w_) in enumerate(zip(buffers(gs), want)):
        assert torch.equal(bits(got), bits(w_)), (k, ring, ind)
    assert [t.data_ptr() for t in buffers(gs)] == ptrs and gs.serial == serial
    assert torch.equal(gs.first_row.view(-1)[slots], torch.full((M,), ind)) and int(gs.first_row.sum()) == M * ind
    assert gs.occupied.view(-1)[slots].tolist() == [True] * (M - 1) + [False]
    # the unmodified begin starts a resident slot as it starts a fresh point: x / stride at every t, zero logits, mask 1
    gs.begin(ind)
    torch.cuda.synchronize()
    for s_, row in zip(sd[res].tolist(), newq[res]):
        c = gs.coords[s_ // N, :, s_ % N]
        assert torch.equal(bits(c), bits((row[1:3] * (1.0 / STRIDE)).expand(S, 2))), s_
        assert not bool(bits(gs.vis[s_ // N, :, s_ % N]).any()) and not bool(bits(gs.conf[s_ // N, :, s_ % N]).any())
        assert int(gs.mask[s_ // N, s_ % N]) == 1


# ----------------------------------------------------------------------------------------------------------------------
# 2. the accumulator rows equal those of the stream that was given the query up front
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3])
def test_support_equals_the_up_front_streams(G):
    """f in [ind, ind + OV): the up-front stream sampled (f, x, y) in the call at w = ind - STEP, at pyramid row f - w -- the row the
    resident assign reads after that call."""
    m = small_model("f16x3")
    twin = fresh_copy(m)
    N, T = 9, S + 2 * STEP
    video, q = stream_inputs(G, N, T, seed=61 + G, frames=[0, 0, 1, 3, 6])
    ind = 2 * STEP
    slots = [(G - 1) * N + n for n in (N - 4, N - 3, N - 2, N - 1)]
    q.view(-1, 3)[slots, 0] = torch.tensor([ind + 0.0, ind + 1.0, ind + 2.5, ind + OV - 1.0], device=dev())
    q0 = q.clone()
    q0.view(-1, 3)[slots] = empty_row()
    for model, table in ((twin, q), (m, q0)):
        model.init_video_online_processing()
        for t0 in chunks(T)[:2]:
            model(video[:, t0:t0 + S], table, iters=2, is_online=True)
    assert m.online_ind == ind and m.stream_resident_frames == (ind - STEP, ind + OV)
    before = [s_.clone() for s_ in m._gstream.support]
    m.stream_assign(slots, q.view(-1, 3)[slots], resident=True)
    torch.cuda.synchronize()
    other = torch.ones(G * N, dtype=torch.bool)
    other[slots] = False
    for l in range(4):
        got, want = m._gstream.support[l], twin._gstream.support[l]
        assert torch.equal(bits(got[slots]), bits(want[slots])), l
        assert float(got[slots].abs().max()) > 0.0
        assert torch.equal(bits(got[other]), bits(before[l][other])) and torch.equal(bits(got[other]), bits(want[other]))
    assert torch.equal(m.stream_queries, q)
    for model in (m, twin):
        model._resolve_deferred_range_check()


# ----------------------------------------------------------------------------------------------------------------------
# 3. end to end against a twin whose slots were assigned the plain way and patched by hand
# ----------------------------------------------------------------------------------------------------------------------
def hand_made_assign(ref, slots, newq):
    """The resident assign spelled with what existed before it: the plain assign with the frame rule lowered, then torch writes of
    the support patches (ops.sample_support on the resident pyramid) and of the carry rows."""
    gs, ind = ref._gstream, ref.online_ind
    gs.assign(slots, newq, min_frame=ind - STEP)
    res = is_resident(newq, ind)
    sd = torch.as_tensor(slots, device=dev())[res]
    for l in range(4):
        gs.support[l][sd] = sampled_support(gs, newq[res], ind, l)
    for s_, row in zip(sd.tolist(), newq[res]):
        for r_ in gs.frame_rows(ind, ind + OV):
            gs.hist[0][s_ // gs.N, r_, s_ % gs.N] = row[1:3]


def model_call(m, feed, video, q, k, t0):
    if feed == "chunks":
        return m(video[:, t0:t0 + S], q, iters=2, is_online=True)[:3]
    return m.stream_push(video[0, :S] if k == 0 else video[0, t0 + S - STEP:t0 + S], q, iters=2)[:3]


E2E = [("chunks", 1, "loop", False, None, "f16x3"), ("chunks", 3, "joint", True, None, "f16x3"), ("push", 3, "loop", True, RING, "f32"),
       ("push", 1, "joint", False, RING, "f16x3"), ("chunks", 3, "loop", False, RING, "f16x3"), ("push", 3, "joint", True, None, "f16x3")]


@pytest.mark.parametrize("feed,G,mode,graph,ring,precision", E2E, ids=["-".join(map(str, c)) for c in E2E])
def test_stream_equals_the_hand_made_twin(monkeypatch, feed, G, mode, graph, ring, precision):
    from cotracker_amd import ops
    m = fresh_copy(small_model(precision, batch_mode=mode, hip_graph=graph))
    ref = fresh_copy(m)
    m.stream_history_frames = ref.stream_history_frames = ring
    captures = []
    orig = ops.WindowGraph._capture

    def counting(self, *a, **k):
        captures.append(self)
        return orig(self, *a, **k)
    monkeypatch.setattr(ops.WindowGraph, "_capture", counting)
    N, T = 10, S + 5 * STEP  # six calls
    video, q = stream_inputs(G, N, T, seed=71 + G, frames=[0, 0, 1, 3, 6, 9])
    q[:, N - 4:] = empty_row()  # four spare slots per group
    last = (G - 1) * N

    def events(ind):
        """Before the calls at ind = 8 and ind = 12 (on the ring its carry rows 12, 13, 14, 0 wrap): resident frames at both ends
        of the pyramid and in between, one future frame; spare slots, a live point, and a slot assigned one call before."""
        if ind == 2 * STEP:
            return [N - 1, last + N - 2, 2], torch.tensor([[ind - STEP, 31.0, 17.5], [ind + OV - 1.0, 70.25, 44.0], [ind + 0.5, 5.0, 60.0]],
                                                          device=dev())
        if ind == 3 * STEP:
            return [N - 3, last + N - 4, N - 1, last + 1], torch.tensor([[ind - 1.0, 88.0, 9.0], [float(ind), 47.3, 30.1], [ind + 2.0, 20.0, 20.0],
                                                                         [ind + OV + 2.0, 60.0, 33.0]], device=dev())
        return None
    marks = []
    for x in (m, ref):
        x.init_video_online_processing()
    for k, t0 in enumerate(chunks(T)):
        ev = events(t0) if k else None
        if ev is not None:
            gs = m._gstream
            state = (len(captures), gs.serial, tuple(t.data_ptr() for t in [gs.queries, *gs.support, gs.coords, gs.vis, gs.conf, gs.mask, *gs.pyr]),
                     len(gs._wins))
            assert m.stream_resident_frames == (t0 - STEP, t0 + OV)
            m.stream_assign(*ev, resident=True)
            hand_made_assign(ref, *ev)
            assert state == (len(captures), gs.serial, tuple(t.data_ptr() for t in [gs.queries, *gs.support, gs.coords, gs.vis, gs.conf, gs.mask,
                                                                                     *gs.pyr]), len(gs._wins))
            marks.append(len(captures))
            assert torch.equal(m.stream_first_row, ref.stream_first_row) and torch.equal(m.stream_queries, ref.stream_queries)
            for a, b in zip(buffers(gs), buffers(ref._gstream)):  # the kernel and the hand-made writes leave the same state
                assert torch.equal(bits(a), bits(b))
        got, want = model_call(m, feed, video, q, k, t0), model_call(ref, feed, video, q, k, t0)
        f0 = t0 if ring is not None else 0  # the frame of output row 0
        own = (f0 + torch.arange(got[0].shape[1])[None, :, None] >= m.stream_first_row[:, None, :]).to(dev())
        for name, x, y in zip(("coords", "vis", "conf"), got, want):
            sel = own[..., None] if x.dim() == 4 else own
            assert x.shape == y.shape and torch.equal(bits(torch.where(sel, x, torch.zeros_like(x))), bits(torch.where(sel, y, torch.zeros_like(y)))), \
                (k, name, maxdiff(x, y))
        assert bool(torch.isfinite(got[0]).all())
    for x in (m, ref):
        x._resolve_deferred_range_check()
    assert m.range_fallbacks == ref.range_fallbacks == 0
    assert int(m.stream_first_row.view(-1)[N - 1]) == 3 * STEP and int(m.stream_first_row.view(-1)[2]) == 2 * STEP
    if graph:  # nothing is captured again: all graphs exist before the first assign
        assert marks and marks[0] > 0 and len(captures) == marks[0], (marks, len(captures))
    else:
        assert not captures
    # the assigned points are tracked: their last window is not the blank track of an empty slot
    c = got[0]
    assert float((c[0, -1, N - 3] - c[0, -1, N - 2]).abs().max()) > 0.0


# ----------------------------------------------------------------------------------------------------------------------
# 4. refusals: raised with every buffer unchanged
# ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_stream_alone():
    m = small_model("f16x3")
    G, N, T = 2, 9, S + 2 * STEP
    video, q = stream_inputs(G, N, T, seed=47, frames=[0, 0, 1, 2, 5])
    q[:, N - 3:] = empty_row()
    m.init_video_online_processing()
    with pytest.raises(RuntimeError, match="no stream is running"):
        m.stream_assign([N - 1], torch.tensor([[1.0, 5.0, 6.0]], device=dev()), resident=True)
    for t0 in chunks(T)[:2]:
        m(video[:, t0:t0 + S], q, iters=2, is_online=True)
    ind = m.online_ind
    assert ind == 2 * STEP and m.stream_resident_frames == (ind - STEP, ind + OV)
    before = [t.clone() for t in buffers(m._gstream)]
    book = (m.stream_occupied, m.stream_first_row)
    with pytest.raises(ValueError, match=rf"\[{ind - STEP}, {ind + OV}\)"):  # the frame has left the pyramid; the message names the range
        m.stream_assign([N - 1], torch.tensor([[ind - STEP - 0.5, 5.0, 6.0]], device=dev()), resident=True)
    with pytest.raises(ValueError, match=rf"\[{ind - STEP}, {ind + OV}\)"):  # one bad row refuses the whole list
        m.stream_assign([N - 1, N - 2], torch.tensor([[ind + 0.0, 5.0, 6.0], [0.0, 5.0, 6.0]], device=dev()), resident=True)
    for f in (ind - STEP, ind - 1, ind, ind + OV - 0.5):  # resident frames WITHOUT the keyword: refused as ever
        with pytest.raises(ValueError, match="left the stream"):
            m.stream_assign([N - 1], torch.tensor([[float(f), 5.0, 6.0]], device=dev()))
    with pytest.raises(ValueError):
        m.stream_assign([N - 1, N - 1], torch.tensor([[ind + 0.0, 5.0, 6.0]], device=dev()).expand(2, 3), resident=True)
    with pytest.raises(ValueError):
        m.stream_assign([N - 1], torch.tensor([[float("nan"), 5.0, 6.0]], device=dev()), resident=True)
    torch.cuda.synchronize()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(buffers(m._gstream), before))
    assert torch.equal(m.stream_occupied, book[0]) and torch.equal(m.stream_first_row, book[1])
    m(video[:, ind:ind + 5], q, iters=2, is_online=True)  # a short chunk closes the stream
    before = [t.clone() for t in buffers(m._gstream)]
    with pytest.raises(RuntimeError, match="ended the stream"):
        m.stream_assign([N - 1], torch.tensor([[ind + 1.0, 5.0, 6.0]], device=dev()), resident=True)
    with pytest.raises(RuntimeError, match="ended the stream"):
        m._gstream.assign([N - 1], torch.tensor([[ind + 1.0, 5.0, 6.0]], device=dev()), resident=True)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(buffers(m._gstream), before))
    m._resolve_deferred_range_check()
    from cotracker_amd.build_cotracker import build_cotracker
    with pytest.raises(NotImplementedError, match="stream_assign"):
        build_cotracker(None, v2=True, window_len=S).stream_assign([0], torch.tensor([[1.0, 5.0, 6.0]], device=dev()), resident=True)


# ----------------------------------------------------------------------------------------------------------------------
# 5. range guard: the re-run on f32 finds the support sample and the carry rows again
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [None, RING], ids=["linear", "ring15"])
def test_range_guard_rerun_after_a_resident_assign(ring):
    from cotracker_amd.synthetic import synthetic_video
    T = S + 4 * STEP  # five calls
    video = synthetic_video(T, *HW, seed=5).to(dev())
    q = torch.tensor([[[0.0, 20.0, 20.0], [2.0, 60.0, 40.0], [0.0, 80.0, 10.0]],
                      [[0.0, 30.0, 50.0], [5.0, 10.0, 10.0], [1.0, 70.0, 30.0]]], device=dev())
    q[:, 2] = empty_row()
    kw = dict(stream_groups=True, stream_slots=True, stream_range_check="immediate")
    exact, m = ctk_support.overflow_model("f32", **kw), ctk_support.overflow_model("f16x3", **kw)
    exact.stream_history_frames = m.stream_history_frames = ring
    grew = []

    def assigns(model):
        def between(k):
            ind = k * STEP
            if k == 1:
                model.stream_assign([2], torch.tensor([[ind + 1.0, 44.0, 33.0]], device=dev()), resident=True)
            if k == 3:  # ind = 12: on the ring the carry rows wrap
                model.stream_assign([5, 1], torch.tensor([[ind - STEP + 0.0, 15.0, 50.0], [ind + OV - 1.0, 70.0, 12.0]], device=dev()),
                                    resident=True)
            grew.append(model.range_fallbacks)
        return between
    want = run_stream(exact, video, q, between=assigns(exact))
    assert exact.range_fallbacks == 0 and all(torch.isfinite(x).all() for o in want for x in o)
    grew.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_stream(m, video, q, between=assigns(m))
    grew.append(m.range_fallbacks)
    assert len(grew) == 5 and grew[1] - grew[0] == 1 and grew[3] - grew[2] == 1, grew  # the calls right behind the two assigns were re-run on f32
    for k, (a, b) in enumerate(zip(got, want)):
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b)), k
    assert torch.equal(m.stream_first_row, exact.stream_first_row) and int(m.stream_first_row[0, 2]) == STEP


# ----------------------------------------------------------------------------------------------------------------------
# 6. predictor: add_queries(resident=True) on a uint8 push_frames stream
# ----------------------------------------------------------------------------------------------------------------------
RAW = (160, 240)  # 2.5x the model resolution
BAND = 1e-6       # emit thresholds 1 / (1 + expf(-x)) products, torch its own sigmoid: equal outside this band (tests/test_gpu_stream_ring.py)


@pytest.mark.parametrize("history", [None, RING], ids=["unbounded", "history15"])
def test_predictor_add_queries_resident_on_a_uint8_push_stream(history):
    from cotracker_amd import ops
    from cotracker_amd.model import CoTrackerThreeOnline
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    from cotracker_amd.weights import fill_synthetic_
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=S)
    model = CoTrackerThreeOnline(stride=STRIDE, corr_radius=3, window_len=S, model_resolution=HW).eval()
    fill_synthetic_(model, seed=5)
    model.hip_graph = True
    p.model, p.interp_shape, p.step = model, HW, STEP
    N, K = 4, 3
    p.spare_points, p.history_frames = K, history
    p = p.to(dev())
    twin = copy.deepcopy(p.model)  # the model-level stream the predictor is compared with
    twin.stream_slots, twin.stream_history_frames = True, history
    g = torch.Generator().manual_seed(12)
    T = S + 3 * STEP
    frames = torch.randint(0, 256, (T, *RAW, 3), dtype=torch.uint8, generator=g).to(dev())
    q = torch.rand(1, N, 3, generator=g) * torch.tensor([1.0, RAW[1] - 1.0, RAW[0] - 1.0])
    q[..., 0] = torch.tensor([0.0, 0.0, 3.0, 9.0])
    q = q.to(dev())
    (H, W), (ih, iw) = RAW, HW
    to_model = torch.tensor([(iw - 1) / (W - 1), (ih - 1) / (H - 1)], device=dev())
    p(torch.zeros(1, 1, 3, *RAW, device=dev()), is_first_step=True, queries=q, add_support_grid=True)
    with pytest.raises(RuntimeError):
        p.resident_frames
    twin.init_video_online_processing()

    def twin_step(a, b):
        buf = torch.empty(b - a, 3, ih, iw, device=dev())
        ops.ingest_frames(frames[a:b], buf, layout="hwc")
        return twin.stream_push(buf, p.queries, iters=6)

    def check(got, want, t0):
        tr, vis = got
        c, vi, cf, _ = want
        f0 = t0 if history is not None else 0
        rows = (f0 + torch.arange(c.shape[1])[None, :, None] >= twin.stream_first_row[:, None, :N + K]).to(dev()) & \
            twin.stream_occupied[:, None, :N + K].to(dev())
        assert tr.shape == c[:, :, :N + K].shape and vis.dtype == torch.bool
        assert torch.equal(tr, c[:, :, :N + K] * c.new_tensor([(W - 1) / (iw - 1), (H - 1) / (ih - 1)]))
        prod = (vi * cf)[:, :, :N + K]
        sure = (prod - 0.6).abs() > BAND
        assert torch.equal(vis & sure, (prod > 0.6) & rows & sure)
        assert not bool(vis[~rows].any())  # nothing is visible below a slot's first row, nor in an empty slot
        return rows
    assert p.push_frames(frames[:S], add_support_grid=True)[0] is not None
    twin_step(0, S)
    check(p.push_frames(frames[S:S + STEP], add_support_grid=True), twin_step(S, S + STEP), STEP)
    ind = 2 * STEP
    assert p.resident_frames == (ind - STEP, ind + OV) == twin.stream_resident_frames
    assert p.push_frames(frames[S + STEP:S + STEP + 2], add_support_grid=True) == (None, None)  # two frames wait in the buffer
    added = torch.tensor([[ind - STEP, 100.0, 60.0],       # the oldest resident frame
                          [ind + OV - 1.0, 20.5, 90.0],    # the newest tracked frame: the picture the user has in front of them
                          [ind + OV + 1.0, 200.0, 31.0]],  # buffered, not run yet: the plain path inside the same call
                         device=dev())
    with pytest.raises(ValueError, match="left the stream"):
        p.add_queries(added)  # without the keyword: as ever
    with pytest.raises(ValueError):
        p.add_queries(torch.tensor([[ind - STEP - 1.0, 5.0, 5.0]], device=dev()), resident=True)
    assert not bool(p.model.stream_occupied[0, N:N + K].any())
    points = p.add_queries(added, resident=True)
    assert points.tolist() == [N, N + 1, N + 2]
    aq = added.clone()
    aq[:, 1:] *= to_model
    twin.stream_assign(points, aq, resident=True)
    assert torch.equal(p.model.stream_queries, twin.stream_queries) and p.model.stream_first_row[0, N:N + K].tolist() == [ind] * K
    rows = check(p.push_frames(frames[S + STEP + 2:S + 2 * STEP], add_support_grid=True), twin_step(S + STEP, S + 2 * STEP), 2 * STEP)
    if history is None:
        assert not bool(rows[0, :ind, N:N + K].any()) and bool(rows[0, ind:, N:N + K].all())
    else:
        assert bool(rows[0, :, N:N + K].all())
    tr, vis = p.push_frames(frames[S + 2 * STEP:], add_support_grid=True)
    check((tr, vis), twin_step(S + 2 * STEP, T), 3 * STEP)
    assert float((tr[0, -1, N] - tr[0, -1, N + 1]).abs().max()) > 0.0  # tracked points, not blank slots
    p.finish()
    twin._resolve_deferred_range_check()
