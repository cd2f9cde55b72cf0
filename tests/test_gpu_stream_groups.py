"""Streaming query groups (-m gpu): model(video [1,T,3,H,W], queries [G,N,3], is_online=True) with model.stream_groups on, the
device-resident stream state behind it (ops.StreamGroups; csrc/stream.hip: ctk_stream_begin / _support / _commit) and its consumer
CoTrackerOnlinePredictor.

The oracle of a grouped stream is G single-group streams, which still run the torch glue of CoTrackerThreeOnline._video_gen.  Checked
as exact: every kernel against the torch expressions it replaces; the model in "loop" mode against G single streams after every
call, with and without the window graph; determinism and group independence of "joint" mode.  "joint" against "loop" is fp32-class
(the bars of tests/test_gpu_groups.py)."""
import copy
import functools
import warnings

import pytest
import torch

import ctk_support
from ctk_support import HW, S, STEP, STRIDE, chunks, count_encodes, dev, maxdiff, run_stream, stream_inputs
from ctk_support import precision_param as precision  # noqa: F401

pytestmark = pytest.mark.gpu

JOINT_PX, JOINT_LOGIT = 2e-4, 2e-5  # joint vs loop (tests/test_gpu_groups.py)
_models = {}
small_model = functools.partial(ctk_support.small_model, _models, batch_mode="loop", hip_graph=False, range_guard=True, stream_groups=True,
                                online_feature_cache=False, stream_range_check="deferred")
overflow_model = functools.partial(ctk_support.overflow_model, stream_groups=True)


# ----------------------------------------------------------------------------------------------------------------------
# the three kernels, each against the torch expressions it replaces
# ----------------------------------------------------------------------------------------------------------------------
def fresh_state(G, N, seed, max_frame):
    from cotracker_amd import ops
    g = torch.Generator().manual_seed(seed)
    q = torch.rand(G, N, 3, generator=g) * torch.tensor([1.0, HW[1] - 1.0, HW[0] - 1.0])
    q[..., 0] = torch.randint(0, max_frame, (G, N), generator=g).float()
    sizes = [(HW[0] // STRIDE >> l, HW[1] // STRIDE >> l) for l in range(4)]
    return ops.StreamGroups(q.to(dev()), S, STEP, STRIDE, sizes), q.to(dev()), g


def test_begin_kernel_is_the_torch_carry_over():
    G, N = 3, 37
    for ind in (0, 4, 8, 20):
        gs, q, g = fresh_state(G, N, 3 + ind, 36)
        # edges: exactly ind + S - step, ind + S - 1, ind + S, frame 0
        q[0, :4, 0] = torch.tensor([ind + S - STEP, ind + S - 1, ind + S, 0.0], device=dev())
        gs.queries.copy_(q.reshape(G * N, 3))
        gs.reserve(ind + S)
        for h_ in gs.hist:
            h_.copy_(torch.randn(h_.shape, generator=g).to(dev()) * 30)
        gs.begin(ind)
        for b in range(G):
            qframes, qcoords = q[b, :, 0].long(), (q[b, :, 1:3] / STRIDE).contiguous()
            coords = qcoords[None].expand(S, N, 2).contiguous()
            vis, conf = torch.zeros(S, N, device=dev()), torch.zeros(S, N, device=dev())
            if ind > 0:  # CoTrackerThreeOnline._video_gen
                overlap = S - STEP
                copy_over = (qframes < ind + overlap)[None, :]
                cprev = gs.hist[0][b, ind:ind + overlap] / STRIDE
                cprev = torch.cat([cprev, cprev[-1:].expand(STEP, -1, -1)], dim=0)
                vprev = gs.hist[1][b, ind:ind + overlap]
                vprev = torch.cat([vprev, vprev[-1:].expand(STEP, -1)], dim=0)
                fprev = gs.hist[2][b, ind:ind + overlap]
                fprev = torch.cat([fprev, fprev[-1:].expand(STEP, -1)], dim=0)
                coords = torch.where(copy_over[..., None], cprev, coords)
                vis, conf = torch.where(copy_over, vprev, vis), torch.where(copy_over, fprev, conf)
            mask = (qframes < ind + S).to(torch.uint8)
            assert torch.equal(gs.coords[b], coords) and torch.equal(gs.vis[b], vis) and torch.equal(gs.conf[b], conf), (ind, b)
            assert torch.equal(gs.mask[b], mask), (ind, b)


def test_support_kernel_is_the_masked_torch_accumulation():
    """A stream of five calls, queries spread over all chunks: after every call the accumulators equal acc + sample_support(all
    points) * mask; rows of points outside the call's range are neither read nor written (sentinel)."""
    from cotracker_amd import ops
    G, N = 3, 29
    gs, q, g = fresh_state(G, N, 11, S + 4 * STEP)
    sent, _, _ = fresh_state(G, N, 11, S + 4 * STEP)
    for s_ in sent.support:
        s_.fill_(7.0)
    qf, qc = q.reshape(G * N, 3)[:, 0].long(), (q.reshape(G * N, 3)[:, 1:3] / STRIDE).contiguous()
    acc = [None] * 4
    touched = torch.zeros(G * N, dtype=torch.bool, device=dev())
    for ind in range(0, 5 * STEP, STEP):
        f0 = torch.randn(S, HW[0] // STRIDE, HW[1] // STRIDE, 128, generator=g)
        f0 = (f0 / f0.norm(dim=-1, keepdim=True)).to(dev())
        for st in (gs, sent):
            st.set_pyramid(f0)
            st.sample_support(ind)
        pyr = ops.build_pyramid(f0, 4)
        left, right = (0 if ind == 0 else ind + STEP), ind + S
        hit = (qf >= left) & (qf < right)
        m_ = hit.float()[:, None, None]
        rel = (qf - ind).float().contiguous()
        for l in range(4):
            assert torch.equal(gs.pyr[l], pyr[l])
            s_ = ops.sample_support(pyr[l], rel, (qc / 2 ** l).contiguous())
            acc[l] = (torch.zeros_like(s_) if acc[l] is None else acc[l]) + s_ * m_
            assert torch.equal(gs.support[l], acc[l]), (ind, l, maxdiff(gs.support[l], acc[l]))
            assert torch.equal(sent.support[l][hit], 7.0 + s_[hit]), (ind, l)
        touched |= hit
        for l in range(4):
            assert bool((sent.support[l][~touched] == 7.0).all()), (ind, l)
    assert bool(touched.all())  # every point was sampled exactly once over the stream


def test_commit_kernel_writes_history_and_flags_nonfinite():
    G, N, ind = 3, 21, 8
    gs, q, g = fresh_state(G, N, 5, 8)
    gs.reserve(ind + S)
    for t_ in (gs.coords, gs.vis, gs.conf):
        t_.copy_(torch.randn(t_.shape, generator=g).to(dev()) * 9)
    before = [h_.clone() for h_ in gs.hist]
    T_valid = 5  # a short last chunk
    gs.commit(ind, T_valid, True)
    want = [gs.coords * float(STRIDE), gs.vis, gs.conf]
    for h_, b_, w_ in zip(gs.hist, before, want):
        assert torch.equal(h_[:, ind:ind + T_valid], w_[:, :T_valid])
        assert torch.equal(h_[:, :ind], b_[:, :ind]) and torch.equal(h_[:, ind + T_valid:], b_[:, ind + T_valid:])
    assert int(gs.nonfinite.item()) == 0
    for h_, t_ in zip(gs.history(ind + T_valid), (gs.coords, gs.vis, gs.conf)):
        assert h_.shape[:3] == (G, ind + T_valid, N)
    gs.vis[2, 6, 3] = float("inf")          # beyond T_valid: not committed, not flagged
    gs.commit(ind, T_valid, True)
    assert int(gs.nonfinite.item()) == 0
    gs.coords[1, 2, 4, 1] = float("nan")
    gs.commit(ind, T_valid, False)          # no flag word handed over
    assert int(gs.nonfinite.item()) == 0
    gs.commit(ind, T_valid, True)
    assert int(gs.nonfinite.item()) == 1
    gs.reserve(100)                          # growth keeps the rows, zero beyond
    assert gs.T_cap >= 100 and torch.equal(gs.hist[1][:, ind:ind + T_valid], gs.vis[:, :T_valid])
    assert float(gs.hist[1][:, 40:].abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------------------------
# model
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_loop_equals_single_streams_bit_for_bit(precision, graph):
    m = small_model(precision)
    G, N, T = 3, 13, S + 4 * STEP  # five chunks
    video, q = stream_inputs(G, N, T)
    single = copy.deepcopy(m)
    single.hip_graph = m.hip_graph = graph
    sep = [run_stream(single, video, q[g:g + 1]) for g in range(G)]
    single._resolve_deferred_range_check()
    calls = count_encodes(m)
    try:
        out = run_stream(m, video, q)
    finally:
        del m._encode
    m._resolve_deferred_range_check()
    assert calls == [S] * 5  # the chunk went through the encoder once per call
    assert m.range_fallbacks == 0 and m.online_ind == 5 * STEP
    for k, (c, v, f) in enumerate(out):
        assert c.shape == (G, S + k * STEP, N, 2) and v.shape == (G, S + k * STEP, N)
        for g in range(G):
            for x, y in zip((c, v, f), sep[g][k]):
                assert torch.equal(x[g], y[0]), (k, g, maxdiff(x[g], y[0]))
    assert not torch.equal(out[-1][0][0], out[-1][0][1])
    assert m.online_coords_predicted.shape == (G, T, N, 2) and len(m.online_track_support) == 4


def test_feature_cache_encodes_only_the_new_frames(precision):
    m = small_model(precision)
    m.online_feature_cache = True
    video, q = stream_inputs(3, 9, S + 3 * STEP, seed=2)
    ref = run_stream(small_model(precision, seed=1), video, q)  # (same model object: cache off, then on)
    m.online_feature_cache = True
    calls = count_encodes(m)
    try:
        out = run_stream(m, video, q)
    finally:
        del m._encode
    assert calls == [S, STEP, STEP, STEP]
    for a, b in zip(out, ref):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_joint_close_to_loop_deterministic_and_independent(precision, graph):
    m = small_model(precision)
    m.hip_graph = graph
    G, N, T = 3, 13, S + 4 * STEP
    video, q = stream_inputs(G, N, T, seed=6)
    loop = run_stream(m, video, q, iters=3)
    m.batch_mode = "joint"
    joint, again = run_stream(m, video, q, iters=3), run_stream(m, video, q, iters=3)
    q2 = q.clone()
    q2[1, :, 1:] = q2[1, :, 1:].flip(0) * 0.5 + 3.0
    other = run_stream(m, video, q2, iters=3)
    m._resolve_deferred_range_check()
    assert m.range_fallbacks == 0
    for k in range(len(loop)):
        assert maxdiff(joint[k][0], loop[k][0]) < JOINT_PX, (k, maxdiff(joint[k][0], loop[k][0]))
        assert maxdiff(joint[k][1], loop[k][1]) < JOINT_LOGIT and maxdiff(joint[k][2], loop[k][2]) < JOINT_LOGIT
        for x, y, z in zip(joint[k], again[k], other[k]):
            assert torch.equal(x, y), k                                     # deterministic
            assert torch.equal(x[0], z[0]) and torch.equal(x[2], z[2]), k   # groups 0 and 2 do not see group 1's queries
    assert not torch.equal(joint[-1][0][1], other[-1][0][1])


def test_more_groups_than_a_joint_window_holds_and_no_recapture(monkeypatch):
    """G = 18 in joint mode with the graph: sub-batches of 16 + 2, one captured graph each, nothing captured after the second
    call -- nor by a second stream of the same shape."""
    from cotracker_amd import _lib, ops
    m = small_model("f16x3")
    G, N, T = _lib.MAX_BATCH + 2, 7, S + 3 * STEP
    video, q = stream_inputs(G, N, T, seed=9)
    loop = run_stream(m, video, q)
    m.batch_mode, m.hip_graph = "joint", True
    captures = []
    orig = ops.WindowGraph._capture

    def counting(self, *a, **k):
        captures.append(len(self.wins))
        return orig(self, *a, **k)
    monkeypatch.setattr(ops.WindowGraph, "_capture", counting)
    m.init_video_online_processing()
    per_call = []
    outs = []
    for t0 in chunks(T):
        c, v, f, _ = m(video[:, t0:t0 + S], q, iters=2, is_online=True)
        outs.append((c.clone(), v.clone(), f.clone()))
        per_call.append(len(captures))
    assert captures == [16, 2] and per_call == [2, 2, 2, 2], (captures, per_call)
    run_stream(m, video, q)
    m._resolve_deferred_range_check()
    assert captures == [16, 2]
    for a, b in zip(outs, loop):
        assert a[0].shape == b[0].shape and maxdiff(a[0], b[0]) < JOINT_PX and maxdiff(a[1], b[1]) < JOINT_LOGIT
    with _lib.option(_lib.OPT_CORR_VERSION, 1):  # the option table is part of the key: other options, other graphs
        m.init_video_online_processing()
        m(video[:, :S], q, iters=2, is_online=True)
    m._resolve_deferred_range_check()
    assert captures == [16, 2, 16, 2]


@pytest.mark.parametrize("mode", ["loop", "joint"])
def test_short_last_chunk_and_one_chunk_stream(precision, mode):
    m = small_model(precision)
    single = copy.deepcopy(m)
    G, N = 2, 10
    video, q = stream_inputs(G, N, S + STEP + 2, seed=3, frames=[0, 1, 5, 9])
    for starts, lengths in (([0, STEP, 2 * STEP], [S, S, 6]), ([0], [5]), ([0], [S])):
        sep = [run_stream(single, video, q[g:g + 1], starts=starts, lengths=lengths) for g in range(G)]
        m.batch_mode = mode
        out = run_stream(m, video, q, starts=starts, lengths=lengths)
        assert out[-1][0].shape == (G, starts[-1] + lengths[-1], N, 2)
        for k in range(len(out)):
            for g in range(G):
                for x, y, tol in zip(out[k], sep[g][k], (JOINT_PX, JOINT_LOGIT, JOINT_LOGIT)):
                    if mode == "loop":
                        assert torch.equal(x[g], y[0]), (starts, k, g)
                    else:
                        assert maxdiff(x[g], y[0]) < tol, (starts, k, g)
    m.init_video_online_processing()
    m(video[:, :5], q, iters=2, is_online=True)
    with pytest.raises(AssertionError, match="shorter than the window"):
        m(video[:, STEP:STEP + S], q, iters=2, is_online=True)


@pytest.mark.parametrize("mode", ["loop", "joint"])
def test_range_guard(mode):
    from cotracker_amd.synthetic import synthetic_video
    video = synthetic_video(12, *HW, seed=5).to(dev())
    q = torch.tensor([[[0.0, 20.0, 20.0], [2.0, 60.0, 40.0], [0.0, 80.0, 10.0]],
                      [[0.0, 30.0, 50.0], [5.0, 10.0, 10.0], [1.0, 70.0, 30.0]]], device=dev())
    exact, m = overflow_model("f32"), overflow_model("f16x3")
    exact.batch_mode = m.batch_mode = mode
    want = run_stream(exact, video, q)
    assert exact.range_fallbacks == 0 and all(torch.isfinite(x).all() for o in want for x in o)
    # without the graph: a warned re-run of the call on the exact-f32 back end, the stream state of all groups put back first
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = run_stream(m, video, q)
    assert m.range_fallbacks == 2 and any(issubclass(x.category, RuntimeWarning) for x in w)
    for a, b in zip(got, want):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    # graph + "immediate": the same, through the graphs
    m.hip_graph, m.stream_range_check = True, "immediate"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_stream(m, video, q)
    assert m.range_fallbacks == 4 and m._pending_range is None
    for a, b in zip(got, want):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    # graph + "deferred" (the default): the NEXT call raises ...
    m.stream_range_check = "deferred"
    m.init_video_online_processing()
    m(video[:, 0:8], q, iters=2, is_online=True)
    with pytest.raises(FloatingPointError, match="f16 range"):
        m(video[:, 4:12], q, iters=2, is_online=True)
    # ... or the start of the next stream; and no NaN survives into that stream's state
    m.init_video_online_processing()
    m(video[:, 0:8], q, iters=2, is_online=True)
    with pytest.raises(FloatingPointError, match="f16 range"):
        m.init_video_online_processing()
    m.precision = "f32"
    later = run_stream(m, video, q)
    for a, b in zip(later, want):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(bool(torch.isfinite(s_).all()) for s_ in m.online_track_support)


def test_deepcopy_and_pickle_in_the_middle_of_a_group_stream():
    import pickle
    m = small_model("f16x3")
    m.hip_graph = True
    video, q = stream_inputs(3, 9, S + 2 * STEP, seed=4)
    want = run_stream(m, video, q)
    m.init_video_online_processing()
    m(video[:, 0:S], q, iters=2, is_online=True)
    for clone in (copy.deepcopy(m), pickle.loads(pickle.dumps(m)).to(dev())):
        assert clone.stream_groups and clone.online_ind == STEP and not clone._graphs and clone.online_f0_tail is None
        for t0 in (STEP, 2 * STEP):
            c, v, f, _ = clone(video[:, t0:t0 + S], q, iters=2, is_online=True)
        clone._resolve_deferred_range_check()
        assert torch.equal(c, want[-1][0]) and torch.equal(v, want[-1][1]) and torch.equal(f, want[-1][2])
    c, *_ = m(video[:, STEP:STEP + S], q, iters=2, is_online=True)  # the original goes on undisturbed
    assert torch.equal(c, want[1][0])
    m._resolve_deferred_range_check()


def test_online_predictor_with_query_groups():
    """CoTrackerOnlinePredictor(queries [G,N,3], add_support_grid=True) equals G predictors, bit for bit in loop mode."""
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    from cotracker_amd.weights import fill_synthetic_
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=S)
    fill_synthetic_(p.model, seed=5)
    p = p.to(dev())
    g = torch.Generator().manual_seed(12)
    T, H, W = S + 2 * STEP, 120, 160
    video = (torch.rand(1, T, 3, H, W, generator=g) * 255).to(dev())
    G, N = 3, 2
    q = (torch.rand(G, N, 3, generator=g) * torch.tensor([1.0, W - 1.0, H - 1.0])).to(dev())
    q[..., 0] = torch.tensor([[0.0, 3.0], [0.0, 9.0], [1.0, 0.0]], device=dev())

    def stream(queries):
        p(video[:, :S], is_first_step=True, queries=queries, add_support_grid=True)
        outs = []
        for t0 in range(0, T - S + 1, STEP):
            tr, vis = p(video[:, t0:t0 + S], queries=queries, add_support_grid=True)
            outs.append((tr.clone(), vis.clone()))
        p.finish()
        return outs

    sep = [stream(q[b:b + 1]) for b in range(G)]
    assert not p.model.stream_groups
    grouped = stream(q)
    assert p.model.stream_groups and p.queries.shape == (G, N + 36, 3)
    for k, (tr, vis) in enumerate(grouped):
        assert tr.shape == (G, S + k * STEP, N, 2) and vis.shape == (G, S + k * STEP, N) and vis.dtype == torch.bool
        for b in range(G):
            assert torch.equal(tr[b], sep[b][k][0][0]) and torch.equal(vis[b], sep[b][k][1][0]), (k, b)
    p.model.batch_mode = "joint"
    joint = stream(q)
    assert maxdiff(joint[-1][0], grouped[-1][0]) < JOINT_PX * 4  # (raw-video pixels)


def test_switch_off_still_raises():
    m = small_model("f16x3")
    m.stream_groups = False
    video, q = stream_inputs(3, 8, S)
    m.init_video_online_processing()
    with pytest.raises(NotImplementedError, match="query-group"):
        m(video, q, iters=2, is_online=True)
    m.stream_groups = True
    assert m(video, q, iters=2, is_online=True)[0].shape == (3, S, 8, 2)
    m._resolve_deferred_range_check()
