"""Query groups over one video (-m gpu): ctk_window_batch.flags = CTK_BATCH_SHARED_FMAPS, model(video[1], queries[G]) and its two
consumers (EvaluationPredictor.query_group, CoTrackerPredictor.dense_chunks_per_call).

The oracle of a grouped call is the sequential call.  What is exact and checked as such: B = 1 with the flag is the single-window
call; the grouped sampler launch keeps every point's arithmetic, so the correlation stage AND the whole shared joint window equal
the same windows passed unshared (flag 0, aliased fmaps) bit for bit; a group does not see the other groups' queries; the call is
deterministic, directly and through its hipGraph; the model in "loop" mode equals G separate calls bit for bit.  "joint" mode is
fp32-class equal to the loop, at the bars tests/test_gpu_batch.py uses for joint against loop.
"""
import functools

import pytest
import torch

import ctk_support
from ctk_support import count_encodes, dev, logit, maxdiff
from ctk_support import precision_default as precision  # noqa: F401

pytestmark = pytest.mark.gpu

JOINT_PX, JOINT_LOGIT = 2e-4, 2e-5  # joint vs loop (tests/test_gpu_batch.py)
_models = {}
small_model = functools.partial(ctk_support.small_model, _models, batch_mode="loop", hip_graph=False, range_guard=True)


def group_tensors(seed, G, S, N, HW=(24, 32), with_mask=True, qseeds=None):
    """G query groups over ONE random unit-norm pyramid, laid out as the flag demands: support[l] [G*N,49,128], coords [G,S,N,2],
    vis / conf [G,S,N], mask [G,N].  qseeds[g] seeds group g's queries (default: seed * 100 + g)."""
    from cotracker_amd import ops
    H, W = HW
    g = torch.Generator().manual_seed(seed)
    f0 = torch.randn(S, H, W, 128, generator=g)
    pyr = ops.build_pyramid((f0 / f0.norm(dim=-1, keepdim=True)).to(dev()), 4)
    qf, qc, cs, ms = [], [], [], []
    for b in range(G):
        gq = torch.Generator().manual_seed(seed * 100 + b if qseeds is None else qseeds[b])
        qf.append(torch.randint(0, S, (N,), generator=gq).float())
        qc.append(torch.rand(N, 2, generator=gq) * torch.tensor([W - 1.0, H - 1.0]))
        cs.append(qc[-1][None] + torch.randn(S, N, 2, generator=gq) * 0.5)
        ms.append((torch.rand(N, generator=gq) < 0.7).to(torch.uint8))
    qf, qc = torch.cat(qf).to(dev()), torch.cat(qc).to(dev())
    sup = [ops.sample_support(pyr[l], qf, (qc / 2 ** l).contiguous()) for l in range(4)]
    coords = torch.stack(cs).to(dev()).contiguous()
    z = torch.zeros(G, S, N, device=dev())
    return pyr, sup, coords, z, z.clone(), (torch.stack(ms).to(dev()) if with_mask else None), (W * 1.0, H * 1.0)


def group_wins(*args, iters=2, **kw):
    from cotracker_amd import ops
    pyr, sup, coords, vis, conf, mask, scale = group_tensors(*args, **kw)
    return ops.group_windows(pyr, sup, coords, vis, conf, scale, point_mask=mask, iters=iters)


def state(wins):
    return [[x.clone() for x in w.keep[2:5]] for w in wins]


# ------------------------------------------------------------------------------------------------------------------
# C level
# ------------------------------------------------------------------------------------------------------------------
def test_shared_b1_is_the_single_window_call(precision):
    from cotracker_amd import ops
    pw = small_model(precision).packed(dev())
    a, b = group_wins(11, 1, 8, 45, iters=3), group_wins(11, 1, 8, 45, iters=3)
    ops.forward_window(a[0], pw)
    ops.forward_windows(b, pw, shared=True)
    for x, y in zip(state(a)[0], state(b)[0]):
        assert torch.equal(x, y)
    assert ops.WindowBatch(b, shared=True).workspace_bytes() == ops.WindowBatch(b).workspace_bytes()


@pytest.fixture
def backend(request):
    """(precision, split-half sampler version): the three samplers -- version 3 (default), version 1, exact-f32."""
    from cotracker_amd import model
    old = model.DEFAULT_PRECISION
    model.DEFAULT_PRECISION = request.param[0]
    yield request.param
    model.DEFAULT_PRECISION = old


@pytest.mark.parametrize("chunk", [None, 70, 29])
@pytest.mark.parametrize("backend", [("f16x3", 3), ("f16x3", 1), ("f32", 3)], indirect=True, ids=["sh3", "sh1", "f32"])
def test_grouped_sampler_launch_equals_per_group_launches(backend, chunk, ctk_option):
    """corr_embed of three groups: ONE grouped sampler launch per chunk piece (flag) against one launch per group (flag 0, the same
    windows with aliased fmaps) -- the same bits in every row, for the split-half samplers 3 and 1 and (precision f32) the
    exact-f32 sampler, with chunks that straddle groups (70 of N = 50: 50 + 20 | 30 + 40 | 10; 29: five pieces per two groups)
    and masked points; and, to fp32 class, against each group's own ctk_corr_embed."""
    from cotracker_amd import _lib, ops
    precision, version = backend
    ctk_option(_lib.OPT_CORR_VERSION, version)
    pw = small_model(precision).packed(dev())
    G, S, N = 3, 8, 50
    wins = group_wins(5, G, S, N)
    shared = ops.corr_embed_batch(wins, pw, points_per_chunk=chunk, shared=True)
    unshared = ops.corr_embed_batch(wins, pw, points_per_chunk=chunk, shared=False)
    assert torch.equal(shared, unshared), maxdiff(shared, unshared)
    assert float(shared[:, :1024].abs().max()) > 0
    rows = shared.view(G, N * S, -1)
    for b in range(G):  # (fp32 class, not bits: the corr_mlp launches of a chunk cover other row counts than one group's)
        one = ops.corr_embed(wins[b], pw)
        assert maxdiff(rows[b], one) <= 1e-5 * max(1.0, float(one.abs().max())), (b, maxdiff(rows[b], one))
    # smaller workspace: one split-half pyramid copy instead of three
    assert ops.WindowBatch(wins, shared=True).workspace_bytes() < ops.WindowBatch(wins).workspace_bytes()


@pytest.mark.parametrize("N,chunk", [(45, None), (77, 100)])
def test_shared_window_exact_properties(precision, N, chunk):
    """A whole shared joint window of three groups: equal to the same windows unshared bit for bit (after the sampler the launches
    are the same), deterministic, its hipGraph replays the same bits, a group does not see the other groups' queries, and every
    group agrees with its own single-window run to fp32 class."""
    from cotracker_amd import ops
    pw = small_model(precision).packed(dev())
    G, S = 3, 8

    def run(qseeds, shared=True, graph=False):
        wins = group_wins(7, G, S, N, qseeds=qseeds)
        if graph:
            gr = ops.WindowBatchGraph(wins, pw, points_per_chunk=chunk, shared=shared)
            assert gr.nodes > 50
            gr.launch()
        else:
            ops.forward_windows(wins, pw, points_per_chunk=chunk, shared=shared)
        torch.cuda.synchronize()
        return state(wins)

    base, again = run([1, 2, 3]), run([1, 2, 3])
    unshared = run([1, 2, 3], shared=False)
    graph = run([1, 2, 3], graph=True)
    other = run([1, 9, 3])
    for b in range(G):
        for x, y, z, u in zip(base[b], again[b], graph[b], unshared[b]):
            assert torch.isfinite(x).all()
            assert torch.equal(x, y) and torch.equal(x, z), b       # deterministic; graph == direct
            assert torch.equal(x, u), (b, maxdiff(x, u))            # shared == unshared
    for b in (0, 2):
        for x, y in zip(base[b], other[b]):
            assert torch.equal(x, y), (b, maxdiff(x, y))            # groups 0 and 2 do not see group 1
    assert not torch.equal(base[1][0], other[1][0])
    singles = group_wins(7, G, S, N, qseeds=[1, 2, 3])
    for b in range(G):
        ops.forward_window(singles[b], pw)
        for x, y, tol in zip(base[b], state(singles)[b], (JOINT_PX / 4, JOINT_LOGIT, JOINT_LOGIT)):
            assert maxdiff(x, y) < tol, (b, maxdiff(x, y))


def test_unshared_layout_under_the_flag_is_refused():
    """On the device too: windows with their own state tensors are not `equally strided slices of one allocation`."""
    from cotracker_amd import ops
    pw = small_model("f16x3").packed(dev())
    wins = group_wins(3, 2, 8, 20)
    c1 = wins[1].keep[2].clone()
    bad = ops.Window(wins[1].keep[0], wins[1].keep[1], c1, wins[1].keep[3], wins[1].keep[4], (32.0, 24.0), iters=2,
                     point_mask=wins[1].keep[5])
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.forward_windows([wins[0], bad], pw, shared=True)


# ------------------------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------------------------
def video_and_queries(G, N, T, HW=(64, 96), seed=0, mixed_frames=True):
    g = torch.Generator().manual_seed(seed)
    video = (torch.rand(1, T, 3, *HW, generator=g) * 255).to(dev())
    q = torch.rand(G, N, 3, generator=g) * torch.tensor([1.0, HW[1] - 1.0, HW[0] - 1.0])
    q[..., 0] = torch.randint(0, T - 2, (G, N), generator=g).float() if mixed_frames else 0.0
    return video, q.to(dev())


@pytest.mark.parametrize("kind,T", [("offline", 10), ("online", 14)])
def test_model_query_groups(precision, kind, T):
    """model(video[1], queries[G]) -- offline (one window) and sliding (three windows, queries at mixed frames: masked tracks and
    carry-over): "loop" equals G separate calls bit for bit and encodes once; "joint" agrees with the loop to fp32 class."""
    m = small_model(precision, kind)
    G, N = 3, 21
    video, q = video_and_queries(G, N, T)
    sep = [m(video, q[g:g + 1], iters=3) for g in range(G)]
    calls = count_encodes(m)
    try:
        loop = m(video, q, iters=3)
        assert len(calls) == 1  # the video went through the encoder once
        m.batch_mode = "joint"
        joint = m(video, q, iters=3)
        assert len(calls) == 2
    finally:
        del m._encode
    assert m.range_fallbacks == 0
    assert loop[0].shape == (G, T, N, 2) and loop[1].shape == (G, T, N) and len(loop) == 4
    assert m.last_logits[0].shape == (G, T, N)
    for g in range(G):
        for x, y in zip(loop[:3], sep[g][:3]):
            assert torch.equal(x[g], y[0]), (g, maxdiff(x[g], y[0]))
    assert maxdiff(joint[0], loop[0]) < JOINT_PX
    assert maxdiff(logit(joint[1]), logit(loop[1])) < JOINT_LOGIT and maxdiff(logit(joint[2]), logit(loop[2])) < JOINT_LOGIT
    assert not torch.equal(loop[0][0], loop[0][1])


def test_model_more_groups_than_a_joint_window_holds():
    """G = 18 > CTK_MAX_BATCH: joint sub-batches of 16 + 2."""
    from cotracker_amd import _lib
    m = small_model("f16x3", "offline")
    G, N, T = _lib.MAX_BATCH + 2, 9, 8
    video, q = video_and_queries(G, N, T, seed=4)
    loop = m(video, q, iters=2)
    m.batch_mode = "joint"
    calls = count_encodes(m)
    try:
        joint = m(video, q, iters=2)
    finally:
        del m._encode
    assert len(calls) == 1 and joint[0].shape == (G, T, N, 2)
    assert maxdiff(joint[0], loop[0]) < JOINT_PX and maxdiff(logit(joint[1]), logit(loop[1])) < JOINT_LOGIT


def test_what_still_raises():
    m = small_model("f16x3", "online")
    video, q = video_and_queries(3, 8, 8)
    m.init_video_online_processing()
    with pytest.raises(NotImplementedError, match="query-group"):
        m(video, q, iters=2, is_online=True)
    with pytest.raises(AssertionError):  # neither equal batch sizes nor one video with G query sets
        m(torch.cat([video, video]), q, iters=2)
    v2 = small_model("f16x3", "v2")
    with pytest.raises(NotImplementedError, match="joint"):
        v2.batch_mode = "joint"
    v2.init_video_online_processing()
    with pytest.raises(NotImplementedError, match="query-group"):
        v2(video, q, iters=2, is_online=True)


def test_v2_query_groups_on_the_loop():
    """CoTracker2 takes the query-group call through the shared base: encoded once, the groups one after the other."""
    m = small_model("f16x3", "v2")
    G, N, T = 2, 12, 12
    video, q = video_and_queries(G, N, T, seed=2)
    sep = [m(video, q[g:g + 1], iters=2) for g in range(G)]
    calls = count_encodes(m)
    try:
        out = m(video, q, iters=2)
    finally:
        del m._encode
    assert len(calls) == 1 and out[0].shape == (G, T, N, 2)
    for g in range(G):
        assert torch.equal(out[0][g], sep[g][0][0]) and torch.equal(out[1][g], sep[g][1][0])


# ------------------------------------------------------------------------------------------------------------------
# the two consumers
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uniform", [0, 6])
def test_evaluation_predictor_query_group(uniform):
    """Single-point evaluation of 10 points, 4 per model call (4 + 4 + 2): the sequential predictor's result -- bit for bit in loop
    mode, fp32 class in joint mode -- with uniformly sampled support points drawn from the torch RNG in the sequential order."""
    from cotracker_amd.evaluation import EvaluationPredictor
    m = small_model("f16x3", "offline")
    g = torch.Generator().manual_seed(8)
    T, H, W = 8, 80, 120
    video = (torch.rand(1, T, 3, H, W, generator=g) * 255).to(dev())
    q = (torch.rand(1, 10, 3, generator=g) * torch.tensor([T - 1.0, W - 1.0, H - 1.0])).to(dev())
    q[..., 0] = q[..., 0].round()
    ev = EvaluationPredictor(m, interp_shape=(64, 96), grid_size=5, local_grid_size=8, single_point=True, n_iters=3,
                             num_uniformly_sampled_pts=uniform)

    def run(group, mode):
        ev.query_group, m.batch_mode = group, mode
        torch.manual_seed(123)
        torch.cuda.manual_seed(123)
        out = ev(video, q)
        m.batch_mode = "loop"
        return out

    seq = run(1, "loop")
    calls = count_encodes(m)
    try:
        loop = run(4, "loop")
        assert len(calls) == 3  # 4 + 4 + 2 points: three model calls, one encoder run each
    finally:
        del m._encode
    joint = run(4, "joint")
    assert seq[0].shape == (1, T, 10, 2)
    assert torch.equal(loop[0], seq[0]) and torch.equal(loop[1], seq[1])
    assert maxdiff(joint[0], seq[0]) < JOINT_PX * 2 and maxdiff(joint[1], seq[1]) < 1e-4  # (raw-video px; visibility * confidence)


@pytest.mark.parametrize("backward", [False, True])
def test_dense_chunks_per_call(backward):
    """Dense mode on a 160 x 240 video: step = 240 // 80 = 3, nine chunks -> calls of 4 + 4 + 1 chunks.  Same tracks as the
    sequential dense call: bit for bit in loop mode, fp32 class in joint mode; with and without backward tracking."""
    from cotracker_amd.predictor import CoTrackerPredictor
    from cotracker_amd.weights import fill_synthetic_
    p = CoTrackerPredictor(checkpoint=None, offline=False, window_len=8)
    fill_synthetic_(p.model, seed=5)
    p = p.to(dev())
    g = torch.Generator().manual_seed(2)
    video = (torch.rand(1, 8, 3, 160, 240, generator=g) * 255).to(dev())
    assert p.dense_chunks_per_call == 1 and p._dense_layout(video)[0] == 9
    seq = p(video, grid_query_frame=2, backward_tracking=backward)
    p.dense_chunks_per_call = 4
    calls = count_encodes(p.model)
    try:
        loop = p(video, grid_query_frame=2, backward_tracking=backward)
        assert len(calls) == 3 * (2 if backward else 1)
    finally:
        del p.model._encode
    assert loop[0].shape == seq[0].shape == (1, 8, 9 * 80 * 53, 2)
    assert torch.equal(loop[0], seq[0]) and torch.equal(loop[1], seq[1])
    p.model.batch_mode = "joint"
    joint = p(video, grid_query_frame=2, backward_tracking=backward)
    assert maxdiff(joint[0], seq[0]) < 1e-3  # (the parity bar of the full-size configurations, tests/test_gpu_batch.py)
    assert float((joint[1] != seq[1]).float().mean()) < 1e-3
    p.dense_group = True
    with pytest.raises(NotImplementedError, match="dense_group"):
        p(video)
