"""Joint batch mode (-m gpu): B videos of equal shape through ONE window call (ctk_forward_window_batch, batch_mode = "joint").

Joint and looped results are fp32-class equal, NOT bit-identical (which GEMM kernel a row tile lands on depends on the total
row count, include/ctk.h).  What is exact and checked here: B = 1 is the single-window call, a video's result does not depend
on the contents of the other videos of its batch, the joint call is deterministic (direct and through its hipGraph), and the
two-level attention batch equals B single-level calls bit for bit.  Parity with the reference is per element, at the usual
bars (1e-3 px, 1e-4 logit), against goldens that already exist (the reference is batch-independent).
"""
import functools
import os
import warnings

import pytest
import torch

import ctk_support
from ctk_support import ROOT, dev, logit, maxdiff, t
from ctk_support import precision_default as precision  # noqa: F401

pytestmark = pytest.mark.gpu

TOL_PX, TOL_LOGIT = 1e-3, 1e-4
_models = {}
small_model = functools.partial(ctk_support.small_model, _models, batch_mode="loop", hip_graph=False, range_guard=True,
                                online_feature_cache=False)


def random_window(seed, S, N, HW=(24, 32), iters=2, with_mask=False, space_attn=True):
    """A window on random unit-norm feature maps (no encoder): what ctk_forward_window consumes."""
    from cotracker_amd import ops
    g = torch.Generator().manual_seed(seed)
    H, W = HW
    f0 = torch.randn(S, H, W, 128, generator=g)
    f0 = (f0 / f0.norm(dim=-1, keepdim=True)).to(dev())
    pyr = ops.build_pyramid(f0, 4)
    qf = torch.randint(0, S, (N,), generator=g).float().to(dev())
    qc = (torch.rand(N, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])).to(dev())
    sup = [ops.sample_support(pyr[l], qf, (qc / 2 ** l).contiguous()) for l in range(4)]
    coords = (qc[None] + torch.randn(S, N, 2, generator=g).to(dev()) * 0.5).contiguous()
    vis = torch.zeros(S, N, device=dev())
    conf = torch.zeros(S, N, device=dev())
    mask = (torch.rand(N, generator=g) < 0.7).to(torch.uint8).to(dev()) if with_mask else None
    return ops.Window(pyr, sup, coords, vis, conf, (W * 1.0, H * 1.0), iters=iters, point_mask=mask, space_attn=space_attn)


def state(win):
    return [x.clone() for x in win.keep[2:5]]


# ------------------------------------------------------------------------------------------------------------------
# 5. the two-level attention batch in isolation
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [400, 1024, 1100])
@pytest.mark.parametrize("Bo", [1, 3])
@pytest.mark.parametrize("shape", ["v2p", "p2v", "vself"])
@pytest.mark.parametrize("backend", ["mfma", "valu"])
def test_two_level_attention(shape, Bo, N, backend, ctk_option):
    """The three space shapes of a joint window -- 64 queries x N keys with key splits, N x 64, 64 x 64 -- with the (video,
    frame) batch and DIFFERENT outer strides for queries and keys: against torch fp64, and bit-identical to Bo separate
    single-level calls on each video's slice (f32 and SH output)."""
    from cotracker_amd import _lib, ops
    if backend == "valu" and (N != 400 or shape == "vself"):
        pytest.skip("the VALU fallback is exercised on one size per cross shape")
    ctk_option(_lib.OPT_ATTENTION_VALU, 1 if backend == "valu" else 0)
    Bi = 8
    N1, N2 = {"v2p": (64, N), "p2v": (N, 64), "vself": (64, 64)}[shape]
    splits = (N + 1023) // 1024 + 1 if shape == "v2p" else 1  # > 1 also where the window would use 1: the partials are batched too
    g = torch.Generator().manual_seed(Bo * 7 + N + len(shape))
    q = torch.randn(Bo, N1, Bi, 384, generator=g).to(dev())
    k = torch.randn(Bo, N2, Bi, 384, generator=g).to(dev())
    v = torch.randn(Bo, N2, Bi, 384, generator=g).to(dev())
    out = ops.attention_batch2(q, k, v, splits=splits)
    osh = ops.attention_batch2(q, k, v, splits=splits, out_split=True)
    qd, kd, vd = (x.double().permute(0, 2, 1, 3).reshape(Bo, Bi, -1, 8, 48).transpose(2, 3) for x in (q, k, v))
    ref = (torch.softmax(qd @ kd.transpose(-1, -2) * 48 ** -0.5, -1) @ vd).transpose(2, 3).reshape(Bo, Bi, N1, 384).permute(0, 2, 1, 3)
    assert maxdiff(out, ref) < 5e-6
    assert maxdiff(ops.unsplit(osh).reshape(Bo, N1, Bi, 384), ref) < 8e-6
    for bo in range(Bo):  # one single-level call per video: [N, Bi, 384] viewed as batch = frame (bs = 1, is = Bi)
        one = ops.attention_batch2(q[bo:bo + 1].contiguous(), k[bo:bo + 1].contiguous(), v[bo:bo + 1].contiguous(), splits=splits)
        assert torch.equal(out[bo], one[0]), (bo, maxdiff(out[bo], one[0]))
        # ... and the plain operator on the frame-major copy of that video
        plain = ops.attention(q[bo].transpose(0, 1).contiguous(), k[bo].transpose(0, 1).contiguous(),
                              v[bo].transpose(0, 1).contiguous(), splits=splits)
        assert torch.equal(out[bo], plain.transpose(0, 1)), (bo, maxdiff(out[bo], plain.transpose(0, 1)))


def test_two_level_attention_masks():
    """Per-video masks (outer mask strides): video bo's keys / queries are masked by ITS row of the mask arrays."""
    from cotracker_amd import ops
    g = torch.Generator().manual_seed(3)
    Bo, Bi, N = 2, 4, 200
    for N1, N2 in ((64, N), (N, 64)):
        q = torch.randn(Bo, N1, Bi, 384, generator=g).to(dev())
        k = torch.randn(Bo, N2, Bi, 384, generator=g).to(dev())
        v = torch.randn(Bo, N2, Bi, 384, generator=g).to(dev())
        km = (torch.rand(Bo, N2, generator=g) < 0.6).to(torch.uint8).to(dev()) if N2 == N else None
        qm = (torch.rand(Bo, N1, generator=g) < 0.6).to(torch.uint8).to(dev()) if N1 == N else None
        out = ops.attention_batch2(q, k, v, key_mask=km, query_mask=qm)
        for bo in range(Bo):
            plain = ops.attention(q[bo].transpose(0, 1).contiguous(), k[bo].transpose(0, 1).contiguous(),
                                  v[bo].transpose(0, 1).contiguous(), key_mask=None if km is None else km[bo].contiguous(),
                                  query_mask=None if qm is None else qm[bo].contiguous())
            assert torch.equal(out[bo], plain.transpose(0, 1)), (N1, N2, bo)


# ------------------------------------------------------------------------------------------------------------------
# 1. - 3. window level: B = 1 identity, no cross-talk, determinism
# ------------------------------------------------------------------------------------------------------------------
def test_b1_is_the_single_window_call(precision):
    from cotracker_amd import ops
    pw = small_model(precision).packed(dev())
    a = random_window(11, 8, 45, iters=3, with_mask=True)
    b = random_window(11, 8, 45, iters=3, with_mask=True)
    ops.forward_window(a, pw)
    ops.forward_windows([b], pw)
    for x, y in zip(state(a), state(b)):
        assert torch.equal(x, y)
    c = random_window(11, 8, 45, iters=3, with_mask=True)
    d = random_window(11, 8, 45, iters=3, with_mask=True)
    g1, gb = ops.WindowGraph(c, pw), ops.WindowBatchGraph([d], pw)
    assert g1.nodes == gb.nodes  # exactly the launches of ctk_forward_window
    g1.launch()
    gb.launch()
    for x, y, z in zip(state(a), state(c), state(d)):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("N,chunk", [(45, None), (100, 70), (77, 100)])
def test_no_cross_talk_and_determinism(precision, N, chunk):
    """B = 2 (and 3): replacing the OTHER videos' pixels and queries leaves video 0's coords / vis / conf bit-identical -- same
    row count, same positions, so no bit may move.  N is not a multiple of 64, and `chunk` points per correlation chunk make a
    chunk straddle the video boundary (70: points 70..139 = 30 of video 0 + 40 of video 1; 100 > N: 77 + 23).  The same joint call
    twice, and its hipGraph, give the same bits."""
    from cotracker_amd import ops
    pw = small_model(precision).packed(dev())
    S = 8

    def run(seeds, graph=False):
        wins = [random_window(s, S, N, iters=2, with_mask=True) for s in seeds]
        if graph:
            gr = ops.WindowBatchGraph(wins, pw, points_per_chunk=chunk)
            gr.launch()
        else:
            ops.forward_windows(wins, pw, points_per_chunk=chunk)
        torch.cuda.synchronize()
        return [state(w) for w in wins]

    base = run([1, 2])
    again = run([1, 2])
    other = run([1, 3])
    graph = run([1, 2], graph=True)
    for b in range(2):
        for x, y, z in zip(base[b], again[b], graph[b]):
            assert torch.equal(x, y) and torch.equal(x, z)               # determinism, graph == direct
    for x, y in zip(base[0], other[0]):
        assert torch.equal(x, y), maxdiff(x, y)                           # video 0 does not see video 1
    assert not torch.equal(base[1][0], other[1][0])
    # every element agrees with its own single-window run to fp32 class (not bits: the GEMM tile dealing differs)
    for b, s in enumerate([1, 2]):
        one = random_window(s, S, N, iters=2, with_mask=True)
        ops.forward_window(one, pw)
        for x, y, tol in zip(base[b], state(one), (2e-4 / 4, 2e-5, 2e-5)):
            assert torch.isfinite(x).all() and maxdiff(x, y) < tol, (b, maxdiff(x, y))
    # three videos, the middle one replaced: the outer two keep their bits
    a3, b3 = run([1, 2, 4]), run([1, 5, 4])
    for b in (0, 2):
        for x, y in zip(a3[b], b3[b]):
            assert torch.equal(x, y)


def test_joint_window_without_space_attention(precision):
    from cotracker_amd import ops
    pw = small_model(precision).packed(dev())
    wins = [random_window(s, 8, 30, iters=2, space_attn=False) for s in (6, 7)]
    ops.forward_windows(wins, pw)
    for s, w in zip((6, 7), wins):
        one = random_window(s, 8, 30, iters=2, space_attn=False)
        ops.forward_window(one, pw)
        for x, y, tol in zip(state(w), state(one), (2e-4 / 4, 2e-5, 2e-5)):
            assert maxdiff(x, y) < tol
        with_space = random_window(s, 8, 30, iters=2)
        ops.forward_window(with_space, pw)
        assert maxdiff(state(w)[0], state(with_space)[0]) > 1e-3  # the flag does something


# ------------------------------------------------------------------------------------------------------------------
# 4. / 6. model level: parity with the reference per element
# ------------------------------------------------------------------------------------------------------------------
def _flipped(v0, q0):
    v1 = v0.flip(1).contiguous()
    q1 = q0.clone()
    q1[..., 1] = 95.0 - q1[..., 1]
    return v1, q1


def test_model_offline_joint(golden, precision):
    g = golden("model_offline")
    m = small_model(precision, "offline", seed=2)
    v0, q0 = t(g["off_video"]), t(g["off_queries"])
    v1, q1 = _flipped(v0, q0)
    single = m(v1, q1, iters=4)
    m.batch_mode = "joint"
    c, v, f, _ = m(torch.cat([v0, v1]), torch.cat([q0, q1]), iters=4)
    assert m.range_fallbacks == 0
    assert maxdiff(c[0], g["off_coords"][0]) < TOL_PX
    assert maxdiff(logit(v[0]), logit(g["off_vis"][0])) < TOL_LOGIT
    assert maxdiff(logit(f[0]), logit(g["off_conf"][0])) < TOL_LOGIT
    assert maxdiff(c[1], single[0][0]) < 2e-4 and maxdiff(logit(v[1]), logit(single[1][0])) < 2e-5
    # an add_space_attn=False forward in joint mode == per element in loop mode (fp32 class)
    cj = m(torch.cat([v0, v1]), torch.cat([q0, q1]), iters=2, add_space_attn=False)
    m.batch_mode = "loop"
    cl = m(torch.cat([v0, v1]), torch.cat([q0, q1]), iters=2, add_space_attn=False)
    assert maxdiff(cj[0], cl[0]) < 2e-4 and maxdiff(logit(cj[1]), logit(cl[1])) < 2e-5


@pytest.mark.parametrize("use_graph", [False, True])
def test_model_online_joint_sliding_and_streaming(golden, precision, use_graph):
    """The construction of test_model_online_batched_streaming (second element: the flipped video with mirrored queries; its
    queries sit on later frames, so early windows carry not-yet-queried tracks in their point_mask) in joint mode."""
    g = golden("model_online")
    m = small_model(precision, "online", seed=1)
    v0, q0 = t(g["on_video"]), t(g["on_queries"])
    v1, q1 = _flipped(v0, q0)
    assert float(q0[..., 0].max()) > 0  # queries on later frames: masked tracks in the first windows
    vb, qb = torch.cat([v0, v1]), torch.cat([q0, q1])
    single_slide = m(v1, q1, iters=4)
    m.hip_graph = use_graph
    m.init_video_online_processing()
    for ind in range(0, v1.shape[1] - 4, 4):
        single_stream = m(v1[:, ind:ind + 8], q1, iters=4, is_online=True)
    single_stream = [x.clone() for x in single_stream[:3]]
    m._resolve_deferred_range_check()

    m.batch_mode = "joint"
    if not use_graph:
        c, v, f, _ = m(vb, qb, iters=4)  # sliding
        assert maxdiff(c[0], g["on_coords"][0]) < TOL_PX
        assert maxdiff(logit(v[0]), logit(g["on_vis"][0])) < TOL_LOGIT
        assert maxdiff(logit(f[0]), logit(g["on_conf"][0])) < TOL_LOGIT
        assert maxdiff(c[1], single_slide[0][0]) < 2e-4 and maxdiff(logit(v[1]), logit(single_slide[1][0])) < 2e-5
    runs = []
    for _ in range(2):
        m.init_video_online_processing()
        for ind in range(0, vb.shape[1] - 4, 4):
            cs, vs, fs, _ = m(vb[:, ind:ind + 8], qb, iters=4, is_online=True)
        runs.append((cs.clone(), vs.clone(), fs.clone()))
        m._resolve_deferred_range_check()
    assert m.range_fallbacks == 0
    if use_graph:
        assert len(m._graphs) == 1 and next(iter(m._graphs.values())).nodes > 100  # ONE graph for the two streams
    for a, b in zip(*runs):
        assert torch.equal(a, b)  # deterministic, state handling included
    cs, vs, fs = runs[0]
    assert maxdiff(cs[0], g["on_stream_coords"][0]) < TOL_PX
    assert maxdiff(logit(vs[0]), logit(g["on_stream_vis"][0])) < TOL_LOGIT
    assert maxdiff(logit(fs[0]), logit(g["on_stream_conf"][0])) < TOL_LOGIT
    assert maxdiff(cs[1], single_stream[0][0]) < 2e-4
    assert maxdiff(logit(vs[1]), logit(single_stream[1][0])) < 2e-5 and maxdiff(logit(fs[1]), logit(single_stream[2][0])) < 2e-5


def test_model_online_joint_feature_cache(golden, precision):
    """online_feature_cache keeps working per element in joint mode (each element encodes through its own cache)."""
    g = golden("model_online")
    m = small_model(precision, "online", seed=1)
    v0, q0 = t(g["on_video"]), t(g["on_queries"])
    v1, q1 = _flipped(v0, q0)
    vb, qb = torch.cat([v0, v1]), torch.cat([q0, q1])
    m.batch_mode = "joint"
    outs = []
    for cache in (False, True):
        m.online_feature_cache = cache
        m.init_video_online_processing()
        for ind in range(0, vb.shape[1] - 4, 4):
            cs, vs, fs, _ = m(vb[:, ind:ind + 8], qb, iters=4, is_online=True)
        outs.append((cs.clone(), vs.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])  # the encoder is per-frame and deterministic


# ------------------------------------------------------------------------------------------------------------------
# 7. range guard: one check for the batch, the whole batch re-runs on the exact-f32 back end
# ------------------------------------------------------------------------------------------------------------------
def test_joint_overflow_gives_defined_result_not_nan():
    """The construction of tests/test_gpu_range.py::test_overflow_gives_defined_result_not_nan (fc1 weights x 3e5: hidden
    activations beyond 65504) on a batch of two in joint mode: one RuntimeWarning, one fallback, finite outputs for both
    elements, equal to the joint exact-f32 run."""
    from cotracker_amd.model import CoTrackerThreeOnline
    from cotracker_amd.synthetic import synthetic_video
    from cotracker_amd.weights import fill_synthetic_

    def build(precision):
        m = CoTrackerThreeOnline(stride=4, corr_radius=3, window_len=8, model_resolution=(64, 96)).eval()
        fill_synthetic_(m, seed=1)
        with torch.no_grad():
            m.updateformer.time_blocks[0].mlp.fc1.weight.mul_(3e5)
            m.updateformer.time_blocks[0].mlp.fc2.weight.mul_(1e-5)
        m.invalidate_packed_weights()
        m.precision = precision
        m.batch_mode = "joint"
        return m.to(dev())

    video = torch.cat([synthetic_video(12, 64, 96, seed=5), synthetic_video(12, 64, 96, seed=6)]).to(dev())
    q = torch.tensor([[[0.0, 20.0, 20.0], [2.0, 60.0, 40.0], [0.0, 80.0, 10.0]]], device=dev()).repeat(2, 1, 1)
    exact = build("f32")
    c32, v32, f32_, _ = exact(video, q, iters=3)
    assert torch.isfinite(c32).all() and exact.range_fallbacks == 0
    m = build("f16x3")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        c, v, f, _ = m(video, q, iters=3)
    assert m.range_fallbacks == 1 and sum(issubclass(x.category, RuntimeWarning) for x in w) == 1
    assert torch.isfinite(c).all() and torch.isfinite(v).all() and torch.isfinite(f).all()
    assert torch.equal(c, c32) and torch.equal(v, v32)
    # joint streaming through the graph: deferred check, the next call raises
    m.hip_graph = True
    m.init_video_online_processing()
    m(video[:, 0:8], q, iters=2, is_online=True)
    with pytest.raises(FloatingPointError, match="f16 range"):
        m(video[:, 4:12], q, iters=2, is_online=True)
    # immediate check: the online states of BOTH elements are restored and the chunk re-runs on f32
    m.stream_range_check = "immediate"
    exact.hip_graph, exact.stream_range_check = True, "immediate"
    for mm in (m, exact):
        mm.init_video_online_processing()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for ind in (0, 4):
            a = m(video[:, ind:ind + 8], q, iters=2, is_online=True)
            b = exact(video[:, ind:ind + 8], q, iters=2, is_online=True)
    assert torch.equal(a[0], b[0]) and torch.isfinite(a[0]).all()


# ------------------------------------------------------------------------------------------------------------------
# 4. at real resolution (tests/test_gpu_scale.py style): C2 twice in one batch, C4 streaming with B = 2
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2", "c4"])
def test_scale_parity_joint(name, precision, golden):
    from cotracker_amd import model as M
    from cotracker_amd.predictor import CoTrackerOnlinePredictor, CoTrackerPredictor
    from cotracker_amd.synthetic import synthetic_video
    from cotracker_amd.weights import fill_synthetic_
    path = os.path.join(ROOT, "tests", "golden", f"scale_{name}.npz")
    if not os.path.exists(path):
        pytest.skip(f"{path} not generated")
    g = golden(f"scale_{name}")
    H, W, T, G, wl = {"c2": (256, 256, 48, 20, 60), "c4": (512, 512, 48, 32, 16)}[name]
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=wl) if name == "c4" else CoTrackerPredictor(checkpoint=None, offline=True, window_len=wl)
    assert p.model.precision == precision
    fill_synthetic_(p.model, seed=0)
    p = p.to(dev())
    p.model.batch_mode = "joint"
    video = synthetic_video(T, H, W, seed=1234).to(dev())
    other = synthetic_video(T, H, W, seed=99).to(dev())
    captured = {}
    fwd = p.model.forward

    def tap(*a, **k):
        out = fwd(*a, **k)
        captured["coords"] = out[0].clone()
        return out

    p.model.forward = tap
    if name == "c2":  # the golden video twice in one batch
        vb = torch.cat([video, video])
        tracks, vis = p(vb, grid_size=G)
        elems = (0, 1)
    else:  # the golden stream beside a different one; the grid queries are repeated per element
        vb = torch.cat([other, video])
        p(video_chunk=vb[:, :2 * p.step], is_first_step=True, grid_size=G)
        p.queries = p.queries.repeat(2, 1, 1)
        for ind in range(0, T - p.step, p.step):
            tracks, vis = p(video_chunk=vb[:, ind: ind + 2 * p.step])
        p.finish()
        assert len(p.model._graphs) == 1
        elems = (1,)
    assert p.model.range_fallbacks == 0
    vl, cl = p.model.last_logits
    for b in elems:
        assert maxdiff(captured["coords"][b], g["coords"]) <= TOL_PX, (b, maxdiff(captured["coords"][b], g["coords"]))
        assert maxdiff(vl[b], g["vis_logit"]) <= TOL_LOGIT and maxdiff(cl[b], g["conf_logit"]) <= TOL_LOGIT
        if "tracks" in g:
            assert maxdiff(tracks[b], g["tracks"]) <= 2 * TOL_PX
