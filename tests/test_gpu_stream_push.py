"""Pushing new frames into a live stream (-m gpu): the ingest kernel (ops.ingest_frames; csrc/ingest.hip: ctk_ingest_frames), the
resident pyramid that keeps its overlap (ops.StreamGroups.advance_pyramid), model.stream_push and
CoTrackerOnlinePredictor.push_frames.

The oracle is this repository's own chunk path: a stream fed overlapping chunks through forward on the device stream state
(stream_slots) returns, call for call, what the pushed stream returns -- torch.equal on tracks and both logits, because the encoder
and the pooling are per frame and the kept features are therefore the bits a re-computation gives.  The kernel is compared with a
float64 restatement computed on the GPU and, bit for bit, with F.interpolate on the GPU.  Shapes and helpers as in
tests/test_gpu_stream_slots.py."""
import functools
import warnings

import pytest
import torch
import torch.nn.functional as F

import ctk_support
from ctk_support import HW, S, STEP, STRIDE, dev, fp64_resize, maxdiff, ulps

pytestmark = pytest.mark.gpu

source = functools.partial(ctk_support.source, device=dev())
nchw = functools.partial(ctk_support.nchw, contiguous=True)
_models = {}
small_model = functools.partial(ctk_support.small_model, _models, batch_mode="loop", hip_graph=False, range_guard=True, stream_groups=False,
                                stream_slots=False, online_feature_cache=False, stream_range_check="deferred")
# the oracle: a copy of the model, fed overlapping chunks through forward on the device stream state
chunk_model = functools.partial(ctk_support.copy_without_stream_state, stream_slots=True)
# query frames spread over the stream
stream_inputs = functools.partial(ctk_support.stream_inputs,
                                  frames=lambda T: [0, 0, 2, 3, 7, 9, T // 2 - 1, T // 2, T // 2 + 1, T - S, T - 5, T - 2])


# ---- the kernel -------------------------------------------------------------------------------------------------------------
CASES = [  # (H, W, h, w)
    (1080, 1920, 384, 512), (480, 640, 384, 512), (100, 100, 384, 512), (37, 53, 19, 31), (64, 96, 64, 96), (160, 240, 64, 96),
    (50, 70, 1, 40), (50, 70, 30, 1), (50, 70, 1, 1), (1, 1, 8, 12), (2, 3, 7, 9),
]


def ingest(src, layout, size, out=None):
    from cotracker_amd import ops
    if out is None:
        out = torch.empty(src.shape[0], 3, *size, device=dev())
    return ops.ingest_frames(src, out, layout=layout)


@pytest.mark.parametrize("H,W,h,w", CASES)
@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_ingest_vs_fp64_and_interpolate(dtype, layout, H, W, h, w):
    src = source(dtype, layout, 2, H, W, seed=H + w)
    got = ingest(src, layout, (h, w))
    x = nchw(src, layout)
    assert ulps(got, fp64_resize(x, (h, w))) <= 3.0
    ref = F.interpolate(x, (h, w), mode="bilinear", align_corners=True)
    assert torch.equal(got, ref), (maxdiff(got, ref), int((got != ref).sum()), ulps(got, ref))  # bit equality is the aim


def test_ingest_uint8_equals_float_and_layouts_agree():
    for layout in ("hwc", "chw"):
        src = source(torch.uint8, layout, 3, 45, 61, seed=9)
        assert torch.equal(ingest(src, layout, (32, 48)), ingest(src.float(), layout, (32, 48)))
    src = source(torch.uint8, "hwc", 3, 45, 61, seed=11)
    assert torch.equal(ingest(src, "hwc", (32, 48)), ingest(src.permute(0, 3, 1, 2).contiguous(), "chw", (32, 48)))
    assert torch.equal(ingest(src, None, (32, 48)), ingest(src, "hwc", (32, 48)))  # the layout is read off the shape


@pytest.mark.parametrize("layout,pad", [("hwc", (5, 7)), ("hwc", (0, 11)), ("chw", (0, 9))])
def test_ingest_strided_source(layout, pad):
    from cotracker_amd import ops
    for dtype in (torch.uint8, torch.float32):
        src = source(dtype, layout, 3, 60, 80, seed=5, pad=pad)
        assert not src.is_contiguous()
        assert torch.equal(ingest(src, layout, (24, 32)), ingest(src.contiguous(), layout, (24, 32)))
        assert torch.equal(ingest(src[1:], layout, (24, 32)), ingest(src, layout, (24, 32))[1:])
    with pytest.raises(ValueError, match="not dense"):
        ops.ingest_frames(source(torch.uint8, "hwc", 2, 60, 80, seed=1)[:, :, ::2], torch.empty(2, 3, 24, 32, device=dev()), layout="hwc")
    with pytest.raises(ValueError, match="not dense"):
        ops.ingest_frames(source(torch.uint8, "chw", 2, 60, 80, seed=1, pad=(4, 0)), torch.empty(2, 3, 24, 32, device=dev()), layout="chw")


def test_ingest_identity_is_a_copy_and_a_row_range_leaves_the_rest_alone():
    src = source(torch.uint8, "hwc", 3, *HW, seed=3)
    assert torch.equal(ingest(src, "hwc", HW), nchw(src, "hwc"))
    big = source(torch.uint8, "hwc", 3, 160, 240, seed=4)
    buf = torch.full((8, 3, *HW), -7.25, device=dev())
    before = buf.clone()
    ingest(big, "hwc", HW, out=buf[2:5])
    assert torch.equal(buf[:2], before[:2]) and torch.equal(buf[5:], before[5:])
    assert torch.equal(buf[2:5], F.interpolate(nchw(big, "hwc"), HW, mode="bilinear", align_corners=True))
    odd = torch.full((4, 3, 19, 31), -7.25, device=dev())  # a width that is stored float by float
    ingest(source(torch.uint8, "chw", 1, 37, 53, seed=6), "chw", (19, 31), out=odd[1:2])
    assert float(odd[0].max()) == -7.25 and float(odd[2:].max()) == -7.25 and float(odd[1].min()) >= 0.0


# ---- the resident pyramid -----------------------------------------------------------------------------------------------------
def test_advance_pyramid_equals_set_pyramid_of_the_full_chunk():
    from cotracker_amd import ops
    g = torch.Generator().manual_seed(2)
    f = torch.randn(S + 2 * STEP + 3, HW[0] // STRIDE, HW[1] // STRIDE, 128, generator=g).to(dev())
    q = torch.zeros(1, 3, 3, device=dev())
    sizes = [(HW[0] // STRIDE >> l, HW[1] // STRIDE >> l) for l in range(4)]
    a, b = ops.StreamGroups(q, S, STEP, STRIDE, sizes), ops.StreamGroups(q, S, STEP, STRIDE, sizes)
    ptrs, serial = [p_.data_ptr() for p_ in a.pyr], a.serial
    a.set_pyramid(f[:S])
    for k, (t0, n) in enumerate([(STEP, STEP), (2 * STEP, STEP), (3 * STEP, 3)]):  # two full steps, then a short closing chunk
        a.advance_pyramid(f[t0 + S - STEP:t0 + S - STEP + n], S - STEP + n)
        b.set_pyramid(f[t0:t0 + S - STEP + n])
        for l in range(4):
            assert torch.equal(a.pyr[l], b.pyr[l]), (k, l, maxdiff(a.pyr[l], b.pyr[l]))
    assert [p_.data_ptr() for p_ in a.pyr] == ptrs and a.serial == serial


# ---- model.stream_push ----------------------------------------------------------------------------------------------------------
def assert_same(got, want, what):
    for name, x, y in zip(("tracks", "vis", "conf"), got, want):
        assert x.shape == y.shape and torch.equal(x, y), (what, name, maxdiff(x, y))


def run_both(m, ref, video, q, iters=2, between=None):
    """Push `video` into m and feed ref its chunks; compare after EVERY call.  Full calls while a whole window fits, then the
    closing chunk of what is left (< STEP new frames).  between(k, model) runs on both before call k."""
    T = video.shape[1]
    m.init_video_online_processing()
    ref.init_video_online_processing()
    starts = list(range(0, max(T - S, 0) + 1, STEP))
    rest = T - (starts[-1] + S) if T >= S else 0
    calls = 0
    for k, t0 in enumerate(starts):
        if k and between is not None:
            between(k, m)
            between(k, ref)
        new = video[0, :S] if k == 0 else video[0, t0 + S - STEP:t0 + S]
        short = T < S
        got = m.stream_push(new, q, iters=iters, final=short)
        want = ref(video[:, t0:t0 + S], q, iters=iters, is_online=True)
        assert_same(got[:3], want[:3], ("call", k))
        assert_same(m.last_logits, ref.last_logits, ("logits", k))
        assert m.online_ind == ref.online_ind == t0 + STEP
        calls += 1
    if rest:
        t0 = starts[-1] + STEP
        got = m.stream_push(video[0, t0 + S - STEP:], q, iters=iters, final=True)
        want = ref(video[:, t0:], q, iters=iters, is_online=True)
        assert got[0].shape[1] == T
        assert_same(got[:3], want[:3], "closing chunk")
        assert_same(m.last_logits, ref.last_logits, "closing logits")
        calls += 1
    m._resolve_deferred_range_check()
    ref._resolve_deferred_range_check()
    return calls


@pytest.mark.parametrize("G,mode", [(1, "loop"), (4, "loop"), (4, "joint")])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_stream_push_equals_forward(precision, graph, G, mode):
    """Six full calls and a closing chunk of STEP - 1 new frames, an assign and a release in the middle, then a second stream on
    the same model: the same buffers, no new graph."""
    from cotracker_amd import ops
    m = small_model(precision)
    m.hip_graph, m.batch_mode = graph, mode
    ref = chunk_model(m)
    N, T = 10, S + 5 * STEP + STEP - 1
    video, q = stream_inputs(G, N, T, seed=3 + G)
    q[-1, 3:5] = torch.tensor([ops.EMPTY_FRAME, 0.0, 0.0], device=dev())  # two slots that wait for an occupant
    newq = torch.tensor([[4.0 * STEP + 1, 30.0, 20.0]], device=dev())

    def between(k, model):
        if k == 3:
            model.stream_assign([(G - 1) * N + 3], newq)
        if k == 4:
            model.stream_release([1])
            assert not bool(model.stream_occupied[0, 1]) and bool(model.stream_occupied[G - 1, 3])

    with pytest.raises(RuntimeError, match="stream_slots is off"):
        m.stream_assign([0], newq)  # no push stream yet, and the switch is off
    assert run_both(m, ref, video, q, between=between) == 7
    assert m.stream_slots is False and m.stream_groups is False  # independent of the switches
    assert m.range_fallbacks == ref.range_fallbacks
    with pytest.raises(AssertionError, match="ends the stream"):
        m.stream_push(video[0, :STEP], q, iters=2)
    with pytest.raises(RuntimeError, match="fed through stream_push"):
        m(video[:, :S], q, iters=2, is_online=True)
    # a second stream on the same model: the resident buffers and the captured graphs serve it
    gs, graphs = m._gstream, dict(m._graphs)
    ptrs = [p_.data_ptr() for p_ in gs.pyr]
    video2, q2 = stream_inputs(G, N, S + 2 * STEP, seed=11)
    assert run_both(m, ref, video2, q2) == 3
    assert m._gstream is gs and [p_.data_ptr() for p_ in gs.pyr] == ptrs
    assert m._graphs.keys() == graphs.keys() and all(m._graphs[k_] is graphs[k_] for k_ in graphs) and bool(graphs) == graph
    # ... and after init_video_online_processing() the model takes chunks again
    m.init_video_online_processing()
    ref.init_video_online_processing()
    m.stream_slots = True  # (the chunk path of G > 1 needs a switch; the push path did not)
    assert_same(m(video2[:, :S], q2, iters=2, is_online=True)[:1], ref(video2[:, :S], q2, iters=2, is_online=True)[:1], "chunks again")
    with pytest.raises(RuntimeError, match="fed through forward"):
        m.stream_push(video2[0, S:S + STEP], q2, iters=2)
    m._resolve_deferred_range_check()
    ref._resolve_deferred_range_check()


@pytest.mark.parametrize("graph", [False, True])
def test_stream_shorter_than_one_window(graph):
    m = small_model("f16x3")
    m.hip_graph = graph
    ref = chunk_model(m)
    video, q = stream_inputs(2, 6, 5, seed=8)
    q[..., 0] = q[..., 0].clamp(max=4.0)
    assert run_both(m, ref, video, q) == 1
    m.init_video_online_processing()
    with pytest.raises(ValueError, match="final=True"):
        m.stream_push(video[0], q, iters=2)  # five frames are no first window unless the caller says the video ends here
    assert m._feed is None


def test_push_frame_counts_are_checked():
    m = small_model("f16x3")
    video, q = stream_inputs(1, 4, S + STEP, seed=9)
    m.init_video_online_processing()
    for n in (STEP, S + 1):
        with pytest.raises((ValueError, AssertionError)):
            m.stream_push(video[0, :n], q, iters=2)
    m.stream_push(video[0, :S], q, iters=2)
    for n in (S, STEP - 1, STEP + 1):
        with pytest.raises(ValueError, match="new frames"):
            m.stream_push(video[0, :n], q, iters=2)
    m.stream_push(video[0, S:], q, iters=2)
    assert m.online_ind == 2 * STEP


def test_forced_range_guard_hit_reruns_on_f32_like_forward():
    """The stress weights of tests/test_gpu_range.py: every window overflows the f16 range (in the arithmetic: no fault) and is
    re-run on the exact-f32 back end; the pyramid advance and the support step are not repeated."""
    from cotracker_amd.model import CoTrackerThreeOnline
    from cotracker_amd.weights import fill_synthetic_
    m = CoTrackerThreeOnline(stride=STRIDE, corr_radius=3, window_len=S, model_resolution=HW).eval()
    fill_synthetic_(m, seed=1)
    with torch.no_grad():
        m.updateformer.time_blocks[0].mlp.fc1.weight.mul_(3e5)
        m.updateformer.time_blocks[0].mlp.fc2.weight.mul_(1e-5)
    m.invalidate_packed_weights()
    m = m.to(dev())
    video, q = stream_inputs(2, 5, S + 2 * STEP + 2, seed=4)
    for graph in (False, True):
        m.hip_graph, m.stream_range_check = graph, "immediate"
        ref = chunk_model(m)
        before = m.range_fallbacks
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert run_both(m, ref, video, q) == 4
        assert m.range_fallbacks - before == 4 == ref.range_fallbacks - before
        exact = chunk_model(m)
        exact.precision, exact.stream_slots = "f32", False
        m.init_video_online_processing()
        exact.init_video_online_processing()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            a = m.stream_push(video[0, :S], q, iters=2)
        b = exact.stream_push(video[0, :S], q, iters=2)
        assert_same(a[:3], b[:3], "the re-run IS the exact-f32 back end") and torch.isfinite(a[0]).all()
    # deferred (the graph default): the NEXT push raises
    m.hip_graph, m.stream_range_check = True, "deferred"
    m.init_video_online_processing()
    m.stream_push(video[0, :S], q, iters=2)
    with pytest.raises(FloatingPointError, match="f16 range"):
        m.stream_push(video[0, S:S + STEP], q, iters=2)


# ---- CoTrackerOnlinePredictor.push_frames ---------------------------------------------------------------------------------------
def small_predictor(G):
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    from cotracker_amd.weights import fill_synthetic_
    from cotracker_amd.model import CoTrackerThreeOnline
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=S)
    model = CoTrackerThreeOnline(stride=STRIDE, corr_radius=3, window_len=S, model_resolution=HW).eval()
    fill_synthetic_(model, seed=5)
    model.hip_graph = True
    p.model, p.interp_shape, p.step = model, HW, STEP
    return p.to(dev())


def predictor_case(G, seed=21):
    H, W = 160, 240  # 2.5x the model resolution
    T = S + 4 * STEP + 3
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, generator=g)
    q = (torch.rand(G, 6, 3, generator=g) * torch.tensor([1.0, W - 1.0, H - 1.0]))
    q[..., 0] = torch.tensor([0.0, 0.0, 3.0, 9.0, 14.0, 20.0])
    return frames, q.to(dev()), torch.tensor([[4.0 * STEP + 2, 100.0, 60.0]], device=dev())


def chunk_predictor_results(G, frames, q, add=None):
    """What forward returns call by call for the float chunks of `frames`, on the device stream state."""
    T = frames.shape[0]
    video = frames.permute(0, 3, 1, 2)[None].float().to(dev())
    ref = small_predictor(G)
    ref.spare_points = 2
    ref(video[:, :1], is_first_step=True, queries=q, add_support_grid=True)
    ref.model.stream_slots = True
    want = []
    for k, t0 in enumerate(range(0, T - S + STEP, STEP)):  # the last chunk is short: 3 new frames
        if k == 3 and add is not None:
            ref.add_queries(add, group=G - 1)
        want.append(tuple(x.clone() for x in ref(video[:, t0:t0 + S], add_support_grid=True)))
    ref.finish()
    assert want[-1][0].shape == (G, T, 8, 2) and len(want) == 6
    return want


@pytest.mark.parametrize("G", [1, 3])
def test_push_frames_uint8_hwc_equals_forward_on_float_chunks(G):
    """A uint8 channels-last source at 2.5x the model resolution, pushed 1, 3, STEP and 3 * STEP + 2 frames at a time, from the
    host and from the device: every partition gives the same bits, and they are the bits of forward on the float chunks (the
    kernel test proves bit equality with F.interpolate), support grid and spare points included."""
    frames, q, _ = predictor_case(G)
    T, H, W = frames.shape[:3]
    want = chunk_predictor_results(G, frames, q)
    for part, where in ((1, "host"), (3, "device"), (STEP, "host"), (3 * STEP + 2, "device")):
        p = small_predictor(G)
        p.spare_points = 2
        p(torch.zeros(1, 1, 3, H, W, device=dev()), is_first_step=True, queries=q, add_support_grid=True)  # a one-frame dummy
        src = frames if where == "host" else frames.to(dev())
        got, done = [], 0
        for i in range(0, T, part):
            out = p.push_frames(src[i:i + part], final=i + part >= T, add_support_grid=True)
            fed = min(i + part, T)
            before, done = done, 0 if fed < S else (fed - S) // STEP + 1 + (fed == T)  # (the closing chunk is one more step)
            assert (out[0] is not None) == (done > before)  # a push that completes no window returns (None, None)
            if out[0] is not None:
                assert out[0].shape[1] == (T if fed == T else S + STEP * (done - 1)) and out[1].dtype == torch.bool
                got.append((done - 1, out))
        p.finish()
        assert got[-1][0] == len(want) - 1
        for k, (a, b) in ((k, (o, want[k])) for k, o in got):  # every result a push returned is forward's k-th result
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (part, k, maxdiff(a[0], b[0]))
        if part == 1:
            assert [k for k, _ in got] == list(range(len(want)))
        assert p._push_buf.shape == (S, 3, *HW)
        with pytest.raises(RuntimeError, match="ended this stream"):
            p.push_frames(src[:1])
        with pytest.raises(RuntimeError, match="fed through stream_push"):
            p(torch.zeros(1, S, 3, H, W, device=dev()))


def test_push_frames_float_planar_and_add_remove_queries():
    """float32 planar frames, four per push; add_queries / remove_queries between two pushes of the running stream."""
    G = 2
    frames, q, add = predictor_case(G, seed=22)
    T, H, W = frames.shape[:3]
    want = chunk_predictor_results(G, frames, q, add=add)
    p = small_predictor(G)
    p.spare_points = 2
    src = frames.permute(0, 3, 1, 2).float().contiguous().to(dev())
    p(src[None, :1], is_first_step=True, queries=q, add_support_grid=True)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.add_queries(add)
    got = []
    for i in range(0, T, STEP):
        if i == S + 2 * STEP:  # windows 0..2 have run: before the fourth
            assert p.add_queries(add, group=G - 1).tolist() == [6]
        out = p.push_frames(src[i:i + STEP], final=i + STEP >= T, add_support_grid=True)
        if out[0] is not None:
            got.append(out)
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (k, maxdiff(a[0], b[0]))
    p.finish()
