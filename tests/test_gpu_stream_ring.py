"""Endless streams (-m gpu): the ring history of the device stream state (ops.StreamGroups(ring_rows=K); csrc/stream.hip:
ctk_stream_*_ring), the emit kernel (ctk_stream_emit), model.stream_history_frames and CoTrackerOnlinePredictor.history_frames /
recent / window_start.

The oracle is this repository's own unbounded stream on the device stream state: call for call, the ring stream returns rows
[ind, ind + T) of what the unbounded stream returns -- torch.equal on tracks and on both probabilities at the model level and on the
tracks at the predictor level.  The predictor's visibility is computed inside the emit kernel with expf, where the unbounded path
uses torch.sigmoid: an expf within 2 ulp moves the product p = sigmoid(v) * sigmoid(c) by at most about 5 ulp of 0.6 = 3e-7, so the
two must agree wherever the unbounded path's own p has |p - 0.6| > BAND = 1e-6 (3x that); at most BAND_SHARE of the elements may lie
inside the band (asserted on the unbounded path's values), and the mismatches found inside it are written to
$CTK_SESSION_OUT/stream_ring_visibility.json (default session_out/).  Shapes and helpers as in tests/test_gpu_stream_push.py."""
import functools
import json
import os
import warnings

import pytest
import torch

import ctk_support
from ctk_support import HW, ROOT, S, STEP, STRIDE, bits, count_encodes, dev, maxdiff

pytestmark = pytest.mark.gpu

BAND, BAND_SHARE, THRESH = 1e-6, 1e-4, 0.6
RINGS = (S, S + STEP + 3, 4 * S)  # the ring wraps every call / at offsets that are no multiples of STEP / every fourth call
CALLS = 40                        # full calls; a short closing chunk follows
T_LONG = S + (CALLS - 1) * STEP + STEP - 1
_models = {}
small_model = functools.partial(ctk_support.small_model, _models, "f16x3", batch_mode="loop", hip_graph=False, range_guard=True,
                                stream_groups=True, stream_slots=True, online_feature_cache=False, stream_range_check="deferred")
fresh_copy = functools.partial(ctk_support.copy_without_stream_state, stream_slots=True)
# query frames at 0 and spread over the whole stream, the last chunks included
stream_inputs = functools.partial(ctk_support.stream_inputs,
                                  frames=lambda T: [0, 0, 2, 3, 7, 9, T // 4, T // 2 - 1, T // 2, T // 2 + 1, T - S, T - 5, T - 2])


def calls_of(T):
    """[(first frame, frames)] of the calls of a stream over T frames: full windows, then the short closing chunk if frames are left."""
    starts = list(range(0, T - S + 1, STEP))
    out = [(t0, S) for t0 in starts]
    if T - (starts[-1] + S):
        out.append((starts[-1] + STEP, T - starts[-1] - STEP))
    return out


def model_call(m, feed, video, q, k, t0, n, iters=2):
    if feed == "chunks":
        return m(video[:, t0:t0 + n], q, iters=iters, is_online=True)
    new = video[0, :n] if k == 0 else video[0, t0 + S - STEP:t0 + n]
    return m.stream_push(new, q, iters=iters, final=n < S)


# ---- 1. identity with the unbounded stream, model level -----------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("G,mode", [(1, "loop"), (1, "joint"), (3, "loop"), (3, "joint")])
@pytest.mark.parametrize("feed", ["chunks", "push"])
def test_model_returns_the_unbounded_streams_rows(feed, G, mode, graph):
    """41 calls (the last one short); the three ring sizes run beside ONE unbounded stream, compared after every call."""
    base = small_model(hip_graph=graph, batch_mode=mode)
    ref = fresh_copy(base)
    rings = []
    for K in RINGS:
        m = fresh_copy(base)
        m.stream_history_frames = K
        m.stream_slots = m.stream_groups = False  # the ring alone sends the stream -- G == 1 fed by chunks included -- onto the device state
        rings.append(m)
    video, q = stream_inputs(G, 9, T_LONG, seed=31 + G)
    for m in [ref, *rings]:
        m.init_video_online_processing()
    calls = calls_of(T_LONG)
    assert len(calls) == CALLS + 1 and calls[-1][1] < S
    for k, (t0, n) in enumerate(calls):
        want = model_call(ref, feed, video, q, k, t0, n)
        assert want[0].shape[1] == t0 + n
        for K, m in zip(RINGS, rings):
            got = model_call(m, feed, video, q, k, t0, n)
            assert m.stream_window_start == t0 and m.online_ind == ref.online_ind
            for name, x, y in zip(("coords", "vis", "conf"), got[:3], want[:3]):
                assert x.shape == y[:, t0:].shape and x.is_contiguous(), (K, k, name, x.shape)
                assert torch.equal(x, y[:, t0:]), (K, k, name, maxdiff(x, y[:, t0:]))
            for x, y in zip(m.last_logits, ref.last_logits):
                assert torch.equal(bits(x), bits(y[:, t0:])), (K, k, "logits")
            gs = m._gstream
            assert gs.ring_rows == K == gs.T_cap and m.online_coords_predicted is gs.hist[0] and gs.hist[0].shape[1] == K
    for m in [ref, *rings]:
        m._resolve_deferred_range_check()
    assert all(m.range_fallbacks == ref.range_fallbacks for m in rings)


# ---- predictors -----------------------------------------------------------------------------------------------------------------
RAW = (160, 240)  # 2.5x the model resolution


def small_predictor(graph=True, mode="loop", history=None, spare=2):
    from cotracker_amd.model import CoTrackerThreeOnline
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    from cotracker_amd.weights import fill_synthetic_
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=S)
    model = CoTrackerThreeOnline(stride=STRIDE, corr_radius=3, window_len=S, model_resolution=HW).eval()
    fill_synthetic_(model, seed=5)
    model.hip_graph, model.batch_mode = graph, mode
    p.model, p.interp_shape, p.step = model, HW, STEP
    p.spare_points, p.history_frames = spare, history
    return p.to(dev())


def predictor_case(G, T, seed=21):
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (T, *RAW, 3), dtype=torch.uint8, generator=g).to(dev())
    q = torch.rand(G, 6, 3, generator=g) * torch.tensor([1.0, RAW[1] - 1.0, RAW[0] - 1.0])
    q[..., 0] = torch.tensor([0.0, 0.0, 3.0, 9.0, float(T // 2), float(T - 6)])
    return frames, q.to(dev())


def first_step(p, q):
    p(torch.zeros(1, 1, 3, *RAW, device=dev()), is_first_step=True, queries=q, add_support_grid=True)
    p.model.stream_slots = True  # (the unbounded chunk stream of one query set runs on the device stream state, like the ring)


def predictor_call(p, feed, frames, k, t0, n):
    if feed == "chunks":
        return p(frames[t0:t0 + n].permute(0, 3, 1, 2)[None].float(), add_support_grid=True)
    new = frames[:n] if k == 0 else frames[t0 + S - STEP:t0 + n]
    return p.push_frames(new, final=n < S, add_support_grid=True)


class Band:
    """The visibility rule of the module docstring, accumulated over the calls of a test."""

    def __init__(self, products):
        """products: every p of the unbounded path that the test is going to compare against.  FIRST, before any comparison: at most
        BAND_SHARE of them lie inside the band."""
        self.total = sum(p.numel() for p in products)
        self.inside = sum(int(((p - THRESH).abs() <= BAND).sum()) for p in products)
        assert self.total > 0 and self.inside <= BAND_SHARE * self.total, (self.inside, self.total)
        self.compared = self.mismatch_inside = 0

    @staticmethod
    def product(ref, f0, f1, N=8):
        """p of frames [f0, f1) from the logits the unbounded predictor's model holds (a clone: the history moves on)."""
        v, c = (x[:, f0:f1, :N] for x in ref.model.last_logits)
        return torch.sigmoid(v) * torch.sigmoid(c)

    def compare(self, got, want, p, what):
        inside = (p - THRESH).abs() <= BAND  # (a NaN product lies outside: it must be "not visible" on both paths)
        assert got.dtype == torch.bool and got.shape == want.shape == p.shape, (what, got.shape, want.shape, p.shape)
        assert torch.equal(got | inside, want | inside) and torch.equal(got & ~inside, want & ~inside), \
            (what, int(((got != want) & ~inside).sum()))
        self.compared += p.numel()
        self.mismatch_inside += int(((got != want) & inside).sum())

    def finish(self, name):
        print(f"visibility band {name}: {self.inside} of {self.total} elements inside, {self.mismatch_inside} mismatches inside "
              f"({self.compared} comparisons)")
        out = os.environ.get("CTK_SESSION_OUT") or os.path.join(ROOT, "session_out")
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "stream_ring_visibility.json")
        rep = json.load(open(path)) if os.path.exists(path) else {}
        rep[name] = {"elements": self.total, "in_band": self.inside, "in_band_mismatches": self.mismatch_inside, "band": BAND}
        with open(path, "w") as f:
            json.dump(rep, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("G,mode", [(1, "loop"), (1, "joint"), (3, "loop"), (3, "joint")])
@pytest.mark.parametrize("feed", ["chunks", "push_u8"])
def test_predictor_returns_the_unbounded_streams_rows(feed, G, mode, graph):
    """As above through CoTrackerOnlinePredictor: float chunks through forward, or uint8 channels-last frames through push_frames;
    support grid and two spare points, so the emit drops points and masks the empty slots."""
    frames, q = predictor_case(G, T_LONG)
    ref = small_predictor(graph, mode)
    first_step(ref, q)
    wants = []  # the unbounded stream first: per call its rows [t0, t0 + n) and their p
    for k, (t0, n) in enumerate(calls_of(T_LONG)):
        want = predictor_call(ref, feed, frames, k, t0, n)
        assert want[0].shape == (G, t0 + n, 8, 2)
        wants.append((want[0][:, t0:].clone(), want[1][:, t0:].clone(), Band.product(ref, t0, t0 + n)))
    band = Band([w[2] for w in wants] * len(RINGS))
    rings = [small_predictor(graph, mode, history=K) for K in RINGS]
    for p in rings:
        first_step(p, q)
    for k, (t0, n) in enumerate(calls_of(T_LONG)):
        for K, p in zip(RINGS, rings):
            got = predictor_call(p, feed, frames, k, t0, n)
            assert p.window_start == t0 and got[0].shape == (G, n, 8, 2) and got[1].shape == (G, n, 8)
            assert torch.equal(got[0], wants[k][0]), (K, k, maxdiff(got[0], wants[k][0]))
            band.compare(got[1], wants[k][1], wants[k][2], (K, k))
            assert not bool(got[1][:, :, 6:].any())  # the spare points are empty slots
    for p in [ref, *rings]:
        p.finish()
    band.finish(f"predictor-{feed}-G{G}-{mode}-{'graph' if graph else 'direct'}")


# ---- 2. slots under the ring, 3. recent(n) --------------------------------------------------------------------------------------
@pytest.mark.parametrize("feed", ["chunks", "push_u8"])
@pytest.mark.parametrize("G", [1, 3])
def test_add_and_remove_queries_under_the_ring_and_recent(feed, G):
    """K = S + STEP + 3 = 15 rows.  Slot 6 gets an occupant before call 3, loses it before call 8 and gets another before call 14,
    long after the ring has wrapped over the first occupant's rows; slot 7 is filled before call 5; point 1 is removed before call
    10.  Every call equals the unbounded stream's rows, nothing is visible below a slot's first row, and recent(n) -- n on both
    sides of the wrap point -- equals the last n rows of the unbounded return."""
    K, T = S + STEP + 3, S + 19 * STEP + 2
    frames, q = predictor_case(G, T, seed=23)
    grp = G - 1
    plan = {3: ("add", [[4.0 * STEP + 2, 100.0, 60.0]]), 5: ("add", [[6.0 * STEP + 1, 30.0, 90.0]]), 8: ("remove", [6]),
            10: ("remove", [1]), 14: ("add", [[16.0 * STEP + 3, 200.0, 20.0], [15.0 * STEP, 10.0, 10.0]])}

    def between(x, k):
        if k in plan:
            what, arg = plan[k]
            if what == "remove":
                x.remove_queries(arg, group=grp)
            else:
                pts = x.add_queries(torch.tensor(arg, device=dev()), group=grp)
                # the lowest free slots: first the spare one, later the removed point's and the released spare
                assert pts.tolist() == {3: [6], 5: [7], 14: [1, 6]}[k]

    def recent_sizes(done):
        wrap = done % K  # recent(n) wraps exactly when n > done % K
        return sorted({1, max(wrap - 1, 1), max(wrap, 1), min(wrap + 1, K), K - 1, K})

    ref = small_predictor()
    first_step(ref, q)
    wants, firsts = [], []  # the unbounded stream first: per call its last K rows, their p, and the slots' first rows
    for k, (t0, n) in enumerate(calls_of(T)):
        between(ref, k)
        want = predictor_call(ref, feed, frames, k, t0, n)
        lo = max(t0 + n - K, 0)
        wants.append((want[0][:, lo:].clone(), want[1][:, lo:].clone(), Band.product(ref, lo, t0 + n)))
        if n == S:  # (the short chunk closes the stream, and with it the model's slot bookkeeping)
            firsts.append(ref.model.stream_first_row)
    products = []
    for k, (t0, n) in enumerate(calls_of(T)):
        products.append(wants[k][2][:, -n:])
        if k >= 2:
            products += [wants[k][2][:, -m_:] for m_ in recent_sizes(t0 + n)]
    band = Band(products)
    p = small_predictor(history=K)
    first_step(p, q)
    for k, (t0, n) in enumerate(calls_of(T)):
        between(p, k)
        got = predictor_call(p, feed, frames, k, t0, n)
        wt, wv, wp = wants[k]
        assert torch.equal(got[0], wt[:, -n:]), (k, maxdiff(got[0], wt[:, -n:]))
        band.compare(got[1], wv[:, -n:], wp[:, -n:], k)
        # first_row masking, on the ring's own return: nothing is visible in an empty slot or below a slot's first row
        if n == S:
            first = p.model.stream_first_row[:, :8]
            assert torch.equal(p.model.stream_first_row, firsts[k])
            first[~p.model.stream_occupied[:, :8]] = torch.iinfo(torch.long).max
        below = (torch.arange(t0, t0 + n)[None, :, None] < first[:, None, :]).to(dev())
        assert not bool((got[1] & below).any()), k
        if k >= 2:
            for m_ in recent_sizes(t0 + n):
                r = p.recent(m_)
                assert r[0].shape == (G, m_, 8, 2) and torch.equal(r[0], wt[:, -m_:]), (k, m_)
                band.compare(r[1], wv[:, -m_:], wp[:, -m_:], (k, "recent", m_))
        if k == 14:
            # the slot's new occupant: the rows of the ring that the first occupant once wrote (frames long gone) and everything
            # before this window are cleared -- tracks exactly zero, nothing visible
            r = p.recent(K)
            old = r[0][grp, :K - n, 6]
            assert float(old.abs().max()) == 0.0 and not bool(r[1][grp, :K - n, 6].any())
    with pytest.raises(ValueError, match="recent"):
        p.recent(K + 1)
    for x in (ref, p):
        x.finish()
    band.finish(f"slots-{feed}-G{G}")


# ---- 4. the emit kernel against the torch expressions ---------------------------------------------------------------------------
@pytest.mark.parametrize("R", [13, None], ids=["ring13", "linear"])
def test_emit_kernel_is_the_torch_expression(R):
    from cotracker_amd import ops
    G, N = 3, 11
    g = torch.Generator().manual_seed(5)
    sizes = [(HW[0] // STRIDE >> l, HW[1] // STRIDE >> l) for l in range(4)]
    gs = ops.StreamGroups(torch.zeros(G, N, 3, device=dev()), S, STEP, STRIDE, sizes, ring_rows=R)
    rows = gs.T_cap
    assert rows == (R or 4 * S)
    gs.hist[0].copy_(torch.randn(G, rows, N, 2, generator=g) * 300.0)
    for h_ in gs.hist[1:]:
        h_.copy_(torch.randn(G, rows, N, generator=g) * 3.0)
    special = [float("inf"), float("-inf"), float("nan"), 0.0, -0.0, 88.0, -88.0, 104.0, -104.0]
    for i, x in enumerate(special):  # both logits, in every combination that matters
        gs.hist[1][0, i % rows, i % N] = x
        gs.hist[2][1, (i + 1) % rows, (i + 3) % N] = x
        gs.hist[1][2, (2 * i) % rows, 2] = x
        gs.hist[2][2, (2 * i) % rows, 2] = special[(i + 1) % len(special)]
    gs.hist[0][1, 3, 4] = torch.tensor([float("nan"), float("inf")])
    gs.committed = 41 if R else rows  # (frames 28 .. 40 live in the ring)
    first = torch.randint(0, 45, (G, N), generator=g).to(torch.int32)
    first[0, 2] = first[2, 5] = torch.iinfo(torch.int32).max  # empty slots
    first = first.to(dev())
    hi = gs.committed
    ranges = [(hi - rows, hi), (hi - 1, hi), (hi - rows, hi - rows + 1), (hi - 9, hi - 2), (hi - 5, hi)] if R else \
        [(0, rows), (3, 4), (5, 20), (rows - 1, rows)]
    band = Band([torch.sigmoid(gs.hist[1]) * torch.sigmoid(gs.hist[2])])  # every product the comparisons below draw from
    before = [h_.clone() for h_ in gs.hist]
    for f0, f1 in ranges:
        idx = (torch.arange(f0, f1) % rows).to(dev())
        if R:
            assert len(gs.frame_rows(f0, f1)) == (2 if f0 % R + (f1 - f0) > R else 1)
        for N_out, scale, use_first in ((N, (1.0, 1.0), False), (7, (2.5, 1.0 / 3.0), True), (1, (239 / 95, 159 / 63), True)):
            t_, v_, c_, vis = gs.emit(f0, f1, N_out, scale, logits=True, thresh=THRESH, first_row=first if use_first else None)
            hc, hv, hf = (h_[:, idx, :N_out] for h_ in gs.hist)
            assert torch.equal(bits(t_), bits(hc * hc.new_tensor(list(scale)))), (f0, f1, N_out)  # the multiplication of _user_result
            assert torch.equal(bits(v_), bits(hv)) and torch.equal(bits(c_), bits(hf)), (f0, f1, N_out)
            p = torch.sigmoid(hv) * torch.sigmoid(hf)
            want = p > THRESH
            if use_first:
                want = want & (torch.arange(f0, f1, device=dev())[None, :, None] >= first[:, None, :N_out])
            band.compare(vis, want, p, (f0, f1, N_out))
            assert not bool(vis[torch.isnan(hv) | torch.isnan(hf)].any())
            only = gs.emit(f0, f1, N_out, scale, logits=False)  # tracks alone
            assert len(only) == 1 and torch.equal(bits(only[0]), bits(t_))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(gs.hist, before))  # emit reads
    for f0, f1 in ((hi - rows - 1, hi) if R else (0, rows + 1), (hi, hi + 1), (5, 5)):
        with pytest.raises(ValueError, match="emit"):
            gs.emit(f0, f1)
    if R:
        with pytest.raises(RuntimeError, match="ring"):
            gs.history(4)
    band.finish(f"kernel-{'ring' if R else 'linear'}")


# ---- 5. bounded state ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("feed", ["chunks", "push"])
def test_state_is_bounded(feed, graph):
    """60 calls on a ring: from call 10 on the device memory in use after a call (its results dropped) does not change, and neither
    do the ring, the state's generation and the captured graphs."""
    m = fresh_copy(small_model(hip_graph=graph, batch_mode="joint"))
    m.stream_history_frames = K = S + STEP + 3
    T = S + 59 * STEP
    video, q = stream_inputs(3, 9, T, seed=41)
    m.init_video_online_processing()
    seen = []
    for k, (t0, n) in enumerate(calls_of(T)):
        out = model_call(m, feed, video, q, k, t0, n)
        assert out[0].shape[1] == S
        del out
        m.last_logits = None  # (the model keeps the last call's emitted logits: the same two small tensors every call)
        gs = m._gstream
        seen.append((torch.cuda.memory_allocated(), gs.T_cap, gs.serial, len(m._graphs), tuple(h_.data_ptr() for h_ in gs.hist)))
    assert len(seen) == 60
    assert all(s_ == seen[10] for s_ in seen[10:]), [s_[0] for s_ in seen]
    assert seen[-1][1] == K and seen[-1][3] == (1 if graph else 0)
    m._resolve_deferred_range_check()


def test_predictor_state_is_bounded():
    """The same through push_frames, add_queries included: the predictor keeps nothing that grows."""
    K, T = 2 * S, S + 59 * STEP
    frames, q = predictor_case(2, T, seed=29)
    p = small_predictor(history=K)
    first_step(p, q)
    seen = []
    for k, (t0, n) in enumerate(calls_of(T)):
        if k == 4:
            p.add_queries(torch.tensor([[5.0 * STEP + 2, 100.0, 60.0]], device=dev()), group=1)
        out = predictor_call(p, "push_u8", frames, k, t0, n)
        assert out[0].shape == (2, S, 8, 2)
        del out
        gs = p.model._gstream
        seen.append((torch.cuda.memory_allocated(), gs.T_cap, gs.serial, len(p.model._graphs)))
    assert all(s_ == seen[10] for s_ in seen[10:]), [s_[0] for s_ in seen]
    p.finish()


# ---- 6. range guard: the carry-over rows wrap --------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_range_guard_rerun_restores_wrapped_rows(graph):
    """The stress weights of tests/test_gpu_range.py: every window overflows the f16 range (in the arithmetic: no fault) and is
    re-run on the exact-f32 back end after the history rows the carry-over reads were put back.  With K = 15 those rows are 12, 13,
    14, 0 at ind = 12 (and wrap again at 27, 42): the ring stream still returns the unbounded stream's bits."""
    K = S + STEP + 3
    ref = ctk_support.overflow_model("f16x3", stream_groups=True, stream_slots=True, hip_graph=graph, stream_range_check="immediate")
    m = ctk_support.overflow_model("f16x3", stream_groups=True, stream_slots=True, hip_graph=graph, stream_range_check="immediate")
    m.stream_history_frames = K
    T = S + 11 * STEP + 2
    video, q = stream_inputs(2, 5, T, seed=4)
    for x in (ref, m):
        x.init_video_online_processing()
    wrapped = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k, (t0, n) in enumerate(calls_of(T)):
            want = model_call(ref, "chunks", video, q, k, t0, n)
            got = model_call(m, "chunks", video, q, k, t0, n)
            wrapped += len(m._gstream.frame_rows(t0, t0 + S - STEP)) == 2
            for name, x, y in zip(("coords", "vis", "conf"), got[:3], want[:3]):
                assert torch.equal(x, y[:, t0:]), (k, name, maxdiff(x, y[:, t0:]))
            assert torch.isfinite(got[0]).all()
    assert wrapped >= 3
    assert m.range_fallbacks == ref.range_fallbacks == len(calls_of(T))


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    m = fresh_copy(small_model())
    with pytest.raises(ValueError, match="window_len"):
        m.stream_history_frames = S - 1
    m.stream_history_frames = S
    video, q = stream_inputs(2, 4, S + STEP, seed=2)
    m.init_video_online_processing()
    m.stream_slots = m.stream_groups = False  # (stream_slots refuses a second video on its own)
    with pytest.raises(NotImplementedError, match="stream_history_frames streams the query sets of ONE video"):
        m(video.expand(2, -1, -1, -1, -1), q, iters=2, is_online=True)
    v2 = ctk_support.small_model({}, "f16x3", kind="v2")
    with pytest.raises(NotImplementedError, match="v2 model"):
        v2.stream_history_frames = 2 * S
    # the frame limit: the call whose window would pass frame 2^24 is refused before anything is launched -- a running stream whose
    # frame counter is set by hand
    for feed in ("chunks", "push"):
        m.init_video_online_processing()
        model_call(m, feed, video, q, 0, 0, S)
        gs = m._gstream
        gs.next_ind = m._online[0].ind = 2 ** 24 - STEP
        torch.cuda.synchronize()
        state = [t_.clone() for t_ in (gs.coords, gs.vis, gs.conf, *gs.hist, *gs.pyr)]
        encodes, committed = count_encodes(m), gs.committed
        with pytest.raises(RuntimeError, match="2\\^24"):
            model_call(m, feed, video, q, 1, STEP, S)
        del m._encode
        torch.cuda.synchronize()
        assert encodes == [] and gs.committed == committed and m._online[0].ind == 2 ** 24 - STEP
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(state, (gs.coords, gs.vis, gs.conf, *gs.hist, *gs.pyr)))
    # the attribute is read at the first call: set while a stream runs on the torch glue, it waits for the next stream
    g1 = fresh_copy(small_model())
    g1.stream_slots = g1.stream_groups = False
    g1.init_video_online_processing()
    a = [x.clone() for x in g1(video[:, :S], q[:1], iters=2, is_online=True)[:3]]
    g1.stream_history_frames = 2 * S
    b = g1(video[:, STEP:], q[:1], iters=2, is_online=True)
    assert g1._gstream is None and a[0].shape[1] == S and b[0].shape[1] == S + STEP
    g1.init_video_online_processing()
    c = g1(video[:, :S], q[:1], iters=2, is_online=True)
    assert g1._gstream.ring_rows == 2 * S and torch.equal(c[0], a[0][:, :S])
    g1._resolve_deferred_range_check()
    # ... and the last admissible window runs: ind + S == 2^24 (the ring does not care how old the stream is)
    m.init_video_online_processing()
    out = m(video[:, :S], q, iters=2, is_online=True)
    assert out[0].shape == (2, S, 4, 2) and m.stream_window_start == 0
    m._online[0].ind = m._gstream.next_ind = 2 ** 24 - S
    out = m(video[:, STEP:], q, iters=2, is_online=True)
    assert out[0].shape == (2, S, 4, 2) and m.stream_window_start == 2 ** 24 - S and torch.isfinite(out[0]).all()
    m._resolve_deferred_range_check()
