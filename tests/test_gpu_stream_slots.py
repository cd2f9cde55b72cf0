"""Slots of a running stream (-m gpu): model.stream_slots, model.stream_assign / stream_release, the kernel behind them
(ops.StreamGroups.assign; csrc/stream.hip: ctk_stream_assign) and CoTrackerOnlinePredictor.spare_points / add_queries /
remove_queries.

Two exact oracles, both this repository's own paths.  (E1) A stream that holds (EMPTY_FRAME, x, y) in a row at its first call
and assigns (f, x, y) before the call in which f enters equals the stream that was given (f, x, y) up front.  (E2) A one-set
stream that still runs the torch glue of CoTrackerThreeOnline._video_gen, handed the query table as it stands call by call (and
whose support rows are zeroed by hand when a slot changes its occupant), equals the slot stream for arbitrary positions, re-use
and release.  Both on the history rows >= first_row of every slot, bit for bit in "loop" mode.  The shapes and helpers are those
of tests/test_gpu_stream_groups.py."""
import copy
import functools
import pickle
import warnings

import pytest
import torch

import ctk_support
from ctk_support import HW, S, STEP, STRIDE, bits, chunks, count_encodes, dev, maxdiff, run_stream, stream_inputs
from ctk_support import precision_param as precision  # noqa: F401

pytestmark = pytest.mark.gpu

JOINT_PX, JOINT_LOGIT = 2e-4, 2e-5  # joint vs loop (tests/test_gpu_groups.py)
_models = {}
small_model = functools.partial(ctk_support.small_model, _models, batch_mode="loop", hip_graph=False, range_guard=True, stream_groups=True,
                                stream_slots=True, online_feature_cache=False, stream_range_check="deferred")
overflow_model = functools.partial(ctk_support.overflow_model, stream_groups=True, stream_slots=True)
# the same model with the slot switch off: G == 1 streams on the torch glue, G > 1 on the grouped path as it was
oracle_of = functools.partial(ctk_support.copy_without_stream_state, stream_slots=False)


def empty_row():
    from cotracker_amd import ops
    return torch.tensor([ops.EMPTY_FRAME, 0.0, 0.0], device=dev())


def call_of(frame):
    """The index of the call whose support range [left, right) holds `frame`."""
    return 0 if frame < S else (int(frame) - S) // STEP + 1


def own_rows(first_row, T):
    """[G,T,N] bool on the device: the history rows that belong to the present occupant of each slot."""
    return (torch.arange(T)[None, :, None] >= first_row[:, None, :]).to(dev())


def assert_own_rows_equal(got, want, first_row, what):
    rows = own_rows(first_row, got[0].shape[1])
    for x, y in zip(got, want):
        y = y.reshape(x.shape)
        sel = rows[..., None] if x.dim() == 4 else rows
        assert torch.equal(torch.where(sel, x, torch.zeros_like(x)), torch.where(sel, y, torch.zeros_like(y))), \
            (what, maxdiff(torch.where(sel, x, torch.zeros_like(x)), torch.where(sel, y, torch.zeros_like(y))))


# ----------------------------------------------------------------------------------------------------------------------
# the kernel against the torch index expressions; every other byte of every buffer stays
# ----------------------------------------------------------------------------------------------------------------------
def buffers(gs):
    return [gs.queries, *gs.support, *gs.hist, gs.coords, gs.vis, gs.conf, gs.mask, *gs.pyr, gs.nonfinite]


@pytest.mark.parametrize("M,rows", [(1, 0), (1, None), (7, 5), (None, None), (None, 0)], ids=["one-0", "one-cap", "seven-5", "all-cap", "all-0"])
def test_assign_kernel_is_the_torch_index_expression(M, rows):
    from cotracker_amd import ops
    G, N = 3, 11
    g = torch.Generator().manual_seed(17)
    sizes = [(HW[0] // STRIDE >> l, HW[1] // STRIDE >> l) for l in range(4)]
    gs = ops.StreamGroups(torch.zeros(G, N, 3, device=dev()), S, STEP, STRIDE, sizes)
    for t in buffers(gs):  # random bytes everywhere (NaN patterns included: compared as integers)
        raw = torch.randint(0, 256, (t.numel() * t.element_size(),), generator=g, dtype=torch.uint8).to(dev())
        t.view(torch.uint8).reshape(-1).copy_(raw)
    M = G * N if M is None else M
    rows = gs.T_cap if rows is None else rows
    slots = torch.randperm(G * N, generator=g)[:M]
    newq = torch.rand(M, 3, generator=g) * 50.0 + 40.0
    want = [t.clone() for t in buffers(gs)]
    ptrs = [t.data_ptr() for t in buffers(gs)]
    serial = gs.serial
    gs.assign(slots, newq.to(dev()), rows=rows)
    torch.cuda.synchronize()
    sd = slots.to(dev())
    want[0][sd] = newq.to(dev())
    for l in range(4):
        want[1 + l][sd] = 0.0
    for h_ in want[5:8]:
        h_[sd // N, :rows, sd % N] = 0.0
    for k, (got, w_) in enumerate(zip(buffers(gs), want)):
        assert torch.equal(bits(got), bits(w_)), (k, M, rows)
    assert [t.data_ptr() for t in buffers(gs)] == ptrs and gs.serial == serial
    occ = torch.ones(G * N, dtype=torch.bool)  # (random bytes are not EMPTY_FRAME; the new frames are not either)
    assert torch.equal(gs.occupied.reshape(-1), occ) and int(gs.first_row.abs().max()) == 0
    gs.release(slots[:1])
    torch.cuda.synchronize()
    assert torch.equal(gs.queries[sd[0]], empty_row()) and not bool(gs.occupied.reshape(-1)[slots[0]])
    assert float(gs.support[2][sd[0]].abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------------------------
# (E1) assigned == given up front
# ----------------------------------------------------------------------------------------------------------------------
E1_FRAMES = {1: (13.0, "just in time"), 2: (22.0, "one call early"), 3: (27.0, "several windows early"), 4: (14.5, "just in time")}


def e1_schedule(q, G):
    """slot -> (frame, the call before which it is assigned), for slots 1..4 of every group."""
    N = q.shape[1]
    plan = {}
    for g in range(G):
        for n, (f, when) in E1_FRAMES.items():
            k = call_of(f)
            plan[g * N + n] = (f, {"just in time": k, "one call early": k - 1, "several windows early": 1}[when])
    return plan


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("G", [1, 3])
def test_assigned_equals_given_up_front(precision, graph, G):
    m = small_model(precision)
    N, T = 9, S + 6 * STEP  # seven calls
    video, q = stream_inputs(G, N, T, seed=21 + G)
    plan = e1_schedule(q, G)
    for slot, (f, _) in plan.items():
        q.view(-1, 3)[slot, 0] = f
    ref = oracle_of(m)
    ref.hip_graph = m.hip_graph = graph
    want = run_stream(ref, video, q)
    ref._resolve_deferred_range_check()
    q0 = q.clone()
    for slot in plan:
        q0.view(-1, 3)[slot, 0] = empty_row()[0]  # same (x, y): the blank track of the up-front stream
    first_rows = []

    def between(k):
        due = [s_ for s_, (_, when) in plan.items() if when == k]
        if due:
            assert m.online_ind == k * STEP
            m.stream_assign(due, q.view(-1, 3)[due])
        first_rows.append(m.stream_first_row)
    calls = count_encodes(m)
    try:
        got = run_stream(m, video, q0, between=between)
    finally:
        del m._encode
    m._resolve_deferred_range_check()
    assert calls == [S] * 7 and m.range_fallbacks == 0
    assert torch.equal(m.stream_queries, q) and bool(m.stream_occupied.all())
    fr = m.stream_first_row.reshape(-1)
    for slot, (f, when) in plan.items():
        assert int(fr[slot]) == when * STEP
    assert int(fr.sum()) == sum(when * STEP for _, when in plan.values())  # every other slot: row 0
    first_rows = [torch.zeros(G, N, dtype=torch.long)] + first_rows
    for k in range(len(got)):
        assert got[k][0].shape == (G, S + k * STEP, N, 2)
        assert_own_rows_equal(got[k], want[k], first_rows[k], (k,))
    # the rows below first_row were cleared
    c, v, f = got[-1]
    cleared = ~own_rows(m.stream_first_row, c.shape[1])
    assert float(c[cleared].abs().max()) == 0.0 and bool((v[cleared] == 0.5).all()) and bool((f[cleared] == 0.5).all())
    assert bool(cleared.any())


# ----------------------------------------------------------------------------------------------------------------------
# (E2) assigned == the glue stream with a changing `queries` argument
# ----------------------------------------------------------------------------------------------------------------------
def glue_streams(ref, G):
    refs = [ref] + [copy.deepcopy(ref) for _ in range(G - 1)]
    for r_ in refs:
        r_.init_video_online_processing()
    return refs


def glue_change(refs, table, slots, rows, N):
    """What an assign means for the hand-driven glue streams: the table row, and zeros in the slot's support rows."""
    for s_, row in zip(slots, rows):
        g, n = divmod(int(s_), N)
        table[g, n] = row
        st = refs[g]._online[0]
        st.track_support = [t_.clone() for t_ in st.track_support]
        for t_ in st.track_support:
            t_[n] = 0.0


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("G", [1, 2])
def test_reuse_and_release_equal_the_hand_driven_glue_stream(precision, graph, G):
    m = small_model(precision)
    m.hip_graph = graph
    ref = oracle_of(m)
    N, T = 8, S + 7 * STEP  # eight calls
    video, q = stream_inputs(G, N, T, seed=31, frames=[0, 0, 1, 3, 6, 9, 13])
    q[:, N - 2:] = empty_row()  # two spare slots per group from the start
    table = q.clone()
    gen = torch.Generator().manual_seed(5)

    def point(frame):
        return torch.tensor([frame, float(torch.rand(1, generator=gen)) * (HW[1] - 1), float(torch.rand(1, generator=gen)) * (HW[0] - 1)],
                            device=dev())
    last = G * N - 2  # a spare slot of the last group: filled, released, filled again, replaced while occupied
    events = {1: [(last, point(8.0)), (N - 1, point(30.0))],            # just in time; far ahead
              2: [(0, empty_row())],                                     # release of a first-call query (group 0)
              3: [(last, empty_row()), (0, point(16.5))],                # release; the freed first-call slot re-used
              4: [(last, point(21.0))],                                  # re-use
              6: [(last, point(29.0)), (2, point(28.0))]}                # an occupied slot gets a new occupant; so does a live point
    refs = glue_streams(ref, G)
    m.init_video_online_processing()
    expected_first = torch.zeros(G, N, dtype=torch.long)
    for k, t0 in enumerate(chunks(T)):
        for slot, row in events.get(k, []):
            if bool((row == empty_row()).all()):
                m.stream_release([slot])
            else:
                m.stream_assign([slot], row[None])
            glue_change(refs, table, [slot], [row], N)
            expected_first.view(-1)[slot] = k * STEP
        got = m(video[:, t0:t0 + S], q, iters=2, is_online=True)[:3]  # (the stale first-call table: shape and device only)
        assert torch.equal(m.stream_queries, table) and torch.equal(m.stream_first_row, expected_first)
        assert torch.equal(m.stream_occupied, (table[..., 0] != empty_row()[0]).cpu())
        for g in range(G):
            want = refs[g](video[:, t0:t0 + S], table[g:g + 1], iters=2, is_online=True)[:3]
            assert_own_rows_equal([x[g:g + 1] for x in got], want, expected_first[g:g + 1], (k, g))
    m._resolve_deferred_range_check()
    for r_ in refs:
        r_._resolve_deferred_range_check()
    assert m.range_fallbacks == 0


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_one_set_stream_without_assign_equals_the_glue_stream(precision, graph):
    m = small_model(precision)
    ref = oracle_of(m)
    ref.hip_graph = m.hip_graph = graph
    video, q = stream_inputs(1, 13, S + 4 * STEP, seed=8)
    want = run_stream(ref, video, q)
    ref._resolve_deferred_range_check()
    assert ref._gstream is None  # the oracle ran the glue
    calls = count_encodes(m)
    try:
        got = run_stream(m, video, q)
    finally:
        del m._encode
    m._resolve_deferred_range_check()
    assert calls == [S] * 5 and m._gstream is not None and m._gstream.G == 1
    for k, (a, b) in enumerate(zip(got, want)):
        assert a[0].shape == (1, S + k * STEP, 13, 2)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), k
    video2 = torch.cat([video, video])
    m.init_video_online_processing()
    with pytest.raises(NotImplementedError, match="ONE video"):
        m(video2[:, :S], torch.cat([q, q]), iters=2, is_online=True)


# ----------------------------------------------------------------------------------------------------------------------
# joint mode, no re-capture
# ----------------------------------------------------------------------------------------------------------------------
def spare_stream(G, N, T, seed):
    video, q = stream_inputs(G, N, T, seed=seed, frames=[0, 0, 1, 2, 5])
    q[:, N - 3:] = empty_row()
    return video, q


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_joint_close_to_loop_deterministic_and_groups_independent(precision, graph):
    m = small_model(precision)
    m.hip_graph = graph
    G, N, T = 3, 10, S + 4 * STEP
    video, q = spare_stream(G, N, T, seed=41)
    new = torch.tensor([[9.0, 30.0, 20.0], [17.0, 70.0, 44.0]], device=dev())

    def between(k):
        if k == 1:
            m.stream_assign([1 * N + N - 1, 1 * N + N - 2], new)  # both in group 1
        if k == 3:
            m.stream_release([1 * N + N - 1])
    runs = {}
    for mode in ("loop", "joint"):
        m.batch_mode = mode
        runs[mode] = run_stream(m, video, q, iters=3, between=between)
        runs[mode + "-again"] = run_stream(m, video, q, iters=3, between=between)
        first = m.stream_first_row
        runs[mode + "-plain"] = run_stream(m, video, q, iters=3)
    m._resolve_deferred_range_check()
    assert m.range_fallbacks == 0
    for k in range(len(runs["loop"])):
        rows = own_rows(first, runs["loop"][k][0].shape[1])
        for i, tol in enumerate((JOINT_PX, JOINT_LOGIT, JOINT_LOGIT)):
            a, b = runs["joint"][k][i], runs["loop"][k][i]
            sel = rows[..., None] if a.dim() == 4 else rows
            assert maxdiff(torch.where(sel, a, b), b) < tol, (k, i)
        for mode in ("loop", "joint"):
            for x, y, z in zip(runs[mode][k], runs[mode + "-again"][k], runs[mode + "-plain"][k]):
                assert torch.equal(x, y), (mode, k)                                    # twice the same bits
                assert torch.equal(x[0], z[0]) and torch.equal(x[2], z[2]), (mode, k)  # groups 0 and 2 do not see the assign
    assert not torch.equal(runs["loop"][-1][0][1], runs["loop-plain"][-1][0][1])


@pytest.mark.parametrize("mode", ["loop", "joint"])
def test_assign_and_release_capture_nothing_and_move_nothing(monkeypatch, mode):
    from cotracker_amd import ops
    m = small_model("f16x3")
    m.batch_mode, m.hip_graph = mode, True
    G, N, T = 3, 10, S + 5 * STEP  # 28 history rows: within the first capacity of 4 * S
    video, q = spare_stream(G, N, T, seed=43)
    captures = []
    orig = ops.WindowGraph._capture

    def counting(self, *a, **k):
        captures.append(len(getattr(self, "wins", [None])))
        return orig(self, *a, **k)
    monkeypatch.setattr(ops.WindowGraph, "_capture", counting)
    seen = []

    def between(k):
        gs = m._gstream
        seen.append((len(captures), gs.serial, tuple(t.data_ptr() for t in buffers(gs)), len(gs._wins)))
        if k in (2, 4):
            m.stream_assign([N - 1, 2 * N + N - 2], torch.tensor([[k * STEP + S - 1.0, 11.0, 12.0], [90.0, 50.0, 30.0]], device=dev()))
        if k == 3:
            m.stream_release([N - 1, 4])
    m._drop_graphs()
    m._gstream = None
    run_stream(m, video, q, between=between)
    between(0)
    m._resolve_deferred_range_check()
    assert len(seen) == 6 and len(set(seen[1:])) == 1, seen  # nothing moves after the second call began
    assert seen[0][1:3] == seen[-1][1:3] and captures == ([3] if mode == "joint" else [1, 1, 1])
    run_stream(m, video, q, between=between)  # the next stream of the same shape: same buffers, same graphs
    m._resolve_deferred_range_check()
    assert len(set(seen[1:])) == 1 and len(captures) == (1 if mode == "joint" else 3)


# ----------------------------------------------------------------------------------------------------------------------
# refusals, range guard, copies
# ----------------------------------------------------------------------------------------------------------------------
def test_every_refusal_raises_and_leaves_the_stream_alone():
    m = small_model("f16x3")
    G, N, T = 2, 9, S + 3 * STEP
    video, q = spare_stream(G, N, T, seed=47)
    want = run_stream(m, video, q)
    ok = torch.tensor([[40.0, 5.0, 6.0]], device=dev())

    def between(k):
        left = k * STEP + STEP
        before = [t.clone() for t in buffers(m._gstream)]
        book = (m.stream_occupied, m.stream_first_row)
        for slots, rows, exc in (([N - 1], torch.tensor([[left - 0.5, 5.0, 6.0]], device=dev()), ValueError),   # below `left`
                                 ([N - 1, N - 2], torch.cat([ok, torch.tensor([[0.0, 1.0, 1.0]], device=dev())]), ValueError),
                                 ([N - 1], torch.tensor([[float("nan"), 5.0, 6.0]], device=dev()), ValueError),
                                 ([N - 1], torch.tensor([[float("inf"), 5.0, 6.0]]), ValueError),
                                 ([N - 1, N - 1], ok.expand(2, 3), ValueError), ([G * N], ok, ValueError), ([-1], ok, ValueError),
                                 ([N - 1], ok.expand(2, 3), ValueError), ([N - 1], ok[:, :2], ValueError), ([], ok[:0], ValueError)):
            with pytest.raises(exc):
                m.stream_assign(slots, rows)
        with pytest.raises(ValueError):
            m.stream_release([G * N])
        m.stream_slots = False
        with pytest.raises(RuntimeError, match="stream_slots is off"):
            m.stream_assign([N - 1], ok)
        m.stream_slots = True
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(buffers(m._gstream), before))
        assert torch.equal(m.stream_occupied, book[0]) and torch.equal(m.stream_first_row, book[1])
    got = run_stream(m, video, q, between=between)
    m._resolve_deferred_range_check()
    for a, b in zip(got, want):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    m.init_video_online_processing()
    with pytest.raises(RuntimeError, match="no stream is running"):
        m.stream_assign([N - 1], ok)
    m(video[:, :S], q, iters=2, is_online=True)
    m.stream_assign([N - 1], ok)  # (the frame just at `left` passes: see the E1 test; this one is far ahead)
    m(video[:, STEP:STEP + 5], q, iters=2, is_online=True)  # a short chunk closes the stream
    with pytest.raises(RuntimeError, match="ended the stream"):
        m.stream_assign([N - 2], ok)
    m._resolve_deferred_range_check()


@pytest.mark.parametrize("mode", ["loop", "joint"])
def test_range_guard_with_an_assign_before_the_call_that_overflows(mode):
    from cotracker_amd.synthetic import synthetic_video
    video = synthetic_video(16, *HW, seed=5).to(dev())
    q = torch.tensor([[[0.0, 20.0, 20.0], [2.0, 60.0, 40.0], [0.0, 80.0, 10.0]],
                      [[0.0, 30.0, 50.0], [5.0, 10.0, 10.0], [1.0, 70.0, 30.0]]], device=dev())
    q[:, 2] = empty_row()
    exact, m = overflow_model("f32"), overflow_model("f16x3")
    exact.batch_mode = m.batch_mode = mode

    def assigns(model):
        def between(k):
            if k == 1:
                model.stream_assign([2], torch.tensor([[9.0, 44.0, 33.0]], device=dev()))
            if k == 2:
                model.stream_assign([5, 1], torch.tensor([[13.0, 15.0, 50.0], [14.0, 70.0, 12.0]], device=dev()))
        return between
    want = run_stream(exact, video, q, between=assigns(exact))
    assert exact.range_fallbacks == 0 and all(torch.isfinite(x).all() for o in want for x in o)
    with warnings.catch_warnings(record=True) as w:  # direct: a warned re-run on f32, the rows the carry-over reads put back first
        warnings.simplefilter("always")
        got = run_stream(m, video, q, between=assigns(m))
    assert m.range_fallbacks == 3 and any(issubclass(x.category, RuntimeWarning) for x in w)
    for a, b in zip(got, want):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(m.stream_first_row, exact.stream_first_row) and int(m.stream_first_row[0, 2]) == STEP
    m.hip_graph, m.stream_range_check = True, "immediate"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_stream(m, video, q, between=assigns(m))
    assert m.range_fallbacks == 6 and m._pending_range is None
    for a, b in zip(got, want):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    m.stream_range_check = "deferred"  # the assign itself never waits for, nor trips over, the pending flag: the NEXT call raises
    m.init_video_online_processing()
    m(video[:, 0:8], q, iters=2, is_online=True)
    assigns(m)(1)
    with pytest.raises(FloatingPointError, match="f16 range"):
        m(video[:, 4:12], q, iters=2, is_online=True)
    m.precision = "f32"
    later = run_stream(m, video, q, between=assigns(m))
    for a, b in zip(later, want):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_deepcopy_and_pickle_in_mid_stream_after_an_assign():
    m = small_model("f16x3")
    m.hip_graph = True
    video, q = spare_stream(2, 9, S + 3 * STEP, seed=53)
    new = torch.tensor([[9.0, 30.0, 20.0], [14.0, 70.0, 44.0]], device=dev())

    def between(k):
        if k == 1:
            m.stream_assign([8, 9 + 7], new)
    want = run_stream(m, video, q, between=between)
    m.init_video_online_processing()
    m(video[:, 0:S], q, iters=2, is_online=True)
    between(1)
    book = (m.stream_occupied, m.stream_first_row, m.stream_queries)
    assert int(book[1][0, 8]) == STEP and bool(book[0][0, 8]) and not bool(book[0][0, 7])
    for clone in (copy.deepcopy(m), pickle.loads(pickle.dumps(m)).to(dev())):
        assert clone.stream_slots and clone.online_ind == STEP and not clone._graphs
        assert all(torch.equal(a, b) for a, b in zip((clone.stream_occupied, clone.stream_first_row, clone.stream_queries), book))
        for t0 in (STEP, 2 * STEP):
            c, v, f, _ = clone(video[:, t0:t0 + S], q, iters=2, is_online=True)
        clone.stream_release([8])
        c, v, f, _ = clone(video[:, 3 * STEP:3 * STEP + S], q, iters=2, is_online=True)
        clone._resolve_deferred_range_check()
        keep = torch.ones(2, 9, dtype=torch.bool)
        keep[0, 8] = False
        assert int(clone.stream_first_row[0, 8]) == 3 * STEP and not bool(clone.stream_occupied[0, 8])
        # (slot 8 left group 0; group 1 does not see it)
        assert torch.equal(c[1], want[-1][0][1]) and torch.equal(v[1], want[-1][1][1]) and torch.equal(f[1], want[-1][2][1])
    c, *_ = m(video[:, STEP:STEP + S], q, iters=2, is_online=True)  # the original goes on undisturbed
    assert torch.equal(c, want[1][0])
    m._resolve_deferred_range_check()


# ----------------------------------------------------------------------------------------------------------------------
# predictor
# ----------------------------------------------------------------------------------------------------------------------
def test_online_predictor_spare_points_add_and_remove():
    import torch.nn.functional as F

    from cotracker_amd import ops
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    from cotracker_amd.weights import fill_synthetic_
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=S)
    fill_synthetic_(p.model, seed=5)
    p = p.to(dev())
    g = torch.Generator().manual_seed(12)
    T, H, W = S + 3 * STEP, 120, 160
    ih, iw = p.interp_shape
    video = (torch.rand(1, T, 3, H, W, generator=g) * 255).to(dev())
    N, K = 2, 3
    q = (torch.rand(1, N, 3, generator=g) * torch.tensor([1.0, W - 1.0, H - 1.0])).to(dev())
    q[..., 0] = torch.tensor([[0.0, 3.0]], device=dev())
    added = torch.tensor([[13.0, 100.0, 60.0], [12.0, 20.0, 90.0]], device=dev())
    scale = torch.tensor([(iw - 1) / (W - 1), (ih - 1) / (H - 1)], device=dev())
    p.spare_points = K
    model = copy.deepcopy(p.model)  # the model-level stream the predictor is compared with
    model.stream_slots = True
    p(video[:, :S], is_first_step=True, queries=q, add_support_grid=True)
    assert p.model.stream_slots and p.queries.shape == (1, N + K + 36, 3) and p.N == N + K
    assert torch.equal(p.queries[0, N:N + K], empty_row().expand(K, 3)) and float(p.queries[0, N + K:, 0].abs().max()) == 0.0
    model.init_video_online_processing()
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.add_queries(added)
    for k, t0 in enumerate(range(0, T - S + 1, STEP)):
        if k == 1:
            with pytest.raises(RuntimeError, match="free slots"):
                p.add_queries(added[:1].expand(K + 1, 3))
            points = p.add_queries(added)
            assert points.tolist() == [N, N + 1]
            aq = added.clone()
            aq[:, 1:] *= scale
            model.stream_assign(points, aq)
        if k == 2:
            p.remove_queries([0, N + 1])
            model.stream_release([0, N + 1])
            with pytest.raises(ValueError):
                p.remove_queries([N + K])
        if k == 3:
            assert p.add_queries(torch.tensor([[22.0, 50.0, 50.0]], device=dev())).tolist() == [0]  # the lowest free slot
            model.stream_assign([0], torch.cat([torch.tensor([22.0], device=dev()), torch.tensor([50.0, 50.0], device=dev()) * scale])[None])
        tr, vis = p(video[:, t0:t0 + S], add_support_grid=True)
        v = F.interpolate(video[0, t0:t0 + S].float(), (ih, iw), mode="bilinear", align_corners=True)[None]
        c, vi, cf, _ = model(v, p.queries, iters=6, is_online=True)
        rows = own_rows(model.stream_first_row[:, :N + K], c.shape[1]) & model.stream_occupied[:, None, :N + K].to(dev())
        assert tr.shape == (1, S + k * STEP, N + K, 2) and vis.dtype == torch.bool
        assert torch.equal(tr, c[:, :, :N + K] * c.new_tensor([(W - 1) / (iw - 1), (H - 1) / (ih - 1)]))
        assert torch.equal(vis, ((vi * cf)[:, :, :N + K] > 0.6) & rows)
        assert not bool(vis[~rows].any())
    p.finish()
    model._resolve_deferred_range_check()
    occ = p.model.stream_occupied[0, :N + K]
    assert occ.tolist() == [True, True, True, False, False] and p.model.stream_first_row[0, 0] == 3 * STEP
    assert float(p.model.stream_queries[0, N + 1, 0]) == ops.EMPTY_FRAME
    # spare_points == 0: the stream is the one it always was
    p.spare_points = 0
    p.model.stream_slots = False
    p(video[:, :S], is_first_step=True, queries=q, add_support_grid=True)
    assert p.queries.shape == (1, N + 36, 3) and not p.model.stream_slots and p._first_row is None
