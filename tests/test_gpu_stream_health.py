"""Track health and replenish (-m gpu): the kernel behind ops.StreamGroups.health (csrc/stream.hip: ctk_stream_health),
model.stream_health, CoTrackerOnlinePredictor.track_health and .replenish.

Every comparison is exact, on integers.  The oracle for `alive` is the project's own ctk_stream_emit -- `visible` with first_row :=
max(first_row, qframe), tracks at scale 1: the same device expression, so there is no tolerance band -- combined with torch integer
and float32 elementwise operations for the bounds, the runs and the cells (one rounding per operation, as the kernel's intrinsics)."""
import ctypes as C
import functools

import pytest
import torch

import ctk_support
from ctk_support import HW, S, STEP, STRIDE, bits, chunks, dev, stream_inputs

pytestmark = pytest.mark.gpu

OV = S - STEP
RING = S + STEP + 3  # 15 rows
BIG = torch.iinfo(torch.int32).max
_models = {}
small_model = functools.partial(ctk_support.small_model, _models, batch_mode="loop", hip_graph=False, range_guard=True, stream_groups=False,
                                stream_slots=False, online_feature_cache=False, stream_range_check="deferred")
fresh_copy = functools.partial(ctk_support.copy_without_stream_state, stream_slots=False)


def buffers(gs):
    return [gs.queries, *gs.support, *gs.hist, gs.coords, gs.vis, gs.conf, gs.mask, *gs.pyr, gs.nonfinite]


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


def f32(v):
    return torch.tensor(float(v), dtype=torch.float32, device=dev())


def oracle(gs, look, grid, thresh, N_out, first32, bounds):
    """-> (lost, cell, cover [G,cells], alive [G,look,N_out], counted) from ctk_stream_emit and torch elementwise operations."""
    from cotracker_amd import ops
    G, N, f1 = gs.G, gs.N, gs.committed
    gh, gw = grid
    x_lo, x_hi, y_lo, y_hi = (f32(b) for b in bounds)
    inv_cw, inv_ch = f32(gw) / (x_hi - x_lo), f32(gh) / (y_hi - y_lo)
    q = gs.queries.view(G, N, 3)[:, :N_out]
    fr = first32[:, :N_out].long()
    start = torch.maximum(fr, q[..., 0].long())
    empty = (fr == BIG) | (q[..., 0] == ops.EMPTY_FRAME)
    pending = ~empty & ((fr >= gs.next_ind) | (start >= f1))
    st32 = first32.clone()
    st32[:, :N_out] = start.clamp(max=BIG).to(torch.int32)
    tracks, visible = gs.emit(f1 - look, f1, N_out=N_out, scale=(1.0, 1.0), logits=False, thresh=thresh, first_row=st32)

    def inside(x, y):
        return (x >= x_lo) & (x <= x_hi) & (y >= y_lo) & (y <= y_hi)

    def cell_of(x, y):
        cx = torch.floor((x - x_lo) * inv_cw).nan_to_num(0.0).clamp(-1.0, float(gw)).to(torch.int64).clamp(0, gw - 1)
        cy = torch.floor((y - y_lo) * inv_ch).nan_to_num(0.0).clamp(-1.0, float(gh)).to(torch.int64).clamp(0, gh - 1)
        return cy * gw + cx

    x, y = tracks[..., 0], tracks[..., 1]
    alive = visible & inside(x, y)
    counted = torch.arange(f1 - look, f1, device=dev())[None, :, None] >= start[:, None, :]
    run = (~alive & counted).flip(1).long().cumprod(1).sum(1)  # the newest frames in a row that count and are not alive
    minus = torch.full_like(run, -1)
    lost = torch.where(empty, minus, torch.where(pending, torch.zeros_like(run), run))
    c_tracked = torch.where(alive[:, -1], cell_of(x[:, -1], y[:, -1]), minus)
    c_pending = torch.where(inside(q[..., 1], q[..., 2]), cell_of(q[..., 1], q[..., 2]), minus)
    cell = torch.where(empty, minus, torch.where(pending, c_pending, c_tracked))
    cover = torch.zeros(G, gh * gw + 1, dtype=torch.int64, device=dev())
    cover.scatter_add_(1, torch.where(cell < 0, torch.full_like(cell, gh * gw), cell), torch.ones_like(cell))
    return lost.int(), cell.int(), cover[:, :gh * gw].int(), alive, counted


def raw_health(gs, look, grid, thresh, N_out, first32, bounds, guard=64):
    """ctk_stream_health through the C ABI with every output followed by `guard` sentinel words -> (lost, cell, cover) and whether all
    sentinels survived."""
    from cotracker_amd import _lib as L
    gh, gw = grid
    k, cells = gs.G * N_out, gs.G * gh * gw
    flat = torch.full((2 * k + cells + 4 * guard,), -77, dtype=torch.int32, device=dev())
    o_lost, o_cell, o_cover = guard, 2 * guard + k, 3 * guard + 2 * k
    a = L.StreamHealth.Args()
    a.G, a.N, a.N_out, a.R, a.f1, a.look, a.ind_next = gs.G, gs.N, N_out, gs.T_cap, gs.committed, look, gs.next_ind
    a.thresh, a.reserved, a.gh, a.gw = thresh, 0, gh, gw
    a.x_lo, a.x_hi, a.y_lo, a.y_hi = bounds
    a.inv_cw, a.inv_ch = float(f32(gw) / (f32(bounds[1]) - f32(bounds[0]))), float(f32(gh) / (f32(bounds[3]) - f32(bounds[2])))
    a.queries = gs.queries.data_ptr()
    a.hist_coords, a.hist_vis, a.hist_conf = (h_.data_ptr() for h_ in gs.hist)
    a.first_row = first32.data_ptr()
    a.lost, a.cell, a.cover = (flat.data_ptr() + 4 * o for o in (o_lost, o_cell, o_cover))
    assert L.load().ctk_stream_health(C.byref(a), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    out = flat[o_lost:o_lost + k].view(gs.G, N_out), flat[o_cell:o_cell + k].view(gs.G, N_out), flat[o_cover:o_cover + cells].view(gs.G, gh * gw)
    guards = torch.cat([flat[:o_lost], flat[o_lost + k:o_cell], flat[o_cell + k:o_cover], flat[o_cover + cells:]])
    return out, bool((guards == -77).all()) and guards.numel() == 4 * guard


def random_state(G, N, ring, f1, ind_next, seed):
    """A StreamGroups with random bytes in every buffer (NaN patterns included) and the books of a stream that has committed f1 frames."""
    from cotracker_amd import ops
    g = torch.Generator().manual_seed(seed)
    sizes = [(HW[0] // STRIDE >> l, HW[1] // STRIDE >> l) for l in range(4)]
    gs = ops.StreamGroups(torch.zeros(G, N, 3, device=dev()), S, STEP, STRIDE, sizes, ring_rows=ring)
    for t in buffers(gs):
        raw = torch.randint(0, 256, (t.numel() * t.element_size(),), generator=g, dtype=torch.uint8).to(dev())
        t.view(torch.uint8).reshape(-1).copy_(raw)
    gs.committed, gs.next_ind = f1, ind_next
    return gs, g


# ----------------------------------------------------------------------------------------------------------------------
# 1. the kernel on hand-set slots: every rule of the header, with the value each must give
# ----------------------------------------------------------------------------------------------------------------------
BOUNDS = (-2.0, 94.0, -2.0, 62.0)  # 96 x 64 model pixels widened by 2: with the 8 x 12 grid a cell is 8 x 8 pixels, 1 / 8 exact
GRID = (8, 12)


def below(v):
    return float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(-float("inf"))))


def above(v):
    return float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(float("inf"))))


@pytest.mark.parametrize("ring,f1,ind_next", [(None, 20, 16), (RING, 33, 32)], ids=["linear32", "ring15-f33"])
def test_kernel_on_hand_set_slots(monkeypatch, ring, f1, ind_next):
    from cotracker_amd import ops
    G, N, N_out = 3, 11, 8
    gs, g = random_state(G, N, ring, f1, ind_next, seed=31 + f1)
    assert gs.T_cap == (32 if ring is None else RING)
    R = gs.T_cap
    deep = min(R, f1)  # the longest look
    nan = float("nan")
    first = torch.randint(0, 40, (G, N), generator=g, dtype=torch.int32)
    first[:, :N_out] = 0
    q = gs.queries.view(G, N, 3)
    q[:, :N_out] = torch.tensor([0.0, 40.0, 30.0], device=dev())
    for h_, v in zip(gs.hist, ((40.0, 30.0), 4.0, 4.0)):  # every judged slot: alive in cell (32 / 8) * 12 + 42 / 8 = 53 on every frame held
        for f in range(f1 - deep, f1):
            h_[:, f % R, :N_out] = torch.tensor(v, device=dev())

    def put(gn, f, xy=None, v=None, c=None):
        for h_, val in zip(gs.hist, (xy, v, c)):
            if val is not None:
                h_[gn[0], f % R, gn[1]] = torch.tensor(val, device=dev())

    def dead(gn, frames):
        for f in frames:
            put(gn, f, v=-4.0, c=-4.0)
    want = {}  # (g, n) -> (lost as a function of look, cell)
    home = 53
    # empty, through either mark
    first[0, 0] = BIG
    want[0, 0] = (lambda L: -1, -1)
    q[0, 1] = torch.tensor([ops.EMPTY_FRAME, 0.0, 0.0], device=dev())
    want[0, 1] = (lambda L: -1, -1)
    # pending: assigned since the last commit, as a resident assign leaves it -- (x, y) and zero logits in the rows: not "lost"
    first[0, 2] = ind_next
    q[0, 2] = torch.tensor([f1 - 2.0, 10.5, 20.25], device=dev())
    for f in range(f1 - deep, f1):
        put((0, 2), f, xy=(10.5, 20.25), v=0.0, c=0.0)
    want[0, 2] = (lambda L: 0, (22 // 8) * 12 + 12 // 8)
    # pending: the query frame has not been tracked; its position lies outside the bounds
    q[0, 3] = torch.tensor([float(f1), -3.0, 10.0], device=dev())
    want[0, 3] = (lambda L: 0, -1)
    want[0, 4] = (lambda L: 0, home)  # alive at the newest frame
    dead((0, 5), [f1 - 1])
    want[0, 5] = (lambda L: 1, -1)
    dead((0, 6), [f1 - 1, f1 - 2, f1 - 3])
    want[0, 6] = (lambda L: min(L, 3), -1)
    dead((0, 7), range(f1 - deep, f1))
    want[0, 7] = (lambda L: L, -1)
    # start inside the lookback: the run is capped by the occupant's age -- through first_row, and through a fractional query frame
    first[1, 0] = ind_next - 1  # (the newest first row that is no pending one)
    dead((1, 0), range(f1 - deep, f1))
    want[1, 0] = (lambda L: min(L, f1 - ind_next + 1), -1)
    q[1, 1, 0] = f1 - 3 + 0.5
    dead((1, 1), range(f1 - deep, f1))
    want[1, 1] = (lambda L: min(L, 3), -1)
    # on each border: inside (x_hi and y_hi are clamped into the last column / row)
    put((1, 2), f1 - 1, xy=(BOUNDS[0], 30.0))
    want[1, 2] = (lambda L: 0, 4 * 12 + 0)
    put((1, 3), f1 - 1, xy=(BOUNDS[1], 30.0))
    want[1, 3] = (lambda L: 0, 4 * 12 + 11)
    put((1, 4), f1 - 1, xy=(40.0, BOUNDS[2]))
    want[1, 4] = (lambda L: 0, 0 * 12 + 5)
    put((1, 5), f1 - 1, xy=(40.0, BOUNDS[3]))
    want[1, 5] = (lambda L: 0, 7 * 12 + 5)
    # one float beyond each border: outside, lost for that one frame
    for gn, xy in (((1, 6), (below(BOUNDS[0]), 30.0)), ((1, 7), (above(BOUNDS[1]), 30.0)), ((2, 0), (40.0, below(BOUNDS[2]))),
                   ((2, 1), (40.0, above(BOUNDS[3])))):
        put(gn, f1 - 1, xy=xy)
        want[gn] = (lambda L: 1, -1)
    put((2, 2), f1 - 1, xy=(nan, 30.0))
    put((2, 3), f1 - 1, v=nan)
    put((2, 4), f1 - 1, c=nan)
    for n in (2, 3, 4):
        want[2, n] = (lambda L: 1, -1)
    put((2, 5), f1 - 1, xy=(38.0, 22.0))  # exactly on a cell edge in x and y: (38 + 2) / 8 = 5, (22 + 2) / 8 = 3 -> the upper cell
    want[2, 5] = (lambda L: 0, 3 * 12 + 5)
    dead((2, 6), range(f1 - deep, f1 - 1))  # alive at the newest frame only: the walk stops there
    want[2, 6] = (lambda L: 0, home)
    dead((2, 7), [f1 - 1, f1 - 2, f1 - 4])  # the run ends at the first alive frame
    want[2, 7] = (lambda L: min(L, 2), -1)
    assert len(want) == G * N_out
    first32 = first.to(dev())
    before = [t.clone() for t in buffers(gs)] + [first32.clone()]
    ptrs = [t.data_ptr() for t in buffers(gs)]
    serial = gs.serial
    calls = library_calls(monkeypatch)
    for look in (1, S, deep):
        del calls[:]
        lost, cell, cover = gs.health(look, GRID, 0.6, N_out, first32, BOUNDS)
        torch.cuda.synchronize()
        assert calls == ["ctk_stream_health"]  # ONE entry point, which launches once
        assert lost.shape == cell.shape == (G, N_out) and cover.shape == (G, 96) and lost.dtype == cell.dtype == cover.dtype == torch.int32
        assert lost._base is cell._base is cover._base and lost._base.numel() == 2 * G * N_out + G * 96
        w_lost = torch.tensor([[want[g_, n][0](look) for n in range(N_out)] for g_ in range(G)], dtype=torch.int32)
        w_cell = torch.tensor([[want[g_, n][1] for n in range(N_out)] for g_ in range(G)], dtype=torch.int32)
        w_cover = torch.stack([torch.bincount(r[r >= 0].long(), minlength=96) for r in w_cell]).int()
        assert torch.equal(lost.cpu(), w_lost), (look, lost.cpu(), w_lost)
        assert torch.equal(cell.cpu(), w_cell), (look, cell.cpu(), w_cell)
        assert torch.equal(cover.cpu(), w_cover), look
        o_lost, o_cell, o_cover, alive, counted = oracle(gs, look, GRID, 0.6, N_out, first32, BOUNDS)
        assert torch.equal(lost, o_lost) and torch.equal(cell, o_cell) and torch.equal(cover, o_cover), look
        (r_lost, r_cell, r_cover), guards = raw_health(gs, look, GRID, 0.6, N_out, first32, BOUNDS)
        assert guards  # nothing behind [G,N_out] rows or the cover is written: no row of a slot n >= N_out
        assert torch.equal(r_lost, lost) and torch.equal(r_cell, cell) and torch.equal(r_cover, cover)
    for k, (got, w_) in enumerate(zip(buffers(gs) + [first32], before)):  # the state is read only
        assert torch.equal(bits(got), bits(w_)), k
    assert [t.data_ptr() for t in buffers(gs)] == ptrs and gs.serial == serial
    # the slots n >= N_out are not read: other bytes there, the same answer
    want_out = [t.clone() for t in gs.health(deep, GRID, 0.6, N_out, first32, BOUNDS)]
    q[:, N_out:] = torch.tensor([3.0, 40.0, 30.0], device=dev())
    first32[:, N_out:] = 0
    for h_ in gs.hist:
        h_[:, :, N_out:] = 0.0
    assert all(torch.equal(a, b) for a, b in zip(gs.health(deep, GRID, 0.6, N_out, first32, BOUNDS), want_out))
    # host checks of ops.StreamGroups.health
    for bad in (dict(look=0), dict(look=deep + 1), dict(N_out=0), dict(N_out=N + 1), dict(grid=(64, 65)), dict(first_row=first32.long()),
                dict(first_row=first32[:, :N_out]), dict(first_row=first32.cpu()), dict(bounds=(5.0, 5.0, 0.0, 1.0))):
        kw = dict(look=S, grid=GRID, thresh=0.6, N_out=N_out, first_row=first32, bounds=BOUNDS)
        kw.update(bad)
        with pytest.raises(ValueError):
            gs.health(**kw)
    gs.committed = 0
    with pytest.raises(ValueError):
        gs.health(1, GRID, 0.6, N_out, first32, BOUNDS)


# ----------------------------------------------------------------------------------------------------------------------
# 2. random contents across a wave and a 256-thread block, 4096 cells, against the oracle
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring,f1,ind_next,look", [(None, 20, 16, S), (RING, 33, 32, RING)], ids=["linear32-look8", "ring15-f33-look15"])
def test_kernel_on_random_contents(ring, f1, ind_next, look):
    from cotracker_amd import ops
    G, N, N_out, grid = 2, 300, 257, (64, 64)
    bounds = (0.0, 95.0, 0.0, 63.0)  # 64 / 95 and 64 / 63: neither reciprocal is exact
    gs, g = random_state(G, N, ring, f1, ind_next, seed=7 + f1)
    R = gs.T_cap
    shape = (G, R, N_out)
    xy = torch.rand(*shape, 2, generator=g) * torch.tensor([115.0, 83.0]) - 10.0  # about a sixth of the positions lie outside
    xy[torch.rand(shape, generator=g) < 0.02] = float("nan")
    logits = [torch.randn(shape, generator=g) * 3.0 + 1.5 for _ in range(2)]
    for l_ in logits:
        l_[torch.rand(shape, generator=g) < 0.02] = float("nan")
    for h_, v in zip(gs.hist, (xy, *logits)):
        h_[:, :, :N_out] = v.to(dev())
    frames = torch.tensor([0.0, 0.0, 0.0, 3.5, f1 - 5.0, f1 - 1.0, f1 - 0.5, float(f1), f1 + 7.0, ops.EMPTY_FRAME])
    q = torch.rand(G, N_out, 3, generator=g) * torch.tensor([1.0, 115.0, 83.0]) - torch.tensor([0.0, 10.0, 10.0])
    q[..., 0] = frames[torch.randint(0, len(frames), (G, N_out), generator=g)]
    gs.queries.view(G, N, 3)[:, :N_out] = q.to(dev())
    firsts = torch.tensor([0, 0, 0, 0, f1 - 6, f1 - 2, ind_next - 1, ind_next, ind_next + 4, BIG], dtype=torch.int32)
    first = torch.randint(0, 40, (G, N), generator=g, dtype=torch.int32)
    first[:, :N_out] = firsts[torch.randint(0, len(firsts), (G, N_out), generator=g)]
    first32 = first.to(dev())
    before = [t.clone() for t in buffers(gs)] + [first32.clone()]
    lost, cell, cover = gs.health(look, grid, 0.6, N_out, first32, bounds)
    o_lost, o_cell, o_cover, alive, counted = oracle(gs, look, grid, 0.6, N_out, first32, bounds)
    assert torch.equal(lost, o_lost), (lost != o_lost).nonzero()[:8]
    assert torch.equal(cell, o_cell), (cell != o_cell).nonzero()[:8]
    assert torch.equal(cover, o_cover)
    (r_lost, r_cell, r_cover), guards = raw_health(gs, look, grid, 0.6, N_out, first32, bounds)
    assert guards and torch.equal(r_lost, lost) and torch.equal(r_cell, cell) and torch.equal(r_cover, cover)
    for k, (got, w_) in enumerate(zip(buffers(gs) + [first32], before)):
        assert torch.equal(bits(got), bits(w_)), k
    # the draw exercises every class, short and long runs, and the block that holds slot 256
    assert set(range(-1, 4)) <= set(lost.unique().tolist()) and int(lost.max()) <= look
    assert int(cover.sum()) == int((cell >= 0).sum()) > 20 and int((cell == -1).sum()) > 20
    assert bool((cell[lost == 0] >= 0).any()) and bool((cell[lost == 0] == -1).any())  # a pending slot outside the bounds


# ----------------------------------------------------------------------------------------------------------------------
# 3. model and predictor: track_health against the oracle on a running stream, replenish against a hand-made twin
# ----------------------------------------------------------------------------------------------------------------------
def make_predictor(model, spare, history):
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=S)
    p.model, p.interp_shape, p.step = model, HW, STEP
    p.spare_points, p.history_frames = spare, history
    return p.to(dev())


CASES = [("chunks", None, False), ("chunks", RING, True), ("push", None, False)]


@pytest.mark.parametrize("feed,history,graph", CASES, ids=["chunks-linear", "chunks-ring15-graph", "push-linear"])
def test_track_health_and_replenish_on_a_running_stream(monkeypatch, feed, history, graph):
    from cotracker_amd import ops
    G, N, K, grid, max_lost = 2, 5, 6, (4, 6), 2
    base = small_model("f16x3")
    p, twin = (make_predictor(fresh_copy(base), K, history) for _ in range(2))
    for x in (p, twin):
        x.model.hip_graph = graph
    captures = []
    orig = ops.WindowGraph._capture

    def counting(self, *a, **k):
        captures.append(self)
        return orig(self, *a, **k)
    monkeypatch.setattr(ops.WindowGraph, "_capture", counting)
    T = S + 4 * STEP  # five calls: a health check after each of the first four, the replenish after the second
    video, q = stream_inputs(G, N, T, seed=83, frames=[0, 0, 1, 3, 6])
    Nu = N + K
    bounds = (0.0, HW[1] - 1.0, 0.0, HW[0] - 1.0)

    def step(x, k, t0):
        if feed == "chunks":
            return x(video[:, t0:t0 + S], add_support_grid=True)
        return x.push_frames(video[0, :S] if k == 0 else video[0, t0 + S - STEP:t0 + S], add_support_grid=True)

    for x in (p, twin):
        x(video[:, :1], is_first_step=True, queries=q, add_support_grid=True)
        with pytest.raises(RuntimeError, match="no stream is running"):
            x.track_health()
    thresh, changed = None, None
    for k, t0 in enumerate(chunks(T)):
        got, ref = step(p, k, t0), step(twin, k, t0)
        if changed is not None:  # after the replenish: the stream equals the twin's, bit for bit, on every point
            assert got[0].shape == ref[0].shape and torch.equal(bits(got[0]), bits(ref[0])) and torch.equal(got[1], ref[1]), k
            assert torch.equal(p.model.stream_queries, twin.model.stream_queries)
        if k == 4:
            break
        gs = p.model._gstream
        assert gs.N == Nu + 36 and gs.committed == t0 + S and gs.next_ind == t0 + STEP
        first32 = p._emit_first_row()
        if thresh is None:  # the median product of the occupied points: a random-weight model puts them all on one side of 0.6
            _, v, c = gs.emit(gs.committed - S, gs.committed, N_out=N)
            since = torch.arange(gs.committed - S, gs.committed, device=dev())[None, :, None] >= q[:, None, :, 0].long()
            thresh = float((torch.sigmoid(v) * torch.sigmoid(c))[since].median())  # (over the frames that count: from the query frame on)
        o_lost, o_cell, o_cover, alive, counted = oracle(gs, S, grid, thresh, Nu, first32, bounds)
        if k == 0:
            assert bool(alive[:, :, :N].any()) and bool((~alive & counted)[:, :, :N].any())  # both classes occur
            assert bool((o_lost[:, N:] == -1).all()) and not bool((o_lost[:, :N] == -1).any())
        lost, cover = p.track_health(look=S, grid=grid, thresh=thresh)
        assert lost.shape == (G, Nu) and cover.shape == (G, *grid) and lost.dtype == cover.dtype == torch.int32
        assert torch.equal(lost, o_lost) and torch.equal(cover.reshape(G, -1), o_cover), k
        for look in (1, 3):
            l2, c2 = p.track_health(look=look, grid=grid, thresh=thresh)
            o2 = oracle(gs, look, grid, thresh, Nu, first32, bounds)
            assert torch.equal(l2, o2[0]) and torch.equal(c2.reshape(G, -1), o2[2]), (k, look)
        if k != 1:
            continue
        # ---- the replenish, between the second and the third call
        occ = p.model.stream_occupied[:, :Nu]
        state = (len(captures), gs.serial, tuple(t.data_ptr() for t in [gs.queries, *gs.support, gs.coords, gs.vis, gs.conf, gs.mask, *gs.pyr]),
                 len(gs._wins))
        newest = p.resident_frames[1] - 1
        assert newest == gs.committed - 1
        calls = library_calls(monkeypatch)
        released, added, seeds = p.replenish(max_lost, grid=grid, look=S, thresh=thresh)
        seen = list(calls)
        assert state == (len(captures), gs.serial, tuple(t.data_ptr() for t in [gs.queries, *gs.support, gs.coords, gs.vis, gs.conf, gs.mask,
                                                                                 *gs.pyr]), len(gs._wins))
        ring = "_ring" if history is not None else ""
        assert seen[0] == "ctk_stream_health" and seen.count("ctk_stream_health") == 1
        assert sorted(seen[1:]) == sorted(["ctk_stream_assign" + ring] * bool(len(released)) + ["ctk_stream_assign_resident" + ring] * bool(len(added)))
        # released: exactly {lost >= max_lost}
        want_rel = (o_lost.cpu() >= max_lost).nonzero()
        assert torch.equal(released, want_rel) and bool(occ[released[:, 0], released[:, 1]].all())
        # added: the row-major empty cells on the lowest free slots, those just released included
        want_add, want_q = [], []
        for g_ in range(G):
            free = sorted(set((~occ[g_]).nonzero().reshape(-1).tolist()) | set(want_rel[want_rel[:, 0] == g_, 1].tolist()))
            empty = (o_cover[g_].cpu() == 0).nonzero().reshape(-1).tolist()
            for n, c in zip(free, empty):
                want_add.append([g_, n])
                want_q.append([float(newest), (c % grid[1] + 0.5) * (HW[1] - 1.0) / grid[1], (c // grid[1] + 0.5) * (HW[0] - 1.0) / grid[0]])
        assert added.tolist() == want_add and len(added) > 0
        assert seeds.shape == (len(added), 3) and torch.equal(seeds[:, 0], torch.full((len(added),), float(newest)))
        assert float((seeds - torch.tensor(want_q)).abs().max()) < 1e-4  # the cell centres (raw video = model resolution here)
        assert bool(p.model.stream_occupied[added[:, 0], added[:, 1]].all())
        assert torch.equal(p.model.stream_first_row[added[:, 0], added[:, 1]], torch.full((len(added),), gs.next_ind))
        # the pending rule: the seeds count at their query positions, their carry rows do not read as lost
        l3, c3 = p.track_health(look=S, grid=grid, thresh=thresh)
        assert bool((l3[added[:, 0], added[:, 1]] == 0).all())
        assert int(c3.sum()) == int(o_cover.sum()) + len(added)
        for g_ in range(G):  # every empty cell that got a seed is covered now
            n_g = sum(1 for a in want_add if a[0] == g_)
            cells_g = (o_cover[g_].cpu() == 0).nonzero().reshape(-1)[:n_g]
            assert bool((c3[g_].reshape(-1).cpu()[cells_g] == 1).all())
        # a second replenish without a step: nothing is lost long enough, and no free slot or no empty cell is left
        del calls[:]
        again = p.replenish(max_lost, grid=grid, look=S, thresh=thresh)
        assert [len(x) for x in again] == [0, 0, 0] and list(calls) == ["ctk_stream_health"]
        # the twin: the same changes by hand
        for g_ in range(G):
            twin.remove_queries(released[released[:, 0] == g_, 1], group=g_) if bool((released[:, 0] == g_).any()) else None
            sel = added[:, 0] == g_
            if bool(sel.any()):
                pts = twin.add_queries(seeds[sel].to(dev()), group=g_, resident=True)
                assert torch.equal(pts, added[sel, 1])
        assert torch.equal(p.model.stream_queries, twin.model.stream_queries)
        assert torch.equal(p.model.stream_first_row, twin.model.stream_first_row) and torch.equal(p._first_row, twin._first_row)
        for a, b in zip(buffers(gs), buffers(twin.model._gstream)):
            assert torch.equal(bits(a), bits(b))
        changed = len(captures)
    if graph:  # nothing is captured again after the replenish
        assert changed > 0 and len(captures) == changed
    else:
        assert not captures
    # the seeds are tracked: not the blank track of an empty slot
    tr = got[0]
    a0, a1 = added[0].tolist(), added[1].tolist()
    assert bool(torch.isfinite(tr).all()) and float((tr[a0[0], -1, a0[1]] - tr[a1[0], -1, a1[1]]).abs().max()) > 0.0
    for x in (p, twin):
        x.finish()


def test_replenish_refusals_on_a_stream():
    G, N, K = 1, 4, 2
    p = make_predictor(fresh_copy(small_model("f16x3")), K, None)
    video, q = stream_inputs(G, N, S + STEP, seed=9, frames=[0, 0, 1])
    p(video[:, :1], is_first_step=True, queries=q, add_support_grid=True)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.replenish(2)
    p(video[:, :S], add_support_grid=True)
    gs = p.model._gstream
    for bad in (dict(max_lost=0), dict(max_lost=3, look=2), dict(max_lost=2, grid=(65, 64)), dict(max_lost=2, group=1), dict(max_lost=2, look=S + 1)):
        with pytest.raises(ValueError):
            p.replenish(**bad)
    p(video[:, STEP:STEP + 5], add_support_grid=True)  # a short chunk closes the stream
    lost, cover = p.track_health()  # reading still works
    assert lost.shape == (G, N + K) and int(cover.sum()) <= N
    before = [t.clone() for t in buffers(gs)]
    with pytest.raises(RuntimeError, match="ended the stream"):
        p.replenish(1)
    torch.cuda.synchronize()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(buffers(gs), before))
    p.finish()
