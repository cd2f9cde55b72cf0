"""Seed points on corners (-m gpu): the kernel behind ops.seed_points (csrc/seed.hip: ctk_seed_points),
CoTrackerOnlinePredictor.replenish(seeds="corners") and the first-step grids of both predictors (grid_seeds = "corners").

Every comparison is exact, on integers (the score) or on bits (the queries and the streams): the reference is the numpy restatement
of tests/seed_reference.py, which tests/test_seed_host.py also holds a g++ build of csrc/seed_math.h against."""
import functools

import numpy as np
import pytest
import torch

import ctk_support
import seed_reference as R
from ctk_support import HW, S, STEP, bits, chunks, dev, stream_inputs, t

pytestmark = pytest.mark.gpu

_models = {}
small_model = functools.partial(ctk_support.small_model, _models, batch_mode="loop", hip_graph=False, range_guard=True, stream_groups=False,
                                stream_slots=False, online_feature_cache=False, stream_range_check="deferred")
fresh_copy = functools.partial(ctk_support.copy_without_stream_state, stream_slots=False)


def textured(h, w, seed, wild=False):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:h, :w]
    f = 128 + 80 * np.sin(xx / 5.0 + rng.rand(3, 1, 1) * 6) * np.cos(yy / 7.0 + rng.rand(3, 1, 1) * 6) + rng.randint(-30, 31, (3, h, w)) \
        + rng.rand(3, h, w)
    f = np.clip(f, 0, 255).astype(np.float32)
    if wild:  # below 0, above 255, a NaN pixel
        f[:, 5:9, 7:30] = -40.5
        f[:, 20:22, :] = 300.0
        f[1, 13, 17] = np.float32("nan")
        f[:, 30, 40] = np.float32("nan")
    return f


@functools.lru_cache(maxsize=None)
def kernel_frames():
    """name -> (frame, {radius: reference score map}): computed once for all kernel cases."""
    from cotracker_amd.synthetic import synthetic_video
    frames = {"37x53": textured(37, 53, 1), "64x96": textured(64, 96, 2, wild=True), "96x128": textured(96, 128, 3),
              "384x512": synthetic_video(1, 384, 512)[0, 0].numpy(), "patch": R.flat_with_patches(64, 96, [(20, 40)], seed=4)}
    radii = {"37x53": (1, 3, 7), "64x96": (3,), "96x128": (3, 7), "384x512": (3,), "patch": (3,)}
    return {k: (f, {r: R.score_map(f, r) for r in radii[k]}) for k, f in frames.items()}


KERNEL_CASES = [  # (frame, grid, keywords)
    ("37x53", (3, 5), {}), ("37x53", (3, 5), dict(radius=1)), ("37x53", (3, 5), dict(radius=7)),
    ("37x53", (3, 5), dict(inset=6)), ("37x53", (3, 5), dict(inset=7)), ("37x53", (3, 5), dict(margin=18)), ("37x53", (3, 5), dict(margin=40)),
    ("37x53", (37, 53), dict(margin=0, inset=0, min_score=0)),  # one pixel per cell: every pixel's score
    ("64x96", (4, 6), dict(bounds=(-2.5, 97.5, -2.5, 65.5))),  # border-widened bounds; the frame holds a NaN pixel and values off 0..255
    ("64x96", (64, 64), dict(margin=0, min_score=0)),  # cells smaller than two pixels along x, some of them empty
    ("64x96", (64, 64), dict(bounds=(-2.5, 97.5, -2.5, 65.5), margin=1)),
    ("96x128", (1, 1), {}), ("96x128", (1, 1), dict(radius=7, margin=0)),  # one workgroup walks many tiles
    ("96x128", (2, 3), dict(min_score=42000)),
    ("384x512", (8, 8), {}), ("384x512", (80, 80), dict(margin=0, inset=0)),
    ("patch", (4, 6), {}),
]


@pytest.mark.parametrize("name,grid,kw", KERNEL_CASES, ids=[f"{n}-{g[0]}x{g[1]}-{'-'.join(f'{k}{v}' for k, v in kw.items() if k != 'bounds')}"
                                                            + ("-wide" if "bounds" in kw else "") for n, g, kw in KERNEL_CASES])
def test_kernel(name, grid, kw):
    from cotracker_amd import ops
    frame, maps = kernel_frames()[name]
    want = R.seed_points(frame, grid, scores=maps[kw.get("radius", 3)], **kw)
    cells = grid[0] * grid[1]
    # the output lies inside a larger allocation: the bytes next to it must stay as they were
    guard = torch.full((cells * 3 + 64,), 0x5A5A5A5A, dtype=torch.int32, device=dev())
    got = ops.seed_points(t(frame), grid, out=guard[32:32 + cells * 3].view(cells, 3), **kw)
    assert got.data_ptr() == guard[32:].data_ptr() and got.shape == (cells, 3) and got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), want)
    assert bool((guard[:32] == 0x5A5A5A5A).all()) and bool((guard[32 + cells * 3:] == 0x5A5A5A5A).all())
    hit = want[:, 2] >= 0
    if name == "384x512" and grid == (8, 8):
        assert hit.all() and int(want[:, 2].min()) == 3351
    if name == "384x512" and grid == (80, 80):
        assert int(hit.sum()) == 6400
    if name == "patch":
        assert 1 <= hit.sum() <= 4 and (want[hit, 2] > 100000).all()
    if kw.get("inset") == 7 or kw.get("margin") == 40:
        assert not hit.any()
    if grid == (64, 64) and "bounds" in kw:
        assert hit.any() and not hit.all()


def test_kernel_is_repeatable_and_refuses():
    from cotracker_amd import ops
    frame = t(kernel_frames()["96x128"][0])
    a, b = ops.seed_points(frame, (5, 7)), ops.seed_points(frame, (5, 7))
    assert torch.equal(a, b)
    for bad in (dict(grid=(0, 4)), dict(grid=(257, 256)), dict(grid=(4, 4), radius=0), dict(grid=(4, 4), radius=8), dict(grid=(4, 4), margin=-1),
                dict(grid=(4, 4), inset=-1), dict(grid=(4, 4), min_score=-1), dict(grid=(4, 4), bounds=(5.0, 5.0, 0.0, 9.0))):
        with pytest.raises(ValueError):
            ops.seed_points(frame, **bad)
    for bad in (frame[:, :, ::2], frame[:2], frame.double(), frame.cpu()):
        with pytest.raises(ValueError):
            ops.seed_points(bad, (4, 4))


# ----------------------------------------------------------------------------------------------------------------------
# 2. replenish(seeds="corners") on a running stream, against the reference on the model-resolution frame and a hand-made twin
# ----------------------------------------------------------------------------------------------------------------------
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


def make_predictor(model, spare):
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=S)
    p.model, p.interp_shape, p.step = model, HW, STEP
    p.spare_points = spare
    return p.to(dev())


def model_frame(raw):
    """One raw frame [3,H,W] (float32 on the device) at model resolution, by the call forward makes (push_frames' ingest has its bits)."""
    return torch.nn.functional.interpolate(raw[None], HW, mode="bilinear", align_corners=True)[0]


def today_calls(released, added, ring=""):
    return sorted(["ctk_stream_assign" + ring] * bool(len(released)) + ["ctk_stream_assign_resident" + ring] * bool(len(added)))


@pytest.mark.parametrize("feed", ["chunks", "push-u8"])
def test_replenish_on_corners(monkeypatch, feed):
    from cotracker_amd import ops
    from cotracker_amd.predictor import choose_replenish
    G, N, K, grid, max_lost = 2, 5, 8, (4, 6), 2
    H, W = HW if feed == "chunks" else (100, 140)
    ih, iw = HW
    T = S + 3 * STEP  # four calls; the replenish after the second
    # a picture that is constant apart from random-dot patches in a few cells of the two upper cell rows
    patches = [(2, 20), (5, 70), (20, 40)] if feed == "chunks" else [(4, 30), (8, 100), (32, 60)]
    still = R.flat_with_patches(H, W, patches, seed=6, size=16 if feed == "chunks" else 24)
    raw = t(still)
    video = raw[None, None].expand(1, T, 3, H, W)
    video_u8 = raw.permute(1, 2, 0).to(torch.uint8)[None].expand(T, H, W, 3).contiguous()
    _, q = stream_inputs(G, N, T, seed=83, frames=[0, 0, 1, 3, 6])
    q[..., 1:] *= q.new_tensor([(W - 1) / (iw - 1), (H - 1) / (ih - 1)])  # raw-video pixels
    base = small_model("f16x3")
    p, twin, p_skip = (make_predictor(fresh_copy(base), K) for _ in range(3))
    captures = []
    orig = ops.WindowGraph._capture

    def counting(self, *a, **k):
        captures.append(self)
        return orig(self, *a, **k)
    monkeypatch.setattr(ops.WindowGraph, "_capture", counting)
    Nu = N + K
    bounds = (0.0, iw - 1.0, 0.0, ih - 1.0)
    frame_np = model_frame(raw).cpu().numpy()
    inset = max(1, int(min((iw - 1.0) / grid[1], (ih - 1.0) / grid[0]) // 4))
    assert inset == 3
    want = R.seed_points(frame_np, grid, bounds=bounds, inset=inset)
    assert 2 <= int((want[:, 2] >= 0).sum()) <= 14  # a few cells hold texture, most are flat

    def step(x, k, t0):
        if feed == "chunks":
            return x(video[:, t0:t0 + S], add_support_grid=True)
        return x.push_frames(video_u8[:S] if k == 0 else video_u8[t0 + S - STEP:t0 + S], add_support_grid=True)

    for x in (p, twin, p_skip):
        x(video[:, :1], is_first_step=True, queries=q, add_support_grid=True)
        with pytest.raises(RuntimeError, match="no stream is running"):
            x.replenish(max_lost, seeds="corners")
    changed = False
    for k, t0 in enumerate(chunks(T)):
        got, ref, got_skip = step(p, k, t0), step(twin, k, t0), step(p_skip, k, t0)
        if changed:  # after the replenish: the stream equals the twin's, bit for bit, on every point
            assert got[0].shape == ref[0].shape and torch.equal(bits(got[0]), bits(ref[0])) and torch.equal(got[1], ref[1]), k
            assert torch.equal(p.model.stream_queries, twin.model.stream_queries)
            assert bool(torch.isfinite(got_skip[0]).all())
        if k != 1:
            continue
        gs = p.model._gstream
        newest = p.resident_frames[1] - 1
        assert newest == gs.committed - 1 == t0 + S - 1
        assert p._newest_frame.shape == (3, ih, iw) and np.array_equal(p._newest_frame.cpu().numpy().view(np.int32), frame_np.view(np.int32))
        _, v, c = gs.emit(gs.committed - S, gs.committed, N_out=N)
        since = torch.arange(gs.committed - S, gs.committed, device=dev())[None, :, None] >= q[:, None, :, 0].long()
        thresh = float((torch.sigmoid(v) * torch.sigmoid(c))[since].median())  # both classes occur: some points are released
        lost0, cover0 = p.track_health(look=S, grid=grid, thresh=thresh)
        occ = p.model.stream_occupied[:, :Nu].clone()
        w_rel, w_add, w_cells = choose_replenish(lost0.cpu().numpy(), cover0.cpu().numpy(), occ.numpy(), max_lost)
        state = (len(captures), gs.serial, tuple(x.data_ptr() for x in [gs.queries, *gs.support, *gs.hist, gs.coords, gs.vis, gs.conf, gs.mask,
                                                                        *gs.pyr]), len(gs._wins))
        calls = library_calls(monkeypatch)
        released, added, seeds = p.replenish(max_lost, grid=grid, look=S, thresh=thresh, seeds="corners")
        seen = list(calls)
        assert state == (len(captures), gs.serial, tuple(x.data_ptr() for x in [gs.queries, *gs.support, *gs.hist, gs.coords, gs.vis, gs.conf,
                                                                                 gs.mask, *gs.pyr]), len(gs._wins))
        assert seen[:2] == ["ctk_stream_health", "ctk_seed_points"] and sorted(seen[2:]) == today_calls(released, added)
        # cells and slots: choose_replenish, as it stands
        assert np.array_equal(released.numpy(), w_rel) and np.array_equal(added.numpy(), w_add) and len(added) > 4
        # the seeds: the reference's pixel of every chosen cell that has one, the centre of the others
        sx, sy = (W - 1) / (iw - 1), (H - 1) / (ih - 1)
        exp = np.zeros((len(w_cells), 3), dtype=np.float32)
        exp[:, 0] = newest
        for i, cell in enumerate(w_cells.tolist()):
            if want[cell, 0] >= 0:
                exp[i, 1], exp[i, 2] = np.float32(float(want[cell, 0]) * sx), np.float32(float(want[cell, 1]) * sy)
            else:
                exp[i, 1] = np.float32((bounds[0] + (cell % grid[1] + 0.5) * ((bounds[1] - bounds[0]) / grid[1])) * sx)
                exp[i, 2] = np.float32((bounds[2] + (cell // grid[1] + 0.5) * ((bounds[3] - bounds[2]) / grid[0])) * sy)
        seeded = want[w_cells, 0] >= 0
        assert 0 < int(seeded.sum()) < len(w_cells)  # both kinds of cell were chosen
        assert seeds.dtype == torch.float32 and np.array_equal(seeds.numpy().view(np.int32), exp.view(np.int32))
        # the next track_health counts exactly one point in every seeded cell (and in every other chosen cell)
        l3, c3 = p.track_health(look=S, grid=grid, thresh=thresh)
        c3 = c3.reshape(G, -1).cpu().numpy()
        assert bool((c3[w_add[:, 0], w_cells] == 1).all()) and bool((l3[added[:, 0], added[:, 1]] == 0).all())
        # skip_flat: the flat cells get no point and their slots stay free
        del calls[:]
        rel_s, add_s, seeds_s = p_skip.replenish(max_lost, grid=grid, look=S, thresh=thresh, seeds="corners", skip_flat=True)
        assert calls[:2] == ["ctk_stream_health", "ctk_seed_points"] and sorted(calls[2:]) == today_calls(rel_s, add_s)
        assert torch.equal(rel_s, released) and torch.equal(add_s, added[torch.from_numpy(seeded)])
        assert torch.equal(bits(seeds_s), bits(seeds[torch.from_numpy(seeded)]))
        occ_s = p_skip.model.stream_occupied[:, :Nu]
        skipped = added[torch.from_numpy(~seeded)]
        assert bool(occ_s[add_s[:, 0], add_s[:, 1]].all()) and not bool(occ_s[skipped[:, 0], skipped[:, 1]].any())
        # a second call without a step adds nothing to the seeded cells; two launches, one wait
        del calls[:]
        again = p.replenish(max_lost, grid=grid, look=S, thresh=thresh, seeds="corners")
        assert [len(x) for x in again] == [0, 0, 0] and list(calls) == ["ctk_stream_health", "ctk_seed_points"]
        # the twin: the same changes by hand
        for g_ in range(G):
            if bool((released[:, 0] == g_).any()):
                twin.remove_queries(released[released[:, 0] == g_, 1], group=g_)
            sel = added[:, 0] == g_
            if bool(sel.any()):
                pts = twin.add_queries(seeds[sel].to(dev()), group=g_, resident=True)
                assert torch.equal(pts, added[sel, 1])
        assert torch.equal(bits(p.model.stream_queries), bits(twin.model.stream_queries))
        assert torch.equal(p.model.stream_first_row, twin.model.stream_first_row) and torch.equal(p._first_row, twin._first_row)
        for a, b in zip(buffers(gs), buffers(twin.model._gstream)):
            assert torch.equal(bits(a), bits(b))
        changed = True
    assert changed and not captures  # (hip_graph is off in these models: nothing to capture at all)
    for x in (p, twin, p_skip):
        x.finish()


def test_default_replenish_makes_the_calls_it_made(monkeypatch):
    """seeds="centre", the default: the health launch, then the release and the assign -- no seed launch."""
    G, N, K, grid = 1, 4, 6, (4, 6)
    p = make_predictor(fresh_copy(small_model("f16x3")), K)
    video, q = stream_inputs(G, N, S, seed=9, frames=[0, 0, 1])
    p(video[:, :1], is_first_step=True, queries=q, add_support_grid=True)
    p(video[:, :S], add_support_grid=True)
    with pytest.raises(ValueError, match="seeds must be"):
        p.replenish(2, grid=grid, seeds="corner")
    calls = library_calls(monkeypatch)
    released, added, seeds = p.replenish(2, grid=grid)
    assert calls[0] == "ctk_stream_health" and sorted(calls[1:]) == today_calls(released, added) and len(added) == K + len(released)
    centres = torch.tensor([[S - 1.0, (c % grid[1] + 0.5) * (HW[1] - 1.0) / grid[1], (c // grid[1] + 0.5) * (HW[0] - 1.0) / grid[0]]
                            for c in range(grid[0] * grid[1])])
    assert all(float((centres - s).abs().max(dim=1).values.min()) < 1e-4 for s in seeds)  # every seed is a cell centre
    # a stream without a newest frame refuses corners before any launch
    p._newest_frame = None
    del calls[:]
    with pytest.raises(RuntimeError, match="no newest frame"):
        p.replenish(2, grid=grid, seeds="corners")
    assert list(calls) == []
    p.finish()


# ----------------------------------------------------------------------------------------------------------------------
# 3. first-step grids: grid_seeds = "corners" on both predictors
# ----------------------------------------------------------------------------------------------------------------------
def grid_videos(B, T):
    """B videos [B,T,3,64,96] whose frames differ: a patch that sits elsewhere in every frame and video, one more per video."""
    out = np.stack([np.stack([R.flat_with_patches(*HW, [(4 + 5 * f, 8 + 6 * f + 20 * b), (40, 20 + 40 * b)], seed=10 * b + f)
                              for f in range(T)]) for b in range(B)])
    return out


def expected_grid(frame, size):
    from cotracker_amd.predictor import get_points_on_a_grid
    lattice = get_points_on_a_grid(size, HW)[0].numpy()
    want = R.seed_points(frame, (size, size))
    hit = want[:, 0] >= 0
    assert 0 < int(hit.sum()) < size * size  # seeds and lattice points both occur
    return np.where(hit[:, None], want[:, :2].astype(np.float32), lattice)


def test_first_step_grid_online():
    from cotracker_amd.predictor import get_points_on_a_grid
    vids = grid_videos(1, S)
    video = t(vids)
    p = make_predictor(fresh_copy(small_model("f16x3")), 0)
    lattice = get_points_on_a_grid(4, HW, device=dev())
    parent = torch.cat([torch.full_like(lattice[:, :, :1], 2.0), lattice], dim=2)  # what the first step builds today
    assert p.grid_seeds == "grid"
    p(video, is_first_step=True, grid_size=4, grid_query_frame=2)
    assert torch.equal(bits(p.queries), bits(parent))
    p.grid_seeds = "corners"
    p(video, is_first_step=True, grid_size=4, grid_query_frame=2)
    assert p.queries.shape == (1, 16, 3) and p.N == 16 and bool((p.queries[:, :, 0] == 2.0).all())
    assert np.array_equal(p.queries[0, :, 1:].cpu().numpy(), expected_grid(vids[0, 2], 4))
    with pytest.raises(ValueError, match="grid_query_frame"):
        p(video[:, :1], is_first_step=True, grid_size=4, grid_query_frame=2)  # a dummy chunk does not hold frame 2
    # raw frames of another size: the seeds are taken at model resolution, on the frame forward's resize gives
    big = torch.nn.functional.interpolate(video[0], (100, 140), mode="bilinear", align_corners=True)[None]
    p(big, is_first_step=True, grid_size=4, grid_query_frame=1)
    small = torch.nn.functional.interpolate(big[0, 1:2], HW, mode="bilinear", align_corners=True)[0]
    assert np.array_equal(p.queries[0, :, 1:].cpu().numpy(), expected_grid(small.cpu().numpy(), 4))
    tracks, vis = p(big[:, :S], grid_size=4, grid_query_frame=1)  # and the stream runs on them
    assert tracks.shape == (1, S, 16, 2) and bool(torch.isfinite(tracks).all())
    p.finish()


def test_first_step_grid_offline(monkeypatch):
    from cotracker_amd.predictor import CoTrackerPredictor, get_points_on_a_grid
    B = 2
    vids = grid_videos(B, S)
    video = t(vids)
    p = CoTrackerPredictor(checkpoint=None, offline=True, window_len=S)
    p.model, p.interp_shape = ctk_support.small_model(_models, "f16x3", kind="offline"), HW
    p = p.to(dev())
    seen = []
    fwd = p.model.forward

    def recording(*a, **k):
        seen.append(k["queries"].clone())
        return fwd(*a, **k)
    monkeypatch.setattr(p.model, "forward", recording)
    lattice = get_points_on_a_grid(4, HW, device=dev())
    parent = torch.cat([torch.full_like(lattice[:, :, :1], 3.0), lattice], dim=2).repeat(B, 1, 1)
    tr0, vi0 = p(video, grid_size=4, grid_query_frame=3)
    assert torch.equal(bits(seen[-1]), bits(parent))  # "grid": today's queries
    p.grid_seeds = "corners"
    tr1, vi1 = p(video, grid_size=4, grid_query_frame=3)
    got = seen[-1]
    assert got.shape == (B, 16, 3) and bool((got[:, :, 0] == 3.0).all())
    for b in range(B):
        assert np.array_equal(got[b, :, 1:].cpu().numpy(), expected_grid(vids[b, 3], 4)), b
    assert not torch.equal(got[0], got[1])  # one launch per video: each has its own seeds
    assert tr1.shape == tr0.shape == (B, S, 16, 2) and bool(torch.isfinite(tr1).all())
    # segm_mask filters afterwards, by its present rule: the rounded positions of video 0's points
    mask = torch.zeros(1, 1, *HW, device=dev())
    mask[:, :, :, :48] = 1.0
    p(video[:1], grid_size=4, grid_query_frame=3, segm_mask=mask)
    exp = expected_grid(vids[0, 3], 4)
    keep = exp[np.rint(exp[:, 0]) < 48]
    assert np.array_equal(seen[-1][0, :len(keep), 1:].cpu().numpy(), keep) and seen[-1].shape[1] == len(keep) + p.support_grid_size ** 2
    with pytest.raises(ValueError, match="grid_query_frame"):
        p(video, grid_size=4, grid_query_frame=S)
