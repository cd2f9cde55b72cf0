"""Predictor wrappers with the reference's public API (cotracker/predictor.py).

``CoTrackerPredictor.forward(video, queries, segm_mask, grid_size, grid_query_frame,
backward_tracking)`` (predictor.py:36-68) and ``CoTrackerOnlinePredictor.forward(video_chunk,
is_first_step, queries, grid_size, grid_query_frame, add_support_grid)`` (predictor.py:230-309)
keep their signatures, defaults, return values and quirks: the offline predictor
thresholds visibility alone at 0.9, the online one thresholds visibility*confidence at 0.6, the
query-frame prediction is overwritten with the query itself, dense mode derives its step from
the raw video width.  All tensor work stays on the GPU (the reference's per-batch Python fix-up
loop, predictor.py:177-185, is a single indexed write here).
"""
import contextlib
import math

import torch
import torch.nn.functional as F

from .build_cotracker import build_cotracker

_NO_STREAM = "no stream is running on the device stream state: run the first step and a tracked one first"


def get_points_on_a_grid(size, extent, center=None, device="cpu"):
    """size x size points covering an (H, W) extent with margin W/64, row-major, as (x, y)
    (behaviour of cotracker/models/core/model_utils.py:83-139)."""
    H, W = float(extent[0]), float(extent[1])
    if size == 1:
        return torch.tensor([W / 2, H / 2], device=device)[None, None]
    cy, cx = (H / 2, W / 2) if center is None else (float(center[0]), float(center[1]))
    m = W / 64
    # endpoints in the reference's evaluation order (python doubles are not associative)
    ys = torch.linspace(m - H / 2 + cy, H / 2 + cy - m, size, device=device)
    xs = torch.linspace(m - W / 2 + cx, W / 2 + cx - m, size, device=device)
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    return torch.stack([gx, gy], dim=-1).reshape(1, -1, 2)


def corner_grid(frames, size, lattice):
    """The first-step grid of grid_seeds = "corners": frames [B,3,ih,iw] float32 (model resolution, on the device), lattice
    [1,size*size,2] = get_points_on_a_grid(size, (ih, iw)) -> [B,size*size,2]: per video, the best-textured pixel (ops.seed_points:
    radius 3, candidates 4 pixels inside the image, score >= 1) of every cell of a uniform size x size partition of the picture,
    row-major like the lattice; a cell without a seed keeps the lattice point of its row and column.  One launch per video and a few
    elementwise ones; no wait."""
    from . import ops
    found = torch.stack([ops.seed_points(f.contiguous(), (size, size)) for f in frames])  # [B,size*size,3] int32
    return torch.where(found[:, :, :1] >= 0, found[:, :, :2].float(), lattice.expand(frames.shape[0], -1, -1))


def _cat(a, b, dim):
    return b if a is None else torch.cat([a, b], dim=dim)


class CoTrackerPredictor(torch.nn.Module):
    def __init__(self, checkpoint="./checkpoints/scaled_offline.pth", offline=True, v2=False, window_len=60):
        super().__init__()
        self.v2 = v2
        self.support_grid_size = 6
        model = build_cotracker(checkpoint, v2=v2, offline=offline, window_len=window_len)
        self.interp_shape = model.model_resolution
        self.model = model
        self.model.eval()
        # Not a reference kwarg (set it after construction; forward's signature is the reference's): "grid" -- a grid_size = g request
        # tracks the reference lattice -- or "corners": the best-textured pixel of every cell of a uniform g x g partition of the
        # picture on frame grid_query_frame (corner_grid); segm_mask filters afterwards, by the same rule.
        self.grid_seeds = "grid"

    @torch.no_grad()
    def forward(self, video, queries: torch.Tensor = None, segm_mask: torch.Tensor = None, grid_size: int = 0,
                grid_query_frame: int = 0, backward_tracking: bool = False):
        if queries is None and grid_size == 0:
            return self._compute_dense_tracks(video, grid_query_frame=grid_query_frame,
                                              backward_tracking=backward_tracking)
        return self._compute_sparse_tracks(video, queries, segm_mask, grid_size,
                                           add_support_grid=(grid_size == 0 or segm_mask is not None),
                                           grid_query_frame=grid_query_frame, backward_tracking=backward_tracking)

    # dense mode: grid_step^2 independent point chunks (predictor.py:70-98).  With `dense_group` set (a process group, or
    # True for the default group) the chunks are dealt out over the ranks and all-gathered (sharding.dense_sharded);
    # otherwise they are tracked in sequence on this device, as in the reference.
    dense_group = None
    # dense mode: chunks per model call.  1 (default) = one call per chunk, as the reference.  G > 1: G chunks go through ONE
    # query-group call of the model (video [1,...], queries [G,n,3]: resized and encoded once per call, `backward_tracking`
    # included -- the flipped video is again one video with G groups; model.py), the last call takes the remainder.  Chunk order
    # and the concatenation along the point axis are unchanged.  One video only, and not together with `dense_group` (both
    # raise).  Not a reference kwarg: set it after construction.
    dense_chunks_per_call = 1

    def _dense_layout(self, video, grid_size=80):
        H, W = video.shape[-2:]
        step = W // grid_size  # the reference derives the step from the raw video WIDTH for both axes (predictor.py:73)
        return step * step, (W // step) * (H // step)

    def _dense_chunk(self, video, offset, grid_query_frame, grid_size=80, backward_tracking=False):
        H, W = video.shape[-2:]
        step = W // grid_size
        gw, gh = W // step, H // step
        pts = torch.zeros(video.shape[0], gw * gh, 3, device=video.device)
        pts[:, :, 0] = grid_query_frame
        pts[:, :, 1] = torch.arange(gw, device=video.device).repeat(gh) * step + offset % step
        pts[:, :, 2] = torch.arange(gh, device=video.device).repeat_interleave(gw) * step + offset // step
        return self._compute_sparse_tracks(video=video, queries=pts, backward_tracking=backward_tracking)

    def _dense_chunks(self, video, offsets, grid_query_frame, grid_size=80, backward_tracking=False):
        """The chunks `offsets` of ONE video as one query-group call; returns them concatenated along the point axis."""
        H, W = video.shape[-2:]
        step = W // grid_size
        gw, gh = W // step, H // step
        pts = torch.zeros(len(offsets), gw * gh, 3, device=video.device)
        off = torch.tensor(list(offsets), device=video.device)[:, None]
        pts[:, :, 0] = grid_query_frame
        pts[:, :, 1] = torch.arange(gw, device=video.device).repeat(gh)[None] * step + off % step
        pts[:, :, 2] = torch.arange(gh, device=video.device).repeat_interleave(gw)[None] * step + off // step
        tracks, vis = self._compute_sparse_tracks(video=video, queries=pts, backward_tracking=backward_tracking)
        T = tracks.shape[1]
        return tracks.transpose(0, 1).reshape(1, T, -1, 2), vis.transpose(0, 1).reshape(1, T, -1)

    def _compute_dense_tracks(self, video, grid_query_frame, grid_size=80, backward_tracking=False):
        per_call = max(1, int(self.dense_chunks_per_call))
        if self.dense_group is not None:
            if per_call > 1:
                raise NotImplementedError("dense_chunks_per_call > 1 together with dense_group (sharded dense mode) is not implemented: "
                                          "set one of them")
            from .sharding import dense_sharded
            return dense_sharded(self, video, grid_query_frame, grid_size, backward_tracking,
                                 group=None if self.dense_group is True else self.dense_group)
        tracks = vis = None
        n_chunks = self._dense_layout(video, grid_size)[0]
        if per_call > 1:
            if video.shape[0] != 1:
                raise ValueError("dense_chunks_per_call > 1 tracks the chunks of ONE video per model call: video must be [1,T,3,H,W]")
            for o0 in range(0, n_chunks, per_call):
                offsets = range(o0, min(o0 + per_call, n_chunks))
                if len(offsets) == 1:
                    t_step, v_step = self._dense_chunk(video, offsets[0], grid_query_frame, grid_size, backward_tracking)
                else:
                    t_step, v_step = self._dense_chunks(video, offsets, grid_query_frame, grid_size, backward_tracking)
                tracks = _cat(tracks, t_step, 2)
                vis = _cat(vis, v_step, 2)
            return tracks, vis
        for offset in range(n_chunks):
            t_step, v_step = self._dense_chunk(video, offset, grid_query_frame, grid_size, backward_tracking)
            tracks = _cat(tracks, t_step, 2)
            vis = _cat(vis, v_step, 2)
        return tracks, vis

    def _resize(self, video):
        B, T, C, H, W = video.shape
        v = F.interpolate(video.reshape(B * T, C, H, W).float(), tuple(self.interp_shape), mode="bilinear",
                          align_corners=True)
        return v.reshape(B, T, 3, self.interp_shape[0], self.interp_shape[1])

    def _compute_sparse_tracks(self, video, queries, segm_mask=None, grid_size=0, add_support_grid=False,
                               grid_query_frame=0, backward_tracking=False):
        B, T, C, H, W = video.shape
        ih, iw = self.interp_shape
        video = self._resize(video)  # predictor.py:112-116
        if queries is not None:
            assert queries.shape[2] == 3
            queries = queries.clone().float()
            queries[:, :, 1:] *= queries.new_tensor([(iw - 1) / (W - 1), (ih - 1) / (H - 1)])
        elif grid_size > 0:
            pts = get_points_on_a_grid(grid_size, self.interp_shape, device=video.device)
            if self.grid_seeds == "corners":
                if self.v2:
                    raise NotImplementedError("grid_seeds = 'corners' on a v2 predictor is not implemented")
                if not 0 <= int(grid_query_frame) < T:
                    raise ValueError(f"grid_seeds = 'corners': grid_query_frame = {grid_query_frame} is not a frame of a {T}-frame video")
                pts = corner_grid(video[:, int(grid_query_frame)], grid_size, pts)
            elif self.grid_seeds != "grid":
                raise ValueError(f"grid_seeds must be 'grid' or 'corners', got {self.grid_seeds!r}")
            if segm_mask is not None:
                segm_mask = F.interpolate(segm_mask, tuple(self.interp_shape), mode="nearest")
                keep = segm_mask[0, 0][pts[0, :, 1].round().long(), pts[0, :, 0].round().long()].bool()
                pts = pts[:, keep]
            queries = torch.cat([torch.full_like(pts[:, :, :1], float(grid_query_frame)), pts], dim=2).repeat(B // pts.shape[0], 1, 1)
        if add_support_grid:
            g = get_points_on_a_grid(self.support_grid_size, self.interp_shape, device=video.device)
            g = torch.cat([torch.zeros_like(g[:, :, :1]), g], dim=2).repeat(B, 1, 1)
            queries = torch.cat([queries, g], dim=1)

        tracks, vis, *_ = self.model.forward(video=video, queries=queries, iters=6)

        if backward_tracking:
            tracks, vis = self._compute_backward_tracks(video, queries, tracks, vis)
            if add_support_grid:
                queries[:, -self.support_grid_size ** 2:, 0] = T - 1
        if add_support_grid:
            tracks = tracks[:, :, : -self.support_grid_size ** 2]
            vis = vis[:, :, : -self.support_grid_size ** 2]
        vis = vis > 0.9  # confidence is ignored by the offline predictor (predictor.py:170-171)

        # the query point itself is the prediction at its query frame, and visible (predictor.py:177-185)
        n = tracks.shape[2]
        B = tracks.shape[0]  # (= queries.shape[0]: the G query groups of a query-group call, dense_chunks_per_call)
        qt = queries[:, :n, 0].long()
        bi = torch.arange(B, device=tracks.device)[:, None].expand(B, n)
        ni = torch.arange(n, device=tracks.device)[None, :].expand(B, n)
        tracks[bi, qt, ni] = queries[:, :n, 1:]
        vis[bi, qt, ni] = True

        tracks = tracks * tracks.new_tensor([(W - 1) / (iw - 1), (H - 1) / (ih - 1)])
        return tracks, vis

    def _compute_backward_tracks(self, video, queries, tracks, vis):  # predictor.py:192-209
        T = video.shape[1]
        inv_q = queries.clone()
        inv_q[:, :, 0] = T - inv_q[:, :, 0] - 1
        inv_tracks, inv_vis, *_ = self.model(video=video.flip(1).contiguous(), queries=inv_q, iters=6)
        inv_tracks, inv_vis = inv_tracks.flip(1), inv_vis.flip(1)
        before = torch.arange(T, device=queries.device)[None, :, None] < queries[:, None, :, 0]
        tracks = torch.where(before[..., None], inv_tracks, tracks)
        vis = torch.where(before, inv_vis, vis)
        return tracks, vis


def choose_replenish(lost, cover, occupied, max_lost, max_new=None):
    """The policy of CoTrackerOnlinePredictor.replenish as a pure host function (numpy; no torch device): lost [G,N] (frames each
    user-visible point has been lost for, -1: an empty slot), cover [G,gh,gw] or [G,cells] (points per cell), occupied [G,N] bool ->
    (released [K,2], added [M,2], cells [M]): the (group, point) rows to release -- every occupied point with lost >= max_lost --,
    the (group, point) rows to seed and the row-major cell index of each seed.  Per group, independently: the cells with cover == 0
    in row-major order, one seed each, on the lowest free slots -- those this call releases included -- until free slots, empty
    cells or `max_new` (per group; None: no limit) run out.  Rows are ordered by group, then point (released) or cell (added)."""
    import numpy as np
    lost, occupied = np.asarray(lost), np.asarray(occupied).astype(bool)
    G, N = lost.shape
    cover = np.asarray(cover).reshape(G, -1)
    assert occupied.shape == (G, N), (occupied.shape, lost.shape)
    drop = occupied & (lost >= max_lost)
    free = ~occupied | drop
    released = np.argwhere(drop).reshape(-1, 2)
    added, cells = [], []
    for g in range(G):
        empty = np.flatnonzero(cover[g] == 0)
        slots = np.flatnonzero(free[g])
        m = min(len(empty), len(slots), len(empty) if max_new is None else max(int(max_new), 0))
        added += [(g, int(n)) for n in slots[:m]]
        cells += [int(c) for c in empty[:m]]
    return released.astype(np.int64), np.asarray(added, dtype=np.int64).reshape(-1, 2), np.asarray(cells, dtype=np.int64)


class CoTrackerOnlinePredictor(torch.nn.Module):
    def __init__(self, checkpoint="./checkpoints/scaled_online.pth", offline=False, v2=False, window_len=16):
        super().__init__()
        self.v2 = v2
        self.support_grid_size = 6
        model = build_cotracker(checkpoint, v2=v2, offline=False, window_len=window_len)
        self.interp_shape = model.model_resolution
        self.step = model.window_len // 2
        self.model = model
        self.model.eval()
        self.model.hip_graph = True  # streaming: replay the captured window graph per chunk (configs[3])
        # Not a reference kwarg (set it after construction, before the first step): K empty slots per query set, which
        # add_queries() fills and remove_queries() empties while the stream runs (model.stream_slots).  The first step builds
        # [user queries N | K empty | support grid], and later steps return the N + K user-visible points.  An empty slot is
        # tracked as a blank point and takes part in the space attention: like the support grid, K is part of the result.
        self.spare_points = 0
        # Not a reference kwarg (set it after construction, before the first step): None (default: every step returns everything
        # since frame 0, as the reference), or K >= window_len for a stream without an end (model.stream_history_frames).  With it
        # set, forward and push_frames return THIS WINDOW's rows -- tracks [.,T,N,2] in raw-video pixels and visibility [.,T,N]
        # (bool: visibility * confidence > 0.6, nothing visible below a slot's first row) for frames window_start ..
        # window_start + T - 1, the N (+ spare_points) user points only -- written by ONE launch (ctk_stream_emit) out of a ring
        # of K history rows: memory and the cost of a step no longer grow with the stream.  The first window_len - step rows
        # supersede what the previous step returned for those frames; older rows are final.  recent(n) returns the last n <= K frames.
        self.history_frames = None
        self._first_row = self._hw = None
        self._first_row32 = None  # (the tensor it was made from, [G,N_model] int32 for ctk_stream_emit)
        self._push_buf = None  # push_frames: the resident [window_len,3,ih,iw] float32 frames the next window still needs
        # The newest tracked frame at model resolution, [3,ih,iw]: a VIEW (nothing is launched or copied for it) of the last resized
        # chunk (forward) or of the push buffer (push_frames), for replenish(seeds="corners").  Valid until the next completed step:
        # a partial push only writes buffer rows below it.
        self._newest_frame = None
        self._colors = None  # draw(): (queries, _first_row, default colours [G,N_model,3]) as they stood when the colours were made
        # Not a reference kwarg (set it after construction; forward's signature is the reference's): how a first step with
        # grid_size = g and no queries places its g * g points.  "grid": the reference lattice.  "corners": a uniform g x g partition
        # of the picture, every cell taking its best-textured pixel (ops.seed_points) on frame grid_query_frame of the resized
        # chunk -- which must hold that frame: a one-frame dummy chunk cannot serve (ValueError) --; a cell without a seed keeps the
        # lattice point of its row and column.  Built on the device without a wait, one launch per video of the batch.
        self.grid_seeds = "grid"
        self._lens = None      # the `lens` property
        self._lens_buf = None  # push_frames with a lens: the corrected uint8 frames of one push, kept per stream shape
        self._push_reset()

    @property
    def lens(self):
        """Not in the reference: None (default: the frames are taken as a pinhole camera's, and nothing anywhere changes by a bit or a
        launch), or an ops.Lens -- the real camera behind the frames given to push_frames.  With a lens set, every arriving uint8 batch
        is first resampled into the pinhole picture of lens.ideal at raw resolution (ops.lens_frames(to="ideal", size=(H, W)): one more
        launch per push, into a scratch buffer kept per stream shape) and then ingested as before.  The stream then lives in ideal
        pixels: tracks, draw(), overlay(), stabilize() and every 3-D reader are right as they stand -- hand pose(), reconstruct(),
        localize() and extend() `intrinsics=predictor.lens.ideal` --, undistort() makes the matching pictures to draw onto and
        to_sensor() carries results back onto the original frames.  float32 frames with a lens set are refused (ValueError): the
        resampler is a uint8 one.  Setting the property while a pushed stream has tracked a window and is not closed raises
        RuntimeError: half a stream would be in other pixels.  forward() does not read `lens`: its chunks are the caller's float
        tensors, which a caller corrects beforehand (ops.lens_frames on the uint8 frames) or afterwards (ops.lens_points on the tracks)."""
        return self._lens

    @lens.setter
    def lens(self, value):
        from . import ops
        if value is not None and not isinstance(value, ops.Lens):
            raise ValueError("lens must be an ops.Lens or None")
        if self._push_tracked and not self._push_closed:
            raise RuntimeError("lens: a pushed stream is running (it has tracked a window and is not closed): its frames so far were "
                               "taken with the old setting; set the lens before the first push, or after final=True")
        self._lens = value

    @torch.no_grad()
    def undistort(self, frames, out=None, border="fill", fill=(0, 0, 0)):
        """Not in the reference: raw sensor frames -- uint8 [F,H,W,3], [F,3,H,W] or one frame, on the device -- resampled into the pinhole
        pictures of lens.ideal at the same size, by one launch and without a wait (ops.lens_frames(to="ideal")): what push_frames did
        to the frames it tracked, for the frames a caller wants to draw() / overlay() onto.  border "fill" / "edge" and fill as
        ops.lens_frames; out: frames of the same shape that do not overlap `frames`.  Needs a lens (RuntimeError), no stream.
        Returns the pictures."""
        from . import ops
        if self._lens is None:
            raise RuntimeError("undistort: no lens is set (predictor.lens = ops.Lens(...))")
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() not in (3, 4):
            raise ValueError("undistort: frames must be a uint8 device tensor [F,H,W,3], [F,3,H,W], [H,W,3] or [3,H,W]")
        one = frames.dim() == 3
        res = ops.lens_frames(frames[None] if one else frames, self._lens, to="ideal", out=(out[None] if one and out is not None else out),
                              border=border, fill=fill)
        return res[0] if one else res

    @torch.no_grad()
    def to_sensor(self, tracks, labels=False):
        """Not in the reference: positions in the ideal pixels the stream lives in -- float32 [...,N,2] on the device, e.g. the tracks
        push_frames returned -- carried onto the original sensor frames (ops.lens_points(to="sensor") with the predictor's lens), for
        ops.draw_tracks on the frames as the camera delivered them.  labels=True: also int8 [...,N] (1 carried, 0 the lens folds
        there, -1 not a position).  Needs a lens (RuntimeError).  Returns a new tensor, or (tensor, labels)."""
        from . import ops
        if self._lens is None:
            raise RuntimeError("to_sensor: no lens is set (predictor.lens = ops.Lens(...))")
        if isinstance(tracks, torch.Tensor) and not tracks.is_contiguous():
            tracks = tracks.contiguous()
        return ops.lens_points(tracks, self._lens, to="sensor", labels=labels)

    def add_queries(self, queries, group: int = 0, resident: bool = False):
        """Between two steps of a running stream (after its first tracked chunk): track queries [M,3] = (frame, x, y) -- frame
        counted from the start of the stream, not below the first frame the stream has not sampled yet (model.stream_assign);
        x, y in pixels of the raw video, rescaled like first-step queries -- in the M lowest free slots of query set `group`.
        Returns their point indices (LongTensor [M]) in the returned tracks.  Fewer than M free slots: RuntimeError, nothing
        assigned.

        resident=True: every frame from resident_frames[0] on is accepted -- the frames of the window just tracked, the newest
        picture the caller has seen among them (a click on it, a detector's output), whose features the stream still holds; frames a
        push_frames stream has buffered but not run yet lie behind that window and are assigned the plain way in the same call.
        The point is tracked from the next step on (visibility is False below that step's first frame)."""
        ih, iw = self.interp_shape
        H, W = self._hw
        q = queries.clone().float()
        if q.dim() != 2 or q.shape[1] != 3:
            raise ValueError("add_queries: queries must be [M,3] = (frame, x, y)")
        q[:, 1:] *= q.new_tensor([(iw - 1) / (W - 1), (ih - 1) / (H - 1)])
        occ = self.model.stream_occupied
        free = (~occ[group, :self.N]).nonzero().reshape(-1)
        if free.numel() < q.shape[0]:
            raise RuntimeError(f"add_queries: {q.shape[0]} queries for {free.numel()} free slots (spare_points = {self.spare_points})")
        points = free[:q.shape[0]]
        if resident:
            self.model.stream_assign(points + group * occ.shape[1], q, resident=True)
        else:
            self.model.stream_assign(points + group * occ.shape[1], q)
        self._mark_rows()
        return points

    @property
    def resident_frames(self):
        """(first, last + 1) of the frames add_queries(resident=True) admits besides later ones: the window the last step tracked
        (model.stream_resident_frames).  RuntimeError while no stream is running."""
        return self.model.stream_resident_frames

    def _health(self, look, grid, thresh, border):
        """One ctk_stream_health launch over the user-visible points -> (lost, cell, cover [G,gh*gw]) on the device and the bounds."""
        if self.v2:
            raise NotImplementedError("CoTracker2 keeps no stream state on the device: track_health / replenish on a v2 predictor is "
                                      "not implemented")
        gh, gw = (int(v) for v in grid)
        if gh < 1 or gw < 1 or gh * gw > 4096:
            raise ValueError(f"the coverage grid must have between 1 and 4096 cells, got {gh} x {gw}")
        if not float(border) >= 0.0:
            raise ValueError("border must be >= 0")
        if getattr(self, "queries", None) is None or self._hw is None:
            raise RuntimeError(_NO_STREAM)
        ih, iw = self.interp_shape
        bounds = (-float(border), iw - 1 + float(border), -float(border), ih - 1 + float(border))
        look = self.model.window_len if look is None else int(look)
        first = self._emit_first_row()
        if first is None:  # no spare_points: every slot holds a query of the first step
            first = torch.zeros(self.queries.shape[:2], dtype=torch.int32, device=self.queries.device)
        return self.model.stream_health(look, (gh, gw), thresh, self.N, first, bounds), bounds

    def track_health(self, look=None, grid=(8, 8), thresh=0.6, border=0.0):
        """Between two steps (or after the last): how the points of the running stream are doing, on the device, by ONE launch and
        without a wait -- for callers with a policy of their own.  -> (lost [G,N] int32, cover [G,gh,gw] int32).  lost[g, n]: for how
        many of the newest frames, counted back from the last tracked one over at most `look` (default window_len) frames and not
        beyond the point's first tracked frame, the point has been lost -- not visible by the rule of the returned visibility
        (visibility * confidence > thresh) or outside the picture widened by `border` model-resolution pixels; 0 for a point
        added since the last step or whose query frame lies ahead; -1 for an empty slot.  cover: how many of the N (+ spare_points)
        user-visible points lie in each cell of a grid = (gh, gw) over that area on the newest frame (points still waiting count
        at their query position)."""
        (lost, _, cover), _ = self._health(look, grid, thresh, border)
        return lost, cover.view(cover.shape[0], int(grid[0]), int(grid[1]))

    def replenish(self, max_lost, grid=(8, 8), look=None, thresh=0.6, border=0.0, max_new=None, group=None, seeds="centre", min_score=1,
                  skip_flat=False):
        """Between two steps of a running stream with spare_points: stop tracking what is lost and seed new points where nothing
        covers the picture.  Every user-visible point lost for >= max_lost frames (track_health's count over `look` >= max_lost
        frames) is released; then, per query set, every cell of the grid that no point covers gets one new query at its centre on
        the newest tracked frame, resident_frames[1] - 1, in row-major cell order on the lowest free slots (those just released
        included) until slots, cells or `max_new` (per query set) run out -- choose_replenish is the rule.  group: one query set
        only (default: all).  One health launch, ONE small device-to-host copy (the call's only wait), then at most one
        release and one resident assign for all query sets together; no graph is captured again.  Returns (released [K,2],
        added [M,2]) as (group, point) rows and queries [M,3] = (frame, x, y) of the seeds in raw-video pixels.  A seed is
        tracked from the next step on; until then it counts as covering its cell, so a second call adds nothing.  RuntimeError,
        before anything is written: no tracked step yet, no slots (spare_points), or a short chunk has ended the stream.

        seeds="corners": a chosen cell takes its best-textured pixel instead of its centre -- ONE more launch (ops.seed_points,
        ctk_seed_points: the corner score of csrc/seed_math.h) right after the health launch, on the newest tracked frame at
        model resolution, over the health bounds and grid, candidates max(1, min(cell width, cell height) // 4) pixels inside
        their cell; still one wait, for two small copies issued after both launches.  A chosen cell whose best score is below
        min_score (a blank wall: the 7 x 7 correlation has no peak there) takes its centre as before, or, with skip_flat=True,
        gets no point: its slot stays free.  choose_replenish picks cells and slots as before.  A stream that holds no newest
        frame (no tracked step since the first step): RuntimeError; any other `seeds`: ValueError; both before any launch."""
        if seeds not in ("centre", "corners"):
            raise ValueError(f"replenish: seeds must be 'centre' or 'corners', got {seeds!r}")
        if int(min_score) < 0:
            raise ValueError("replenish: min_score must be >= 0")
        max_lost = int(max_lost)
        look = self.model.window_len if look is None else int(look)
        if max_lost < 1:
            raise ValueError("replenish: max_lost must be >= 1")
        if look < max_lost:
            raise ValueError(f"replenish: look = {look} frames cannot show a point lost for max_lost = {max_lost}")
        if self.v2:
            raise NotImplementedError("CoTracker2 keeps no stream state on the device: track_health / replenish on a v2 predictor is "
                                      "not implemented")
        gh, gw = (int(v) for v in grid)
        if gh < 1 or gw < 1 or gh * gw > 4096:
            raise ValueError(f"the coverage grid must have between 1 and 4096 cells, got {gh} x {gw}")
        if not float(border) >= 0.0:
            raise ValueError("border must be >= 0")
        if getattr(self, "queries", None) is None or self._hw is None:
            raise RuntimeError("no stream is running: run the first step and a tracked one first")
        newest = self.resident_frames[1] - 1  # (RuntimeError: no tracked step, no slots, a closed stream)
        G, Nm = self.queries.shape[:2]
        if group is not None and not 0 <= int(group) < G:
            raise ValueError(f"replenish: group outside [0, {G})")
        if seeds == "corners" and self._newest_frame is None:
            raise RuntimeError("replenish(seeds='corners'): the stream holds no newest frame: run a tracked step first")
        (lost, _, cover), (x_lo, x_hi, y_lo, y_hi) = self._health(look, (gh, gw), thresh, border)
        corner = None
        if seeds == "corners":
            from . import ops
            inset = max(1, int(min((x_hi - x_lo) / gw, (y_hi - y_lo) / gh) // 4))
            corner = ops.seed_points(self._newest_frame, (gh, gw), bounds=(x_lo, x_hi, y_lo, y_hi), inset=inset, min_score=int(min_score))
            n_h = lost._base.numel()
            host = torch.empty(n_h + corner.numel(), dtype=torch.int32, pin_memory=True)
            host[:n_h].copy_(lost._base, non_blocking=True)
            host[n_h:].copy_(corner.view(-1), non_blocking=True)
            torch.cuda.current_stream(lost.device).synchronize()  # the one wait, for both copies
            flat, corner = host[:n_h].numpy(), host[n_h:].view(gh * gw, 3)
        else:
            flat = lost._base.cpu().numpy()  # the one wait: lost | cell | cover are one allocation
        lost_h, cover_h = flat[:G * self.N].reshape(G, self.N).copy(), flat[2 * G * self.N:].reshape(G, gh * gw).copy()
        if group is not None:  # the other query sets: nothing lost, nothing uncovered
            other = [g for g in range(G) if g != int(group)]
            lost_h[other], cover_h[other] = 0, 1
        occ = self.model.stream_occupied[:, :self.N].numpy()
        released, added, cells = choose_replenish(lost_h, cover_h, occ, max_lost, max_new)
        (H, W), (ih, iw) = self._hw, self.interp_shape
        q = torch.zeros(len(added), 3)
        if len(added):
            c = torch.from_numpy(cells)
            q[:, 0] = float(newest)
            q[:, 1] = ((x_lo + ((c % gw).double() + 0.5) * ((x_hi - x_lo) / gw)) * ((W - 1) / (iw - 1))).float()
            q[:, 2] = ((y_lo + (torch.div(c, gw, rounding_mode="floor").double() + 0.5) * ((y_hi - y_lo) / gh)) * ((H - 1) / (ih - 1))).float()
            if corner is not None:  # a cell with a seed: its integer model-resolution pixel, through the arithmetic of the centres
                found = corner[c]
                has = found[:, 0] >= 0
                q[has, 1] = (found[has, 0].double() * ((W - 1) / (iw - 1))).float()
                q[has, 2] = (found[has, 1].double() * ((H - 1) / (ih - 1))).float()
                if skip_flat:  # a flat cell gets no point; its slot stays free
                    keep = has.numpy()
                    q, added, cells = q[has], added[keep], cells[keep]
        if len(released):
            self.model.stream_release(torch.from_numpy(released[:, 0] * Nm + released[:, 1]))
        if len(added):
            qm = q.clone()
            qm[:, 1:] *= qm.new_tensor([(iw - 1) / (W - 1), (ih - 1) / (H - 1)])  # (add_queries' rescaling, operation for operation)
            self.model.stream_assign(torch.from_numpy(added[:, 0] * Nm + added[:, 1]), qm, resident=True)
        if len(released) or len(added):
            self._mark_rows()
        return torch.from_numpy(released), torch.from_numpy(added), q

    def remove_queries(self, points, group: int = 0):
        """Between two steps of a running stream: stop tracking the listed points (any of the N + K user-visible ones) of query set
        `group`; their slots are free for add_queries()."""
        points = torch.as_tensor(points).reshape(-1).long().cpu()
        if points.numel() and (int(points.min()) < 0 or int(points.max()) >= self.N):
            raise ValueError(f"remove_queries: point index outside [0, {self.N})")
        self.model.stream_release(points + group * self.queries.shape[1])
        self._mark_rows()

    @property
    def window_start(self):
        """history_frames: the frame number of row 0 of the last result (None before the first tracked step)."""
        gs = getattr(self.model, "_gstream", None)
        return self.model.stream_window_start if gs is not None and gs.live and gs.ring_rows is not None else None

    def _quiet(self):
        """model.quiet_return() for the model call of a step: on a ring stream the model steps the state and this predictor emits
        the result itself.  (A model without the method has no ring: nothing to ask.)"""
        return getattr(self.model, "quiet_return", contextlib.nullcontext)()

    def _emit_first_row(self):
        """_first_row ([G,N] long, the user-visible points) as ctk_stream_emit wants it: int32 over all N_model points of the query
        table, INT32_MAX for an empty slot.  Rebuilt only when add / remove changed it."""
        if self._first_row is None:
            return None
        if self._first_row32 is None or self._first_row32[0] is not self._first_row:
            big = torch.iinfo(torch.int32).max
            fr = torch.zeros(self.queries.shape[:2], dtype=torch.int32, device=self._first_row.device)
            fr[:, :self.N] = self._first_row.clamp(max=big).to(torch.int32)
            self._first_row32 = (self._first_row, fr)
        return self._first_row32[1]

    def _emit_result(self, f0, f1):
        """Frames [f0, f1) as a step hands them back, by one launch: the N user-visible points, tracks in raw-video pixels (the
        float32 multiplication of _user_result), visibility * confidence thresholded at 0.6 and masked by the slots' first rows."""
        (H, W), (ih, iw) = self._hw, self.interp_shape
        return self.model.stream_emit(f0, f1, N_out=self.N, scale=((W - 1) / (iw - 1), (H - 1) / (ih - 1)), logits=False, thresh=0.6,
                                      first_row=self._emit_first_row())

    def recent(self, n: int):
        """history_frames: (tracks [.,n,N,2], visibility [.,n,N]) of the last n frames tracked so far, in frame order, n <=
        min(frames so far, history_frames); one launch."""
        gs = getattr(self.model, "_gstream", None)
        if gs is None or not gs.live or gs.ring_rows is None:  # (the running stream's own ring: history_frames as the first step read it)
            raise RuntimeError("recent(n) reads the ring history of a running stream: set history_frames before the first step")
        done, n = gs.committed, int(n)
        if not 1 <= n <= min(done, gs.ring_rows):
            raise ValueError(f"recent: n must lie in [1, {min(done, gs.ring_rows)}] (frames so far: {done}, history_frames: "
                             f"{gs.ring_rows})")
        return self._emit_result(done - n, done)

    def _draw_colors(self, gs):
        """Default colours of draw(): ops.rainbow_colors over the y of every slot's query -- the point's position on its first row --,
        uint8 [G,N_model,3] on the device, read from the resident query table of the stream state `gs` that draw() has validated
        (any stream on the device state: slots or not, running or just closed).  Rebuilt only when the query table changed: a first
        step replaces self.queries, add / remove / replenish replace self._first_row."""
        held = getattr(self, "_colors", None)
        if held is None or held[0] is not self.queries or held[1] is not self._first_row:
            from . import ops
            held = self._colors = (self.queries, self._first_row, ops.rainbow_colors(gs.queries.reshape(gs.G, gs.N, 3)[..., 2]))
        return held[2]

    @torch.no_grad()
    def draw(self, frames, first_frame=None, trail=8, radius=4, half_width=1, colors=None, out=None, group=None):
        """Not in the reference, whose cotracker/utils/visualizer.py draws on the host: the N (+ spare_points) user-visible points
        of the running stream drawn onto `frames` -- raw-video resolution, uint8, [F,H,W,3] or [F,3,H,W] (or one frame), on the
        device -- in place (or into `out`), by two launches and without a wait (ops.StreamGroups.draw: the stream's own history and
        logits, no emit in between).  Picture j shows frame first_frame + j; default: the newest F tracked frames.  A point that
        the returned visibility calls visible (visibility * confidence > 0.6, at or above its slot's first row) is a disc of
        `radius` pixels, any other tracked one a ring; `trail` segments of `half_width` join the visible positions of the frames
        before, fading quadratically.  colors: uint8 [N,3] or [G,N,3] for the user-visible points; default a rainbow over the
        points' query y, rebuilt only when add_queries / remove_queries / replenish changed the query table.  group: one query set
        only (default: all, drawn in order).  ValueError when first_frame - trail has left the ring (history_frames) or the
        pictures lie beyond what has been tracked.  Returns the drawn frames."""
        gs, scale = self._running("draw")
        frames, out, one, layout, first_frame = self._raw_frames(frames, out, first_frame, gs, "draw")
        G, Nm = self.queries.shape[:2]
        dev = self.queries.device
        if colors is None:
            colors = self._draw_colors(gs)
        else:
            c = torch.as_tensor(colors)
            if c.dtype != torch.uint8 or c.shape[-1] != 3 or c.numel() not in (self.N * 3, G * self.N * 3):
                raise ValueError(f"draw: colors must be uint8 [{self.N},3] or [{G},{self.N},3]")
            colors = torch.zeros(G, Nm, 3, dtype=torch.uint8, device=dev)
            colors[:, :self.N] = c.to(dev).reshape(-1, self.N, 3)
        res = self.model.stream_draw(frames, first_frame, colors, N_out=self.N, scale=scale, thresh=0.6, first_row=self._emit_first_row(),
                                     trail=trail, radius=radius, half_width=half_width, out=out, layout=layout, group=group)
        return res[0] if one else res

    @torch.no_grad()
    def camera_motion(self, n=None, first_frame=None, lag=1, model="similarity", tol=2.0, hypotheses=128, min_base=16.0, seed=0, group=None):
        """Not in the reference, whose cotracker/utils/visualizer.py subtracts the mean displacement of points a user mask calls
        background, on the host: how the camera moved from frame f - lag to frame f of the running stream, fitted robustly to the N
        (+ spare_points) user-visible points, and which points moved differently -- by one launch and without a wait
        (ops.StreamGroups.motion: the stream's own history and logits, no emit in between).  The rows are the n frames from
        first_frame on; default: the newest `step` frames (those tracked so far), ending at the newest; n = 1: the newest frame only.
        A point counts on a pair of frames when the returned visibility calls it visible on both (visibility * confidence > 0.6, at
        or above its slot's first row).  model "similarity" or "translation"; tol and min_base are raw-video pixels, as are the
        matrices: raw-video position on frame f = motion @ (position on frame f - lag, 1).  group: one query set only.  ValueError
        when first_frame - lag has left the ring (history_frames) or the frames lie beyond what has been tracked.  Returns
        (motion float32 [G,n,2,3], inlier int8 [G,n,N]: -1 not on both frames, 0 moves differently, 1 moves with the camera; stats
        int32 [G,n,4] = (points on both frames, inliers, best hypothesis or -1, 0)), on the device; a frame without a fit has the
        identity."""
        gs, scale = self._running("camera_motion")
        first_frame, n = self._newest_frames(gs, n, first_frame, "camera_motion")
        return self.model.stream_motion(first_frame, n, N_out=self.N, scale=scale, thresh=0.6, first_row=self._emit_first_row(), lag=lag,
                                        model=model, tol=tol, hypotheses=hypotheses, min_base=min_base, seed=seed, group=group)

    @torch.no_grad()
    def stabilize(self, frames, first_frame=None, alpha=0.1, zoom=1.0, border="fill", fill=(0, 0, 0), out=None, group=0, reset=False,
                  model="similarity", tol=2.0, hypotheses=128, min_base=16.0, seed=0):
        """Not in the reference: `frames` -- raw-video resolution, uint8, [F,H,W,3] or [F,3,H,W] (or one frame), on the device, as
        draw() takes them -- steadied by the camera motion of the running stream, by three launches and without a wait
        (ops.StreamGroups.stabilize: camera_motion's fit with lag 1 on the stream's own history and logits, ops.smooth_path,
        ops.warp_frames).  Picture j shows frame first_frame + j; default: the newest F tracked frames.  The N (+ spare_points)
        user-visible points of query set `group` vote, where the returned visibility calls them visible (visibility * confidence >
        0.6, at or above their slot's first row); model "similarity" or "translation", tol and min_base in raw-video pixels.
        alpha: 0 locks onto the first steadied frame for ever, 1 corrects nothing, in between a steady pan of v pixels a frame is
        followed (1 - alpha) v / alpha pixels behind.  zoom > 1 enlarges the middle to hide the border a correction uncovers; border
        "fill" paints what lies outside the picture with `fill`, "edge" repeats the edge pixels.  The path goes on from call to call:
        the first call for a group, or reset=True, locks onto first_frame (that picture is copied, or only zoomed: the motion
        from the frame before into it is not part of the path); any other call must start at the frame the last one ended
        on, with the same alpha (ValueError otherwise, as when first_frame - 1 has left the ring or the pictures lie beyond what has
        been tracked).  A new first step drops the path.  Call draw() first when marks are wanted: the marks are then warped with the
        picture.  A point at raw position x of a frame appears at inverse(warp) x of the steadied one.  The stream's tracks are
        untouched.  Returns (frames_out: a new tensor, or `out`; warp float32 [n,2,3] on the device)."""
        gs, scale = self._running("stabilize")
        frames, out, one, layout, first_frame = self._raw_frames(frames, out, first_frame, gs, "stabilize")
        res, warp = self.model.stream_stabilize(frames, first_frame, group=group, reset=reset, alpha=alpha, zoom=zoom, border=border, fill=fill,
                                                out=out, layout=layout, N_out=self.N, scale=scale, thresh=0.6,
                                                first_row=self._emit_first_row(), model=model, tol=tol, hypotheses=hypotheses,
                                                min_base=min_base, seed=seed)
        return (res[0] if one else res), warp

    def _running(self, who):
        """The running stream's device state for the readers of its history (draw .. follow), and the scale of history positions to
        raw-video pixels."""
        if self.v2:
            raise NotImplementedError(f"CoTracker2 keeps no stream state on the device: {who} on a v2 predictor is not implemented")
        gs = getattr(self.model, "_gstream", None)
        if getattr(self, "queries", None) is None or self._hw is None or gs is None or not gs.live or gs.committed == 0:
            raise RuntimeError(_NO_STREAM)
        (H, W), (ih, iw) = self._hw, self.interp_shape
        return gs, ((W - 1) / (iw - 1), (H - 1) / (ih - 1))

    def _raw_frames(self, frames, out, first_frame, gs, who):
        """Raw-video pictures as draw() and stabilize() take them -> (frames [F,...], out, whether one frame was given, the layout by
        the stream's H x W, first_frame: default the newest F tracked frames)."""
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() not in (3, 4):
            raise ValueError(f"{who}: frames must be a uint8 device tensor [F,H,W,3], [F,3,H,W], [H,W,3] or [3,H,W]")
        one = frames.dim() == 3
        if one:
            frames = frames[None]
            out = out[None] if out is not None else None
        H, W = self._hw
        hwc, chw = tuple(frames.shape[1:]) == (H, W, 3), tuple(frames.shape[1:]) == (3, H, W)
        if not (hwc or chw):
            raise ValueError(f"{who}: expected {H} x {W} frames, [F,{H},{W},3] or [F,3,{H},{W}]; got {tuple(frames.shape)}")
        done, F_ = gs.committed, frames.shape[0]
        first_frame = done - F_ if first_frame is None else int(first_frame)
        if first_frame < 0 or first_frame + F_ > done:
            raise ValueError(f"{who}: pictures of frames [{first_frame}, {first_frame + F_}) lie beyond what has been tracked ({done} frames)")
        return frames, out, one, ("hwc" if hwc and not chw else ("chw" if chw and not hwc else None)), first_frame

    def _newest_frames(self, gs, n, first_frame, who):
        """(n, first_frame) of a reader -> (first_frame, n); default: the newest `step` frames, ending at the newest."""
        done = gs.committed
        n = (min(self.step, done) if first_frame is None else done - int(first_frame)) if n is None else int(n)
        first_frame = done - n if first_frame is None else int(first_frame)
        if n < 1 or first_frame < 0 or first_frame + n > done:
            raise ValueError(f"{who}: frames [{first_frame}, {first_frame + n}) lie beyond what has been tracked ({done} frames)")
        return first_frame, n

    @torch.no_grad()
    def pin(self, frame=None, group=0):
        """Not in the reference: keeps where the points of query set `group` are on `frame` (default: the newest tracked one) --
        device copies of that frame's row of the stream's history (positions, and the visibility the returned results would call
        visible) and the frame number, by one launch and without a wait.  The anchor (ops.FieldAnchor) is what propagate() carries a
        picture of that frame on with after a ring (history_frames) has dropped the frame itself.  A frame still inside the window
        being tracked is refined by the next step: pin it once it is final, or pin again.  ValueError when the frame has left the
        ring or has not been tracked."""
        from . import ops
        gs, _ = self._running("pin")
        frame, group = gs.committed - 1 if frame is None else int(frame), int(group)
        if not 0 <= group < gs.G:
            raise ValueError(f"pin: group must lie in [0, {gs.G})")
        if not 0 <= frame < gs.committed:
            raise ValueError(f"pin: frame {frame} lies beyond what has been tracked ({gs.committed} frames)")
        coords, visible = self.model.stream_emit(frame, frame + 1, N_out=None, scale=(1.0, 1.0), logits=False, thresh=0.6,
                                                 first_row=self._emit_first_row())
        return ops.FieldAnchor(coords[group:group + 1, 0], visible[group:group + 1, 0].view(torch.uint8), frame, group)

    @torch.no_grad()
    def propagate(self, picture, anchor_or_frame, first_frame=None, n=None, cell=16, radius=2, border="fill", fill=(0, 0, 0), out=None,
                  group=0):
        """Not in the reference, which lays a grid on a segm_mask of the first frame and cannot say where that mask is later: a
        `picture` -- raw-video resolution, uint8, [H,W,3], [3,H,W] or a mask [H,W], on the device -- that shows frame
        `anchor_or_frame` (a frame number the history still holds, or an anchor from pin()) carried onto the n frames from
        first_frame on along the N (+ spare_points) user-visible points of query set `group`, by four launches and without a wait
        (ops.StreamGroups.field on the stream's own history and logits, then ops.warp_field).  Default: the frames of the window
        just tracked, as in draw().  A dense displacement field is interpolated from the points visible on both frames (cell: pixels
        per grid cell, a power of two 4..64; radius: the reach of a point in cells, 1..4; holes are filled from coarser levels) and
        the picture is resampled backwards through it, bilinear in 1/256 pixel; border "fill" paints what comes from outside the
        picture with `fill`, "edge" repeats the edge pixels.  The weighting is zeroth order: exact to about a tenth of a pixel
        inside a covered region, biased near its rim and blocky across large holes.  The stream's tracks are untouched.  Returns the
        pictures [n, ...] in the layout of `picture` (a new tensor, or `out`)."""
        from . import ops
        who = "propagate"
        gs, scale = self._running(who)
        H, W = self._hw
        if not (isinstance(picture, torch.Tensor) and picture.dtype == torch.uint8 and picture.is_cuda and
                tuple(picture.shape) in ((H, W, 3), (3, H, W), (H, W))):
            raise ValueError(f"{who}: picture must be a uint8 device tensor [{H},{W},3], [3,{H},{W}] or [{H},{W}]")
        first_frame, n = self._newest_frames(gs, n, first_frame, who)
        if isinstance(anchor_or_frame, ops.FieldAnchor):
            if anchor_or_frame.group != int(group):
                raise ValueError(f"{who}: the anchor was pinned on group {anchor_or_frame.group}, not {group}")
            where = dict(anchor=anchor_or_frame)
        else:
            where = dict(to=int(anchor_or_frame))
        layout = None if picture.dim() == 2 else ("hwc" if tuple(picture.shape) == (H, W, 3) else "chw")
        src = picture[None].expand(n, *picture.shape)  # (a frame stride of 0: every output picture reads the one source)
        a, out, _ = ops._warp_field_args(src, None, cell, border, fill, out, None, layout, 0, who)
        field = self.model.stream_field(first_frame, n, size=(H, W), cell=cell, radius=radius, N_out=self.N, scale=scale, thresh=0.6,
                                        first_row=self._emit_first_row(), group=int(group), **where)[0]
        ops._warp_field_launch(a, field[0], who)
        return out

    @torch.no_grad()
    def dense_flow(self, n=None, first_frame=None, lag=1, cell=16, radius=2, group=0, out=None):
        """Not in the reference (whose dense mode tracks every pixel at the full cost of the model): a dense flow picture of each of
        the n frames from first_frame on (default: the frames of the window just tracked) interpolated from the N (+ spare_points)
        user-visible points of query set `group`, by four launches and without a wait (ops.StreamGroups.field with `lag`, then the
        flow output of ops.warp_field).  flow[j, y, x] = the displacement in raw-video pixels from pixel (x, y) of frame f to the
        matching position on frame f - lag (a negative lag: forward flow, towards frames already tracked).  cell, radius and the
        limits are propagate()'s.  Returns float32 [n,H,W,2] on the device (a new tensor, or `out`)."""
        from . import ops
        who = "dense_flow"
        gs, scale = self._running(who)
        H, W = self._hw
        first_frame, n = self._newest_frames(gs, n, first_frame, who)
        a, _, flow = ops._warp_field_args(None, (H, W), cell, "fill", (0, 0, 0), None, True if out is None else out, None, n, who,
                                          device=self.queries.device)
        field = self.model.stream_field(first_frame, n, size=(H, W), cell=cell, radius=radius, lag=lag, N_out=self.N, scale=scale,
                                        thresh=0.6, first_row=self._emit_first_row(), group=int(group))[0]
        ops._warp_field_launch(a, field[0], who)
        return flow

    @torch.no_grad()
    def split_objects(self, frame=None, lag=8, objects=4, group=0, model="similarity", tol=2.0, hypotheses=128, min_base=16.0, min_points=8,
                      seed=0):
        """Not in the reference: which of the N (+ spare_points) user-visible points of query set `group` move together between
        frame - lag and `frame` (default: the newest tracked one) -- one launch of ctk_fit_objects in split mode
        (ops.StreamGroups.objects on the stream's own history and logits) and one pin(frame), without a wait.  Round 0 fits all points
        visible on both frames, round r + 1 what round r's inliers left; a round with fewer than min_points inliers ends the rounds.
        The round order is by size: most inliers first -- usually the background --, decided per pair of frames and NOT stable from
        pair to pair; that is why one splits once and follows by labels.  model, tol, hypotheses, min_base (raw-video pixels) and
        seed are camera_motion()'s.  ValueError when frame - lag is negative or has left the ring (history_frames) or the frame has
        not been tracked.  Returns an ops.ObjectSet: labels int8 [N_model] on the device (r = the point moved with round r; -1 = no
        round took it, it was not seen on both frames, or it is no user-visible point), the anchor pinned on `frame`, and `objects`."""
        from . import ops
        who = "split_objects"
        gs, scale = self._running(who)
        frame, lag, group = gs.committed - 1 if frame is None else int(frame), int(lag), int(group)
        if not 0 <= group < gs.G:
            raise ValueError(f"{who}: group must lie in [0, {gs.G})")
        if not 0 <= frame < gs.committed or lag < 1 or frame - lag < 0:
            raise ValueError(f"{who}: frames {frame - lag} and {frame} must both have been tracked ({gs.committed} frames), lag >= 1")
        label = self.model.stream_objects(frame, 1, objects=objects, lag=lag, N_out=self.N, scale=scale, thresh=0.6,
                                          first_row=self._emit_first_row(), model=model, tol=tol, hypotheses=hypotheses, min_base=min_base,
                                          min_points=min_points, seed=seed, group=group)[1]
        labels = torch.full((gs.N,), -1, dtype=torch.int8, device=label.device)
        labels[:self.N] = torch.where(label[0, 0] == ops.OBJECT_NONE, torch.full_like(label[0, 0], -1), label[0, 0])
        return ops.ObjectSet(labels, self.pin(frame, group), int(objects))

    @torch.no_grad()
    def label_objects(self, boxes, frame=None, group=0):
        """Not in the reference: the objects a user boxed on `frame` (default: the newest tracked one).  boxes [L,4] = (x0, y0, x1, y1)
        in raw-video pixels, L <= 16: a user-visible point of query set `group` that is visible on `frame` and lies inside box r
        (borders included) gets label r; where boxes overlap the lowest r wins; every other point gets -1.  Elementwise torch on the
        device and one pin(frame), without a wait.  Returns an ops.ObjectSet (see split_objects) for follow()."""
        from . import ops
        who = "label_objects"
        gs, scale = self._running(who)
        boxes = torch.as_tensor(boxes, dtype=torch.float32)
        if boxes.dim() != 2 or boxes.shape[1] != 4 or not 1 <= boxes.shape[0] <= ops.L.Objects.OBJECTS_MAX:
            raise ValueError(f"{who}: boxes must be [L,4] = (x0, y0, x1, y1) with L in 1..{ops.L.Objects.OBJECTS_MAX}")
        anchor = self.pin(frame, group)
        boxes = boxes.to(anchor.coords.device)
        x, y = anchor.coords[0, :, 0] * scale[0], anchor.coords[0, :, 1] * scale[1]
        inside = ((x[None] >= boxes[:, 0:1]) & (x[None] <= boxes[:, 2:3]) & (y[None] >= boxes[:, 1:2]) & (y[None] <= boxes[:, 3:4]) &
                  (anchor.visible[0] != 0)[None])
        inside[:, self.N:] = False
        lowest = inside.to(torch.int8).argmax(dim=0).to(torch.int8)  # (the first True)
        labels = torch.where(inside.any(dim=0), lowest, torch.full_like(lowest, -1))
        return ops.ObjectSet(labels, anchor, boxes.shape[0])

    @torch.no_grad()
    def follow(self, objects, n=None, first_frame=None, model="similarity", tol=2.0, hypotheses=128, min_base=16.0, min_points=8, seed=0):
        """Not in the reference: where the objects of an ops.ObjectSet (split_objects / label_objects) are on the n frames from
        first_frame on (default: the frames of the window just tracked, as in camera_motion()) -- one launch of ctk_fit_objects in
        labels mode against the set's anchor (ops.StreamGroups.objects on the stream's own history and logits), without a wait.  The
        anchor outlives the ring (history_frames): nothing is chained and nothing drifts.  Object r is fitted to the points labelled
        r that are visible on the frame and on the anchor (a slot released and reassigned after the anchor was taken drops out); the
        objects are independent, and one with fewer than min_points inliers has no fit on that frame.  model, tol, hypotheses,
        min_base (raw-video pixels) and seed are camera_motion()'s.  Returns, on the device: motion float32 [n,L,2,3]: raw-video
        position on frame f = motion @ (position on the anchor's frame, 1), the identity where there is no fit; label int8
        [n,N]: -1 not on both frames, r = moves with object r, 127 = labelled for no object or does not move with its own; stats int32
        [n,L,4] = (points of the object on both frames, inliers, best hypothesis or -1, 0); box float32 [n,L,4] = (min x, min y, max
        x, max y) of the object's inliers on frame f in raw-video pixels, max < min where there is no fit."""
        from . import ops
        who = "follow"
        gs, scale = self._running(who)
        if not isinstance(objects, ops.ObjectSet):
            raise ValueError(f"{who}: objects must be an ops.ObjectSet (split_objects, label_objects)")
        first_frame, n = self._newest_frames(gs, n, first_frame, who)
        motion, label, stats, box = self.model.stream_objects(first_frame, n, labels=objects.labels[None], objects=objects.objects,
                                                              anchor=objects.anchor, N_out=self.N, scale=scale, thresh=0.6,
                                                              first_row=self._emit_first_row(), model=model, tol=tol, hypotheses=hypotheses,
                                                              min_base=min_base, min_points=min_points, seed=seed, group=objects.anchor.group)
        return motion[0], label[0], stats[0], box[0].to(torch.float32) / 16.0

    @torch.no_grad()
    def follow_planes(self, objects, n=None, first_frame=None, inverse=False, tol=2.0, hypotheses=128, min_base=16.0, min_points=8, seed=0):
        """Not in the reference: where the objects of an ops.ObjectSet (split_objects / label_objects) are on the n frames from
        first_frame on (default: the frames of the window just tracked) when each is a planar surface seen under perspective -- a
        screen, a wall, a sign, a pitch -- which follow()'s similarity slides and shears on: one launch of ctk_fit_planes against the
        set's anchor (ops.StreamGroups.planes on the stream's own history and logits), without a wait.  Object r is fitted to the points
        labelled r that are visible on the frame and on the anchor; the objects are independent, and one with fewer than min_points
        inliers (or fewer than four points) has no fit on that frame.  inverse=True: the matrices map frame f onto the anchor's frame
        (what a backward warp needs; fitted that way round, nothing is inverted).  tol, hypotheses, min_base (raw-video pixels) and seed
        are ops.fit_planes'.  Returns, on the device: homography float32 [n,L,3,3] in raw-video pixels: (X, Y, Z) = H @ (x, y, 1) of
        a position on the anchor's frame, position on frame f = (X / Z, Y / Z), the identity where there is no fit; label int8 [n,N]:
        -1 not on both frames, r = moves with object r, 127 = labelled for no object or does not move with its own; stats int32 [n,L,4]
        = (points of the object on both frames, inliers, best hypothesis or -1, 1 if the refit fell back); box float32 [n,L,4] = (min
        x, min y, max x, max y) of the object's inliers on frame f in raw-video pixels, max < min where there is no fit."""
        from . import ops
        who = "follow_planes"
        gs, scale = self._running(who)
        if not isinstance(objects, ops.ObjectSet):
            raise ValueError(f"{who}: objects must be an ops.ObjectSet (split_objects, label_objects)")
        first_frame, n = self._newest_frames(gs, n, first_frame, who)
        hom, label, stats, box = self.model.stream_planes(first_frame, n, labels=objects.labels[None], planes=objects.objects,
                                                          anchor=objects.anchor, inverse=inverse, N_out=self.N, scale=scale, thresh=0.6,
                                                          first_row=self._emit_first_row(), tol=tol, hypotheses=hypotheses,
                                                          min_base=min_base, min_points=min_points, seed=seed, group=objects.anchor.group)
        return hom[0], label[0], stats[0], box[0].to(torch.float32) / 16.0

    @torch.no_grad()
    def epipolar(self, n=None, first_frame=None, lag=8, tol=1.0, hypotheses=512, min_base=16.0, min_points=16, seed=0, mask=None, group=0):
        """Not in the reference: which of the N (+ spare_points) user-visible points of query set `group` are consistent with ONE
        camera moving through a scene with depth between frame f - lag and frame f, on the n frames from first_frame on (default: the
        frames of the window just tracked, as in camera_motion()) -- one launch of ctk_fit_epipolar (ops.StreamGroups.epipolar on the
        stream's own history and logits), without a wait.  camera_motion()'s similarity and follow_planes()' homography call the
        nearer half of a static scene outliers once the camera translates; a fundamental matrix holds for a static point at any
        depth, so what violates it moves by itself.  Each frame scores `hypotheses` seeded eight-point samples with the Sampson bound
        `tol` (raw-video pixels; every sample point at least min_base pixels from the first), refits the best over its inliers and
        once more over the inliers of that; a best sample with fewer than min_points (>= 8) inliers is no fit.  mask: int8 / uint8 /
        bool [N_model] on the device, nonzero = the point may be sampled and refitted on; every point is classified either way.
        ValueError when first_frame - lag is negative or has left the ring (history_frames) or the frames lie beyond what has been
        tracked.  Returns, on the device: fundamental float32 [n,3,3] in raw-video pixels: (X, Y, 1) F (x, y, 1)^T = 0 for a static
        point at (x, y) on frame f - lag and (X, Y) on frame f, all zero where there is no fit; label int8 [n,N]: -1 not on both frames,
        0 violates the matrix (or there is no fit), 1 consistent with it; error float32 [n,N]: the squared Sampson distance in
        pixels^2, -1 without a correspondence or a fit; stats int32 [n,4] = (points that may be fitted on, inliers among them, best
        hypothesis or -1, bit 0 / 1: the first / second refit fell back).  Without parallax -- a planar scene, a camera that only
        turns or stands -- the matrix is not unique and the labels mean "consistent with some camera motion": compare with
        follow_planes().  A point that moves along its own epipolar line is not seen.  One pinhole camera: a real lens is corrected in
        front of the fit -- set `lens` before pushing (ctk_lens_frames), or run ops.lens_points (ctk_lens_points) over tracks made on
        sensor pixels."""
        who = "epipolar"
        gs, scale = self._running(who)
        group = int(group)
        if not 0 <= group < gs.G:
            raise ValueError(f"{who}: group must lie in [0, {gs.G})")
        first_frame, n = self._newest_frames(gs, n, first_frame, who)
        fund, label, error, stats = self.model.stream_epipolar(first_frame, n, mask=None if mask is None else mask[None], lag=lag,
                                                               N_out=self.N, scale=scale, thresh=0.6, first_row=self._emit_first_row(),
                                                               tol=tol, hypotheses=hypotheses, min_base=min_base, min_points=min_points,
                                                               seed=seed, group=group)
        return fund[0], label[0], error[0], stats[0]

    @torch.no_grad()
    def pose(self, intrinsics, n=None, first_frame=None, lag=8, tol=1.0, hypotheses=512, min_base=16.0, min_points=16, seed=0, mask=None,
             group=0):
        """Not in the reference: how the camera turned and in which direction it moved between frame f - lag and frame f, and how
        deep each of the N (+ spare_points) user-visible points of query set `group` is, on the n frames from first_frame on (default:
        the frames of the window just tracked, as in epipolar()) -- the launch of ctk_fit_epipolar and then the launch of ctk_fit_pose
        on its matrix and labels (ops.StreamGroups.epipolar and .pose on the stream's own history and logits): two launches, no wait.
        intrinsics: (fx, fy, cx, cy), four Python floats, one pinhole camera in raw-video pixels (a caller who does not know them:
        calibrate() reads the focal length off the tracks, intrinsics() makes the four floats).  tol, hypotheses, min_base, seed and
        mask are epipolar()'s; min_points holds for both: the matrix needs that many inliers, the pose that many points labelled 1.
        The range errors are epipolar()'s.  Returns, on the device: pose float32 [n,3,4] = (R | t) with X_f = R X_(f - lag) + t in
        camera coordinates and |t| = 1, (I | 0) where there is no fit; depth float32 [n,N,2] = (depth on frame f - lag, depth on frame
        f) in units of that frame's baseline, NaN without a correspondence or a fit; label int8 [n,N], epipolar()'s: a point labelled
        0 moves by itself and its depth means nothing; stats int32 [n,4] = (points fitted on, those of them in front of both cameras,
        the chosen candidate or -1, bit 0 / 1: the first / second refinement round fell back, bit 2: an entry was left out of one).
        The scale is unknown and changes from frame to frame; one pinhole camera without distortion; without parallax -- a camera that
        only turns or stands, a planar scene -- there is no pose: look at stats[:, 1] / stats[:, 0] and compare with follow_planes().
        No bundle adjustment over more than two frames.  A real lens is corrected in front of the fit: set `lens` before
        pushing (ctk_lens_frames), or run ops.lens_points (ctk_lens_points) over tracks made on sensor pixels, and pass lens.ideal."""
        who = "pose"
        gs, scale = self._running(who)
        group = int(group)
        if not 0 <= group < gs.G:
            raise ValueError(f"{who}: group must lie in [0, {gs.G})")
        first_frame, n = self._newest_frames(gs, n, first_frame, who)
        mask = None if mask is None else mask[None]
        source = dict(lag=lag, N_out=self.N, scale=scale, thresh=0.6, first_row=self._emit_first_row(), group=group)
        fund, label, _, _ = self.model.stream_epipolar(first_frame, n, mask=mask, tol=tol, hypotheses=hypotheses, min_base=min_base,
                                                       min_points=min_points, seed=seed, **source)
        pose, depth, stats = self.model.stream_pose(first_frame, n, intrinsics, fund, label, mask=mask, min_points=min_points, **source)
        return pose[0], depth[0], label[0], stats[0]

    @torch.no_grad()
    def calibrate(self, n=None, first_frame=None, lag=8, candidates=64, span=(0.25, 4.0), focals=None, principal=None, tol=1.0,
                  hypotheses=512, min_base=16.0, min_points=16, min_frames=1, contrast=1.5, seed=0, mask=None, group=0, state=None):
        """Not in the reference: the focal length of the camera, for a caller who does not know the intrinsics pose() and everything
        behind it ask for, read off the tracks of query set `group` on the n frames from first_frame on (default: the frames of the
        window just tracked, as in epipolar()) -- the launch of ctk_fit_epipolar and then the two launches of ctk_fit_focal on its
        matrices and labels (ops.StreamGroups.epipolar and .focal on the stream's own history and logits): three launches, no wait.
        Each frame f is paired with frame f - lag; `candidates` focal lengths geometric over span * W of the raw video (or `focals`:
        ascending host numbers, or a float32 device tensor) are swept through pose()'s rules, each pair scores each candidate in
        pixels, and the scores are summed.  principal: (cx, cy) in raw-video pixels, assumed, not estimated; None: the picture centre
        ((W - 1) / 2, (H - 1) / 2), or with `lens` set the principal point of lens.ideal -- the calibration is then of lens.ideal's
        picture, the one the stream tracks.  tol, hypotheses, min_base, seed and mask are epipolar()'s; min_points holds for both.
        state: what an earlier call returned: its curve is added to, so that evidence accumulates over windows (its candidates and
        principal point are used again; candidates, span, focals and principal are then not looked at).  The range errors are
        epipolar()'s.  Returns (focal, state): focal a float32 device scalar, 0 where there is no fit yet -- fewer than min_frames
        pairs took part, or the curve's largest total is below `contrast` times its smallest: the camera has not TURNED between the
        frames of the pairs (under a pure translation every focal length explains the matrices equally well) --; state = (curve int64
        [K+2] on the device, focals float32 [K] on the device, principal).  intrinsics(focal, state[2]) makes the four floats.  Known
        limits: square pixels, an assumed principal point, a camera that must turn, ONE fixed focal length per accumulation (start a
        new state after a zoom), no distortion estimate, no second finer sweep, no bundle adjustment."""
        who = "calibrate"
        gs, scale = self._running(who)
        group = int(group)
        if not 0 <= group < gs.G:
            raise ValueError(f"{who}: group must lie in [0, {gs.G})")
        first_frame, n = self._newest_frames(gs, n, first_frame, who)
        curve = None
        if state is not None:
            if not (isinstance(state, tuple) and len(state) == 3 and isinstance(state[0], torch.Tensor) and isinstance(state[1], torch.Tensor)):
                raise ValueError(f"{who}: state must be what an earlier calibrate() returned: (curve, focals, principal)")
            curve, focals, principal = state[0][None], state[1], state[2]
        elif principal is None:
            H, W = self._hw
            principal = ((W - 1) * 0.5, (H - 1) * 0.5) if self._lens is None else tuple(float(v) for v in self._lens.ideal[2:4])
        principal = (float(principal[0]), float(principal[1]))
        mask = None if mask is None else mask[None]
        source = dict(lag=lag, N_out=self.N, scale=scale, thresh=0.6, first_row=self._emit_first_row(), group=group)
        fund, label, _, _ = self.model.stream_epipolar(first_frame, n, mask=mask, tol=tol, hypotheses=hypotheses, min_base=min_base,
                                                       min_points=min_points, seed=seed, **source)
        focal, curve, _, _, focals = self.model.stream_focal(first_frame, n, fund, label, focals=focals, size=self._hw, candidates=candidates,
                                                             span=span, principal=principal, mask=mask, tol=tol, min_points=min_points,
                                                             min_frames=min_frames, contrast=contrast, curve=curve, **source)
        return focal[0], (curve[0], focals, principal)

    def intrinsics(self, focal, principal=None):
        """Not in the reference: (f, f, cx, cy) as four Python floats -- what pose(), reconstruct(), localize() and extend() take --
        from calibrate()'s focal length.  THE one device-to-host copy of the calibration: it waits for the stream's work up to the
        calibrate() call.  principal: (cx, cy), or calibrate()'s state (its principal point is used), or None: the picture centre, or
        with `lens` set the principal point of lens.ideal (calibrate()'s own default).  ValueError when focal is 0: there is no fit
        yet -- the camera has not turned between the paired frames, or too few frames took part; push more frames and pass the
        state on."""
        who = "intrinsics"
        if isinstance(principal, tuple) and len(principal) == 3 and isinstance(principal[0], torch.Tensor):
            principal = principal[2]
        if principal is None:
            if self._hw is None:
                raise RuntimeError(f"{who}: no stream has been started, so the picture centre is unknown: pass principal")
            H, W = self._hw
            principal = ((W - 1) * 0.5, (H - 1) * 0.5) if self._lens is None else tuple(float(v) for v in self._lens.ideal[2:4])
        f = float(focal.item() if isinstance(focal, torch.Tensor) else focal)  # the one wait
        if not (math.isfinite(f) and f > 0.0):
            raise ValueError(f"{who}: focal is {f}: calibrate() has no fit yet (the camera has not turned between the paired frames, "
                             "or too few frames took part)")
        return (f, f, float(principal[0]), float(principal[1]))

    @torch.no_grad()
    def reconstruct(self, intrinsics, frame=None, lag=8, max_depth=64.0, group=0, tol=1.0, hypotheses=512, min_base=16.0, min_points=16,
                    seed=0, mask=None):
        """Not in the reference: the static points of query set `group` in 3-D, reconstructed ONCE from the pair (frame - lag, frame)
        (default: the newest tracked frame) -- pose() for that one pair (two launches), ops.structure_from_pose (elementwise torch: the
        depth on `frame` times the point's ray) and one pin(frame), without a wait.  intrinsics: (fx, fy, cx, cy), four Python floats,
        one pinhole camera in raw-video pixels (unknown: calibrate() and intrinsics()); tol, hypotheses, min_base, min_points, seed and mask are pose()'s; max_depth (in
        baselines of the pair) drops far points, which carry no parallax: a parameter, not a measured optimum.  ValueError when
        frame - lag is negative or has left the ring (history_frames) or the frame has not been tracked, as split_scene().  Returns an
        ops.Structure: points float32 [N_model,3] on the device in the camera coordinates of `frame`, valid int8 [N_model] (labelled
        static, both depths finite and > 0, no deeper than max_depth), the anchor pinned on `frame`, the intrinsics; localize() takes
        it.  The unit is the baseline of this pair, for as long as the structure is used.  A structure lives as long as enough of its
        points stay tracked: points that replenish() adds later are not in it until extend() puts them there (triangulating new points
        from localised frames and restating the structure on a newer frame; refining what it holds is not built).  One pinhole camera,
        no lens distortion; the structure is never refined (no bundle adjustment); without parallax on the pair (a camera that only turns or stands, a plane) there is no structure: valid is all
        zero.  A real lens is corrected in front of the fit: set `lens` before
        pushing (ctk_lens_frames), or run ops.lens_points (ctk_lens_points) over tracks made on sensor pixels, and pass lens.ideal."""
        from . import ops
        who = "reconstruct"
        gs, scale = self._running(who)
        frame, lag, group = gs.committed - 1 if frame is None else int(frame), int(lag), int(group)
        if not 0 <= group < gs.G:
            raise ValueError(f"{who}: group must lie in [0, {gs.G})")
        if not 0 <= frame < gs.committed or lag < 1 or frame - lag < 0:
            raise ValueError(f"{who}: frames {frame - lag} and {frame} must both have been tracked ({gs.committed} frames), lag >= 1")
        _, depth, label, _ = self.pose(intrinsics, 1, frame, lag=lag, tol=tol, hypotheses=hypotheses, min_base=min_base,
                                       min_points=min_points, seed=seed, mask=mask, group=group)
        anchor = self.pin(frame, group)
        pts, ok = ops.structure_from_pose(anchor.coords[0, :self.N], intrinsics, depth[0], label[0], max_depth=max_depth, scale=scale)
        points = torch.zeros((gs.N, 3), dtype=torch.float32, device=pts.device)
        valid = torch.zeros((gs.N,), dtype=torch.int8, device=pts.device)
        points[:self.N], valid[:self.N] = pts, ok
        return ops.Structure(points, valid, anchor, intrinsics)

    @torch.no_grad()
    def localize(self, structure, n=None, first_frame=None, tol=2.0, hypotheses=256, min_points=16, seed=0, epipolar_tol=1.0,
                 epipolar_hypotheses=512, min_base=16.0):
        """Not in the reference: where the camera is on the n frames from first_frame on (default: the frames of the window just
        tracked, as in pose()) in the ONE unit and the ONE coordinate system of an ops.Structure (reconstruct()) -- every pose of every
        later call can be compared with every other, which pose() alone cannot give (its |t| = 1 on every frame).  THREE launches and
        no wait, each against the structure's anchor, which outlives the ring (history_frames), so nothing is chained and nothing
        drifts: ctk_fit_epipolar with structure.valid as the mask (epipolar_tol, epipolar_hypotheses, min_base and seed are
        epipolar()'s), ctk_fit_pose on its matrix and labels, and ctk_fit_resection with that pose as the seed: its translation is
        rescaled against the structure by `hypotheses` sampled points, the candidate with most points within `tol` pixels of their
        reprojection wins and is refined by three Gauss-Newton rounds on the reprojection error.  min_points holds for all three (the
        first two need at least 8).  Returns, on the device: pose float32 [n,3,4] = (R | t) with X_f = R X_anchor + t in camera
        coordinates, (I | 0) where there is no fit -- and exactly (I | 0) on the structure's own frame; label int8 [n,N]: -1 not on
        both frames or not in the structure, 0 outside tol (a point of the structure that has begun to move), behind the camera or no
        fit, 1 within tol; error float32 [n,N]: the squared reprojection error in px^2, -1 where the label is -1 or there is no fit;
        stats int32 [n,4] = (points fitted on, points labelled 1, the winning candidate or -1, bits 0 / 1 / 4: a refinement round fell
        back, bit 2: an entry was left out, bit 3: more than 4096 points, bit 5: the frame is the structure's own).  The camera's
        position in the structure's coordinates is -R^T t.  The limits are reconstruct()'s: the unit is the baseline of its pair; the
        structure lives as long as enough of its points stay tracked (stats[:, 1] tells), points added later by replenish() are not in
        it until extend() puts them there (triangulating new points from localised frames; when stats[:, 1] falls, extend in time --
        refining the structure is not built); the seed comes from the
        two-view pose, so a frame without parallax against the anchor that is not the anchor itself (a camera that only turned)
        relies on the fixed candidates (R0, 0) and (I, 0) -- there is no minimal P3P solver; one pinhole camera, no lens distortion;
        no bundle adjustment.  ValueError for frames not yet tracked; NotImplementedError on a v2 predictor.  A real lens is corrected in front of the fit: set `lens` before
        pushing (ctk_lens_frames), or run ops.lens_points (ctk_lens_points) over tracks made on sensor pixels, and pass lens.ideal.
        resect() asks the same question without a seed: its candidates come from three points of the structure each."""
        from . import ops
        who = "localize"
        gs, scale = self._running(who)
        if not isinstance(structure, ops.Structure):
            raise ValueError(f"{who}: structure must be an ops.Structure (reconstruct)")
        first_frame, n = self._newest_frames(gs, n, first_frame, who)
        mask, anchor, cam = structure.valid[None], structure.anchor, structure.intrinsics
        source = dict(anchor=anchor, N_out=self.N, scale=scale, thresh=0.6, first_row=self._emit_first_row(), group=anchor.group)
        two_view = max(int(min_points), 8)
        fund, label, _, _ = self.model.stream_epipolar(first_frame, n, mask=mask, tol=epipolar_tol, hypotheses=epipolar_hypotheses,
                                                       min_base=min_base, min_points=two_view, seed=seed, **source)
        seeds, _, _ = self.model.stream_pose(first_frame, n, cam, fund, label, mask=mask, min_points=two_view, **source)
        pose, label, error, stats = self.model.stream_resection(first_frame, n, cam, structure.points[None], mask, seeds, tol=tol,
                                                                hypotheses=hypotheses, min_points=min_points, seed=seed, **source)
        return pose[0], label[0], error[0], stats[0]

    @torch.no_grad()
    def resect(self, structure, n=None, first_frame=None, tol=2.0, hypotheses=256, min_points=16, seed=0):
        """Not in the reference: localize()'s question -- where the camera is on the n frames from first_frame on (default: the frames
        of the window just tracked) in the unit and coordinates of an ops.Structure -- answered from the structure alone, by ONE
        launch against the structure's anchor and no wait: ctk_fit_p3p (include/ctk.h, "fit p3p").  Each of the `hypotheses`
        candidates is the pose that three sampled structure points fix; the one with most points within `tol` pixels of their
        reprojection wins and is refined by localize()'s three Gauss-Newton rounds.  No two-view fit comes first, so it holds where
        localize()'s seed fails: when most points of the structure have begun to move (three clean points a sample instead of
        eight), and on a planar structure.  Returns (pose, label, error, stats) exactly as localize() shapes them -- they go into
        extend(poses=(pose, stats)) and world_pose() as they stand; stats[:, 2] lies in 0 .. hypotheses, the last being (I | 0), the
        pose of the structure's own frame.  Limits: the Newton rounds start at the points' own distances from the structure's
        camera and find the P3P root nearest to them, one root per triple -- measured on camera displacements up to the depth of
        the nearest point; the rest are localize()'s (the unit is the baseline of the structure's pair; the structure lives as long
        as enough of its points stay tracked; one pinhole camera, no lens distortion; no bundle adjustment).  ValueError for frames
        not yet tracked; NotImplementedError on a v2 predictor."""
        from . import ops
        who = "resect"
        gs, scale = self._running(who)
        if not isinstance(structure, ops.Structure):
            raise ValueError(f"{who}: structure must be an ops.Structure (reconstruct)")
        first_frame, n = self._newest_frames(gs, n, first_frame, who)
        anchor = structure.anchor
        pose, label, error, stats = self.model.stream_p3p(
            first_frame, n, structure.intrinsics, structure.points[None], structure.valid[None], tol=tol, hypotheses=hypotheses,
            min_points=min_points, seed=seed, anchor=anchor, N_out=self.N, scale=scale, thresh=0.6, first_row=self._emit_first_row(),
            group=anchor.group)
        return pose[0], label[0], error[0], stats[0]

    @torch.no_grad()
    def align(self, a, b, mask=None, tol=2.0, depth_tol=0.1, hypotheses=256, min_points=8, seed=0):
        """Not in the reference: the similarity that maps ops.Structure `a` onto ops.Structure `b` of the running stream, over the
        slots both hold -- what carries a trajectory over a loss (a new reconstruct() has a unit and a camera of its own), and what
        compares an extended structure with a fresh reconstruction of the same slots.  ONE launch and no wait: ctk_fit_align
        (include/ctk.h, "fit align").  Each of the `hypotheses` candidates is the similarity three sampled common points fix; the one
        with most points within `tol` pixels (in b's camera, b.intrinsics) and `depth_tol` of b's depth wins and is refined by three
        Gauss-Newton rounds.  Nothing of the stream is read, waited for, re-captured or re-allocated.  Returns, on the device: sim
        float32 [3,4] = (s R | t) with X_b = s R X_a + t (all zero: no fit), scale float32 [] = s (0: no fit), label int8 [N_model]:
        1 the two agree, 0 they do not (the point moved between the two, or no fit), -1 not in both; error float32 [N_model]: the
        squared pixel distance (-1: label -1 or no fit); stats int32 [4] = (points fitted on, points labelled 1, the winning
        candidate or -1, bits as ops.fit_align).  ops.merge_structures(a, b, sim, label) makes one structure of the two;
        ops.compose_similarity restates a pose against a.  Limits: one similarity per pair; at least three non-collinear common
        points; no covariance; a degenerate inlier set keeps the candidate's transform (bit 1).  ValueError for structures of
        different slot counts; NotImplementedError on a v2 predictor."""
        from . import ops
        who = "align"
        self._running(who)
        if not (isinstance(a, ops.Structure) and isinstance(b, ops.Structure)):
            raise ValueError(f"{who}: a and b must be ops.Structure (reconstruct, extend)")
        sim, scale, label, error, stats = self.model.stream_align(a.points, a.valid, b.points, b.valid, b.intrinsics, mask=mask, tol=tol,
                                                                  depth_tol=depth_tol, hypotheses=hypotheses, min_points=min_points, seed=seed)
        return sim[0], scale[0], label[0], error[0], stats[0]

    @torch.no_grad()
    def georeference(self, structure, known, slots, intrinsics=None, tol=2.0, depth_tol=0.1, hypotheses=256, min_points=3, seed=0):
        """Not in the reference: an ops.Structure put into a caller's metric frame from a few surveyed points.  known: float32 [M,3],
        the points of the slots `slots` (M integers, distinct, each a slot of the structure) in the metric frame; they are scattered
        into an [N_model,3] buffer with a validity mask (elementwise torch) and align()'s one launch finds X_metric = s R X_structure
        + t: `scale` is metres per structure unit.  No wait.  The tolerance is in the pixels of `intrinsics` (fx, fy, cx, cy), a
        camera of the metric frame that looks along its z axis, so the known points need z > 0 there; a caller without such a camera
        passes None -- the structure's own intrinsics -- and states the known points in the axes of the structure's anchor camera
        (x right, y down, z forward, in metres).  Returns align()'s tuple; ops.apply_similarity(sim, structure.points) are the
        metric points, ops.compose_similarity(pose, sim, scale) the metric pose.  Three known points fix the similarity and leave
        nothing to judge it by: give more where there are more (6 and min_points=4 drop one wrong survey point).  Limits: align()'s."""
        from . import ops
        who = "georeference"
        self._running(who)
        if not isinstance(structure, ops.Structure):
            raise ValueError(f"{who}: structure must be an ops.Structure (reconstruct, extend)")
        pts = structure.points
        slots = torch.as_tensor(slots, dtype=torch.long, device=pts.device).reshape(-1)
        if not (isinstance(known, torch.Tensor) and known.dtype == torch.float32 and tuple(known.shape) == (slots.numel(), 3)):
            raise ValueError(f"{who}: known must be a float32 tensor [{slots.numel()},3], one row per slot")
        metric = torch.zeros_like(pts)
        valid = torch.zeros_like(structure.valid)
        metric[slots], valid[slots] = known.to(pts.device), 1
        cam = structure.intrinsics if intrinsics is None else intrinsics
        sim, scale, label, error, stats = self.model.stream_align(pts, structure.valid, metric, valid, cam, tol=tol, depth_tol=depth_tol,
                                                                  hypotheses=hypotheses, min_points=min_points, seed=seed)
        return sim[0], scale[0], label[0], error[0], stats[0]

    @torch.no_grad()
    def extend(self, structure, frame=None, n=None, first_frame=None, tol=2.0, min_views=3, min_parallax=1.0, refine=False, poses=None,
               **localize_kw):
        """Not in the reference: points added to an ops.Structure, and the structure restated on a newer frame -- the keyframe step
        that lets a trajectory go on after the points it started with have left the picture.  Every user-visible point of the
        structure's query set that is tracked on at least min_views of the n frames from first_frame on (default: the frames of the
        window just tracked; at most 256) becomes a 3-D point in the structure's unit, the old points are carried along, and all of
        them are stated in the camera of `frame` (default: the newest tracked frame; it must lie inside the n frames), on which the
        new anchor is pinned: slots that replenish() filled after the old anchor was taken have real positions on the new one, so
        localize() can fit on them.  FIVE launches and no wait; nothing is re-captured or re-allocated: localize() over the n frames
        (three; tol is its tolerance too, localize_kw are its other options; skipped when poses = (pose, stats) of such a call is
        given), one launch of ctk_fit_structure (include/ctk.h, "fit structure": a linear midpoint start, three Gauss-Newton rounds on
        the reprojection error gated at 4, 2 and 1 x tol pixels, at least min_views views and at least half of the point's
        observations within tol, a parallax of at least min_parallax degrees;
        refine: the old points are triangulated too and an accepted new point wins), and pin(frame).  Returns a new ops.Structure:
        points float32 [N_model,3] in the camera coordinates of `frame`, valid int8 [N_model] (1: carried or newly accepted), the
        anchor pinned on `frame`, the intrinsics, and origin float32 [3,4]: the pose of `frame` against the camera of the first
        structure of the chain, so that world_pose(structure, pose) of every later localize() is in one unit and one world.  When
        `frame` could not be localised there is no structure: valid is all zero, as after a reconstruct() without parallax, and the
        caller keeps the old one.  Limits: a point stays in the structure's fits only while it is visible on the keyframe; poses chain
        once per keyframe, not per frame, and each link carries the error of one localize(); no bundle adjustment -- neither the poses
        nor the carried points are refined; the parallax rule looks at the first counted view against the others only; a frame still
        inside the window being tracked is refined by the next step (pin()'s limit); one pinhole camera, no lens distortion.
        ValueError for frames not yet tracked or a `frame` outside the n frames; NotImplementedError on a v2 predictor.  A real lens is corrected in front of the fit: set `lens` before
        pushing (ctk_lens_frames), or run ops.lens_points (ctk_lens_points) over tracks made on sensor pixels, and pass lens.ideal."""
        from . import ops
        who = "extend"
        gs, scale = self._running(who)
        if not isinstance(structure, ops.Structure):
            raise ValueError(f"{who}: structure must be an ops.Structure (reconstruct)")
        first_frame, n = self._newest_frames(gs, n, first_frame, who)
        frame = gs.committed - 1 if frame is None else int(frame)
        if not first_frame <= frame < first_frame + n:
            raise ValueError(f"{who}: frame {frame} must lie inside the frames [{first_frame}, {first_frame + n}) that are triangulated over")
        if poses is None:
            pose, _, _, stats = self.localize(structure, n, first_frame, tol=tol, **localize_kw)
        else:
            pose, stats = poses
        anchor, cam = structure.anchor, structure.intrinsics
        pts, label, _, _, origin = self.model.stream_structure(
            first_frame, n, cam, pose[None], pose_stats=stats[None], structure=structure.points[None], valid=structure.valid[None],
            source_frame=anchor.frame, origin=None if structure.origin is None else structure.origin[None], into=frame - first_frame,
            N_out=self.N, scale=scale, thresh=0.6, first_row=self._emit_first_row(), tol=tol, min_views=min_views,
            min_parallax=min_parallax, refine=refine, group=anchor.group)
        pinned = self.pin(frame, anchor.group)
        points = torch.zeros((gs.N, 3), dtype=torch.float32, device=pts.device)
        valid = torch.zeros((gs.N,), dtype=torch.int8, device=pts.device)
        points[:self.N], valid[:self.N] = pts[0], (label[0] >= 1).to(torch.int8)
        return ops.Structure(points, valid, pinned, cam, origin[0])

    def world_pose(self, structure, pose):
        """A pose [...,3,4] that localize() gave against `structure` -> the same pose against the camera of the first structure of its
        chain of extend() calls: ops.compose_pose(pose, structure.origin) (elementwise torch, no wait)."""
        from . import ops
        if not isinstance(structure, ops.Structure):
            raise ValueError("world_pose: structure must be an ops.Structure (reconstruct, extend)")
        return ops.compose_pose(pose, structure.origin)

    @torch.no_grad()
    def split_scene(self, frame=None, lag=8, group=0, tol=1.0, hypotheses=512, min_base=16.0, min_points=16, seed=0, mask=None):
        """Not in the reference: the N (+ spare_points) user-visible points of query set `group` split into the static scene and what
        moves by itself between frame - lag and `frame` (default: the newest tracked one), under a camera that may translate through
        a scene with depth -- where split_objects() cuts the static scene into depth layers and calls them objects.  One launch of
        ctk_fit_epipolar (epipolar() has the rules and the limits; tol, hypotheses, min_base, min_points, seed and mask are its),
        elementwise torch and one pin(frame), without a wait.  ValueError when frame - lag is negative or has left the ring
        (history_frames) or the frame has not been tracked.  Returns an ops.ObjectSet with objects = 2: labels int8 [N_model] on the
        device (0 = the static scene, 1 = moves independently, -1 = not seen on both frames, or no user-visible point; all
        correspondences are 1 where no matrix was fitted) and the anchor pinned on `frame`; follow() and follow_planes() take it
        unchanged."""
        from . import ops
        who = "split_scene"
        gs, scale = self._running(who)
        frame, lag, group = gs.committed - 1 if frame is None else int(frame), int(lag), int(group)
        if not 0 <= group < gs.G:
            raise ValueError(f"{who}: group must lie in [0, {gs.G})")
        if not 0 <= frame < gs.committed or lag < 1 or frame - lag < 0:
            raise ValueError(f"{who}: frames {frame - lag} and {frame} must both have been tracked ({gs.committed} frames), lag >= 1")
        label = self.epipolar(1, frame, lag=lag, tol=tol, hypotheses=hypotheses, min_base=min_base, min_points=min_points, seed=seed,
                              mask=mask, group=group)[1][0]
        labels = torch.full((gs.N,), -1, dtype=torch.int8, device=label.device)
        labels[:self.N] = torch.where(label < 0, label, 1 - label)
        return ops.ObjectSet(labels, self.pin(frame, group), 2)

    def _plane_index(self, objects, index, who):
        from . import ops
        if not isinstance(objects, ops.ObjectSet):
            raise ValueError(f"{who}: objects must be an ops.ObjectSet (split_objects, label_objects)")
        index = int(index)
        if not 0 <= index < objects.objects:
            raise ValueError(f"{who}: index must lie in [0, {objects.objects})")
        return index

    @torch.no_grad()
    def overlay(self, frames, picture, corners, objects, index=0, first_frame=None):
        """Not in the reference: a `picture` -- uint8, [h,w,3] or a mask-like [h,w], on the device -- pinned onto the planar object
        `index` of an ops.ObjectSet so that it stays put, drawn IN PLACE onto raw-resolution uint8 frames ([F,H,W,3], [F,3,H,W] or one
        frame; picture j shows frame first_frame + j, default: the newest F tracked frames).  The picture's corner pixels (0, 0),
        (w - 1, 0), (w - 1, h - 1), (0, h - 1) sit at corners [4,2] (host values, raw pixels) on the anchor's frame.  Steps:
        follow_planes(inverse=True); one small device matmul with the constant inverse(ops.quad_matrix), which ops.quad_constant keeps on
        the device per quad (the host solve and the non-blocking upload happen on the first call for a quad only); a zero matrix where a frame
        has no fit, so that it gets nothing; ops.warp_planes(border="keep") -- two launches plus elementwise torch, no wait.  A [h,w]
        picture is drawn into all three channels.  No alpha blending, no anti-aliased edge.  The stream's tracks are untouched.
        Returns the frames."""
        from . import ops
        who = "overlay"
        gs, _ = self._running(who)
        index = self._plane_index(objects, index, who)
        frames, _, one, layout, first_frame = self._raw_frames(frames, None, first_frame, gs, who)
        if not (isinstance(picture, torch.Tensor) and picture.dtype == torch.uint8 and picture.is_cuda and
                (picture.dim() == 2 or (picture.dim() == 3 and picture.shape[2] == 3))):
            raise ValueError(f"{who}: picture must be a uint8 device tensor [h,w,3] or [h,w]")
        layout = layout or "hwc"
        size = tuple(picture.shape[:2])
        quad = ops.quad_constant(corners, size, frames.device, inverse=True)  # (cached: the host solve and the upload happen once per quad)
        pic = picture[..., None].expand(*size, 3) if picture.dim() == 2 else picture
        pic = (pic if layout == "hwc" else pic.permute(2, 0, 1)).contiguous()
        hom, _, stats, _ = self.follow_planes(objects, frames.shape[0], first_frame, inverse=True)
        m = ops.plane_matrices(hom[:, index], stats[:, index], quad, inverse=True)
        ops.warp_planes(pic[None], m, out=frames, border="keep", layout=layout)
        return frames[0] if one else frames

    @torch.no_grad()
    def rectify(self, frames, corners, objects, index=0, size=(256, 256), first_frame=None, border="fill", fill=(0, 0, 0), out=None):
        """Not in the reference: the planar object `index` of an ops.ObjectSet shown upright -- the quad whose corners sit at corners
        [4,2] (host values, raw pixels) on the anchor's frame, resampled from each of the raw-resolution uint8 `frames` (as in overlay())
        into an h x w picture, size = (h, w), through the forward matrices: follow_planes(); one small device matmul with
        ops.quad_matrix; ops.warp_planes -- two launches plus elementwise torch, no wait.  border, fill and out are ops.warp_planes'
        ("fill" or "edge").  A frame without a fit shows the quad where it was on the anchor's frame.  Returns [n,h,w,3] (or [n,3,h,w]
        for planar frames; [h,w,3] for one frame, as overlay() returns one frame for one; a new tensor, or `out`)."""
        from . import ops
        who = "rectify"
        gs, _ = self._running(who)
        index = self._plane_index(objects, index, who)
        frames, out, one, layout, first_frame = self._raw_frames(frames, out, first_frame, gs, who)
        if border not in ops.WARP_BORDERS:
            raise ValueError(f"{who}: border must be one of {sorted(ops.WARP_BORDERS)}, got {border!r}")
        quad = ops.quad_constant(corners, size, frames.device, inverse=False)  # (cached, as in overlay())
        hom, _, stats, _ = self.follow_planes(objects, frames.shape[0], first_frame)
        m = ops.plane_matrices(hom[:, index], stats[:, index], quad, inverse=False)
        res = ops.warp_planes(frames, m, size=size, out=out, border=border, fill=fill, layout=layout or "hwc")
        return res[0] if one else res

    def _mark_rows(self):
        """The row from which each user-visible point carries information, on the device: visibility is False below it, and
        everywhere in an empty slot.  Refreshed from the model's host bookkeeping by add / remove only."""
        occ, first = self.model.stream_occupied, self.model.stream_first_row
        first[~occ] = torch.iinfo(torch.long).max
        self._first_row = first[:, :self.N].to(self.queries.device)

    def _with_spare(self, queries):
        """First step: the query sets followed by spare_points empty slots each (the support grid comes after them)."""
        K = int(self.spare_points)
        if K <= 0:
            return queries
        if self.v2:
            raise NotImplementedError("CoTracker2 takes the queries of a stream at its first step: spare_points on a v2 predictor is "
                                      "not implemented")
        from .ops import EMPTY_FRAME
        G, N = queries.shape[:2]
        self.N = N + K
        self.model.stream_slots = True
        first = torch.zeros(G, N + K, dtype=torch.long)
        first[:, N:] = torch.iinfo(torch.long).max
        self._first_row = first.to(queries.device)
        return torch.cat([queries, queries.new_tensor([EMPTY_FRAME, 0.0, 0.0]).expand(G, K, 3)], dim=1)

    def finish(self):
        """Not in the reference (its stream has no end marker): examine the f16-range check of the LAST chunk, which graph
        streaming defers to the next call (behaviours table).  Raises FloatingPointError like that next call
        would; a no-op for CoTracker2 (unguarded) and when nothing is pending."""
        resolve = getattr(self.model, "_resolve_deferred_range_check", None)
        if resolve is not None:
            resolve()

    @torch.no_grad()
    def forward(self, video_chunk, is_first_step: bool = False, queries: torch.Tensor = None, grid_size: int = 5,
                grid_query_frame: int = 0, add_support_grid=False):
        B, T, C, H, W = video_chunk.shape
        ih, iw = self.interp_shape
        if is_first_step:  # predictor.py:242-274: reset state, remember the queries, no tracking yet
            self.model.init_video_online_processing()
            self._prev_chunk = None
            self._push_reset()
            self._first_row, self._hw = None, (H, W)
            self._newest_frame = None
            if self.grid_seeds not in ("grid", "corners"):
                raise ValueError(f"grid_seeds must be 'grid' or 'corners', got {self.grid_seeds!r}")
            if self.v2:
                if self.history_frames is not None:
                    raise NotImplementedError("CoTracker2 returns the tracks of the whole stream: history_frames on a v2 predictor is "
                                              "not implemented")
            else:
                self.model.stream_history_frames = self.history_frames
            if queries is not None:
                assert queries.shape[2] == 3
                self.N = queries.shape[1]
                queries = queries.clone().float()
                queries[:, :, 1:] *= queries.new_tensor([(iw - 1) / (W - 1), (ih - 1) / (H - 1)])
                queries = self._with_spare(queries)
                if add_support_grid:
                    g = get_points_on_a_grid(self.support_grid_size, self.interp_shape, device=video_chunk.device)
                    g = torch.cat([torch.zeros_like(g[:, :, :1]), g], dim=2)
                    queries = torch.cat([queries, g.expand(queries.shape[0], -1, -1)], dim=1)  # (every query group gets the grid)
                if queries.shape[0] > 1 and B == 1 and not self.v2:
                    # G query sets over the one live stream (model.stream_groups): later calls return tracks [G,T,N,2] and
                    # visibility [G,T,N].  (CoTracker2 streams one query set per video: its model call raises, as before.)
                    self.model.stream_groups = True
            elif grid_size > 0:
                pts = get_points_on_a_grid(grid_size, self.interp_shape, device=video_chunk.device)
                if self.grid_seeds == "corners":
                    if self.v2:
                        raise NotImplementedError("grid_seeds = 'corners' on a v2 predictor is not implemented")
                    if not 0 <= int(grid_query_frame) < T:
                        raise ValueError(f"grid_seeds = 'corners' reads frame grid_query_frame = {grid_query_frame} of the first step's "
                                         f"chunk, which holds {T} frame(s)")
                    frames = F.interpolate(video_chunk[:, int(grid_query_frame)].float(), tuple(self.interp_shape), mode="bilinear",
                                           align_corners=True)
                    pts = corner_grid(frames, grid_size, pts)
                self.N = grid_size ** 2
                queries = self._with_spare(torch.cat([torch.full_like(pts[:, :, :1], float(grid_query_frame)), pts], dim=2))
            self.queries = queries
            return (None, None)

        self._hw = (H, W)
        # streaming feature cache (opt-in, model.online_feature_cache): prove ON THE HOST that this chunk's first T - step frames
        # are the memory of the previous chunk's last T - step frames (a view of the same resident video advanced by `step`
        # frames) and tell the model -- it only ever sees the freshly resized tensor below.  No device work, no wait.
        if getattr(self.model, "online_feature_cache", False):
            from .model import tail_aliases
            prev = getattr(self, "_prev_chunk", None)
            self.model._overlap_hint = bool(tail_aliases(prev, video_chunk, 1, self.step))
            self._prev_chunk = video_chunk  # a reference: keeps the allocation alive until the next call
            try:
                video_chunk._ctk_version = video_chunk._version
            except Exception:
                pass
        v = F.interpolate(video_chunk.reshape(B * T, C, H, W).float(), tuple(self.interp_shape), mode="bilinear",
                          align_corners=True).reshape(B, T, 3, ih, iw)
        self._newest_frame = v[0, T - 1] if B == 1 else None  # (a view of v; the device stream state holds one video)
        if self.v2:  # CoTracker2 returns (tracks, visibility, train_data): no confidence (predictor.py:283-286)
            tracks, vis, _ = self.model(video=v, queries=self.queries, iters=6, is_online=True)
            conf = None
        else:
            with self._quiet():
                tracks, vis, conf, _ = self.model(video=v, queries=self.queries, iters=6, is_online=True)
            if tracks is None:  # the stream runs on a ring (the model decides: history_frames as it stood at the first step)
                return self._emit_result(self.model.stream_window_start, self.model._gstream.committed)
        return self._user_result(tracks, vis, conf, add_support_grid)

    def _user_result(self, tracks, vis, conf, add_support_grid):
        """What a step hands back: the user-visible points, visibility thresholded, tracks in pixels of the raw video."""
        (H, W), (ih, iw) = self._hw, self.interp_shape
        if add_support_grid:
            tracks, vis = tracks[:, :, :self.N], vis[:, :, :self.N]
            conf = conf[:, :, :self.N] if conf is not None else None
        if conf is not None:
            vis = vis * conf  # predictor.py:297-298
        vis = vis > 0.6
        if self._first_row is not None:  # spare_points: nothing is visible in an empty slot, nor before a slot's occupant arrived
            vis = vis & (torch.arange(vis.shape[1], device=vis.device)[None, :, None] >= self._first_row[:, None, :])
        return tracks * tracks.new_tensor([(W - 1) / (iw - 1), (H - 1) / (ih - 1)]), vis

    # -- live stream: push new frames, every frame resized, encoded and pooled once -------------------------------------------
    def _push_reset(self):
        self._push_fill = 0         # frames waiting in the buffer
        self._push_tracked = False  # the first window of this stream has run
        self._push_closed = False   # final=True has ended the stream

    def _ingest(self, src, dst, layout):
        from . import ops
        ops.ingest_frames(src, dst, layout=layout)

    @torch.no_grad()
    def push_frames(self, frames, final: bool = False, layout: str = None, add_support_grid=False):
        """Feed a live stream its NEW frames only, as a camera or a decoder delivers them; not in the reference, whose forward wants
        a float chunk that holds the previous call's last `step` frames again (online_demo.py:54-62 restacks and converts them on
        every step).  Call it after the unchanged first step, ``forward(chunk, is_first_step=True, queries=...)``, which only reads
        the chunk's shape and device: a one-frame dummy [1,1,3,H,W] of the right H, W on the right device does.

        frames: uint8 or float32, channels-last [n,H,W,3] or planar [n,3,H,W], or ONE frame [H,W,3] / [3,H,W]; `layout` ("hwc" /
        "chw") settles the corner where both readings fit (H == 3 or W == 3).  On the device, or on the host: a host tensor is
        uploaded as it is -- uint8 stays uint8 -- with one copy.  Any number of frames per call: they are resized on arrival by one
        launch (ops.ingest_frames: the values of forward's F.interpolate) straight into a resident [window_len,3,ih,iw] float32
        buffer, allocated once per stream shape; nothing of the raw frames is kept.  Whenever the buffer holds what the next window
        needs -- window_len frames for the first one, `step` for every later one -- one model.stream_push runs: the k-th tracking
        step happens as soon as frames < k*step + window_len have arrived, whatever the partition, and returns what the k-th tracked
        forward call returns for the chunk of those frames, while every frame is encoded and pooled once.  A push that completes
        several windows runs them all and returns the last result; one that completes none returns (None, None).

        final=True: the stream ends with this push; 1 .. step-1 leftover frames (or fewer than window_len when no window has run:
        a video shorter than one window) are tracked as the short closing chunk.  After it push_frames raises until the next first
        step.  add_support_grid: as in forward, pass what the first step was given.  Returns (tracks, visibility) shaped, scaled
        and thresholded as forward returns them; add_queries / remove_queries work between two pushes.  One stream is fed one way:
        forward on a pushed stream raises (model.stream_push)."""
        if self.v2:
            raise NotImplementedError("CoTracker2 streams are fed overlapping chunks through forward(): push_frames on a v2 predictor "
                                      "is not implemented")
        if self._hw is None or getattr(self, "queries", None) is None:
            raise RuntimeError("push_frames: run the first step first: forward(chunk, is_first_step=True, queries=...)")
        if self._push_closed:
            raise RuntimeError("push_frames: final=True has ended this stream; start the next one with a first step")
        if not isinstance(frames, torch.Tensor) or frames.dtype not in (torch.uint8, torch.float32) or frames.dim() not in (3, 4):
            raise ValueError("push_frames: frames must be a uint8 or float32 tensor [n,H,W,3], [n,3,H,W], [H,W,3] or [3,H,W]")
        if self._lens is not None and frames.dtype != torch.uint8:
            raise ValueError("push_frames: with a lens set the frames must be uint8 (ops.lens_frames resamples uint8 pictures)")
        if frames.dim() == 3:
            frames = frames[None]
        H, W = self._hw
        hwc, chw = tuple(frames.shape[1:]) == (H, W, 3), tuple(frames.shape[1:]) == (3, H, W)
        if layout is None and hwc and chw:
            raise ValueError(f"push_frames: {tuple(frames.shape)} frames read both ways: pass layout='hwc' or 'chw'")
        layout = layout or ("hwc" if hwc else "chw")
        if layout not in ("hwc", "chw") or not (hwc if layout == "hwc" else chw):
            raise ValueError(f"push_frames: expected {H} x {W} frames, [n,{H},{W},3] or [n,3,{H},{W}]; got {tuple(frames.shape)}"
                             + (f" for layout {layout!r}" if layout else ""))
        dev = self.queries.device
        if frames.device != dev:
            frames = frames.to(dev, non_blocking=True)  # the one copy; uint8 stays uint8
        if self._lens is not None:
            frames = self._undistorted(frames, layout)
        S, step = self.model.window_len, self.step
        ih, iw = self.interp_shape
        buf = self._push_buf
        if buf is None or tuple(buf.shape) != (S, 3, ih, iw) or buf.device != dev:
            buf = self._push_buf = torch.empty(S, 3, ih, iw, device=dev, dtype=torch.float32)
        out, i, n = None, 0, frames.shape[0]
        while i < n:
            need = step if self._push_tracked else S
            k = min(n - i, need - self._push_fill)
            self._ingest(frames[i:i + k], buf[self._push_fill:self._push_fill + k], layout)
            i, self._push_fill = i + k, self._push_fill + k
            if self._push_fill == need:
                out = self._push_step(buf[:need], False)
        if final:
            if self._push_fill > 0:
                out = self._push_step(buf[:self._push_fill], True)
            self._push_closed = True
        if out is None:
            return (None, None)
        if out[0] is None:  # history_frames: the last window's rows, out of the ring
            return self._emit_result(self.model.stream_window_start, self.model._gstream.committed)
        return self._user_result(*out, add_support_grid)

    def _undistorted(self, frames, layout):
        """push_frames with a lens: the arriving sensor frames as the pinhole pictures of lens.ideal at raw resolution, one launch, in a
        scratch buffer that is allocated once per stream shape (and grows only with a longer push)."""
        from . import ops
        n, buf = frames.shape[0], self._lens_buf
        if buf is None or buf.device != frames.device or tuple(buf.shape[1:]) != tuple(frames.shape[1:]) or buf.shape[0] < n:
            buf = self._lens_buf = torch.empty(tuple(frames.shape), dtype=torch.uint8, device=frames.device)
        return ops.lens_frames(frames, self._lens, to="ideal", size=self._hw, out=buf[:n], layout=layout)

    def _push_step(self, new_frames, final):
        with self._quiet():  # (a ring stream: the result is emitted by push_frames, one launch for the user points)
            tracks, vis, conf, _ = self.model.stream_push(new_frames, self.queries, iters=6, final=final)
        self._push_fill, self._push_tracked = 0, True
        self._newest_frame = None if final else new_frames[new_frames.shape[0] - 1]  # (a view of the push buffer)
        return tracks, vis, conf
