"""Goldens at BASELINE.json scale: the UNMODIFIED reference on CPU fp32 at the real 384x512 model resolution.

Needs a checkout of the reference (facebookresearch/co-tracker):

    COTRACKER_REFERENCE=<checkout> python tests/golden/make_golden_scale.py c2 c4 c3_g40 c3_g80      # any subset, in this order of cost

Workloads are bench.py's (same synthetic video seed 1234, same ``fill_synthetic_(seed=0)`` weights):
  c2      BASELINE configs[1]: CoTrackerPredictor(offline=True, window_len=60), 256x256, T=48, grid 20 (N=400)
  c4      BASELINE configs[3]: CoTrackerOnlinePredictor(window_len=16), 512x512, grid 32 (N=1024), 5 chunk calls (T=48)
  c3_g40  BASELINE configs[2] video (512x512, T=120), CoTrackerPredictor(offline=False, window_len=16), grid 40 (N=1600)
  c3_g80  BASELINE configs[2] exactly: grid 80 (N=6400), 14 windows x 6 iterations, jointly tracked
  v2_c2   SURVEY 8f-3: CoTrackerPredictor(v2=True, window_len=8) (hub recipe cotracker2), 512x512, T=48, grid 20, 6 iterations,
          damped feedback (cotracker_amd.weights.V2_DAMP; conf_logit duplicates vis_logit: CoTracker2 has no confidence head)
Stored per workload (OUTPUTS ONLY -- inputs and weights are regenerated from seeds on both sides):
  coords  [T,N,2]  model-level tracks in model-resolution pixels (model.forward()[0])
  vis_logit / conf_logit [T,N]  PRE-sigmoid (the argument of the reference's own torch.sigmoid call, captured by wrapping
          torch.sigmoid while the reference runs; the reference source is not touched)
  tracks  [T,N,2] / vis [T,N] bool   predictor-level outputs (raw-video pixels, thresholded visibility)
  noise_* the same run with a different intra-op thread count (the reference's own reduction-order noise floor):
          max |a-b| over coords (px) / logits, plus its 99.9th percentile
  threads, noise_threads, seconds, torch version.
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ["COTRACKER_REFERENCE"])  # a checkout of facebookresearch/co-tracker

from cotracker.predictor import CoTrackerPredictor, CoTrackerOnlinePredictor  # noqa: E402

from cotracker_amd.weights import fill_synthetic_, fill_synthetic_v2_damped_  # noqa: E402
from cotracker_amd.synthetic import synthetic_video  # noqa: E402

CONFIGS = {
    # name: (H, W, T, grid, kind, window_len, threads, noise_threads)
    "c2": (256, 256, 48, 20, "offline", 60, 8, 1),
    "c4": (512, 512, 48, 32, "online", 16, 8, 3),
    "c3_g40": (512, 512, 120, 40, "sliding", 16, 8, 3),
    "c3_g80": (512, 512, 120, 80, "sliding", 16, 8, 5),
    # explicit queries at RANDOM frames (grid = sqrt of the point count): exercises, at the real resolution, the paths the
    # frame-0 grids never touch -- support masked until a track's query frame enters the window, per-window carry-over of
    # only the already-queried tracks, the 6x6 support grid the predictor appends, backward tracking (a second, time-flipped
    # model pass merged for the frames before each query)
    "c3_q": (512, 512, 64, 32, "queries", 16, 8, 3),
    # round 3: the BASELINE configs that were benchmarked without a reference golden
    # configs[0] stand-in: assets/apple.mp4 is 1296x720, 50 frames, but no video decoder exists offline -> a synthetic video of
    # exactly that size through hubconf's cotracker3_offline recipe (CoTrackerPredictor(offline=True, window_len=60)), grid 10
    "c1": (720, 1296, 50, 10, "offline", 60, 8, 1),
    # configs[2] video as ONE offline window of 120 frames (cotracker3_offline.py:139-216), N=1600
    "c3_off": (512, 512, 120, 40, "offline", 60, 8, 3),
    # configs[4], the per-GPU unit of work: chunk 0 (8 779 points) of the 265x265 quasi-dense grid, explicit queries at
    # frame 0, sliding windows (bench.py --workload c5_shard, rank 0); every 4th point is stored
    "c5_chunk0": (512, 512, 120, 265, "chunk0", 16, 8, 5),
    # round 4: CoTracker2 at BASELINE scale -- hub recipe cotracker2 (CoTrackerPredictor(v2=True, window_len=8)),
    # the reference's default 6 iterations per window, 11 sliding windows.  With xavier-random weights the CoTracker2 map
    # (coordinates AND track features fed back through 6 + 6 transformer layers) is chaotic: the reference itself moves
    # 0.76 px / 0.75 logit between 8 and 3 CPU threads at the CoTracker3 head scale, 0.08 px with heads x0.25, and damping the
    # feature path or the residual branches does not help (heads x0.25, updater x0 : still 0.06 px) -- the coordinate feedback
    # drives it.  cotracker_amd.weights.V2_DAMP (flow-head scale 0.02 instead of 8, track_feat_updater x0.1) makes six iterations reproducible
    # (8 vs 3 threads: ~1e-4 px) while every stage still runs on non-trivial data (tracks move up to ~3 px per window).
    "v2_c2": (512, 512, 48, 20, "v2", 8, 8, 3),
}
STORE_EVERY = {"c3_g80": 4, "c5_chunk0": 4}  # jointly tracked, every k-th point stored (fixture size)


def c5_chunk0_queries(H, W, G, interp_shape=(384, 512)):
    """bench.py's c5_shard queries of rank 0, computed on the CPU with the REFERENCE's grid helper."""
    from cotracker.models.core.model_utils import get_points_on_a_grid
    from cotracker_amd.sharding import chunk_bounds
    ih, iw = interp_shape
    to_raw = torch.tensor([(W - 1) / (iw - 1), (H - 1) / (ih - 1)])
    pts = get_points_on_a_grid(G, (ih, iw)) * to_raw
    q_all = torch.cat([torch.zeros_like(pts[:, :, :1]), pts], dim=2)
    lo, hi = chunk_bounds(G * G, 8, 0)
    return q_all[:, lo:hi].contiguous()


class SigmoidTap:
    """Records the arguments of torch.sigmoid while active (the reference applies it to the final logits:
    cotracker3_online.py:524-525, cotracker3_offline.py:215-216)."""

    def __enter__(self):
        self.args = []
        self.orig = torch.sigmoid

        def tapped(x):
            self.args.append(x.detach().clone())
            return self.orig(x)

        torch.sigmoid = tapped
        return self

    def __exit__(self, *a):
        torch.sigmoid = self.orig


@torch.no_grad()
def run(name, threads):
    H, W, T, G, kind, wl, _, _ = CONFIGS[name]
    torch.set_num_threads(threads)
    torch.manual_seed(0)
    video = synthetic_video(T, H, W, seed=1234)
    captured = {}
    if kind == "online":
        p = CoTrackerOnlinePredictor(checkpoint=None, window_len=wl)
    elif kind == "v2":
        p = CoTrackerPredictor(checkpoint=None, v2=True, window_len=wl)
    else:
        p = CoTrackerPredictor(checkpoint=None, offline=(kind == "offline"), window_len=wl)  # "sliding" / "queries": online weights
    if kind == "v2":
        fill_synthetic_v2_damped_(p.model, seed=0)  # cotracker_amd.weights.V2_DAMP: heads x 0.02 (instead of 8), updater x 0.1
    else:
        fill_synthetic_(p.model, seed=0)
    model_forward = p.model.forward

    def tap_forward(*a, **k):
        out = model_forward(*a, **k)
        captured["coords"] = out[0].detach().clone()
        return out

    p.model.forward = tap_forward
    t0 = time.time()
    with SigmoidTap() as tap:
        if kind == "queries":
            g = torch.Generator().manual_seed(77)
            n = G * G
            q = torch.stack([torch.randint(0, T - 8, (n,), generator=g).float(), torch.rand(n, generator=g) * (W - 1),
                             torch.rand(n, generator=g) * (H - 1)], dim=1)[None]
            q[0, : n // 4, 0] = 0
            tracks, vis = p(video, queries=q, backward_tracking=True)
            captured["coords"] = tracks  # two model passes are merged: the predictor-level tracks are the comparable output
        elif kind == "chunk0":
            q = c5_chunk0_queries(H, W, G)
            captured["queries"] = q
            tracks, vis = p(video, queries=q)
        elif kind == "online":
            p(video_chunk=video[:, :2 * p.step], is_first_step=True, grid_size=G)
            for ind in range(0, T - p.step, p.step):
                tracks, vis = p(video_chunk=video[:, ind: ind + 2 * p.step])
        else:
            tracks, vis = p(video, grid_size=G)
    dt = time.time() - t0
    if kind == "v2":  # CoTracker2 has no confidence head: ONE sigmoid, on the visibility logits (cotracker.py:373); stored twice
        vis_logit = conf_logit = tap.args[-1]
    else:
        vis_logit, conf_logit = tap.args[-2], tap.args[-1]  # the last two sigmoid calls are the returned vis / conf (queries: of the backward pass)
    out = dict(coords=captured["coords"][0], vis_logit=vis_logit[0].reshape(vis_logit.shape[1], -1),
               conf_logit=conf_logit[0].reshape(conf_logit.shape[1], -1), tracks=tracks[0], vis=vis[0])
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["n_points_total"] = np.int64(out["coords"].shape[1])
    if "queries" in captured:
        out["queries"] = captured["queries"][0].numpy()
    print(f"{name}: threads={threads} {dt:.1f} s  {T * out['coords'].shape[1] / dt:.1f} tracked-point-frames/s", flush=True)
    return out, dt


def main():
    for name in sys.argv[1:]:
        _, _, T, G, kind, wl, th, nth = CONFIGS[name]
        a, dt = run(name, th)
        b, dtn = run(name, nth)
        stats = {}
        for k in ("coords", "vis_logit", "conf_logit"):
            d = np.abs(a[k].astype(np.float64) - b[k].astype(np.float64))
            stats[f"noise_{k}_max"] = d.max()
            stats[f"noise_{k}_p999"] = np.quantile(d, 0.999)
            stats[f"noise_{k}_median"] = np.median(d)
        stats["noise_vis_flips"] = int((a["vis"] != b["vis"]).sum())
        print(name, {k: float(v) for k, v in stats.items()}, flush=True)
        every = STORE_EVERY.get(name, 1)
        if every > 1:  # the noise statistics above are over ALL points; the stored outputs are a strided subset
            idx = np.arange(0, a["coords"].shape[1], every, dtype=np.int32)
            stats["vis_true_count"] = int(a["vis"].sum())
            stats["point_index"] = idx
            for k in ("coords", "vis_logit", "conf_logit"):
                a[k] = a[k][:, idx]
            a.pop("tracks"), a.pop("vis")
        path = os.path.join(HERE, f"scale_{name}.npz")
        np.savez_compressed(path, **a, **stats, threads=th, noise_threads=nth, seconds=dt, noise_seconds=dtn,
                            host_cpus=os.cpu_count(),
                            meta=np.array(f"torch {torch.__version__}; facebookresearch/co-tracker@2025-03-04; "
                                          f"{kind} window_len={wl} grid={G} T={T}"))
        print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB", flush=True)


if __name__ == "__main__":
    main()
