#!/usr/bin/env python
"""Joint batch mode against the loop over the videos, measured like a bench.py line but OUTSIDE bench.py (whose headline, gates and
extra lines stay as they are):

    python tools/bench_batch.py [--workload c4_online_b4|c2_offline_b8|all] [--steps 12] [--warmup 3] [--precision f16x3|f32] [--no-profile]

Prints ONE JSON line per workload.  Each workload builds on a bench.py workload (video size, window length, grid, seeded synthetic
weights and pixels) with B videos; `model.batch_mode = "joint"` (ONE window call for the B videos) and the default `"loop"` are timed IN
THE SAME PROCESS, ALTERNATING, after warming both (every shape, and both graph captures), over at least 12 calls each:
  ms_joint, ms_loop, ratio (= ms_joint / ms_loop), spread_joint_ms / spread_loop_ms (mean, median, min, max, std over the calls),
  value_joint / value_loop  -- tracked-point-frames/s of all videos together,
  update_only_joint / _loop -- the call minus resize + CNN encoder (timed apart on the same frames): the update path's own rate,
  kernels_joint, hip_kernels_ms, gemm_fraction, launches_per_call_joint -- the library's HIP-event recorder over one more joint call,
  graph_nodes (streaming), max_abs_diff_joint_vs_loop_px -- per element, the last call's tracks of the two modes.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from bench import WORKLOADS  # noqa: E402  (the base workloads: sizes, window lengths, descriptions)

BATCH_WORKLOADS = {
    # name: (base workload, B, description)
    "c4_online_b4": ("c4_online", 4, "4 live 512x512 streams, N=1024 each, 16-frame chunks advancing 8, one hipGraph per call: joint "
                     "(one graph for the 4 windows) vs loop (4 replays of the single-window graph)"),
    "c2_offline_b8": ("c2_offline", 8, "8 clips 256x256 T=48, N=400 each, cotracker3_offline: joint (one 8-video window call) vs loop"),
}


def update_only(points, frames, sec_per_step, encoder_ms):
    """Throughput of the update path alone: the step minus the resize and the CNN encoder (timed apart on the same frames)."""
    if encoder_ms is None or sec_per_step * 1e3 <= encoder_ms:
        return None
    return {"encoder_and_resize_ms": round(encoder_ms, 2), "update_ms": round(sec_per_step * 1e3 - encoder_ms, 2),
            "value": round(points * frames / (sec_per_step - encoder_ms * 1e-3), 1), "unit": "tracked-point-frames/s",
            "what": "step minus (bilinear resize to the model resolution + CNN encoder + L2 normalisation) of the frames one step "
                    "encodes, those timed alone after the timed steps (2 repetitions after 1 warm-up)"}


def encoder_resize_ms(pred, frames):
    """ms of the predictor's resize + the model's encoder for `frames` [F,3,H,W] (what one step spends before the update path)."""
    import torch.nn.functional as F
    model = pred.model
    if not hasattr(model, "_encode"):
        return None

    def once():
        v = F.interpolate(frames.float(), tuple(pred.interp_shape), mode="bilinear", align_corners=True)
        return model._encode(v, 200)

    try:
        once()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            once()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / 2 * 1e3
    except Exception:  # a reported split, never a reason to lose the bench line
        return None


def batch_line(name, dev, precision="f16x3", steps=12, warmup=3, profile=True):
    """`name` of BATCH_WORKLOADS: the joint call and the loop timed IN THE SAME PROCESS, ALTERNATING (joint, loop, joint, ...)
    after warming both (every shape, and both graph captures), every call bracketed by a device synchronisation so that the
    spread of both is known.  ratio = ms_joint / ms_loop (< 1: the joint call is faster)."""
    import numpy as np
    from cotracker_amd import model as M
    from cotracker_amd import ops
    from cotracker_amd.predictor import CoTrackerOnlinePredictor, CoTrackerPredictor
    from cotracker_amd.synthetic import synthetic_video
    from cotracker_amd.weights import fill_synthetic_
    base, B, desc = BATCH_WORKLOADS[name]
    H, W, T, G, offline, wl, _ = WORKLOADS[base]
    streaming = base == "c4_online"
    steps = max(int(steps), 12)
    old, M.DEFAULT_PRECISION = M.DEFAULT_PRECISION, precision
    try:
        def make(mode):
            pr = CoTrackerOnlinePredictor(checkpoint=None, window_len=wl) if streaming else CoTrackerPredictor(
                checkpoint=None, offline=offline, window_len=wl)
            fill_synthetic_(pr.model, seed=0)
            pr = pr.to(dev)
            pr.model.batch_mode = mode
            return pr
        # streaming keeps per-stream state inside the model: one predictor per mode, each advancing its own copy of the streams
        preds = {"joint": make("joint"), "loop": make("loop")}
    finally:
        M.DEFAULT_PRECISION = old
    calls = steps + warmup + 1  # + the profiled call
    if streaming:
        T = preds["joint"].step * (calls + 2)
    video = torch.cat([synthetic_video(T, H, W, seed=1234 + b) for b in range(B)]).to(dev)
    cur = {"joint": 0, "loop": 0}
    if streaming:
        for pr in preds.values():
            pr(video_chunk=video[:, :2 * pr.step], is_first_step=True, grid_size=G)
            pr.queries = pr.queries.repeat(B, 1, 1)
        frames = preds["joint"].step

        def call(mode):
            pr, i = preds[mode], cur[mode]
            cur[mode] += pr.step
            return pr(video_chunk=video[:, i:i + 2 * pr.step])
    else:
        frames = T

        def call(mode):
            return preds[mode](video, grid_size=G)

    def timed(mode):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call(mode)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(warmup):
        for mode in ("joint", "loop"):
            timed(mode)
    ms, last = {"joint": [], "loop": []}, {}
    for _ in range(steps):
        for mode in ("joint", "loop"):
            dt, last[mode] = timed(mode)
            ms[mode].append(dt)
    for pr in preds.values():
        finish = getattr(pr, "finish", None)
        if finish is not None:
            finish()

    def stats(v):
        a = np.asarray(v)
        return {"mean": round(float(a.mean()), 3), "median": round(float(np.median(a)), 3), "min": round(float(a.min()), 3),
                "max": round(float(a.max()), 3), "std": round(float(a.std()), 3), "calls": int(a.size)}

    mj, ml = float(np.mean(ms["joint"])), float(np.mean(ms["loop"]))
    N = G * G
    # both modes saw the same chunks in the same order: per-element difference of the last call's tracks (model-resolution px)
    diff = (last["joint"][0].double() - last["loop"][0].double()).abs().flatten(1).max(dim=1).values
    line = {"workload": name, "description": desc, "precision": precision, "batch": B, "points_per_video": N, "frames_per_call": frames,
            "steps": steps, "warmup": warmup, "protocol": "joint and loop alternate in one process; every call is bracketed by a device "
            "synchronisation", "ms_joint": round(mj, 3), "ms_loop": round(ml, 3), "ratio": round(mj / ml, 4),
            "spread_joint_ms": stats(ms["joint"]), "spread_loop_ms": stats(ms["loop"]),
            "value_joint": round(B * N * frames / (mj * 1e-3), 1), "value_loop": round(B * N * frames / (ml * 1e-3), 1),
            "unit": "tracked-point-frames/s (all videos together)",
            "max_abs_diff_joint_vs_loop_px": [float(x) for x in diff.cpu()],
            "range_fallbacks": int(sum(pr.model.range_fallbacks for pr in preds.values()))}
    enc = encoder_resize_ms(preds["joint"], video[:, :2 * preds["joint"].step if streaming else T].reshape(-1, 3, H, W))
    line["update_only_joint"] = update_only(B * N, frames, mj * 1e-3, enc)
    line["update_only_loop"] = update_only(B * N, frames, ml * 1e-3, enc)
    if streaming:
        line["graph_nodes"] = {k: (next(iter(pr.model._graphs.values())).nodes if pr.model._graphs else 0) for k, pr in preds.items()}
        line["graph_launches_per_call"] = {"joint": 1, "loop": B}
    if profile:
        # one more joint call with the library's HIP-event recorder on (direct launches: events cannot sit inside a graph)
        pj = preds["joint"]
        pj.model.hip_graph = False
        ops.profile_enable(True)
        t1 = time.perf_counter()
        call("joint")
        torch.cuda.synchronize()
        prof_ms = (time.perf_counter() - t1) * 1e3
        rows = ops.profile_read()
        ops.profile_enable(False)
        rows.sort(key=lambda r: -r["total_ms"])
        total = sum(r["total_ms"] for r in rows)
        gemm_ms = sum(r["total_ms"] for r in rows if r["name"].startswith("gemm"))
        line["kernels_joint"] = [{"name": r["name"], "launches": r["launches"], "total_ms": round(r["total_ms"], 3),
                                  "avg_us": round(1e3 * r["total_ms"] / max(r["launches"], 1), 1)} for r in rows]
        line["hip_kernels_ms"] = round(total, 2)
        line["launches_per_call_joint"] = int(sum(r["launches"] for r in rows))
        line["gemm_fraction"] = round(gemm_ms / total, 4) if total > 0 else None
        line["profiled_call_ms"] = round(prof_ms, 2)
    del preds, video, last
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=sorted(BATCH_WORKLOADS) + ["all"])
    ap.add_argument("--steps", type=int, default=12, help="timed calls per mode (at least 12)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f32"])
    ap.add_argument("--no-profile", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for name in (sorted(BATCH_WORKLOADS) if args.workload == "all" else [args.workload]):
        line = batch_line(name, dev, precision=args.precision, steps=args.steps, warmup=args.warmup, profile=not args.no_profile)
        line.update({"metric": "tracked-point-frames/sec (B*N*T/s), joint batch mode", "value": line["value_joint"], "n_gpus": 1,
                     "higher_is_better": True})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
