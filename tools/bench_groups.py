#!/usr/bin/env python
"""Query groups over one video against the sequential calls, measured OUTSIDE bench.py (whose headline and gates stay as they are):

    python tools/bench_groups.py [--workload eval_c2|dense_512|all] [--steps 3] [--warmup 1] [--precision f16x3|f32]
                                 [--query-group 16] [--dense-chunks 12] [--out FILE]

Prints ONE JSON line per workload (and appends it to --out).  Two consumers of the query-group call model(video[1], queries[G]):
  eval_c2    EvaluationPredictor(single_point=True) on 32 points of a 256 x 256, T = 48 clip (cotracker3_offline, window 60):
             one model call per point (point + 8x8 local grid + 5x5 global grid = 90 queries) against `query_group` points per call;
  dense_512  CoTrackerPredictor dense mode on a 512 x 512, T = 24 clip (36 chunks of 85 x 85 points): one model call per chunk
             against `dense_chunks_per_call` chunks per call.
Three rows each -- sequential (the attribute at 1), loop_shared (grouped calls, batch_mode "loop": one encoder run per call, the
groups' windows one after the other) and joint_shared (batch_mode "joint": shared-pyramid joint windows) -- timed IN THE SAME
PROCESS, ALTERNATING, after warming all three, every call between two HIP events; ms is the mean over the timed calls.
ratio_* = ms of the row / ms_sequential; max_abs_diff_*_px = the row's tracks against the sequential ones (loop_shared must be 0).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROWS = ("sequential", "loop_shared", "joint_shared")


def eval_c2(dev, group, _chunks):
    from cotracker_amd.build_cotracker import build_cotracker
    from cotracker_amd.evaluation import EvaluationPredictor
    from cotracker_amd.synthetic import synthetic_video
    from cotracker_amd.weights import fill_synthetic_
    H = W = 256
    T, P = 48, 32
    m = build_cotracker(None, offline=True, window_len=60).eval()
    fill_synthetic_(m, seed=0)
    ev = EvaluationPredictor(m.to(dev), single_point=True)
    video = synthetic_video(T, H, W, seed=1234).to(dev)
    g = torch.Generator().manual_seed(7)
    q = torch.rand(1, P, 3, generator=g) * torch.tensor([T - 1.0, W - 1.0, H - 1.0])
    q[..., 0] = q[..., 0].floor()
    q = q.to(dev)

    def call(row):
        ev.query_group = 1 if row == "sequential" else group
        m.batch_mode = "joint" if row == "joint_shared" else "loop"
        return ev(video, q)[0]
    info = {"description": f"single-point evaluation of {P} points, 256x256 T={T}, 90 queries per point, cotracker3_offline",
            "points": P, "frames": T, "queries_per_point": 90, "query_group": group, "model_calls_sequential": P,
            "model_calls_grouped": -(-P // group)}
    return call, m, info


def dense_512(dev, _group, chunks):
    from cotracker_amd.predictor import CoTrackerPredictor
    from cotracker_amd.synthetic import synthetic_video
    from cotracker_amd.weights import fill_synthetic_
    H = W = 512
    T = 24
    p = CoTrackerPredictor(checkpoint=None, offline=True, window_len=60)
    fill_synthetic_(p.model, seed=0)
    p = p.to(dev)
    video = synthetic_video(T, H, W, seed=1234).to(dev)
    n_chunks, per_chunk = p._dense_layout(video)

    def call(row):
        p.dense_chunks_per_call = 1 if row == "sequential" else chunks
        p.model.batch_mode = "joint" if row == "joint_shared" else "loop"
        return p(video)[0]
    info = {"description": f"one dense call, 512x512 T={T}: {n_chunks} chunks of {per_chunk} points, cotracker3_offline",
            "chunks": n_chunks, "points_per_chunk": per_chunk, "frames": T, "dense_chunks_per_call": chunks,
            "model_calls_sequential": n_chunks, "model_calls_grouped": -(-n_chunks // chunks)}
    return call, p.model, info


WORKLOADS = {"eval_c2": eval_c2, "dense_512": dense_512}


def bench_line(name, dev, precision, steps, warmup, group, chunks):
    from cotracker_amd import model as M
    old, M.DEFAULT_PRECISION = M.DEFAULT_PRECISION, precision
    try:
        call, model, info = WORKLOADS[name](dev, group, chunks)
    finally:
        M.DEFAULT_PRECISION = old

    def timed(row):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = call(row)
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    for _ in range(warmup):
        for row in ROWS:
            timed(row)
    ms, last = {r: [] for r in ROWS}, {}
    for _ in range(steps):
        for row in ROWS:
            dt, last[row] = timed(row)
            ms[row].append(dt)
    mean = {r: sum(v) / len(v) for r, v in ms.items()}
    line = {"workload": name, **info, "precision": precision, "steps": steps, "warmup": warmup,
            "protocol": "the three rows alternate in one process; every call lies between two HIP events",
            "range_fallbacks": int(model.range_fallbacks)}
    for r in ROWS:
        line["ms_" + r] = round(mean[r], 2)
        line["calls_ms_" + r] = [round(x, 2) for x in ms[r]]
    for r in ROWS[1:]:
        line["ratio_" + r] = round(mean[r] / mean["sequential"], 4)
        line[f"max_abs_diff_{r}_px"] = float((last[r].double() - last["sequential"].double()).abs().max())
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=sorted(WORKLOADS) + ["all"])
    ap.add_argument("--steps", type=int, default=3, help="timed calls per row")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f32"])
    ap.add_argument("--query-group", type=int, default=16, help="eval_c2: evaluated points per model call")
    ap.add_argument("--dense-chunks", type=int, default=12, help="dense_512: chunks per model call")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for name in (sorted(WORKLOADS) if args.workload == "all" else [args.workload]):
        line = bench_line(name, dev, args.precision, max(1, args.steps), max(0, args.warmup), args.query_group, args.dense_chunks)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
