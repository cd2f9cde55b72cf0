#!/usr/bin/env python
"""The joint streaming call of tools/bench_batch.py's c4_online_b4 (B live 512x512 streams, N = 1024 each, one hipGraph per call) ALONE, a few
calls after the warm-up, for a kernel trace: under the profiler every launch of a call is one row, so one launch per Linear for
all B videos shows as calls / (timed calls) in the stats.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/trace_joint_stream.py [--batch 4] [--calls 3] [--mode joint|loop]
    python tools/summarize_rocprof.py OUT profiles/<summary>.txt
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--mode", default="joint", choices=["joint", "loop"])
    ap.add_argument("--no-graph", action="store_true")
    args = ap.parse_args()
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    from cotracker_amd.synthetic import synthetic_video
    from cotracker_amd.weights import fill_synthetic_
    dev = torch.device("cuda:0")
    pred = CoTrackerOnlinePredictor(checkpoint=None, window_len=16)
    fill_synthetic_(pred.model, seed=0)
    pred = pred.to(dev)
    pred.model.batch_mode = args.mode
    pred.model.hip_graph = not args.no_graph
    T = pred.step * (args.calls + 3)
    video = torch.cat([synthetic_video(T, 512, 512, seed=1234 + b) for b in range(args.batch)]).to(dev)
    pred(video_chunk=video[:, :2 * pred.step], is_first_step=True, grid_size=32)
    pred.queries = pred.queries.repeat(args.batch, 1, 1)
    for i in range(args.calls + 1):  # the first call captures the graph
        tracks, vis = pred(video_chunk=video[:, i * pred.step:(i + 2) * pred.step])
    pred.finish()
    torch.cuda.synchronize()
    print(f"{args.mode}: {args.calls + 1} calls of {args.batch} streams, tracks {tuple(tracks.shape)}, finite {bool(torch.isfinite(tracks).all())}")


if __name__ == "__main__":
    main()
