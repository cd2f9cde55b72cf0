#!/usr/bin/env python
"""Pushing new frames into a live stream (CoTrackerOnlinePredictor.push_frames), measured OUTSIDE bench.py with the conventions of
bench_stream_slots.py:

    python tools/bench_stream_push.py [--passes 3] [--calls 6] [--precision f16x3|f32] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_stream_push.py --trace ROW --calls K
    python tools/bench_stream_push.py --trace-summary OUT_A OUT_B --calls K_A K_B --row ROW [--out FILE]

The C4 shape on the online predictor (window 16, 1024 points, iters 6, window graph on), ONE query set:
  chunks        forward fed float chunks that are views of a resident 384 x 512 video, feature cache off;
  chunks_cache  the same with model.online_feature_cache, where the alias proof holds;
  push_f32      push_frames fed model-resolution float frames, eight per call (sixteen for the first window);
  chunks_1080   forward fed float [1,16,3,1080,1920] chunks copied from a uint8 channels-last ring -- what a live source has to do
                today (the copy and the conversion are inside the timed call);
  push_u8_1080  push_frames fed the ring's uint8 [8,1080,1920,3] frames as they are.
The rows run IN ONE PROCESS, ALTERNATING pass by pass; every call lies between two HIP events; ms_* is the median over the calls
after the first two windows of every pass.

--trace runs ONE row alone for a kernel trace (no counters in that run); --trace-summary takes two such traces of K_A < K_B calls:
kernels per steady-state call by name, minus the kernel nodes of the window graph the row replays = the launches OUTSIDE the window
graph per call, and the median duration of the ingest launch.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

from bench_stream_groups import HW, NoTimer, S, Timer, graph_nodes, grid, kernel_rows, lib_sha, short  # noqa: E402

ROWS = ("chunks", "chunks_cache", "push_f32", "chunks_1080", "push_u8_1080")
STEP = S // 2
BIG = (1080, 1920)
RING = S + 5 * STEP  # frames resident per source, walked round


def setup(dev, precision):
    from cotracker_amd import model as M
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    from cotracker_amd.synthetic import synthetic_video
    from cotracker_amd.weights import fill_synthetic_
    old, M.DEFAULT_PRECISION = M.DEFAULT_PRECISION, precision
    try:
        p = CoTrackerOnlinePredictor(checkpoint=None, window_len=S)
    finally:
        M.DEFAULT_PRECISION = old
    assert tuple(p.interp_shape) == HW
    fill_synthetic_(p.model, seed=0)
    p = p.to(dev)
    small = synthetic_video(RING, *HW, seed=1234).to(dev)  # [1,T,3,384,512] float, 0..255
    g = torch.Generator().manual_seed(7)
    big = torch.randint(0, 256, (RING, *BIG, 3), dtype=torch.uint8, generator=g).to(dev)  # the uint8 ring of a decoder
    return p, small, big


def make_rows(p, small, big, dev):
    """One predictor per row (a row keeps its stream state, its buffers and its graph between passes)."""
    import copy
    preds = {}

    def stream(row, calls, on_call):
        if row not in preds:
            preds[row] = copy.deepcopy(p)
            preds[row].model.online_feature_cache = row == "chunks_cache"
        x = preds[row]
        is_big = row.endswith("1080")
        H, W = BIG if is_big else HW
        q = grid(32, 0.0)[None].to(dev)
        q[..., 1:] *= q.new_tensor([(W - 1) / (HW[1] - 1), (H - 1) / (HW[0] - 1)])
        x(torch.zeros(1, 1, 3, H, W, device=dev), is_first_step=True, queries=q)
        out = None
        for i in range(calls):
            t0 = (i % 6) * STEP
            with on_call(i):
                if row in ("chunks", "chunks_cache"):
                    out = x(small[:, t0:t0 + S])[0]
                elif row == "chunks_1080":
                    out = x(big[t0:t0 + S].permute(0, 3, 1, 2).float()[None])[0]
                elif row == "push_f32":
                    out = x.push_frames(small[0, t0:t0 + S] if i == 0 else small[0, t0 + S - STEP:t0 + S])[0]
                else:
                    out = x.push_frames(big[t0:t0 + S] if i == 0 else big[t0 + S - STEP:t0 + S])[0]
        x.finish()
        return out
    stream.preds = preds
    return stream


def bench_line(dev, precision, passes, calls):
    p, small, big = setup(dev, precision)
    stream = make_rows(p, small, big, dev)
    for row in ROWS:  # warm every row: weights packed, graphs captured
        stream(row, 3, NoTimer())
    ms, last = {r: [] for r in ROWS}, {}
    for _ in range(passes):
        for row in ROWS:
            last[row] = stream(row, calls, Timer(ms[row], 2)).clone()
    med = {r: statistics.median(v) for r, v in ms.items()}
    line = {"workload": "c4_one_set_push", "points": 1024, "frames": list(HW), "raw_frames_1080": list(BIG), "window_len": S, "iters": 6,
            "precision": precision, "hip_graph": True, "passes": passes, "calls_per_pass": calls, "timed_calls_per_row": len(ms["chunks"]),
            "protocol": "rows alternate pass by pass in one process; every call between two HIP events; median over the calls after "
                        "the first two windows of each pass",
            "libctk_sha256": lib_sha()}
    for r in ROWS:
        line["ms_" + r] = round(med[r], 3)
        line["min_max_ms_" + r] = [round(min(ms[r]), 3), round(max(ms[r]), 3)]
    line["push_f32_le_chunks_cache_le_chunks"] = bool(med["push_f32"] <= med["chunks_cache"] <= med["chunks"])
    line["push_u8_1080_minus_push_f32_ms"] = round(med["push_u8_1080"] - med["push_f32"], 3)
    line["ratio_push_f32_over_chunks"] = round(med["push_f32"] / med["chunks"], 4)
    line["ratio_push_u8_1080_over_chunks_1080"] = round(med["push_u8_1080"] / med["chunks_1080"], 4)
    # same frames, same queries: the pushed stream against the chunk stream on the torch glue (bit-identical to the device state)
    line["push_f32_equals_chunks_bit_for_bit"] = bool(torch.equal(last["push_f32"], last["chunks"]))
    line["push_u8_1080_equals_chunks_1080_bit_for_bit"] = bool(torch.equal(last["push_u8_1080"], last["chunks_1080"]))
    line["range_fallbacks"] = int(sum(x.model.range_fallbacks for x in stream.preds.values()))
    torch.cuda.empty_cache()
    return line


def trace_run(dev, precision, row, calls):
    p, small, big = setup(dev, precision)
    out = make_rows(p, small, big, dev)(row, calls, NoTimer())
    torch.cuda.synchronize()
    print(json.dumps({"trace": row, "calls": calls, "finite": bool(torch.isfinite(out).all())}))


def kernel_us(d, pattern):
    """Durations (us) of the launches whose bare kernel name contains `pattern`, from a rocprofv3 kernel trace."""
    out = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if pattern in short(r["Kernel_Name"]):
                    out.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return out


def trace_summary(dev, precision, row, dirs, calls):
    (da, db), (ka, kb) = dirs, calls
    a, b = kernel_rows(da), kernel_rows(db)
    per_call = {n: (b.get(n, 0) - a.get(n, 0)) / (kb - ka) for n in sorted(set(a) | set(b))}
    per_call = {n: v for n, v in per_call.items() if v}
    p, small, big = setup(dev, precision)  # the kernel nodes the row replays per call: the graph a short run leaves behind
    stream = make_rows(p, small, big, dev)
    stream(row, 2, NoTimer())
    nodes = graph_nodes(stream.preds[row].model)
    total = sum(per_call.values())
    ingest = sorted(kernel_us(db, "ingest_kernel"))
    line = {"trace_summary": row, "workload": "c4_one_set_push", "calls": [ka, kb], "kernels_per_call": round(total, 2),
            "graph_kernel_nodes_per_call": nodes, "launches_outside_graph_per_call": round(total - nodes, 2),
            "libctk_sha256": lib_sha(), "kernels_per_call_by_name": {n: round(v, 2) for n, v in per_call.items()}}
    if ingest:  # (the first window's launch takes 16 frames: the median is a steady 8-frame launch)
        line["ingest_launches"], line["ingest_us_median"], line["ingest_us_min_max"] = len(ingest), round(statistics.median(ingest), 2), \
            [round(ingest[0], 2), round(ingest[-1], 2)]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3, help="stream passes per row")
    ap.add_argument("--calls", type=int, nargs="+", default=[6], help="calls per pass (two values with --trace-summary)")
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f32"])
    ap.add_argument("--trace", default=None, choices=ROWS, help="run this row alone, for rocprofv3 --kernel-trace")
    ap.add_argument("--trace-summary", nargs=2, default=None, metavar=("OUT_A", "OUT_B"))
    ap.add_argument("--row", default="push_u8_1080", choices=ROWS)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.trace:
        trace_run(dev, args.precision, args.trace, args.calls[0])
        return
    if args.trace_summary:
        line = trace_summary(dev, args.precision, args.row, args.trace_summary, args.calls)
    else:
        line = bench_line(dev, args.precision, max(1, args.passes), max(3, args.calls[0]))
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
