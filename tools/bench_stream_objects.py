#!/usr/bin/env python
"""Objects of a live stream followed on the device (CoTrackerOnlinePredictor.label_objects / follow), measured OUTSIDE bench.py with the
conventions of bench_stream_motion.py:

    python tools/bench_stream_objects.py [--passes 3] [--calls 8] [--precision f16x3|f32] [--out profiles/stream_objects_bench.json]

The C4 shape on the online predictor (window 16, 384 x 512 model resolution, iters 6, window graph on), ONE query set of 1024
points, fed by push_frames with 1080 x 1920 uint8 channels-last frames, eight per call (sixteen for the first window):
  plain   the push only;
  follow  the push plus follow() of the eight frames just pushed, for four objects boxed after the second window (the four quarters
          of the picture: every point belongs to one) -- inside the timed call.
The rows run IN ONE PROCESS, ALTERNATING pass by pass; every call lies between two HIP events; ms_* is the median over the calls
after the first two windows of every pass, with the smallest and largest single call next to it: the follow / plain ratio is to be
read against that spread.  Then, between the calls of one stream and alternating, the stream time (HIP events) on the eight newest
frames of
  labels  the one launch of ctk_fit_objects in labels mode for L = 4 (against the anchor);
  split   the one launch of ctk_fit_objects in split mode for L = 4 (lag 1);
  masked  what a caller does without it: L ctk_fit_motion launches on L masked `visible` tensors of the emitted tracks, the masks
          included, the emit not.

What must hold: `follow` returns the tracks of `plain` bit for bit (the fit only reads the stream state).  No time is gated: nobody
has measured this kernel before."""

import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

from bench_stream_groups import NoTimer, S, Timer, grid, lib_sha  # noqa: E402
from bench_stream_motion import HW, POINTS, RAW, STEP, setup  # noqa: E402

ROWS = ("plain", "follow")
OBJECTS = 4
KINDS = ("labels", "split", "masked")


def quarters(dev):
    H, W = RAW
    return torch.tensor([[0.0, 0.0, W / 2, H / 2], [W / 2, 0.0, W, H / 2], [0.0, H / 2, W / 2, H], [W / 2, H / 2, W, H]], device=dev)


def make_rows(p, raw, dev):
    """One predictor per row (a row keeps its stream state, its buffers and its graph between passes)."""
    preds = {}
    scale = torch.tensor([1.0, (RAW[1] - 1) / (HW[1] - 1), (RAW[0] - 1) / (HW[0] - 1)])

    def stream(row, calls, on_call, after_call=None):
        if row not in preds:
            preds[row] = copy.deepcopy(p)
        x = preds[row]
        x(torch.zeros(1, 1, 3, *RAW, device=dev), is_first_step=True, queries=(grid(32, 0.0) * scale)[None].to(dev))
        outs, chosen = [], None
        for i in range(calls):
            t0 = (i % 6) * STEP
            new = raw[t0:t0 + S] if i == 0 else raw[t0 + S - STEP:t0 + S]
            with on_call(i):
                out = x.push_frames(new)
                if chosen is not None and row == "follow":
                    x.follow(chosen, STEP)
            if i == 1:  # (outside the timed calls: the median leaves the first two windows out)
                chosen = x.label_objects(quarters(dev))
            outs.append((out[0].clone(), out[1].clone()))
            if after_call is not None:
                after_call(x, i, chosen)
        x.finish()
        return outs
    stream.preds = preds
    return stream


def alone_line(stream, reps):
    """Between the calls of one `plain` stream: the three kinds alone, alternating."""
    from cotracker_amd import ops
    gpu_ms = {kind: [] for kind in KINDS}
    counts = []

    def after_call(x, i, chosen):
        if i < 2:
            return
        gs = x.model._gstream
        done = gs.committed
        (H, W), (ih, iw) = x._hw, x.interp_shape
        common = dict(N_out=x.N, scale=((W - 1) / (iw - 1), (H - 1) / (ih - 1)), thresh=0.6, first_row=x._emit_first_row(), group=0,
                      objects=OBJECTS)
        labels = chosen.labels[None]
        tracks, visible = x.model.stream_emit(done - STEP - 1, done, N_out=x.N, scale=common["scale"], logits=False, thresh=0.6,
                                              first_row=common["first_row"])

        def run(kind):
            if kind == "labels":
                return x.model.stream_objects(done - STEP, STEP, labels=labels, anchor=chosen.anchor, **common)
            if kind == "split":
                return x.model.stream_objects(done - STEP, STEP, lag=1, **common)
            return [ops.fit_motion(tracks, visible & (chosen.labels[:x.N] == r)[None, None], lag=1, first_frame=1, frames=STEP)
                    for r in range(OBJECTS)]
        for _ in range(reps):
            for kind in KINDS:
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                res = run(kind)
                b.record()
                b.synchronize()
                gpu_ms[kind].append(a.elapsed_time(b))
                if kind == "labels":
                    counts.extend(res[2][0, :, :, :2].reshape(-1, 2).tolist())
    stream("plain", 5, NoTimer(), after_call)
    line = {"alone_protocol": "labels: one ctk_fit_objects launch in labels mode (L = 4, anchor form); split: one in split mode (L = 4, lag 1); "
                              "masked: L ctk_fit_motion launches on L masked visible tensors of the emitted tracks, masks included -- each "
                              "over the eight newest frames, alternating between the calls of one stream, each between two HIP events after "
                              "a device synchronise; the first of each kind is left out",
            "alone_frames": STEP, "alone_points": POINTS, "objects": OBJECTS}
    for kind, v in gpu_ms.items():
        v = v[1:]
        line[f"{kind}_gpu_ms_median"] = round(statistics.median(v), 4)
        line[f"{kind}_gpu_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    line["alone_evaluations_timed"] = len(gpu_ms["labels"]) - 1
    line["ratio_labels_over_masked"] = round(line["labels_gpu_ms_median"] / line["masked_gpu_ms_median"], 4)
    line["ratio_split_over_masked"] = round(line["split_gpu_ms_median"] / line["masked_gpu_ms_median"], 4)
    line["labels_faster_than_masked_beyond_spread"] = bool(max(gpu_ms["labels"][1:]) < min(gpu_ms["masked"][1:]))
    line["object_points_inliers_min"] = [min(v[0] for v in counts), min(v[1] for v in counts)]
    line["object_points_inliers_max"] = [max(v[0] for v in counts), max(v[1] for v in counts)]
    return line


def bench_line(dev, precision, passes, calls, reps):
    p, raw = setup(dev, precision)
    stream = make_rows(p, raw, dev)
    for row in ROWS:  # warm every row: weights packed, graphs captured
        stream(row, 3, NoTimer())
    ms, last = {r: [] for r in ROWS}, {}
    for _ in range(passes):
        for row in ROWS:
            last[row] = stream(row, calls, Timer(ms[row], 2))
    med = {r: statistics.median(v) for r, v in ms.items()}
    line = {"workload": "c4_one_set_push_u8_1080p", "points": POINTS, "frames": list(HW), "raw_frames": list(RAW), "window_len": S, "iters": 6,
            "precision": precision, "hip_graph": True, "model": "similarity", "hypotheses": 128, "objects": OBJECTS, "passes": passes,
            "calls_per_pass": calls, "timed_calls_per_row": len(ms["plain"]),
            "protocol": "rows alternate pass by pass in one process; every call (the push and what follows it) between two HIP events; "
                        "median over the calls after the first two windows of each pass",
            "libctk_sha256": lib_sha()}
    for r in ROWS:
        line["ms_" + r] = round(med[r], 3)
        line["min_max_ms_" + r] = [round(min(ms[r]), 3), round(max(ms[r]), 3)]
    line["ratio_follow_over_plain"] = round(med["follow"] / med["plain"], 4)
    line["ms_follow_minus_plain"] = round(med["follow"] - med["plain"], 3)
    line["spread_plain_max_over_min"] = round(max(ms["plain"]) / min(ms["plain"]), 4)
    same = all(torch.equal(ta, tb) and torch.equal(va, vb) for (ta, va), (tb, vb) in zip(last["plain"], last["follow"]))
    line["follow_equals_plain_bit_for_bit"] = bool(same)
    line.update(alone_line(stream, reps))
    line["range_fallbacks"] = int(sum(x_.model.range_fallbacks for x_ in stream.preds.values()))
    line["conditions_hold"] = bool(same)
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3, help="stream passes per row")
    ap.add_argument("--calls", type=int, default=8, help="calls per pass")
    ap.add_argument("--reps", type=int, default=5, help="evaluations of each kind timed after every call of one plain stream")
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f32"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_objects_bench.json"), help="append the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    line = bench_line(dev, args.precision, max(1, args.passes), max(4, args.calls), max(2, args.reps))
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
    if line.get("conditions_hold") is False:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
