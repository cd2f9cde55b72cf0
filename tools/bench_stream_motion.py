#!/usr/bin/env python
"""The camera motion of a live stream fitted on the device (CoTrackerOnlinePredictor.camera_motion), measured OUTSIDE bench.py with
the conventions of bench_stream_draw.py:

    python tools/bench_stream_motion.py [--passes 3] [--calls 8] [--precision f16x3|f32] [--out profiles/stream_motion_bench.json]

The C4 shape on the online predictor (window 16, 384 x 512 model resolution, iters 6, window graph on), ONE query set of 1024
points, fed by push_frames with 1080 x 1920 uint8 channels-last frames, eight per call (sixteen for the first window):
  plain   the push only;
  motion  the push plus camera_motion() of the eight frames just pushed (similarity, 128 hypotheses) -- inside the timed call.
The rows run IN ONE PROCESS, ALTERNATING pass by pass; every call lies between two HIP events; ms_* is the median over the calls
after the first two windows of every pass, with the smallest and largest single call next to it: the motion / plain ratio is to be
read against that spread.  Then, between the calls of one stream and alternating: the stream time (HIP events) of the one launch
alone on the eight newest frames, for 128 and for 1024 hypotheses, both models.

What must hold: `motion` returns the tracks of `plain` bit for bit (the fit only reads the stream state).  No time is gated: nobody
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

from bench_stream_groups import HW, NoTimer, S, Timer, grid, lib_sha  # noqa: E402

ROWS = ("plain", "motion")
STEP = S // 2
RING = S + 5 * STEP  # frames resident, walked round
RAW = (1080, 1920)
POINTS = 1024
KS = (128, 1024)


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
    small = synthetic_video(RING, *HW, seed=1234).to(dev)[0]  # [T,3,384,512] float, 0..255
    raw = torch.empty(RING, *RAW, 3, dtype=torch.uint8, device=dev)
    for i in range(RING):  # (frame by frame: the float 1080p copy of the whole ring is not needed at once)
        big = torch.nn.functional.interpolate(small[i:i + 1], RAW, mode="bilinear", align_corners=True)
        raw[i] = big[0].permute(1, 2, 0).round().clamp(0, 255).to(torch.uint8)
    return p.to(dev), raw


def make_rows(p, raw, dev):
    """One predictor per row (a row keeps its stream state, its buffers and its graph between passes)."""
    preds = {}
    scale = torch.tensor([1.0, (RAW[1] - 1) / (HW[1] - 1), (RAW[0] - 1) / (HW[0] - 1)])

    def stream(row, calls, on_call, after_call=None):
        if row not in preds:
            preds[row] = copy.deepcopy(p)
        x = preds[row]
        x(torch.zeros(1, 1, 3, *RAW, device=dev), is_first_step=True, queries=(grid(32, 0.0) * scale)[None].to(dev))
        outs = []
        for i in range(calls):
            t0 = (i % 6) * STEP
            new = raw[t0:t0 + S] if i == 0 else raw[t0 + S - STEP:t0 + S]
            with on_call(i):
                out = x.push_frames(new)
                if row == "motion":
                    x.camera_motion(STEP)
            outs.append((out[0].clone(), out[1].clone()))
            if after_call is not None:
                after_call(x, i)
        x.finish()
        return outs
    stream.preds = preds
    return stream


def motion_line(stream, reps):
    """Between the calls of one `plain` stream: the one launch alone, per model and hypothesis count."""
    kinds = [(m, k) for m in ("similarity", "translation") for k in KS]
    gpu_ms = {kind: [] for kind in kinds}
    inliers = []

    def after_call(x, i):
        if i < 2:
            return
        for _ in range(reps):
            for kind in kinds:
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                res = x.camera_motion(STEP, model=kind[0], hypotheses=kind[1])
                b.record()
                b.synchronize()
                gpu_ms[kind].append(a.elapsed_time(b))
                if kind == kinds[0]:
                    inliers.extend(res[2][0, :, :2].tolist())
    stream("plain", 5, NoTimer(), after_call)
    line = {"motion_protocol": "the one launch of camera_motion() over the eight newest frames, per model and hypothesis count, alternating "
                               "between the calls of one stream, each between two HIP events after a device synchronise; the first of each "
                               "kind is left out",
            "motion_frames": STEP, "motion_points": POINTS, "launches": 1}
    for (m, k), v in gpu_ms.items():
        v = v[1:]
        line[f"{m}_k{k}_gpu_ms_median"] = round(statistics.median(v), 4)
        line[f"{m}_k{k}_gpu_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    line["motion_evaluations_timed"] = len(gpu_ms[kinds[0]]) - 1
    line["correspondences_inliers_min"] = [min(v[0] for v in inliers), min(v[1] for v in inliers)]
    line["correspondences_inliers_max"] = [max(v[0] for v in inliers), max(v[1] for v in inliers)]
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
            "precision": precision, "hip_graph": True, "model": "similarity", "hypotheses": 128, "passes": passes, "calls_per_pass": calls,
            "timed_calls_per_row": len(ms["plain"]),
            "protocol": "rows alternate pass by pass in one process; every call (the push and what follows it) between two HIP events; "
                        "median over the calls after the first two windows of each pass",
            "libctk_sha256": lib_sha()}
    for r in ROWS:
        line["ms_" + r] = round(med[r], 3)
        line["min_max_ms_" + r] = [round(min(ms[r]), 3), round(max(ms[r]), 3)]
    line["ratio_motion_over_plain"] = round(med["motion"] / med["plain"], 4)
    line["ms_motion_minus_plain"] = round(med["motion"] - med["plain"], 3)
    line["spread_plain_max_over_min"] = round(max(ms["plain"]) / min(ms["plain"]), 4)
    same = all(torch.equal(ta, tb) and torch.equal(va, vb) for (ta, va), (tb, vb) in zip(last["plain"], last["motion"]))
    line["motion_equals_plain_bit_for_bit"] = bool(same)
    line.update(motion_line(stream, reps))
    line["range_fallbacks"] = int(sum(x_.model.range_fallbacks for x_ in stream.preds.values()))
    line["conditions_hold"] = bool(same)
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3, help="stream passes per row")
    ap.add_argument("--calls", type=int, default=8, help="calls per pass")
    ap.add_argument("--reps", type=int, default=5, help="launches of each kind timed after every call of one plain stream")
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f32"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_motion_bench.json"), help="append the JSON line to this file")
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
