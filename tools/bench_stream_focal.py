#!/usr/bin/env python
"""The focal length of a live stream's camera on the device (CoTrackerOnlinePredictor.calibrate), measured OUTSIDE bench.py with the
conventions of bench_stream_pose.py:

    python tools/bench_stream_focal.py [--passes 3] [--calls 8] [--precision f16x3|f32] [--out profiles/stream_focal_bench.json]

The C4 shape on the online predictor (window 16, 384 x 512 model resolution, iters 6, window graph on), ONE query set of 1024
points, fed by push_frames with 1080 x 1920 uint8 channels-last frames, eight per call (sixteen for the first window):
  plain      the push only;
  calibrate  the push plus calibrate() over the eight frames just pushed (lag 8, 512 hypotheses, 64 candidates, the defaults; the
             state is passed on from call to call) -- the launch of ctk_fit_epipolar and the two launches of ctk_fit_focal, inside the
             timed call.
The rows run IN ONE PROCESS, ALTERNATING pass by pass; every call lies between two HIP events; ms_* is the median over the calls
after the first two windows of every pass, with the smallest and largest single call next to it: `calibrate - plain` is to be read
against the spread of single plain calls, and the line says whether it exceeds it.  host_ms_in_calibrate is the wall clock the host
itself spends inside the call, enqueueing (no synchronise in it).  Then, between the calls of one stream and alternating, the stream
time (HIP events) over the same eight frames and all 1024 points of
  focal     the two launches of ctk_fit_focal at 64 candidates on the matrices and labels of one ctk_fit_epipolar call made before;
  pose_x64  64 launches of ctk_fit_pose, one per candidate camera, on the same matrices and labels: what the sweep replaces,
and their ratio.  The sweep stages each fit list once per four candidates and keeps F * K / 4 workgroups in flight where a pose
launch has F: the expectation -- not a bar -- is that `focal` is faster than `pose_x64` beyond the spread of single evaluations
(`focal_faster_beyond_spread`).  The events bracket what the stream did between them: where the host enqueues 64 launches more
slowly than the device runs them, `pose_x64` holds that wait too -- which is what a caller of 64 launches would see.  Synthetic weights track nothing real, so the counts say what the walk over the lists cost, not what
a scene looks like, and the focal length that comes out means nothing.

What must hold: `calibrate` returns the tracks of `plain` bit for bit (it only reads the stream state).  No time is gated."""

import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

from bench_stream_groups import NoTimer, S, Timer, grid, lib_sha  # noqa: E402
from bench_stream_motion import HW, POINTS, RAW, STEP, setup  # noqa: E402
from cotracker_amd import ops  # noqa: E402

ROWS = ("plain", "calibrate")
KINDS = ("focal", "pose_x64")
LAG, HYPOTHESES, CANDIDATES = 8, 512, 64
CENTRE = ((RAW[1] - 1) / 2.0, (RAW[0] - 1) / 2.0)


def make_rows(p, raw, dev):
    """One predictor per row (a row keeps its stream state, its buffers and its graph between passes)."""
    preds, host_ms, counts, states = {}, [], [], {}
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
            res = None
            with on_call(i):
                out = x.push_frames(new)
                h0 = time.perf_counter()
                if row == "calibrate" and i >= 1:  # (from the second window on frame f - 8 has been tracked)
                    res = x.calibrate(STEP, lag=LAG, hypotheses=HYPOTHESES, candidates=CANDIDATES, state=states.get(i - 1))
                    states[i] = res[1]
                    host_ms.append((time.perf_counter() - h0) * 1e3)  # (the host's own time in the call: nothing in it waits for the device)
            if res is not None:
                counts.append(res[1][0][CANDIDATES:].tolist())  # (frames that took part and their entries, so far)
            outs.append((out[0].clone(), out[1].clone()))
            if after_call is not None:
                after_call(x, i)
        x.finish()
        states.clear()
        return outs
    stream.preds, stream.host_ms, stream.counts = preds, host_ms, counts
    return stream


def alone_line(stream, reps, dev):
    """Between the calls of one `plain` stream: the two launches alone, alternating, over the same eight frames."""
    gpu_ms = {kind: [] for kind in KINDS}
    counts = {kind: [] for kind in KINDS}

    def after_call(x, i):
        if i < 2:
            return
        done = x.model._gstream.committed
        (H, W), (ih, iw) = x._hw, x.interp_shape
        common = dict(N_out=x.N, scale=((W - 1) / (iw - 1), (H - 1) / (ih - 1)), thresh=0.6, first_row=x._emit_first_row(), group=0,
                      lag=LAG)
        fund, label = x.model.stream_epipolar(done - STEP, STEP, hypotheses=HYPOTHESES, **common)[:2]  # (what both read)
        focals = ops.focal_candidates(RAW, dev, candidates=CANDIDATES)
        cams = [(f, f) + CENTRE for f in focals.tolist()]  # (host numbers, made outside the timing)

        def run(kind):
            if kind == "focal":
                res = x.model.stream_focal(done - STEP, STEP, fund, label, focals=focals, principal=CENTRE, min_points=16, **common)
                return res[3][:, [0, 2]]
            for cam in cams:
                res = x.model.stream_pose(done - STEP, STEP, cam, fund, label, min_points=16, **common)
            return res[2][0, :, :2]
        for _ in range(reps):
            for kind in KINDS:
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                res = run(kind)
                b.record()
                b.synchronize()
                gpu_ms[kind].append(a.elapsed_time(b))
                counts[kind].extend(res.tolist())
    stream("plain", 5, NoTimer(), after_call)
    line = {"alone_protocol": "each kind over the same eight frames, alternating between the calls of one stream, each between two HIP "
                              "events after a device synchronise; the first of each kind is left out",
            "alone_frames": STEP, "alone_points": POINTS, "alone_lag": LAG, "alone_hypotheses": HYPOTHESES,
            "alone_candidates": CANDIDATES}
    for kind, v in gpu_ms.items():
        v = v[1:]
        line[f"{kind}_gpu_ms_median"] = round(statistics.median(v), 4)
        line[f"{kind}_gpu_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        line[f"{kind}_points_counted_min"] = [min(c[0] for c in counts[kind]), min(c[1] for c in counts[kind])]
        line[f"{kind}_points_counted_max"] = [max(c[0] for c in counts[kind]), max(c[1] for c in counts[kind])]
    line["alone_evaluations_timed"] = len(gpu_ms["focal"]) - 1
    line["ratio_focal_over_pose_x64"] = round(line["focal_gpu_ms_median"] / line["pose_x64_gpu_ms_median"], 4)
    line["focal_faster_beyond_spread"] = bool(line["focal_gpu_ms_min_max"][1] < line["pose_x64_gpu_ms_min_max"][0])
    return line


def bench_line(dev, precision, passes, calls, reps):
    p, raw = setup(dev, precision)
    stream = make_rows(p, raw, dev)
    for row in ROWS:  # warm every row: weights packed, graphs captured
        stream(row, 3, NoTimer())
    del stream.host_ms[:], stream.counts[:]
    ms, last = {r: [] for r in ROWS}, {}
    for _ in range(passes):
        for row in ROWS:
            last[row] = stream(row, calls, Timer(ms[row], 2))
    med = {r: statistics.median(v) for r, v in ms.items()}
    line = {"workload": "c4_one_set_push_u8_1080p", "points": POINTS, "frames": list(HW), "raw_frames": list(RAW), "window_len": S, "iters": 6,
            "precision": precision, "hip_graph": True, "hypotheses": HYPOTHESES, "lag": LAG, "candidates": CANDIDATES, "principal": list(CENTRE), "passes": passes,
            "calls_per_pass": calls, "timed_calls_per_row": len(ms["plain"]),
            "protocol": "rows alternate pass by pass in one process; every call (the push and what follows it) between two HIP events; "
                        "median over the calls after the first two windows of each pass",
            "libctk_sha256": lib_sha()}
    for r in ROWS:
        line["ms_" + r] = round(med[r], 3)
        line["min_max_ms_" + r] = [round(min(ms[r]), 3), round(max(ms[r]), 3)]
    line["ratio_calibrate_over_plain"] = round(med["calibrate"] / med["plain"], 4)
    line["ms_calibrate_minus_plain"] = round(med["calibrate"] - med["plain"], 3)
    line["spread_plain_ms"] = round(max(ms["plain"]) - min(ms["plain"]), 3)
    line["spread_plain_max_over_min"] = round(max(ms["plain"]) / min(ms["plain"]), 4)
    line["calibrate_minus_plain_exceeds_plain_spread"] = bool(med["calibrate"] - med["plain"] > max(ms["plain"]) - min(ms["plain"]))
    line["host_ms_in_calibrate"] = round(statistics.median(stream.host_ms), 3)
    line["host_ms_in_calibrate_min_max"] = [round(min(stream.host_ms), 3), round(max(stream.host_ms), 3)]
    line["stream_frames_entries_counted_max"] = [max(c[0] for c in stream.counts), max(c[1] for c in stream.counts)]
    same = all(torch.equal(ta, tb) and torch.equal(va, vb) for (ta, va), (tb, vb) in zip(last["plain"], last["calibrate"]))
    line["calibrate_equals_plain_bit_for_bit"] = bool(same)
    line.update(alone_line(stream, reps, dev))
    line["range_fallbacks"] = int(sum(x_.model.range_fallbacks for x_ in stream.preds.values()))
    line["conditions_hold"] = bool(same)
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3, help="stream passes per row")
    ap.add_argument("--calls", type=int, default=8, help="calls per pass")
    ap.add_argument("--reps", type=int, default=5, help="evaluations of each launch timed after every call of one plain stream")
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f32"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_focal_bench.json"), help="append the JSON line to this file")
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
