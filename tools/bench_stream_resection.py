#!/usr/bin/env python
"""The camera path of a live stream in one unit, on the device (CoTrackerOnlinePredictor.reconstruct / localize), measured OUTSIDE
bench.py with the conventions of bench_stream_pose.py:

    python tools/bench_stream_resection.py [--passes 3] [--calls 8] [--precision f16x3|f32] [--out profiles/stream_resection_bench.json]

The C4 shape on the online predictor (window 16, 384 x 512 model resolution, iters 6, window graph on), ONE query set of 1024
points, fed by push_frames with 1080 x 1920 uint8 channels-last frames, eight per call (sixteen for the first window):
  plain     the push only;
  localize  the push plus localize() over the eight frames just pushed against a structure that reconstruct() made once, after the
            second window (lag 8; a pinhole camera of focal length 1000 px centred on the picture; the defaults: 512 epipolar
            hypotheses, 256 resection hypotheses) -- the launches of ctk_fit_epipolar, ctk_fit_pose and ctk_fit_resection, inside
            the timed call.
The rows run IN ONE PROCESS, ALTERNATING pass by pass; every call lies between two HIP events; ms_* is the median over the calls
after the first two windows of every pass, with the smallest and largest single call next to it: `localize - plain` is to be read
against the spread of single plain calls, and the line says whether it exceeds it (`localize_minus_plain_exceeds_plain_spread`).
host_ms_in_localize is the wall clock the host itself spends inside the call, enqueueing (no synchronise in it).  Then, between the
calls of one stream and alternating, the stream time (HIP events) over the same eight frames, each against the same anchor, of
  resection  the one launch of ctk_fit_resection (256 hypotheses) over ALL points -- a structure of every point at depth 1 on its anchor
             ray and a tolerance every point in front of the camera meets, so that every candidate is scored and the three rounds sum
             over the whole list: what the launch costs at the stream's size, whatever the synthetic weights track;
  pose       the one launch of ctk_fit_pose, no mask, on the matrices and labels of one ctk_fit_epipolar call made before the timing;
  epipolar   the one launch of ctk_fit_epipolar, no mask, with the SAME hypothesis count as the resection launch (256);
  resection_stream  the launch as localize() made it, on the structure reconstruct() kept (few points: synthetic weights),
and the ratio resection / epipolar with whether it lies beyond the spread of single evaluations.  No speed is promised: a resection
candidate is one scalar and a projection per point, an epipolar hypothesis an 8-point elimination and a Sampson test per point.
How many points were fitted on and how many lie within tol is reported: synthetic weights track nothing real, so the counts say what
the walk over the list cost, not what a scene looks like.

What must hold: `localize` returns the tracks of `plain` bit for bit (it only reads the stream state).  No time is gated: nobody has
measured this kernel before."""

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

ROWS = ("plain", "localize")
KINDS = ("resection", "pose", "epipolar", "resection_stream")
WIDE = 1.0e4  # a tolerance in pixels that every point in front of the camera meets
LAG, HYPOTHESES = 8, 256  # (of the resection launch; the two-view launches inside localize() keep their 512)
CAMERA = (1000.0, 1000.0, (RAW[1] - 1) / 2.0, (RAW[0] - 1) / 2.0)


def make_rows(p, raw, dev):
    """One predictor per row (a row keeps its stream state, its buffers and its graph between passes)."""
    preds, host_ms, counts, structures = {}, [], [], {}
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
                if row == "localize" and i == 1:  # (from the second window on frame f - 8 has been tracked; this call is not timed)
                    structures[row] = x.reconstruct(CAMERA, lag=LAG)
                elif row == "localize" and i >= 2:
                    res = x.localize(structures[row], STEP, hypotheses=HYPOTHESES)
                    host_ms.append((time.perf_counter() - h0) * 1e3)  # (the host's own time in the call: nothing in it waits for the device)
            if res is not None:
                counts.extend(res[3][:, :2].tolist())
            outs.append((out[0].clone(), out[1].clone()))
            if after_call is not None:
                after_call(x, i)
        x.finish()
        return outs
    stream.preds, stream.host_ms, stream.counts = preds, host_ms, counts
    return stream


def alone_line(stream, reps, dev):
    """Between the calls of one `plain` stream: the three launches alone, alternating, over the same eight frames and anchor."""
    gpu_ms = {kind: [] for kind in KINDS}
    counts = {kind: [] for kind in KINDS}

    held = {}

    def after_call(x, i):
        if i == 1:
            held["s"] = x.reconstruct(CAMERA, lag=LAG)
        if i < 2:
            return
        s = held["s"]
        done = x.model._gstream.committed
        (H, W), (ih, iw) = x._hw, x.interp_shape
        common = dict(N_out=x.N, scale=((W - 1) / (iw - 1), (H - 1) / (ih - 1)), thresh=0.6, first_row=x._emit_first_row(), group=0,
                      anchor=s.anchor)
        # Synthetic weights track nothing real, so reconstruct() keeps only a few points.  What the launches cost at the stream's
        # size is measured on ALL points: a structure of every point at depth 1 on its anchor ray and a tolerance that every point
        # in front of the camera meets, so that all 256 + 3 candidates are scored and the three rounds sum over the whole list;
        # the pose and epipolar launches without a mask.  `resection_stream` is the launch as localize() made it.
        from cotracker_amd import ops
        n_model = s.points.shape[0]
        ones = torch.ones(n_model, 2, device=dev)
        full_pts, full_valid = ops.structure_from_pose(s.anchor.coords[0], CAMERA, ones, ones[:, 0].to(torch.int8), scale=common["scale"])
        full_pts, full_valid = full_pts[None].contiguous(), full_valid[None].contiguous()
        fund, label = x.model.stream_epipolar(done - STEP, STEP, hypotheses=HYPOTHESES, **common)[:2]  # (what the pose launch reads)
        seeds = x.model.stream_pose(done - STEP, STEP, CAMERA, fund, label, min_points=16, **common)[0]  # (and the resection launch)
        mask = s.valid[None]
        fund_s, label_s = x.model.stream_epipolar(done - STEP, STEP, mask=mask, **common)[:2]
        seeds_s = x.model.stream_pose(done - STEP, STEP, CAMERA, fund_s, label_s, mask=mask, min_points=16, **common)[0]

        def run(kind):
            if kind == "epipolar":
                return x.model.stream_epipolar(done - STEP, STEP, hypotheses=HYPOTHESES, **common)[3][0, :, :2]
            if kind == "pose":
                return x.model.stream_pose(done - STEP, STEP, CAMERA, fund, label, min_points=16, **common)[2][0, :, :2]
            if kind == "resection_stream":
                return x.model.stream_resection(done - STEP, STEP, CAMERA, s.points[None], mask, seeds_s, hypotheses=HYPOTHESES,
                                                **common)[3][0, :, :2]
            return x.model.stream_resection(done - STEP, STEP, CAMERA, full_pts, full_valid, seeds, tol=WIDE, hypotheses=HYPOTHESES,
                                            **common)[3][0, :, :2]
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
    line = {"alone_protocol": "each launch over the same eight frames, alternating between the calls of one stream, each between two HIP "
                              "events after a device synchronise; the first of each kind is left out",
            "alone_frames": STEP, "alone_points": POINTS, "alone_source": "the anchor of reconstruct()", "alone_hypotheses": HYPOTHESES}
    for kind, v in gpu_ms.items():
        v = v[1:]
        line[f"{kind}_gpu_ms_median"] = round(statistics.median(v), 4)
        line[f"{kind}_gpu_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        line[f"{kind}_points_counted_min"] = [min(c[0] for c in counts[kind]), min(c[1] for c in counts[kind])]
        line[f"{kind}_points_counted_max"] = [max(c[0] for c in counts[kind]), max(c[1] for c in counts[kind])]
    line["alone_evaluations_timed"] = len(gpu_ms["resection"]) - 1
    line["ratio_resection_over_epipolar_launch"] = round(line["resection_gpu_ms_median"] / line["epipolar_gpu_ms_median"], 4)
    line["ratio_resection_over_pose_launch"] = round(line["resection_gpu_ms_median"] / line["pose_gpu_ms_median"], 4)
    r, e = line["resection_gpu_ms_min_max"], line["epipolar_gpu_ms_min_max"]
    line["resection_vs_epipolar_beyond_spread"] = bool(r[1] < e[0] or e[1] < r[0])  # (the single evaluations do not overlap)
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
            "precision": precision, "hip_graph": True, "hypotheses": HYPOTHESES, "lag": LAG, "camera": list(CAMERA), "passes": passes,
            "calls_per_pass": calls, "timed_calls_per_row": len(ms["plain"]),
            "protocol": "rows alternate pass by pass in one process; every call (the push and what follows it) between two HIP events; "
                        "median over the calls after the first two windows of each pass",
            "libctk_sha256": lib_sha()}
    for r in ROWS:
        line["ms_" + r] = round(med[r], 3)
        line["min_max_ms_" + r] = [round(min(ms[r]), 3), round(max(ms[r]), 3)]
    line["ratio_localize_over_plain"] = round(med["localize"] / med["plain"], 4)
    line["ms_localize_minus_plain"] = round(med["localize"] - med["plain"], 3)
    line["spread_plain_ms"] = round(max(ms["plain"]) - min(ms["plain"]), 3)
    line["spread_plain_max_over_min"] = round(max(ms["plain"]) / min(ms["plain"]), 4)
    line["localize_minus_plain_exceeds_plain_spread"] = bool(med["localize"] - med["plain"] > max(ms["plain"]) - min(ms["plain"]))
    line["host_ms_in_localize"] = round(statistics.median(stream.host_ms), 3)
    line["host_ms_in_localize_min_max"] = [round(min(stream.host_ms), 3), round(max(stream.host_ms), 3)]
    line["stream_points_within_tol_min"] = [min(c[0] for c in stream.counts), min(c[1] for c in stream.counts)]
    line["stream_points_within_tol_max"] = [max(c[0] for c in stream.counts), max(c[1] for c in stream.counts)]
    same = all(torch.equal(ta, tb) and torch.equal(va, vb) for (ta, va), (tb, vb) in zip(last["plain"], last["localize"]))
    line["localize_equals_plain_bit_for_bit"] = bool(same)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_resection_bench.json"), help="append the JSON line to this file")
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
