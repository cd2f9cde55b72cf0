#!/usr/bin/env python
"""The camera of a live stream against a structure WITHOUT a seed (CoTrackerOnlinePredictor.resect, one launch of ctk_fit_p3p) next to
localize() (three launches), measured OUTSIDE bench.py with the conventions of bench_stream_resection.py:

    python tools/bench_stream_p3p.py [--passes 3] [--calls 8] [--precision f16x3|f32] [--out profiles/stream_p3p_bench.json]

The C4 shape on the online predictor (window 16, 384 x 512 model resolution, iters 6, window graph on), ONE query set of 1024
points, fed by push_frames with 1080 x 1920 uint8 channels-last frames, eight per call (sixteen for the first window):
  plain     the push only;
  localize  the push plus localize() over the eight frames just pushed against a structure that reconstruct() made once, after the
            second window (lag 8; a pinhole camera of focal length 1000 px centred on the picture; the defaults);
  resect    the push plus resect() over the same frames against such a structure (256 hypotheses, the default).
The rows run IN ONE PROCESS, ALTERNATING pass by pass; every call lies between two HIP events; ms_* is the median over the calls
after the first two windows of every pass, with the smallest and largest single call next to it.  Then, between the calls of one
stream and alternating, 14 timed evaluations each of the stream time (HIP events) over the same eight frames and the same anchor of
  p3p    the ONE launch of ctk_fit_p3p (256 hypotheses) over ALL 1024 points -- a structure of every point at depth 1 on its anchor
         ray and a tolerance every point in front of the camera meets, so that every candidate that stands is scored over the whole
         list and the three rounds sum over it: what the launch costs at the stream's size, whatever the synthetic weights track;
  chain  the THREE launches as localize() runs them -- ctk_fit_epipolar (512 hypotheses, the structure's mask), ctk_fit_pose,
         ctk_fit_resection (256 hypotheses) -- on the same structure, mask and tolerance, between one pair of events.
The expectation, not a gate: the one launch takes no longer than the three together.  The line says whether it is met and whether the
single evaluations of the two overlap (`p3p_vs_chain_beyond_spread`); inside the spread nothing is claimed.

What must hold: `localize` and `resect` return the tracks of `plain` bit for bit (they only read the stream state)."""

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
from bench_stream_resection import CAMERA, LAG, WIDE  # noqa: E402

ROWS = ("plain", "localize", "resect")
KINDS = ("p3p", "chain")
HYPOTHESES = 256


def make_rows(p, raw, dev):
    """One predictor per row (a row keeps its stream state, its buffers and its graph between passes)."""
    preds, counts, structures = {}, {r: [] for r in ROWS}, {}
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
                if row != "plain" and i == 1:  # (from the second window on frame f - 8 has been tracked; this call is not timed)
                    structures[row] = x.reconstruct(CAMERA, lag=LAG)
                elif row == "localize" and i >= 2:
                    res = x.localize(structures[row], STEP, hypotheses=HYPOTHESES)
                elif row == "resect" and i >= 2:
                    res = x.resect(structures[row], STEP, hypotheses=HYPOTHESES)
            if res is not None:
                counts[row].extend(res[3][:, :2].tolist())
            outs.append((out[0].clone(), out[1].clone()))
            if after_call is not None:
                after_call(x, i)
        x.finish()
        return outs
    stream.preds, stream.counts = preds, counts
    return stream


def alone_line(stream, reps, dev):
    """Between the calls of one `plain` stream: the one launch and the three, alternating, over the same eight frames and anchor."""
    from cotracker_amd import ops
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
        # Synthetic weights track nothing real, so reconstruct() keeps only a few points.  What the launches cost at the stream's size
        # is measured on ALL points: a structure of every point at depth 1 on its anchor ray, every point valid, and a tolerance that
        # every point in front of the camera meets.
        ones = torch.ones(s.points.shape[0], 2, device=dev)
        full_pts, full_valid = ops.structure_from_pose(s.anchor.coords[0], CAMERA, ones, ones[:, 0].to(torch.int8), scale=common["scale"])
        full_pts, full_valid = full_pts[None].contiguous(), full_valid[None].contiguous()

        def run(kind):
            if kind == "p3p":
                return x.model.stream_p3p(done - STEP, STEP, CAMERA, full_pts, full_valid, tol=WIDE, hypotheses=HYPOTHESES, **common)[3][0, :, :2]
            fund, label, _, _ = x.model.stream_epipolar(done - STEP, STEP, mask=full_valid, tol=1.0, hypotheses=512, min_base=16.0,
                                                        min_points=16, seed=0, **common)
            seeds = x.model.stream_pose(done - STEP, STEP, CAMERA, fund, label, mask=full_valid, min_points=16, **common)[0]
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
    line = {"alone_protocol": "the one launch and the three launches over the same eight frames, alternating between the calls of one "
                              "stream, each between two HIP events after a device synchronise; the first of each kind is left out",
            "alone_frames": STEP, "alone_points": POINTS, "alone_source": "the anchor of reconstruct()", "alone_hypotheses": HYPOTHESES,
            "chain_epipolar_hypotheses": 512}
    for kind, v in gpu_ms.items():
        v = v[1:]
        line[f"{kind}_gpu_ms_median"] = round(statistics.median(v), 4)
        line[f"{kind}_gpu_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        line[f"{kind}_points_counted_min"] = [min(c[0] for c in counts[kind]), min(c[1] for c in counts[kind])]
        line[f"{kind}_points_counted_max"] = [max(c[0] for c in counts[kind]), max(c[1] for c in counts[kind])]
    line["alone_evaluations_timed"] = len(gpu_ms["p3p"]) - 1
    line["ratio_p3p_over_chain"] = round(line["p3p_gpu_ms_median"] / line["chain_gpu_ms_median"], 4)
    a, c = line["p3p_gpu_ms_min_max"], line["chain_gpu_ms_min_max"]
    line["p3p_vs_chain_beyond_spread"] = bool(a[1] < c[0] or c[1] < a[0])  # (the single evaluations do not overlap)
    line["expectation_one_launch_no_longer_than_three"] = bool(line["p3p_gpu_ms_median"] <= line["chain_gpu_ms_median"])
    return line


def bench_line(dev, precision, passes, calls, reps):
    p, raw = setup(dev, precision)
    stream = make_rows(p, raw, dev)
    for row in ROWS:  # warm every row: weights packed, graphs captured
        stream(row, 3, NoTimer())
    for v in stream.counts.values():
        del v[:]
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
    spread = max(ms["plain"]) - min(ms["plain"])
    line["spread_plain_ms"] = round(spread, 3)
    for r in ROWS[1:]:
        line[f"ms_{r}_minus_plain"] = round(med[r] - med["plain"], 3)
        line[f"{r}_minus_plain_exceeds_plain_spread"] = bool(med[r] - med["plain"] > spread)
        line[f"{r}_points_within_tol_min"] = [min(c[0] for c in stream.counts[r]), min(c[1] for c in stream.counts[r])]
        line[f"{r}_points_within_tol_max"] = [max(c[0] for c in stream.counts[r]), max(c[1] for c in stream.counts[r])]
    same = all(torch.equal(ta, tb) and torch.equal(va, vb) for r in ROWS[1:] for (ta, va), (tb, vb) in zip(last["plain"], last[r]))
    line["readers_equal_plain_bit_for_bit"] = bool(same)
    line.update(alone_line(stream, reps, dev))
    line["range_fallbacks"] = int(sum(x_.model.range_fallbacks for x_ in stream.preds.values()))
    line["conditions_hold"] = bool(same)
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3, help="stream passes per row")
    ap.add_argument("--calls", type=int, default=8, help="calls per pass")
    ap.add_argument("--reps", type=int, default=5, help="evaluations of each kind timed after every call of one plain stream (5: 14 timed)")
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f32"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_p3p_bench.json"), help="append the JSON line to this file")
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
