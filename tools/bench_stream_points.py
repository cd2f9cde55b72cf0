#!/usr/bin/env python
"""Points added to the structure of a live stream, on the device (CoTrackerOnlinePredictor.extend), measured OUTSIDE bench.py with the
conventions of bench_stream_resection.py:

    python tools/bench_stream_points.py [--passes 3] [--calls 8] [--precision f16x3|f32] [--out profiles/stream_points_bench.json]

The C4 shape on the online predictor (window 16, 384 x 512 model resolution, iters 6, window graph on), ONE query set of 1024
points with 64 spare slots, fed by push_frames with 1080 x 1920 uint8 channels-last frames, eight per call (sixteen for the first
window):
  plain   the push only;
  extend  the push plus extend() over the eight frames just pushed onto the newest of them, against a structure that reconstruct()
          made once, after the second window (lag 8; a pinhole camera of focal length 1000 px centred on the picture; the defaults
          of localize() and extend()) -- the launches of ctk_fit_epipolar, ctk_fit_pose, ctk_fit_resection and ctk_fit_structure and
          the pin, inside the timed call.  The extended structure is not kept: every call extends the same one.
The rows run IN ONE PROCESS, ALTERNATING pass by pass; every call lies between two HIP events; ms_* is the median over the calls
after the first two windows of every pass, with the smallest and largest single call next to it: `extend - plain` is to be read
against the spread of single plain calls, and the line says whether it exceeds it.  host_ms_in_extend is the wall clock the host
itself spends inside the call, enqueueing (no synchronise in it).  Then, between the calls of one stream and alternating, the stream
time (HIP events) over the same eight frames of
  structure  the one launch of ctk_fit_structure over ALL slots: eight views under planted poses (a camera that steps sideways, so
             that every view counts), no old structure, a tolerance every point in front of the cameras meets, so that every slot
             walks the views five times: what the launch costs at the stream's size, whatever the synthetic weights track;
  resection  the one launch of ctk_fit_resection (256 hypotheses) over ALL points, as bench_stream_resection.py times it;
and the ratio structure / resection with whether it lies beyond the spread of single evaluations.  No speed is promised: nobody has
measured this kernel before.  How many slots were observed, started and accepted is reported: synthetic weights track nothing real,
so the counts say what the walk cost, not what a scene looks like.

What must hold: `extend` returns the tracks of `plain` bit for bit (it only reads the stream state)."""

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

ROWS = ("plain", "extend")
KINDS = ("structure", "resection")
WIDE = 1.0e4  # a tolerance in pixels that every point in front of the camera meets
LAG, HYPOTHESES, SPARE = 8, 256, 64
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
                if row == "extend" and i == 1:  # (from the second window on frame f - 8 has been tracked; this call is not timed)
                    structures[row] = x.reconstruct(CAMERA, lag=LAG)
                elif row == "extend" and i >= 2:
                    res = x.extend(structures[row], n=STEP, hypotheses=HYPOTHESES)
                    host_ms.append((time.perf_counter() - h0) * 1e3)  # (the host's own time in the call: nothing in it waits for the device)
            if res is not None:
                counts.append(int(res.valid.sum()))
            outs.append((out[0].clone(), out[1].clone()))
            if after_call is not None:
                after_call(x, i)
        x.finish()
        return outs
    stream.preds, stream.host_ms, stream.counts = preds, host_ms, counts
    return stream


def alone_line(stream, reps, dev):
    """Between the calls of one `plain` stream: the two launches alone, alternating, over the same eight frames."""
    from cotracker_amd import ops
    gpu_ms = {kind: [] for kind in KINDS}
    seen = {"observed": [], "started": [], "accepted": []}
    held = {}

    def after_call(x, i):
        if i == 1:
            held["s"] = x.reconstruct(CAMERA, lag=LAG)
        if i < 2:
            return
        s = held["s"]
        done = x.model._gstream.committed
        (H, W), (ih, iw) = x._hw, x.interp_shape
        common = dict(N_out=x.N, scale=((W - 1) / (iw - 1), (H - 1) / (ih - 1)), thresh=0.6, first_row=x._emit_first_row(), group=0)
        n_model = s.points.shape[0]
        ones = torch.ones(n_model, 2, device=dev)
        full_pts, full_valid = ops.structure_from_pose(s.anchor.coords[0], CAMERA, ones, ones[:, 0].to(torch.int8), scale=common["scale"])
        full_pts, full_valid = full_pts[None].contiguous(), full_valid[None].contiguous()
        fund, label = x.model.stream_epipolar(done - STEP, STEP, hypotheses=HYPOTHESES, anchor=s.anchor, **common)[:2]
        seeds = x.model.stream_pose(done - STEP, STEP, CAMERA, fund, label, min_points=16, anchor=s.anchor, **common)[0]
        planted = torch.eye(3, 4, device=dev).repeat(1, STEP, 1, 1)
        planted[0, :, 0, 3] = -0.05 * torch.arange(STEP, device=dev)  # the camera steps sideways: every view counts

        def run(kind):
            if kind == "structure":
                return x.model.stream_structure(done - STEP, STEP, CAMERA, planted, into=STEP - 1, tol=WIDE, min_views=2, **common)[3][0]
            return x.model.stream_resection(done - STEP, STEP, CAMERA, full_pts, full_valid, seeds, tol=WIDE, hypotheses=HYPOTHESES,
                                            anchor=s.anchor, **common)[3][0]
        for _ in range(reps):
            for kind in KINDS:
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                res = run(kind)
                b.record()
                b.synchronize()
                gpu_ms[kind].append(a.elapsed_time(b))
                if kind == "structure":
                    seen["observed"].append(int((res[:, 0] >= 2).sum()))
                    seen["started"].append(int(((res[:, 0] >= 2) & (res[:, 3] & 8 == 0)).sum()))
                    seen["accepted"].append(int(((res[:, 1] >= 2) & (res[:, 3] & (8 | 16 | 64) == 0)).sum()))
    stream("plain", 5, NoTimer(), after_call)
    line = {"alone_protocol": "each launch over the same eight frames, alternating between the calls of one stream, each between two HIP "
                              "events after a device synchronise; the first of each kind is left out",
            "alone_frames": STEP, "alone_slots": POINTS + SPARE, "alone_hypotheses": HYPOTHESES, "structure_block_threads": 64}
    for kind, v in gpu_ms.items():
        v = v[1:]
        line[f"{kind}_gpu_ms_median"] = round(statistics.median(v), 4)
        line[f"{kind}_gpu_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    for k_, v in seen.items():
        line[f"structure_slots_{k_}_min_max"] = [min(v), max(v)]
    line["alone_evaluations_timed"] = len(gpu_ms["structure"]) - 1
    line["ratio_structure_over_resection_launch"] = round(line["structure_gpu_ms_median"] / line["resection_gpu_ms_median"], 4)
    r, e = line["structure_gpu_ms_min_max"], line["resection_gpu_ms_min_max"]
    line["structure_vs_resection_beyond_spread"] = bool(r[1] < e[0] or e[1] < r[0])  # (the single evaluations do not overlap)
    return line


def bench_line(dev, precision, passes, calls, reps):
    p, raw = setup(dev, precision)
    p.spare_points = SPARE
    stream = make_rows(p, raw, dev)
    for row in ROWS:  # warm every row: weights packed, graphs captured
        stream(row, 3, NoTimer())
    del stream.host_ms[:], stream.counts[:]
    ms, last = {r: [] for r in ROWS}, {}
    for _ in range(passes):
        for row in ROWS:
            last[row] = stream(row, calls, Timer(ms[row], 2))
    med = {r: statistics.median(v) for r, v in ms.items()}
    line = {"workload": "c4_one_set_push_u8_1080p", "points": POINTS, "spare_points": SPARE, "frames": list(HW), "raw_frames": list(RAW),
            "window_len": S, "iters": 6, "precision": precision, "hip_graph": True, "hypotheses": HYPOTHESES, "lag": LAG, "camera": list(CAMERA),
            "passes": passes, "calls_per_pass": calls, "timed_calls_per_row": len(ms["plain"]),
            "protocol": "rows alternate pass by pass in one process; every call (the push and what follows it) between two HIP events; "
                        "median over the calls after the first two windows of each pass",
            "libctk_sha256": lib_sha()}
    for r in ROWS:
        line["ms_" + r] = round(med[r], 3)
        line["min_max_ms_" + r] = [round(min(ms[r]), 3), round(max(ms[r]), 3)]
    line["ratio_extend_over_plain"] = round(med["extend"] / med["plain"], 4)
    line["ms_extend_minus_plain"] = round(med["extend"] - med["plain"], 3)
    line["spread_plain_ms"] = round(max(ms["plain"]) - min(ms["plain"]), 3)
    line["extend_minus_plain_exceeds_plain_spread"] = bool(med["extend"] - med["plain"] > max(ms["plain"]) - min(ms["plain"]))
    line["host_ms_in_extend"] = round(statistics.median(stream.host_ms), 3)
    line["host_ms_in_extend_min_max"] = [round(min(stream.host_ms), 3), round(max(stream.host_ms), 3)]
    line["stream_points_in_extended_structure_min_max"] = [min(stream.counts), max(stream.counts)]
    same = all(torch.equal(ta, tb) and torch.equal(va, vb) for (ta, va), (tb, vb) in zip(last["plain"], last["extend"]))
    line["extend_equals_plain_bit_for_bit"] = bool(same)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_points_bench.json"), help="append the JSON line to this file")
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
