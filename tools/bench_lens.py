#!/usr/bin/env python
"""Lens distortion taken out of a live stream's frames on the device (ops.lens_frames, ops.lens_points, CoTrackerOnlinePredictor.lens),
measured OUTSIDE bench.py with the conventions of bench_stream_stabilize.py:

    python tools/bench_lens.py [--passes 3] [--calls 8] [--reps 14] [--precision f16x3|f32] [--out profiles/lens_bench.json]

Launches alone, over eight 1080 x 1920 uint8 channels-last pictures, ALTERNATING in one process, each between two HIP events after a
device synchronise (the first of each kind is left out; medians, and the smallest .. largest single value):
  copy        out.copy_(frames): the memory bound for these bytes on this machine;
  warp        ops.warp_frames under the identity: the 2 x 3 resampler (Q24 coordinates stepped per pixel, LDS-staged);
  planes      ops.warp_planes under the identity: the 3 x 3 resampler, which pays a double division per pixel and picture;
  lens_ideal  ops.lens_frames(to="ideal") with the action lens (-0.28, 0.09, 1e-3, -8e-4, -0.013) at f = 1000: the closed form in
              double, once per pixel for all eight pictures; memory read directly;
  lens_sensor ops.lens_frames(to="sensor"): eight Newton rounds in double per pixel, once for all eight pictures;
  torch       what a caller writes: uint8 -> float, F.grid_sample on a map made OUTSIDE the timed region (in torch's favour), round,
              -> uint8;
  points      ops.lens_points over [1, 8, 1024, 2], to ideal: for the record.
The yardstick of lens_ideal is `planes`, the kernel of the same process -- never a number from a file.  What is expected, and only
tested: lens_ideal takes no longer than planes beyond the spread of single evaluations.  lens_sensor has no expectation attached.

Per call: the C4 shape on the online predictor (window 16, 384 x 512 model resolution, iters 6, window graph on), ONE query set of 1024
points, fed by push_frames with 1080p uint8 frames, eight per call (sixteen for the first window); rows `plain` (no lens) and `lens`
(predictor.lens set: one more launch per push) alternate pass by pass.

What must hold: the zero lens copies the pictures bit for bit, and a stream with the zero lens returns the tracks of a stream without
one bit for bit.  The largest difference between lens_ideal and torch's float32 result is recorded, in grey levels.  No time is gated."""

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
from bench_stream_motion import POINTS, RAW, STEP, setup  # noqa: E402

ROWS = ("plain", "lens")
KINDS = ("copy", "warp", "planes", "lens_ideal", "lens_sensor", "torch", "points")
CAMERA = (1000.0, 1000.0, (RAW[1] - 1) / 2, (RAW[0] - 1) / 2)
ACTION = (-0.28, 0.09, 1e-3, -8e-4, -0.013)


def make_rows(p, raw, dev, lens):
    """One predictor per row (a row keeps its stream state, its buffers and its graph between passes)."""
    preds = {}
    scale = torch.tensor([1.0, (RAW[1] - 1) / (HW[1] - 1), (RAW[0] - 1) / (HW[0] - 1)])

    def stream(row, calls, on_call, lens_of_row=None):
        if row not in preds:
            preds[row] = copy.deepcopy(p)
        x = preds[row]
        x(torch.zeros(1, 1, 3, *RAW, device=dev), is_first_step=True, queries=(grid(32, 0.0) * scale)[None].to(dev))
        x.lens = lens_of_row if lens_of_row is not None else (lens if row == "lens" else None)
        outs = []
        for i in range(calls):
            t0 = (i % 6) * STEP
            new = raw[t0:t0 + S] if i == 0 else raw[t0 + S - STEP:t0 + S]
            with on_call(i):
                out = x.push_frames(new)
            outs.append((out[0].clone(), out[1].clone()))
        x.finish()
        return outs
    stream.preds = preds
    return stream


def torch_map(dev):
    """grid_sample's grid [1,H,W,2] (align_corners=True) for the pinhole picture of the action lens: the closed form in float64."""
    H, W = RAW
    k1, k2, p1, p2, k3 = ACTION
    fx, fy, cx, cy = CAMERA
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    x, y = (xs - cx) / fx, (ys - cy) / fy
    r2 = x * x + y * y
    rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    qx = fx * (x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) + cx
    qy = fy * (y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y) + cy
    return torch.stack([2 * qx / (W - 1) - 1, 2 * qy / (H - 1) - 1], dim=-1)[None].float()


def torch_remap(frames, grid_):
    x = frames.permute(0, 3, 1, 2).float()
    y = torch.nn.functional.grid_sample(x, grid_.expand(x.shape[0], -1, -1, -1), mode="bilinear", padding_mode="zeros", align_corners=True)
    return y.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def launch_line(raw, reps, dev, lens):
    from cotracker_amd import ops
    frames = raw[:STEP].contiguous()
    out = torch.empty_like(frames)
    eye2 = torch.tensor([[1.0, 0, 0], [0, 1.0, 0]], device=dev).expand(STEP, 2, 3).contiguous()
    eye3 = torch.eye(3, device=dev).expand(STEP, 3, 3).contiguous()
    grid_ = torch_map(dev)
    g = torch.Generator().manual_seed(0)
    pts = (torch.rand(1, STEP, POINTS, 2, generator=g) * torch.tensor([RAW[1] - 1.0, RAW[0] - 1.0])).to(dev)
    pts_out = torch.empty_like(pts)
    zero = ops.Lens(CAMERA, (0.0,) * 5)
    copies = bool(torch.equal(ops.lens_frames(frames, zero, out=out), frames)) and \
        bool(torch.equal(ops.lens_frames(frames, zero, to="sensor", out=out), frames))
    diff = (torch_remap(frames, grid_).int() - ops.lens_frames(frames, lens, out=out).int()).abs()
    calls = {"copy": lambda: out.copy_(frames), "warp": lambda: ops.warp_frames(frames, eye2, out=out),
             "planes": lambda: ops.warp_planes(frames, eye3, out=out), "lens_ideal": lambda: ops.lens_frames(frames, lens, out=out),
             "lens_sensor": lambda: ops.lens_frames(frames, lens, to="sensor", out=out), "torch": lambda: torch_remap(frames, grid_),
             "points": lambda: ops.lens_points(pts, lens, out=pts_out)}
    gpu_ms = {k: [] for k in KINDS}
    for _ in range(reps + 1):
        for kind in KINDS:
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            calls[kind]()
            b.record()
            b.synchronize()
            gpu_ms[kind].append(a.elapsed_time(b))
    line = {"launch_protocol": "copy / warp (identity) / planes (identity) / lens_ideal / lens_sensor / torch / points over eight 1080p "
                               "channels-last pictures, alternating in one process, each between two HIP events after a device "
                               "synchronise; the first of each kind is left out",
            "launch_frames": STEP, "launch_bytes_in_plus_out": 2 * STEP * RAW[0] * RAW[1] * 3, "points_shape": list(pts.shape)}
    for k, v in gpu_ms.items():
        v = v[1:]
        line[f"{k}_gpu_ms_median"] = round(statistics.median(v), 4)
        line[f"{k}_gpu_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    line["launch_evaluations_timed"] = reps
    spread = max(line[f"{k}_gpu_ms_min_max"][1] - line[f"{k}_gpu_ms_min_max"][0] for k in ("planes", "lens_ideal"))
    line["lens_ideal_minus_planes_gpu_ms"] = round(line["lens_ideal_gpu_ms_median"] - line["planes_gpu_ms_median"], 4)
    line["single_evaluation_spread_gpu_ms"] = round(spread, 4)
    line["lens_ideal_no_slower_than_planes_beyond_the_spread"] = bool(line["lens_ideal_minus_planes_gpu_ms"] <= spread)
    line["ratio_lens_ideal_over_copy"] = round(line["lens_ideal_gpu_ms_median"] / line["copy_gpu_ms_median"], 3)
    line["ratio_torch_over_lens_ideal"] = round(line["torch_gpu_ms_median"] / line["lens_ideal_gpu_ms_median"], 3)
    line["ratio_lens_sensor_over_lens_ideal"] = round(line["lens_sensor_gpu_ms_median"] / line["lens_ideal_gpu_ms_median"], 3)
    line["lens_ideal_vs_torch_max_grey_levels"] = int(diff.max())
    line["zero_lens_copies_bit_for_bit"] = copies
    return line


def bench_line(dev, precision, passes, calls, reps):
    from cotracker_amd import ops
    p, raw = setup(dev, precision)
    lens = ops.Lens(CAMERA, ACTION)
    stream = make_rows(p, raw, dev, lens)
    for row in ROWS:  # warm every row: weights packed, graphs captured
        stream(row, 3, NoTimer())
    ms, last = {r: [] for r in ROWS}, {}
    for _ in range(passes):
        for row in ROWS:
            last[row] = stream(row, calls, Timer(ms[row], 2))
    zero = stream("lens", calls, NoTimer(), lens_of_row=ops.Lens(CAMERA, (0.0,) * 5))
    same = all(torch.equal(ta, tb) and torch.equal(va, vb) for (ta, va), (tb, vb) in zip(last["plain"], zero))
    med = {r: statistics.median(v) for r, v in ms.items()}
    line = {"workload": "c4_one_set_push_u8_1080p", "points": POINTS, "frames": list(HW), "raw_frames": list(RAW), "window_len": S, "iters": 6,
            "precision": precision, "hip_graph": True, "camera": list(CAMERA), "coefficients": list(ACTION),
            "passes": passes, "calls_per_pass": calls, "timed_calls_per_row": len(ms["plain"]),
            "protocol": "rows alternate pass by pass in one process; every call (the push) between two HIP events; median over the calls "
                        "after the first two windows of each pass",
            "libctk_sha256": lib_sha()}
    for r in ROWS:
        line["ms_" + r] = round(med[r], 3)
        line["min_max_ms_" + r] = [round(min(ms[r]), 3), round(max(ms[r]), 3)]
    line["ms_lens_minus_plain"] = round(med["lens"] - med["plain"], 3)
    line["ratio_lens_over_plain"] = round(med["lens"] / med["plain"], 4)
    line["spread_plain_max_minus_min_ms"] = round(max(ms["plain"]) - min(ms["plain"]), 3)
    line["zero_lens_stream_equals_plain_bit_for_bit"] = bool(same)
    line.update(launch_line(raw, reps, dev, lens))
    line["range_fallbacks"] = int(sum(x_.model.range_fallbacks for x_ in stream.preds.values()))
    line["conditions_hold"] = bool(same and line["zero_lens_copies_bit_for_bit"])
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3, help="stream passes per row")
    ap.add_argument("--calls", type=int, default=8, help="calls per pass")
    ap.add_argument("--reps", type=int, default=14, help="launches of each kind that are timed")
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f32"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens_bench.json"), help="append the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    line = bench_line(dev, args.precision, max(1, args.passes), max(4, args.calls), max(14, args.reps))
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
    if line.get("conditions_hold") is False:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
