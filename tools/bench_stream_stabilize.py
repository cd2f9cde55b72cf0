#!/usr/bin/env python
"""The frames of a live stream steadied on the device (CoTrackerOnlinePredictor.stabilize), measured OUTSIDE bench.py with the
conventions of bench_stream_motion.py:

    python tools/bench_stream_stabilize.py [--passes 3] [--calls 8] [--precision f16x3|f32] [--out profiles/stream_stabilize_bench.json]

The C4 shape on the online predictor (window 16, 384 x 512 model resolution, iters 6, window graph on), ONE query set of 1024
points, fed by push_frames with 1080 x 1920 uint8 channels-last frames, eight per call (sixteen for the first window):
  plain      the push only;
  stabilize  the push plus stabilize() of the eight frames just pushed into a buffer allocated once (similarity, 128 hypotheses,
             alpha 0.1, zoom 1.1) -- inside the timed call.
The rows run IN ONE PROCESS, ALTERNATING pass by pass; every call lies between two HIP events; ms_* is the median over the calls
after the first two windows of every pass, with the smallest and largest single call next to it: stabilize - plain is to be read
against that spread.  Then, between the calls of one stream and alternating, over eight 1080p channels-last pictures and the matrices
the stream's own stabilize() call produced: the stream time (HIP events) of
  copy   out.copy_(frames): the memory bound for these bytes on this machine;
  torch  uint8 -> float, affine_grid, grid_sample(bilinear, align_corners=True), round, -> uint8: what a caller writes today;
  warp   ops.warp_frames, one launch: the kernel the library ships, which stages a tile's source box in LDS;
  direct the same call through the direct form of the kernel (byte loads from memory, no LDS), which only the dev build of the
         library carries (ctk_debug_warp_frames_direct; `make dev`): the measurement behind the decision recorded in DESIGN.md;
  path   ops.smooth_path over the eight motions, one launch.

What must hold: `stabilize` returns the tracks of `plain` bit for bit (it only reads the stream state), and `direct` writes the bytes of
`warp`.  The largest difference between
warp and torch's float32 result is recorded, in grey levels.  No time is gated: no ratio is fixed in advance."""

import argparse
import copy
import ctypes as C
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

ROWS = ("plain", "stabilize")
KINDS = ("copy", "torch", "warp", "direct", "path")
ALPHA, ZOOM = 0.1, 1.1


def make_rows(p, raw, dev):
    """One predictor per row (a row keeps its stream state, its buffers and its graph between passes)."""
    preds = {}
    scale = torch.tensor([1.0, (RAW[1] - 1) / (HW[1] - 1), (RAW[0] - 1) / (HW[0] - 1)])
    steady = torch.empty(STEP, *RAW, 3, dtype=torch.uint8, device=dev)

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
                if row == "stabilize":
                    x.stabilize(new[-STEP:], alpha=ALPHA, zoom=ZOOM, out=steady)
            outs.append((out[0].clone(), out[1].clone()))
            if after_call is not None:
                after_call(x, i, new[-STEP:])
        x.finish()
        return outs
    stream.preds = preds
    return stream


def torch_theta(warp, H, W):
    """Pixel matrices (output pixel -> source position) -> affine_grid's theta for align_corners=True, in float64 on the host."""
    to_px = torch.tensor([[(W - 1) / 2, 0, (W - 1) / 2], [0, (H - 1) / 2, (H - 1) / 2], [0, 0, 1]], dtype=torch.float64)
    full = torch.cat([warp.double().cpu(), torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand(warp.shape[0], 1, 3)], dim=1)
    return (torch.linalg.inv(to_px) @ full @ to_px)[:, :2].float()


def torch_warp(frames, theta):
    x = frames.permute(0, 3, 1, 2).float()
    g = torch.nn.functional.affine_grid(theta, list(x.shape), align_corners=True)
    y = torch.nn.functional.grid_sample(x, g, mode="bilinear", padding_mode="zeros", align_corners=True)
    return y.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def launch_line(stream, reps, dev):
    """Between the calls of one `plain` stream: the launches alone, alternating."""
    from cotracker_amd import ops
    gpu_ms = {k: [] for k in KINDS}
    worst, seen = [0], []
    out, out2 = (torch.empty(STEP, *RAW, 3, dtype=torch.uint8, device=dev) for _ in range(2))
    # the direct form of the warp kernel lives in the dev build of the library only (make dev): the same arguments, the same bytes
    dev_lib = C.CDLL(os.path.join(ROOT, "co-tracker_amd", "libctk_hip_dev.so"))
    dev_lib.ctk_debug_warp_frames_direct.restype, dev_lib.ctk_debug_warp_frames_direct.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    same_bytes = []

    def after_call(x, i, frames):
        if i < 2:
            return
        _, warp = x.stabilize(frames, alpha=ALPHA, zoom=ZOOM, out=out, reset=True)
        motion = x.camera_motion(STEP)[0][:1].contiguous()
        theta = torch_theta(warp, *RAW).to(dev)
        state = ops.smooth_path(motion, alpha=ALPHA)[1]
        args, _ = ops._warp_args(frames, out2, "fill", (0, 0, 0), None, "direct")
        args.matrices = warp.data_ptr()
        stream_h = torch.cuda.current_stream().cuda_stream
        assert dev_lib.ctk_debug_warp_frames_direct(C.byref(args), stream_h) == 0
        same_bytes.append(bool(torch.equal(out2, ops.warp_frames(frames, warp, out=out))))
        diff = (torch_warp(frames, theta).int() - ops.warp_frames(frames, warp, out=out).int()).abs()
        worst[0] = max(worst[0], int(diff.max()))
        seen.append(float((warp - torch.tensor([[1.0, 0, 0], [0, 1.0, 0]], device=dev)).abs().amax()))
        calls = {"copy": lambda: out.copy_(frames), "torch": lambda: torch_warp(frames, theta),
                 "warp": lambda: ops.warp_frames(frames, warp, out=out),
                 "direct": lambda: dev_lib.ctk_debug_warp_frames_direct(C.byref(args), stream_h), "path": lambda: ops.smooth_path(motion, state, alpha=ALPHA)}
        for _ in range(reps):
            for kind in KINDS:
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                calls[kind]()
                b.record()
                b.synchronize()
                gpu_ms[kind].append(a.elapsed_time(b))
    stream("plain", 5, NoTimer(), after_call)
    line = {"launch_protocol": "copy / torch / warp / direct / path over the eight newest 1080p channels-last pictures with the matrices the stream's "
                               "own stabilize() produced, alternating between the calls of one stream, each between two HIP events after "
                               "a device synchronise; the first of each kind is left out",
            "launch_frames": STEP, "launch_bytes_in_plus_out": 2 * STEP * RAW[0] * RAW[1] * 3}
    for k, v in gpu_ms.items():
        v = v[1:]
        line[f"{k}_gpu_ms_median"] = round(statistics.median(v), 4)
        line[f"{k}_gpu_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    line["launch_evaluations_timed"] = len(gpu_ms["warp"]) - 1
    line["ratio_warp_over_copy"] = round(line["warp_gpu_ms_median"] / line["copy_gpu_ms_median"], 3)
    line["ratio_torch_over_warp"] = round(line["torch_gpu_ms_median"] / line["warp_gpu_ms_median"], 3)
    line["warp_beats_torch_beyond_the_spread"] = bool(line["warp_gpu_ms_min_max"][1] < line["torch_gpu_ms_min_max"][0])
    line["warp_vs_torch_max_grey_levels"] = worst[0]
    # the staged-variant decision: the staged kernel is kept only if its median lies below the direct form's by more than the spread
    # of single evaluations
    spread = max(line[f"{k}_gpu_ms_min_max"][1] - line[f"{k}_gpu_ms_min_max"][0] for k in ("warp", "direct"))
    line["direct_equals_warp_bit_for_bit"] = all(same_bytes)
    line["direct_minus_warp_gpu_ms"] = round(line["direct_gpu_ms_median"] - line["warp_gpu_ms_median"], 4)
    line["single_evaluation_spread_gpu_ms"] = round(spread, 4)
    line["staged_wins_beyond_the_spread"] = bool(line["direct_minus_warp_gpu_ms"] > spread)
    line["largest_matrix_entry_off_identity"] = round(max(seen), 3)
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
            "precision": precision, "hip_graph": True, "model": "similarity", "hypotheses": 128, "alpha": ALPHA, "zoom": ZOOM,
            "passes": passes, "calls_per_pass": calls, "timed_calls_per_row": len(ms["plain"]),
            "protocol": "rows alternate pass by pass in one process; every call (the push and what follows it) between two HIP events; "
                        "median over the calls after the first two windows of each pass",
            "libctk_sha256": lib_sha()}
    for r in ROWS:
        line["ms_" + r] = round(med[r], 3)
        line["min_max_ms_" + r] = [round(min(ms[r]), 3), round(max(ms[r]), 3)]
    line["ratio_stabilize_over_plain"] = round(med["stabilize"] / med["plain"], 4)
    line["ms_stabilize_minus_plain"] = round(med["stabilize"] - med["plain"], 3)
    line["spread_plain_max_over_min"] = round(max(ms["plain"]) / min(ms["plain"]), 4)
    line["spread_plain_max_minus_min_ms"] = round(max(ms["plain"]) - min(ms["plain"]), 3)
    same = all(torch.equal(ta, tb) and torch.equal(va, vb) for (ta, va), (tb, vb) in zip(last["plain"], last["stabilize"]))
    line["stabilize_equals_plain_bit_for_bit"] = bool(same)
    line.update(launch_line(stream, reps, dev))
    line["range_fallbacks"] = int(sum(x_.model.range_fallbacks for x_ in stream.preds.values()))
    line["conditions_hold"] = bool(same and line["direct_equals_warp_bit_for_bit"])
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3, help="stream passes per row")
    ap.add_argument("--calls", type=int, default=8, help="calls per pass")
    ap.add_argument("--reps", type=int, default=6, help="launches of each kind timed after every call of one plain stream (3 calls)")
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f32"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_stabilize_bench.json"), help="append the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    line = bench_line(dev, args.precision, max(1, args.passes), max(4, args.calls), max(6, args.reps))
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
    if line.get("conditions_hold") is False:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
