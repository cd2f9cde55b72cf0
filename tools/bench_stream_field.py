#!/usr/bin/env python
"""A mask carried along the tracked points of a live stream on the device (CoTrackerOnlinePredictor.pin / propagate), measured
OUTSIDE bench.py with the conventions of bench_stream_stabilize.py:

    python tools/bench_stream_field.py [--passes 3] [--calls 8] [--precision f16x3|f32] [--out profiles/stream_field_bench.json]

The C4 shape on the online predictor (window 16, 384 x 512 model resolution, iters 6, window graph on), ONE query set of 1024
points, fed by push_frames with 1080 x 1920 uint8 channels-last frames, eight per call (sixteen for the first window):
  plain      the push only;
  propagate  the push plus propagate() of a 1080p mask, pinned on the first frame of the stream after the first window, onto the
             eight frames just pushed, into a buffer allocated once (cell 16, radius 2) -- inside the timed call.
The rows run IN ONE PROCESS, ALTERNATING pass by pass; every call lies between two HIP events; ms_* is the median over the calls
after the first two windows of every pass, with the smallest and largest single call next to it: propagate - plain is to be read
against that spread.  Then, between the calls of one stream and alternating, for the eight newest frames against the pinned one: the
stream time (HIP events) of
  field  the stream's field() (ctk_track_field: three launches) from the resident history;
  warp   ops.warp_field of the mask through those fields (one launch);
  flow   ops.warp_field's flow output alone (one launch);
  torch  a torch chain of the same job on the emitted rows: tent weights and integer sums scattered onto the node grid with
         index_add_ (int64: deterministic), a divide, F.interpolate to the picture, grid_sample(bilinear) of the mask -- no hole
         filling, so it does less.
What must hold: `propagate` returns the tracks of `plain` bit for bit (it only reads the stream state).  No time is gated: no ratio is
fixed in advance."""

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

ROWS = ("plain", "propagate")
KINDS = ("field", "warp", "flow", "torch")
CELL, RADIUS = 16, 2


def make_rows(p, raw, dev):
    """One predictor per row (a row keeps its stream state, its buffers and its graph between passes)."""
    preds = {}
    scale = torch.tensor([1.0, (RAW[1] - 1) / (HW[1] - 1), (RAW[0] - 1) / (HW[0] - 1)])
    carried = torch.empty(STEP, *RAW, dtype=torch.uint8, device=dev)
    mask = (torch.rand(RAW, device=dev) > 0.5).to(torch.uint8) * 255

    def stream(row, calls, on_call, after_call=None):
        if row not in preds:
            preds[row] = copy.deepcopy(p)
        x = preds[row]
        x(torch.zeros(1, 1, 3, *RAW, device=dev), is_first_step=True, queries=(grid(32, 0.0) * scale)[None].to(dev))
        outs, anchor = [], None
        for i in range(calls):
            t0 = (i % 6) * STEP
            new = raw[t0:t0 + S] if i == 0 else raw[t0 + S - STEP:t0 + S]
            with on_call(i):
                out = x.push_frames(new)
                if row == "propagate":
                    if anchor is None:
                        anchor = x.pin(frame=0)
                    x.propagate(mask, anchor, n=STEP, cell=CELL, radius=RADIUS, out=carried)
            outs.append((out[0].clone(), out[1].clone()))
            if after_call is not None:
                after_call(x, i, mask)
        x.finish()
        return outs
    stream.preds = preds
    return stream


def torch_chain(tracks, visible, src_row, mask, cs, radius):
    """tracks [F,N,2] raw pixels, visible [F,N], src_row = (positions [N,2], visible [N]) -> the mask carried onto the F frames."""
    H, W = mask.shape
    c = 1 << cs
    gh, gw = ((H - 1) >> cs) + 2, ((W - 1) >> cs) + 2
    F_, N = tracks.shape[:2]
    P, Q = torch.round(tracks * 16).long(), torch.round(src_row[0] * 16).long()[None]
    ok = visible.bool() & src_row[1].bool()[None]
    d = Q - P
    rad = radius * c * 16
    sums = torch.zeros(F_, gh * gw, 3, dtype=torch.int64, device=tracks.device)
    i0, j0 = P[..., 0] // (c * 16), P[..., 1] // (c * 16)
    frame = torch.arange(F_, device=tracks.device)[:, None].expand(F_, N)
    for dj in range(-radius + 1, radius + 1):
        for di in range(-radius + 1, radius + 1):
            i, j = i0 + di, j0 + dj
            wx = (1024 - ((P[..., 0] - i * c * 16).abs() * 1024) // rad).clamp(min=0)
            wy = (1024 - ((P[..., 1] - j * c * 16).abs() * 1024) // rad).clamp(min=0)
            w = wx * wy * (ok & (i >= 0) & (i < gw) & (j >= 0) & (j < gh))
            at = (frame * (gh * gw) + j.clamp(0, gh - 1) * gw + i.clamp(0, gw - 1)).reshape(-1)
            sums.view(-1, 3).index_add_(0, at, torch.stack([w, w * d[..., 0], w * d[..., 1]], dim=-1).reshape(-1, 3))
    field = (sums[..., 1:].double() / sums[..., :1].clamp(min=1).double() / 16.0).float().reshape(F_, gh, gw, 2).permute(0, 3, 1, 2)
    dense = torch.nn.functional.interpolate(field, ((gh - 1) * c + 1, (gw - 1) * c + 1), mode="bilinear", align_corners=True)[..., :H, :W]
    ys, xs = torch.meshgrid(torch.arange(H, device=mask.device, dtype=torch.float32), torch.arange(W, device=mask.device, dtype=torch.float32),
                            indexing="ij")
    g = torch.stack([(xs + dense[:, 0]) * (2.0 / (W - 1)) - 1.0, (ys + dense[:, 1]) * (2.0 / (H - 1)) - 1.0], dim=-1)
    y = torch.nn.functional.grid_sample(mask[None, None].float().expand(F_, 1, H, W), g, mode="bilinear", padding_mode="zeros", align_corners=True)
    return y[:, 0].round().clamp(0, 255).to(torch.uint8)


def launch_line(stream, reps, dev):
    """Between the calls of one `plain` stream: the launches alone, alternating."""
    from cotracker_amd import ops
    gpu_ms = {k: [] for k in KINDS}
    out = torch.empty(STEP, *RAW, dtype=torch.uint8, device=dev)
    flow = torch.empty(STEP, *RAW, 2, dtype=torch.float32, device=dev)
    kept, worst, levels = {}, [0.0], []
    cs = CELL.bit_length() - 1

    def after_call(x, i, mask):
        if i == 0:
            kept["anchor"] = x.pin(frame=0)
        if i < 2:
            return
        gs, scale = x._running("bench")
        done = gs.committed
        kw = dict(size=RAW, cell=CELL, radius=RADIUS, anchor=kept["anchor"], N_out=x.N, scale=scale, thresh=0.6, first_row=x._emit_first_row(), group=0)
        field, _, stats = x.model.stream_field(done - STEP, STEP, **kw)
        levels.append(int(stats[0, :, 2].max()))
        tracks, visible = x._emit_result(done - STEP, done)
        src = x._emit_result(0, 1)
        ours = ops.warp_field(mask[None].expand(STEP, *RAW), field[0], cell=CELL, out=out)
        theirs = torch_chain(tracks[0], visible[0], (src[0][0, 0], src[1][0, 0]), mask, cs, RADIUS)
        worst[0] = max(worst[0], float((ours.int() - theirs.int()).abs().float().mean()))
        a_flow, _, _ = ops._warp_field_args(None, RAW, CELL, "fill", (0, 0, 0), None, flow, None, STEP, "bench", device=dev)
        calls = {"field": lambda: x.model.stream_field(done - STEP, STEP, **kw),
                 "warp": lambda: ops.warp_field(mask[None].expand(STEP, *RAW), field[0], cell=CELL, out=out),
                 "flow": lambda: ops._warp_field_launch(a_flow, field[0], "bench"),
                 "torch": lambda: torch_chain(tracks[0], visible[0], (src[0][0, 0], src[1][0, 0]), mask, cs, RADIUS)}
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
    line = {"launch_protocol": "field / warp / flow / torch for the eight newest 1080p frames against the pinned first frame, alternating "
                               "between the calls of one stream, each between two HIP events after a device synchronise; the first of each "
                               "kind is left out",
            "launch_frames": STEP, "cell": CELL, "radius": RADIUS}
    for k, v in gpu_ms.items():
        v = v[1:]
        line[f"{k}_gpu_ms_median"] = round(statistics.median(v), 4)
        line[f"{k}_gpu_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    line["launch_evaluations_timed"] = len(gpu_ms["warp"]) - 1
    ours = line["field_gpu_ms_median"] + line["warp_gpu_ms_median"]
    line["field_plus_warp_gpu_ms"] = round(ours, 4)
    line["ratio_torch_over_field_plus_warp"] = round(line["torch_gpu_ms_median"] / ours, 3)
    line["ours_beats_torch_beyond_the_spread"] = bool(line["field_gpu_ms_min_max"][1] + line["warp_gpu_ms_min_max"][1] < line["torch_gpu_ms_min_max"][0])
    line["mask_vs_torch_mean_grey_levels"] = round(worst[0], 3)
    line["highest_pyramid_level_used"] = max(levels)
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
            "precision": precision, "hip_graph": True, "passes": passes, "calls_per_pass": calls, "timed_calls_per_row": len(ms["plain"]),
            "protocol": "rows alternate pass by pass in one process; every call (the push and what follows it) between two HIP events; "
                        "median over the calls after the first two windows of each pass",
            "libctk_sha256": lib_sha()}
    for r in ROWS:
        line["ms_" + r] = round(med[r], 3)
        line["min_max_ms_" + r] = [round(min(ms[r]), 3), round(max(ms[r]), 3)]
    line["ratio_propagate_over_plain"] = round(med["propagate"] / med["plain"], 4)
    line["ms_propagate_minus_plain"] = round(med["propagate"] - med["plain"], 3)
    line["spread_plain_max_over_min"] = round(max(ms["plain"]) / min(ms["plain"]), 4)
    line["spread_plain_max_minus_min_ms"] = round(max(ms["plain"]) - min(ms["plain"]), 3)
    same = all(torch.equal(ta, tb) and torch.equal(va, vb) for (ta, va), (tb, vb) in zip(last["plain"], last["propagate"]))
    line["propagate_equals_plain_bit_for_bit"] = bool(same)
    line.update(launch_line(stream, reps, dev))
    line["range_fallbacks"] = int(sum(x_.model.range_fallbacks for x_ in stream.preds.values()))
    line["conditions_hold"] = bool(same)
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3, help="stream passes per row")
    ap.add_argument("--calls", type=int, default=8, help="calls per pass")
    ap.add_argument("--reps", type=int, default=6, help="launches of each kind timed after every call of one plain stream (3 calls)")
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f32"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_field_bench.json"), help="append the JSON line to this file")
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
