#!/usr/bin/env python
"""Slots on a running stream (model.stream_slots), measured OUTSIDE bench.py with the conventions of bench_stream_groups.py:

    python tools/bench_stream_slots.py [--passes 3] [--calls 6] [--precision f16x3|f32] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_stream_slots.py --trace ROW --calls K
    python tools/bench_stream_slots.py --trace-summary OUT_A OUT_B --calls K_A K_B --row ROW [--out FILE]

The C4 shape on the cotracker3_online model (window 16, 384 x 512 frames, window graph on, iters = 6), ONE query set:
  glue        queries [1,1024,3], stream_slots off: the torch glue of _video_gen around the captured window graph;
  slots       the same stream with stream_slots on: the device-resident stream state, three stream launches per call;
  spare64     1024 points + 64 empty slots (1088 rows), stream_slots on;
  plain1088   1088 real points, stream_slots on -- an empty slot costs what a point costs, so spare64 should equal it.
The rows stream the same resident video IN ONE PROCESS, ALTERNATING pass by pass; every chunk call lies between two HIP events;
ms_* is the median over the calls after the first two windows of every pass.  Then the cost of an assign: a spare64 stream is
driven to ind ~ 1000 frames, and stream_assign of 1, 16 and 256 slots (queries given on the host, frames far ahead) is timed
`--assigns` times each: mean HIP-event time (the launch and the two small copies) and mean host time of the call.  The resident
form, stream_assign(resident=True) with the query on the newest tracked frame (online_ind + window_len // 2 - 1: every slot samples
its 4 x 49 x 128 support floats from the resident pyramid), is timed in the same stream, ALTERNATING with the plain one size by size;
ratio_resident_over_plain_K is the quotient of the two HIP-event means.  --assign-only skips the four stream rows.

--trace runs ONE of glue / slots alone for a kernel trace (no counters in that run); --trace-summary takes two such traces of
K_A < K_B calls: kernels per steady-state call and, minus the kernel nodes of the window graph the row replays, the launches
OUTSIDE the window graph per call, by kernel name.
"""
import argparse
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

from bench_stream_groups import HW, ITERS, NoTimer, S, Timer, graph_nodes, grid, kernel_rows, lib_sha  # noqa: E402

ROWS = ("glue", "slots", "spare64", "plain1088")
STEP = S // 2


def setup(dev, precision):
    from cotracker_amd import model as M
    from cotracker_amd.model import CoTrackerThreeOnline
    from cotracker_amd.synthetic import synthetic_video
    from cotracker_amd.weights import fill_synthetic_
    old, M.DEFAULT_PRECISION = M.DEFAULT_PRECISION, precision
    try:
        m = CoTrackerThreeOnline(window_len=S, model_resolution=HW).eval()
    finally:
        M.DEFAULT_PRECISION = old
    fill_synthetic_(m, seed=0)
    m = m.to(dev)
    m.hip_graph = True
    return m, synthetic_video(S + 5 * STEP, *HW, seed=1234).to(dev)


def queries(row, dev):
    from cotracker_amd import ops
    q = grid(32, 0.0)
    if row == "spare64":
        q = torch.cat([q, torch.tensor([ops.EMPTY_FRAME, 0.0, 0.0]).expand(64, 3)])
    if row == "plain1088":
        q = torch.cat([q, grid(8, 1.0)])
    return q[None].to(dev)


def make_rows(m, dev):
    """One model per row (a row keeps its stream state and its graph between passes, as a long-running tracker does)."""
    import copy
    models, qs = {}, {}

    def stream(row, video, calls, on_call, after_call=None):
        if row not in models:
            models[row] = copy.deepcopy(m)
            models[row].stream_slots = row != "glue"
            qs[row] = queries(row, dev)
        x, q = models[row], qs[row]
        x.init_video_online_processing()
        for i in range(calls):
            t0 = (i % 6) * STEP  # (a resident video of six chunks, walked round: what the frames show does not change the time)
            with on_call(i):
                out = x(video[:, t0:t0 + S], q, iters=ITERS, is_online=True)[0]
            if after_call is not None:
                after_call(x, i)
        x._resolve_deferred_range_check()
        return out
    stream.models = models
    return stream


def bench_line(dev, precision, passes, calls, assigns, assign_only=False):
    m, video = setup(dev, precision)
    stream = make_rows(m, dev)
    line = {"workload": "c4_one_set", "points": 1024, "frames": list(HW), "window_len": S, "iters": ITERS, "precision": precision,
            "hip_graph": True, "libctk_sha256": lib_sha()}
    if not assign_only:
        line.update(rows_line(stream, video, passes, calls))
    line.update(assign_line(stream, video, assigns))
    torch.cuda.empty_cache()
    return line


def rows_line(stream, video, passes, calls):
    for row in ROWS:  # warm every row: weights packed, graphs captured
        stream(row, video, 3, NoTimer())
    ms, last = {r: [] for r in ROWS}, {}
    for _ in range(passes):
        for row in ROWS:
            last[row] = stream(row, video, calls, Timer(ms[row], 2))
    med = {r: statistics.median(v) for r, v in ms.items()}
    line = {"passes": passes, "calls_per_pass": calls, "timed_calls_per_row": len(ms["glue"]),
            "protocol": "rows alternate pass by pass in one process; every chunk call between two HIP events; median over the calls "
                        "after the first two windows of each pass"}
    for r in ROWS:
        line["ms_" + r] = round(med[r], 3)
        line["min_max_ms_" + r] = [round(min(ms[r]), 3), round(max(ms[r]), 3)]
    line["ratio_slots_over_glue"] = round(med["slots"] / med["glue"], 4)
    line["ratio_spare64_over_plain1088"] = round(med["spare64"] / med["plain1088"], 4)
    line["slots_equals_glue_bit_for_bit"] = bool(torch.equal(last["slots"], last["glue"]))
    line["range_fallbacks"] = int(sum(x.range_fallbacks for x in stream.models.values()))

    return line


def assign_line(stream, video, assigns):
    """The cost of an assign at ind ~ 1000 frames: three sizes, plain and resident alternating, between the calls of one long
    spare64 stream."""
    sizes = (1, 16, 256)
    turns = [(k, kind) for k in sizes for kind in ("plain", "resident")]
    gpu_ms, host_ms = {t_: [] for t_ in turns}, {t_: [] for t_ in turns}
    far = torch.tensor([[1.0e6, 100.0, 100.0]]).expand(256, 3).contiguous()
    warm = 1000 // STEP

    def after_call(x, i):
        if i < warm:
            return
        k, kind = turn = turns[(i - warm) % len(turns)]
        slots = torch.arange(1088 - k, 1088)
        q = far[:k]
        if kind == "resident":  # the newest frame the stream has tracked
            q = torch.tensor([[x.online_ind + STEP - 1.0, 100.0, 100.0]]).expand(k, 3).contiguous()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        if kind == "resident":
            x.stream_assign(slots, q, resident=True)
        else:
            x.stream_assign(slots, q)
        b.record()
        host_ms[turn].append((time.perf_counter() - t0) * 1e3)
        b.synchronize()
        gpu_ms[turn].append(a.elapsed_time(b))
    stream("spare64", video, warm + assigns * len(turns), NoTimer(), after_call)
    x = stream.models["spare64"]
    line = {"assign_at_ind": int(x.online_ind), "assign_history_rows_cleared": int(x._gstream.committed),
            "assign_protocol": "plain and resident alternate size by size between the calls of one stream; HIP events around the call "
                               "(the launch and the two small copies); the first assign of each kind and size is left out of the mean"}
    for k in sizes:  # (the first assign of a stream reads the frame column of the table once: left out of the mean)
        for kind, tag in (("plain", "assign"), ("resident", "assign_resident")):
            line[f"{tag}_{k}_gpu_ms_mean"] = round(statistics.mean(gpu_ms[k, kind][1:]), 4)
            line[f"{tag}_{k}_gpu_ms_min_max"] = [round(min(gpu_ms[k, kind][1:]), 4), round(max(gpu_ms[k, kind][1:]), 4)]
            line[f"{tag}_{k}_host_ms_mean"] = round(statistics.mean(host_ms[k, kind][1:]), 4)
        line[f"ratio_resident_over_plain_{k}"] = round(statistics.mean(gpu_ms[k, "resident"][1:]) / statistics.mean(gpu_ms[k, "plain"][1:]), 4)
    line["assigns_timed_per_size"] = len(gpu_ms[1, "plain"]) - 1
    line["range_fallbacks_assign_stream"] = int(x.range_fallbacks)
    return line


def trace_run(dev, precision, row, calls):
    m, video = setup(dev, precision)
    out = make_rows(m, dev)(row, video, calls, NoTimer())
    torch.cuda.synchronize()
    print(json.dumps({"trace": row, "calls": calls, "finite": bool(torch.isfinite(out).all())}))


def trace_summary(dev, precision, row, dirs, calls):
    (da, db), (ka, kb) = dirs, calls
    a, b = kernel_rows(da), kernel_rows(db)
    per_call = {n: (b.get(n, 0) - a.get(n, 0)) / (kb - ka) for n in sorted(set(a) | set(b))}
    per_call = {n: v for n, v in per_call.items() if v}
    m, video = setup(dev, precision)  # the kernel nodes the row replays per call: the graph a short run leaves behind
    stream = make_rows(m, dev)
    stream(row, video, 2, NoTimer())
    nodes = graph_nodes(stream.models[row])
    total = sum(per_call.values())
    return {"trace_summary": row, "workload": "c4_one_set", "calls": [ka, kb], "kernels_per_call": round(total, 2),
            "graph_kernel_nodes_per_call": nodes, "launches_outside_graph_per_call": round(total - nodes, 2),
            "stream_kernels_per_call": {n: v for n, v in per_call.items() if "stream_" in n}, "libctk_sha256": lib_sha(),
            "kernels_per_call_by_name": {n: round(v, 2) for n, v in per_call.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3, help="stream passes per row")
    ap.add_argument("--calls", type=int, nargs="+", default=[6], help="chunk calls per pass (two values with --trace-summary)")
    ap.add_argument("--assigns", type=int, default=12, help="timed assigns per size")
    ap.add_argument("--assign-only", action="store_true", help="time the assigns (plain and resident) only, not the four stream rows")
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f32"])
    ap.add_argument("--trace", default=None, choices=ROWS, help="run this row alone, for rocprofv3 --kernel-trace")
    ap.add_argument("--trace-summary", nargs=2, default=None, metavar=("OUT_A", "OUT_B"))
    ap.add_argument("--row", default="slots", choices=ROWS)
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
        line = bench_line(dev, args.precision, max(1, args.passes), max(3, args.calls[0]), max(2, args.assigns) + 1, args.assign_only)
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
