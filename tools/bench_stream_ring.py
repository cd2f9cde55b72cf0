#!/usr/bin/env python
"""A stream that does not stop (CoTrackerOnlinePredictor.history_frames), measured OUTSIDE bench.py with the conventions of
bench_stream_push.py:

    python tools/bench_stream_ring.py [--late-frame 16384] [--history 64] [--precision f16x3|f32] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_stream_ring.py --trace ROW --calls K
    python tools/bench_stream_ring.py --trace-summary OUT_A OUT_B --calls K_A K_B --row ROW [--out FILE]

The C4 shape on the online predictor (window 16, 1024 points, iters 6, window graph on), ONE query set, fed by push_frames with
model-resolution float frames, eight per call (sixteen for the first window), in two modes:
  unbounded  history_frames = None: every call returns everything since frame 0 (the reference's contract);
  ring       history_frames = 64: every call returns its window's 16 rows out of a ring of 64 history rows.
Each mode is timed at two ages of the stream: calls 5 .. 25 ("early") and the 20 calls after frame --late-frame ("late").  Three
streams run IN ONE PROCESS, ALTERNATING call by call: unbounded, ring and a second unbounded one, which stops after the early
calls -- the difference of the two unbounded early medians is the run-to-run spread every comparison below is held against.
Every call lies between two HIP events; the result of a call is held until the next one replaces it.  mib_* is what the stream
itself holds on the device -- its copy of the model, its state, its last result --: the sum of the changes of
torch.cuda.memory_allocated() over its own calls (the other streams allocate only inside theirs).  ms_* is the median over the
timed calls of the row.

--trace runs ONE mode alone for a kernel trace (no counters in that run); --trace-summary takes two such traces of K_A < K_B calls:
kernels per call by name, minus the kernel nodes of the window graph the mode replays = the launches OUTSIDE the window graph per
pushed call.
"""
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

from bench_stream_groups import HW, NoTimer, S, Timer, graph_nodes, grid, kernel_rows, lib_sha  # noqa: E402
from bench_stream_push import RING as SOURCE_FRAMES  # noqa: E402
from bench_stream_push import setup  # noqa: E402

MODES = ("unbounded", "ring")
STEP = S // 2
EARLY = (5, 25)  # calls [5, 25)
LATE_CALLS = 20


class Stream:
    """One pushed stream of one mode over a resident float video that is walked round."""

    def __init__(self, p, small, dev, history):
        before = torch.cuda.memory_allocated()
        self.p, self.small, self.i, self.out = copy.deepcopy(p), small, 0, None
        self.p.history_frames = history
        self.p(torch.zeros(1, 1, 3, *HW, device=dev), is_first_step=True, queries=grid(32, 0.0)[None].to(dev))
        self.bytes = torch.cuda.memory_allocated() - before  # what THIS stream holds: the sum of the changes its own calls made

    def call(self, timer):
        t0 = (self.i % 6) * STEP
        new = self.small[0, t0:t0 + S] if self.i == 0 else self.small[0, t0 + S - STEP:t0 + S]
        before = torch.cuda.memory_allocated()
        with timer(self.i):
            self.out = self.p.push_frames(new)
        self.i += 1
        self.bytes += torch.cuda.memory_allocated() - before
        return self.bytes

    @property
    def frames(self):
        return S + (self.i - 1) * STEP if self.i else 0


def bench_line(dev, precision, history, late_frame):
    p, small, _ = setup(dev, precision)
    assert SOURCE_FRAMES == S + 5 * STEP
    warm = [Stream(p, small, dev, h) for h in (None, history)]  # weights packed; each mode's graph is captured by its own stream
    for x in warm:
        for _ in range(3):
            x.call(NoTimer())
        x.p.finish()
    del warm
    torch.cuda.empty_cache()
    rows = {"unbounded": Stream(p, small, dev, None), "ring": Stream(p, small, dev, history), "unbounded_2": Stream(p, small, dev, None)}
    ms = {f"{r}_{age}": [] for r in rows for age in ("early", "late")}
    mem = {k: [] for k in ms}
    for i in range(EARLY[1]):
        for r, x in rows.items():
            mem[r + "_early"].append(x.call(Timer(ms[r + "_early"], EARLY[0])))
    rows.pop("unbounded_2").p.finish()
    first_late = (late_frame - S) // STEP + 1  # the first call whose window starts at or after late_frame - S + STEP
    while rows["ring"].i < first_late:
        for x in rows.values():
            x.call(NoTimer())
    frames_at_late = rows["ring"].frames
    for i in range(LATE_CALLS):
        for r, x in rows.items():
            mem[r + "_late"].append(x.call(Timer(ms[r + "_late"], 0)))
    med = {k: statistics.median(v) for k, v in ms.items() if v}
    spread = abs(med["unbounded_early"] - med["unbounded_2_early"])
    line = {"workload": "c4_one_set_ring", "points": 1024, "frames": list(HW), "window_len": S, "iters": 6, "precision": precision,
            "hip_graph": True, "history_frames": history, "early_calls": list(EARLY), "late_after_frame": late_frame,
            "frames_before_first_late_call": frames_at_late, "late_calls": LATE_CALLS,
            "protocol": "three pushed streams (unbounded, ring, a second unbounded one for the early calls) alternate call by call in one "
                        "process; every call between two HIP events; median over the timed calls; mib_* = the stream's own device memory "
                        "(model copy, state, last result): the changes of memory_allocated() summed over its own calls",
            "libctk_sha256": lib_sha()}
    for k in med:
        line["ms_" + k] = round(med[k], 3)
        line["min_max_ms_" + k] = [round(min(ms[k]), 3), round(max(ms[k]), 3)]
    for k, v in mem.items():
        if v and not k.startswith("unbounded_2"):
            line["mib_" + k] = [round(v[0] / 2 ** 20, 2), round(v[-1] / 2 ** 20, 2)]  # after the first and the last call of the row
    line["spread_unbounded_early_ms"] = round(spread, 3)
    line["ring_late_minus_ring_early_ms"] = round(med["ring_late"] - med["ring_early"], 3)
    line["ring_early_minus_unbounded_early_ms"] = round(med["ring_early"] - med["unbounded_early"], 3)
    line["unbounded_late_minus_unbounded_early_ms"] = round(med["unbounded_late"] - med["unbounded_early"], 3)
    line["ring_late_within_spread_of_ring_early"] = bool(med["ring_late"] <= med["ring_early"] + spread)
    line["ring_early_within_spread_of_unbounded_early"] = bool(med["ring_early"] <= med["unbounded_early"] + spread)
    line["ring_memory_constant_from_call_10"] = bool(len(set(mem["ring_early"][10:] + mem["ring_late"])) == 1)
    # the same frames and queries: the ring's last window is the unbounded stream's last rows
    u, r = rows["unbounded"].out, rows["ring"].out
    line["ring_tracks_equal_unbounded_rows_bit_for_bit"] = bool(torch.equal(r[0], u[0][:, -S:]))
    line["ring_visibility_mismatches"] = int((r[1] != u[1][:, -S:]).sum())
    line["range_fallbacks"] = int(sum(x.p.model.range_fallbacks for x in rows.values()))
    for x in rows.values():
        x.p.finish()
    return line


def trace_run(dev, precision, history, mode, calls):
    p, small, _ = setup(dev, precision)
    x = Stream(p, small, dev, history if mode == "ring" else None)
    for _ in range(calls):
        x.call(NoTimer())
    x.p.finish()
    torch.cuda.synchronize()
    print(json.dumps({"trace": mode, "calls": calls, "finite": bool(torch.isfinite(x.out[0]).all())}))


def trace_summary(dev, precision, history, mode, dirs, calls):
    (da, db), (ka, kb) = dirs, calls
    a, b = kernel_rows(da), kernel_rows(db)
    per_call = {n: (b.get(n, 0) - a.get(n, 0)) / (kb - ka) for n in sorted(set(a) | set(b))}
    per_call = {n: v for n, v in per_call.items() if v}
    p, small, _ = setup(dev, precision)  # the kernel nodes the mode replays per call: the graph a short run leaves behind
    x = Stream(p, small, dev, history if mode == "ring" else None)
    for _ in range(2):
        x.call(NoTimer())
    x.p.finish()
    nodes = graph_nodes(x.p.model)
    total = sum(per_call.values())
    return {"trace_summary": mode, "workload": "c4_one_set_ring", "history_frames": history if mode == "ring" else None, "calls": [ka, kb],
            "kernels_per_call": round(total, 2), "graph_kernel_nodes_per_call": nodes, "launches_outside_graph_per_call": round(total - nodes, 2),
            "libctk_sha256": lib_sha(), "kernels_per_call_by_name": {n: round(v, 2) for n, v in per_call.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--late-frame", type=int, default=16384, help="the late calls are the first 20 after this many frames")
    ap.add_argument("--history", type=int, default=64, help="history_frames of the ring mode")
    ap.add_argument("--calls", type=int, nargs="+", default=[6], help="calls of a --trace run (two values with --trace-summary)")
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f32"])
    ap.add_argument("--trace", default=None, choices=MODES, help="run this mode alone, for rocprofv3 --kernel-trace")
    ap.add_argument("--trace-summary", nargs=2, default=None, metavar=("OUT_A", "OUT_B"))
    ap.add_argument("--row", default="ring", choices=MODES)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.trace:
        trace_run(dev, args.precision, args.history, args.trace, args.calls[0])
        return
    if args.trace_summary:
        line = trace_summary(dev, args.precision, args.history, args.row, args.trace_summary, args.calls)
    else:
        line = bench_line(dev, args.precision, args.history, max(args.late_frame, S + EARLY[1] * STEP))
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
