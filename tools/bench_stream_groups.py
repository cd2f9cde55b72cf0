#!/usr/bin/env python
"""Streaming query groups (model.stream_groups) against G separate streams, measured OUTSIDE bench.py:

    python tools/bench_stream_groups.py [--workload c4x4|small16|all] [--passes 3] [--calls 6] [--precision f16x3|f32] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_stream_groups.py --trace ROW --workload W --calls K
    python tools/bench_stream_groups.py --trace-summary OUT_A OUT_B --calls K_A K_B --row ROW --workload W [--out FILE]

Two shapes on the cotracker3_online model (window 16, 384 x 512 frames, window graph on, iters = 6):
  c4x4     4 groups x 1024 points (a 32 x 32 grid each, shifted per group): four C4 streams over one video;
  small16  16 groups x 101 points (1 point + 6 x 6 support grid + 8 x 8 grid): sixteen single-object trackers.
Three rows -- separate (G models, each streaming its own query set: G encoder runs and G window graphs per chunk), loop (one grouped
stream, batch_mode "loop") and joint (batch_mode "joint": shared-pyramid joint windows, one graph per sub-batch) -- stream the same
resident video IN ONE PROCESS, ALTERNATING pass by pass; every chunk call lies between two HIP events; ms_* is the median over the
calls after the first two windows of every pass.  encoder_ms: the encoder alone on one chunk (median), encoder_share_* = encoder
time of the row's call / ms of the row.  One JSON line per workload, with the library's sha256.

--trace runs ONE row alone for a kernel trace (no counters in that run); --trace-summary takes two such traces of K_A < K_B calls:
kernels per steady-state call = (rows_B - rows_A) / (K_B - K_A), and, minus the kernel nodes of the window graphs the row replays
per call, the launches OUTSIDE the window graph per call (encoder and pyramid included), by kernel name.
"""
import argparse
import copy
import csv
import glob
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROWS = ("separate", "loop", "joint")
S, HW, ITERS = 16, (384, 512), 6


def grid(n, shift):
    ys, xs = torch.meshgrid(torch.linspace(20, HW[0] - 21, n), torch.linspace(20, HW[1] - 21, n), indexing="ij")
    return torch.stack([torch.zeros(n * n), xs.reshape(-1) + shift, ys.reshape(-1) + shift], dim=1)


def queries(name):
    if name == "c4x4":
        return torch.stack([grid(32, 2.0 * g) for g in range(4)])
    g_ = torch.Generator().manual_seed(3)
    out = []
    for g in range(16):
        pt = torch.cat([torch.zeros(1, 1), torch.rand(1, 2, generator=g_) * torch.tensor([HW[1] - 1.0, HW[0] - 1.0])], dim=1)
        out.append(torch.cat([pt, grid(6, 0.0), grid(8, 0.5 * g)]))
    return torch.stack(out)


def setup(name, dev, precision):
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
    m.hip_graph, m.stream_groups = True, True
    return m, queries(name).to(dev), synthetic_video


def make_rows(m, q):
    G = q.shape[0]
    singles = []

    def stream(row, video, calls, on_call):
        step = S // 2
        if row == "separate":
            while len(singles) < G:
                singles.append(copy.deepcopy(m))
            models = singles
        else:
            m.batch_mode = "joint" if row == "joint" else "loop"
            models = [m]
        for x in models:
            x.init_video_online_processing()
        for i in range(calls):
            chunk = video[:, i * step:i * step + S]
            with on_call(i):
                if row == "separate":
                    out = [x(chunk, q[g:g + 1], iters=ITERS, is_online=True)[0] for g, x in enumerate(models)]
                else:
                    out = [m(chunk, q, iters=ITERS, is_online=True)[0]]
        for x in models:
            x._resolve_deferred_range_check()
        return torch.cat(out)
    return stream


class Timer:
    def __init__(self, sink, skip):
        self.sink, self.skip = sink, skip

    def __call__(self, i):
        self.i = i
        return self

    def __enter__(self):
        self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.a.record()

    def __exit__(self, *exc):
        self.b.record()
        self.b.synchronize()
        if self.i >= self.skip:
            self.sink.append(self.a.elapsed_time(self.b))
        return False


class NoTimer:
    def __call__(self, i):
        return self

    def __enter__(self):
        pass

    def __exit__(self, *exc):
        return False


def lib_sha():
    from cotracker_amd import _lib
    return hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()


def graph_nodes(m):
    return sum(g.nodes for g in m._graphs.values())


def bench_line(name, dev, precision, passes, calls):
    m, q, synthetic_video = setup(name, dev, precision)
    G, N = q.shape[:2]
    video = synthetic_video(S + (calls - 1) * (S // 2), *HW, seed=1234).to(dev)
    stream = make_rows(m, q)
    for row in ROWS:  # warm every row: weights packed, graphs captured
        stream(row, video, 3, NoTimer())
    ms, last = {r: [] for r in ROWS}, {}
    for _ in range(passes):
        for row in ROWS:
            last[row] = stream(row, video, calls, Timer(ms[row], 2))
    enc = []
    for i in range(7):
        with Timer(enc, 0)(i):
            m._encode(video[0, :S].float(), 200)
    enc_ms = statistics.median(enc[2:])
    med = {r: statistics.median(v) for r, v in ms.items()}
    line = {"workload": name, "groups": G, "points_per_group": N, "frames": list(HW), "window_len": S, "iters": ITERS,
            "precision": precision, "hip_graph": True, "passes": passes, "calls_per_pass": calls, "timed_calls_per_row": len(ms["loop"]),
            "protocol": "rows alternate pass by pass in one process; every chunk call between two HIP events; median over the calls "
                        "after the first two windows of each pass",
            "libctk_sha256": lib_sha(), "encoder_ms": round(enc_ms, 3), "range_fallbacks": int(m.range_fallbacks)}
    for r in ROWS:
        line["ms_" + r] = round(med[r], 3)
        line["min_max_ms_" + r] = [round(min(ms[r]), 3), round(max(ms[r]), 3)]
        line["encoder_share_" + r] = round(enc_ms * (G if r == "separate" else 1) / med[r], 4)
    for r in ROWS[1:]:
        line["ratio_" + r] = round(med[r] / med["separate"], 4)
        line[f"max_abs_diff_{r}_px"] = float((last[r].double() - last["separate"].double()).abs().max())
    line["joint_beats_separate"] = bool(med["joint"] < med["separate"])
    torch.cuda.empty_cache()
    return line


def trace_run(name, dev, precision, row, calls):
    m, q, synthetic_video = setup(name, dev, precision)
    video = synthetic_video(S + (calls - 1) * (S // 2), *HW, seed=1234).to(dev)
    stream = make_rows(m, q)
    out = stream(row, video, calls, NoTimer())
    torch.cuda.synchronize()
    print(json.dumps({"trace": row, "workload": name, "calls": calls, "finite": bool(torch.isfinite(out).all())}))


def short(name):
    """`void (anonymous namespace)::stream_begin_kernel(int, ...)` / a mangled `_ZN12_GLOBAL__N_1...` -> the bare kernel name."""
    import re
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    m_ = re.match(r"_ZN12_GLOBAL__N_1(\d+)", name)
    if m_:
        k = int(m_.group(1))
        return name[m_.end():m_.end() + k]
    name = re.split(r"[(<]", name, maxsplit=1)[0]
    return name.split("::")[-1] or "?"


def kernel_rows(d):
    names = {}
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {d}")
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                n = short(r["Kernel_Name"])
                names[n] = names.get(n, 0) + 1
    return names


def trace_summary(name, dev, precision, row, dirs, calls):
    (da, db), (ka, kb) = dirs, calls
    a, b = kernel_rows(da), kernel_rows(db)
    per_call = {n: (b.get(n, 0) - a.get(n, 0)) / (kb - ka) for n in sorted(set(a) | set(b))}
    per_call = {n: v for n, v in per_call.items() if v}
    # the kernel nodes the row replays per call: the graphs a short run of the row leaves behind (not under the profiler)
    m, q, synthetic_video = setup(name, dev, precision)
    video = synthetic_video(S + 2 * (S // 2), *HW, seed=1234).to(dev)
    G = q.shape[0]
    if row == "separate":
        one = copy.deepcopy(m)
        one.init_video_online_processing()
        one(video[:, :S], q[:1], iters=ITERS, is_online=True)
        one._resolve_deferred_range_check()
        nodes, graphs = graph_nodes(one) * G, G
    else:
        make_rows(m, q)(row, video, 2, NoTimer())
        nodes, graphs = graph_nodes(m), len(m._graphs)
    total = sum(per_call.values())
    stream_k = {n: v for n, v in per_call.items() if "stream_" in n}
    return {"trace_summary": row, "workload": name, "groups": G, "calls": [ka, kb], "kernels_per_call": round(total, 2),
            "graph_launches_per_call": graphs, "graph_kernel_nodes_per_call": nodes,
            "launches_outside_graph_per_call": round(total - nodes, 2), "stream_kernels_per_call": stream_k,
            "libctk_sha256": lib_sha(), "kernels_per_call_by_name": {n: round(v, 2) for n, v in per_call.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["c4x4", "small16", "all"])
    ap.add_argument("--passes", type=int, default=3, help="stream passes per row")
    ap.add_argument("--calls", type=int, nargs="+", default=[6], help="chunk calls per pass (two values with --trace-summary)")
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f32"])
    ap.add_argument("--trace", default=None, choices=ROWS, help="run this row alone, for rocprofv3 --kernel-trace")
    ap.add_argument("--trace-summary", nargs=2, default=None, metavar=("OUT_A", "OUT_B"))
    ap.add_argument("--row", default="joint", choices=ROWS)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    names = ["c4x4", "small16"] if args.workload == "all" else [args.workload]
    for name in names:
        if args.trace:
            trace_run(name, dev, args.precision, args.trace, args.calls[0])
            continue
        if args.trace_summary:
            line = trace_summary(name, dev, args.precision, args.row, args.trace_summary, args.calls)
        else:
            line = bench_line(name, dev, args.precision, max(1, args.passes), max(3, args.calls[0]))
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
