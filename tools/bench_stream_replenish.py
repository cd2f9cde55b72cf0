#!/usr/bin/env python
"""Track health and replenish on a live stream (CoTrackerOnlinePredictor.track_health / .replenish), measured OUTSIDE bench.py with
the conventions of bench_stream_slots.py:

    python tools/bench_stream_replenish.py [--passes 3] [--calls 8] [--precision f16x3|f32] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_stream_replenish.py --trace ROW --calls K
    python tools/bench_stream_replenish.py --trace-summary OUT_A OUT_B --calls K_A K_B --row ROW [--out FILE]

The C4 shape on the online predictor (window 16, 384 x 512 frames, iters 6, window graph on), ONE query set of 1024 points with 64
spare slots, fed by push_frames (eight model-resolution float frames per call, sixteen for the first window):
  plain      the stream as it is;
  health     the same stream with a track_health() after every call (it only reads: the tracks must not change);
  replenish  the same stream with a replenish(max_lost) after every call, inside the timed call;
  corners    the same with replenish(max_lost, seeds="corners"): one ctk_seed_points launch and one small copy more per call.
The rows run IN ONE PROCESS, ALTERNATING pass by pass; every call lies between two HIP events; ms_* is the median over the calls
after the first two windows of every pass, with the smallest and largest single call next to it.  Then, between the calls of one
stream: the stream time (HIP events) of the ONE health launch against a torch restatement of the same lost / cover over the same
history rows (torch_health below) and the ONE seed launch (ops.seed_points on the newest tracked frame, the health grid and bounds,
replenish's inset) on the same stream, alternating, and the host time of replenish() -- the launch, its one device-to-host copy (the
call's only wait), the host policy, the release and the resident assign.

What must hold: the health path is ONE launch (--trace-summary), `health` equals `plain` bit for bit on every point, and `replenish`
equals `plain` bit for bit on the points it did not touch for as long as it has changed nothing.  From the first seed on the other
points move too -- an occupied slot takes part in the space attention, an empty one is masked out -- so the comparison over ALL
calls is reported as measured, not required.

--trace runs `--calls` health evaluations of ONE kind (health / torch) alone on a synthetic state of the same shape, for a kernel
trace (no counters in that run); --trace-summary takes two such traces of K_A < K_B evaluations -> launches per evaluation by name.
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

from bench_stream_groups import HW, NoTimer, S, Timer, grid, kernel_rows, lib_sha  # noqa: E402

ROWS = ("plain", "health", "replenish", "corners")
STEP = S // 2
RING = S + 5 * STEP  # frames resident, walked round
POINTS, SPARE = 1024, 64
GRID, MAX_LOST, THRESH = (8, 8), 4, 0.6
BIG = torch.iinfo(torch.int32).max


def torch_health(gs, look, grid_hw, thresh, N_out, first32, bounds):
    """lost / cell / cover of ctk_stream_health with torch operators (torch's own sigmoid: equal to the kernel's outside a band of
    about 1e-6 around the threshold), over the same history rows."""
    from cotracker_amd import ops
    G, N, f1, R = gs.G, gs.N, gs.committed, gs.T_cap
    gh, gw = grid_hw
    dev = gs.queries.device
    x_lo, x_hi, y_lo, y_hi = (torch.tensor(float(b), dtype=torch.float32, device=dev) for b in bounds)
    inv_cw, inv_ch = gw / (x_hi - x_lo), gh / (y_hi - y_lo)
    rows = torch.arange(f1 - look, f1, device=dev) % R
    q = gs.queries.view(G, N, 3)[:, :N_out]
    fr = first32[:, :N_out].long()
    start = torch.maximum(fr, q[..., 0].long())
    empty = (fr == BIG) | (q[..., 0] == ops.EMPTY_FRAME)
    pending = ~empty & ((fr >= gs.next_ind) | (start >= f1))
    hc, hv, hf = (h_.index_select(1, rows)[:, :, :N_out] for h_ in gs.hist)
    x, y = hc[..., 0], hc[..., 1]

    def inside(x, y):
        return (x >= x_lo) & (x <= x_hi) & (y >= y_lo) & (y <= y_hi)

    def cell_of(x, y):
        cx = torch.floor((x - x_lo) * inv_cw).nan_to_num(0.0).clamp(0, gw - 1).long()
        cy = torch.floor((y - y_lo) * inv_ch).nan_to_num(0.0).clamp(0, gh - 1).long()
        return cy * gw + cx

    counted = torch.arange(f1 - look, f1, device=dev)[None, :, None] >= start[:, None, :]
    alive = (torch.sigmoid(hv) * torch.sigmoid(hf) > thresh) & inside(x, y) & counted
    run = (~alive & counted).flip(1).long().cumprod(1).sum(1)
    minus = torch.full_like(run, -1)
    lost = torch.where(empty, minus, torch.where(pending, torch.zeros_like(run), run))
    c_tracked = torch.where(alive[:, -1], cell_of(x[:, -1], y[:, -1]), minus)
    c_pending = torch.where(inside(q[..., 1], q[..., 2]), cell_of(q[..., 1], q[..., 2]), minus)
    cell = torch.where(empty, minus, torch.where(pending, c_pending, c_tracked))
    cover = torch.zeros(G, gh * gw + 1, dtype=torch.int64, device=dev)
    cover.scatter_add_(1, torch.where(cell < 0, torch.full_like(cell, gh * gw), cell), torch.ones_like(cell))
    return lost.int(), cell.int(), cover[:, :gh * gw].int()


def setup(dev, precision):
    from cotracker_amd import model as M
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    from cotracker_amd.synthetic import synthetic_video
    from cotracker_amd.weights import fill_synthetic_
    old, M.DEFAULT_PRECISION = M.DEFAULT_PRECISION, precision
    try:
        p = CoTrackerOnlinePredictor(checkpoint=None, window_len=S)
    finally:
        M.DEFAULT_PRECISION = old
    assert tuple(p.interp_shape) == HW
    fill_synthetic_(p.model, seed=0)
    p.spare_points = SPARE
    return p.to(dev), synthetic_video(RING, *HW, seed=1234).to(dev)  # [1,T,3,384,512] float, 0..255


def make_rows(p, video, dev):
    """One predictor per row (a row keeps its stream state, its buffers and its graph between passes)."""
    import copy
    preds = {}

    def stream(row, calls, on_call, after_call=None):
        if row not in preds:
            preds[row] = copy.deepcopy(p)
        x = preds[row]
        x(torch.zeros(1, 1, 3, *HW, device=dev), is_first_step=True, queries=grid(32, 0.0)[None].to(dev))
        outs, log = [], []
        for i in range(calls):
            t0 = (i % 6) * STEP
            with on_call(i):
                out = x.push_frames(video[0, t0:t0 + S] if i == 0 else video[0, t0 + S - STEP:t0 + S])
                if row == "health":
                    x.track_health(grid=GRID, thresh=THRESH)
                elif row == "replenish":
                    log.append(x.replenish(MAX_LOST, grid=GRID, thresh=THRESH))
                elif row == "corners":
                    log.append(x.replenish(MAX_LOST, grid=GRID, thresh=THRESH, seeds="corners"))
            outs.append((out[0].clone(), out[1].clone()))
            if after_call is not None:
                after_call(x, i)
        x.finish()
        return outs, log
    stream.preds = preds
    return stream


def compare(plain, other, log):
    """-> (every point equal over all calls, the untouched points equal over all calls, the untouched points equal up to and including
    the call behind which the first change was made, that call's index or None)."""
    touched = torch.zeros(POINTS + SPARE, dtype=torch.bool)
    first_change, all_eq, untouched_eq, untouched_eq_before = None, True, True, True
    for i, ((ta, va), (tb, vb)) in enumerate(zip(plain, other)):
        keep = (~touched).to(ta.device)
        all_eq &= bool(torch.equal(ta, tb) and torch.equal(va, vb))
        eq = bool(torch.equal(ta[:, :, keep], tb[:, :, keep]) and torch.equal(va[:, :, keep], vb[:, :, keep]))
        untouched_eq &= eq
        if first_change is None:
            untouched_eq_before &= eq
        if i < len(log):
            released, added, _ = log[i]
            if (len(released) or len(added)) and first_change is None:
                first_change = i
            touched[released[:, 1]] = True
            touched[added[:, 1]] = True
    return all_eq, untouched_eq, untouched_eq_before, first_change


def health_line(stream, reps):
    """Between the calls of one `plain` stream: the health launch against torch_health, alternating; then replenish() host time on the
    `replenish` stream (its own after-call log: what it released and seeded)."""
    from cotracker_amd import ops
    gpu_ms = {"health": [], "torch": [], "seed": []}
    agree, seeded = [], []

    def after_call(x, i):
        if i < 2:
            return
        gs = x.model._gstream
        first32 = x._emit_first_row()
        ih, iw = x.interp_shape
        args = (S, GRID, THRESH, x.N, first32, (0.0, iw - 1.0, 0.0, ih - 1.0))
        for _ in range(reps):
            for kind in ("health", "torch", "seed"):
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                if kind == "seed":
                    out = ops.seed_points(x._newest_frame, GRID, bounds=args[5], inset=max(1, int(min((iw - 1.0) / GRID[1], (ih - 1.0) / GRID[0]) // 4)))
                else:
                    out = gs.health(*args) if kind == "health" else torch_health(gs, *args)
                b.record()
                b.synchronize()
                gpu_ms[kind].append(a.elapsed_time(b))
                if kind == "health":
                    mine = out
                elif kind == "seed":
                    seeded.append(int((out[:, 0] >= 0).sum()))
                else:
                    agree.append((int((mine[0] != out[0]).sum()), int((mine[2] != out[2]).sum())))
    stream("plain", 5, NoTimer(), after_call)
    line = {"health_protocol": "the ctk_stream_health launch and the torch restatement alternate between the calls of one stream, each "
                               "between two HIP events after a device synchronise; the first pair is left out",
            "health_look": S, "health_grid": list(GRID), "health_points": POINTS + SPARE}
    for kind in ("health", "torch", "seed"):
        v = gpu_ms[kind][1:]
        line[f"{kind}_gpu_ms_median"] = round(statistics.median(v), 4)
        line[f"{kind}_gpu_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    line["ratio_torch_over_health"] = round(statistics.median(gpu_ms["torch"][1:]) / statistics.median(gpu_ms["health"][1:]), 2)
    line["health_evaluations_timed"] = len(gpu_ms["health"]) - 1
    line["ratio_seed_over_health"] = round(statistics.median(gpu_ms["seed"][1:]) / statistics.median(gpu_ms["health"][1:]), 2)
    line["seed_cells_with_a_seed_min_max"] = [min(seeded), max(seeded)]
    line["torch_lost_cover_elements_differing_max"] = [max(a[0] for a in agree), max(a[1] for a in agree)]
    return line


def bench_line(dev, precision, passes, calls, reps):
    p, video = setup(dev, precision)
    stream = make_rows(p, video, dev)
    for row in ROWS:  # warm every row: weights packed, graphs captured
        stream(row, 3, NoTimer())
    ms, last, host_ms = {r: [] for r in ROWS}, {}, []
    for _ in range(passes):
        for row in ROWS:
            last[row] = stream(row, calls, Timer(ms[row], 2))
    # host time of replenish() alone: one more pass of the replenish row with the call wrapped
    x = stream.preds["replenish"]
    orig = x.replenish

    def timed(*a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = orig(*a, **k)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        return out
    x.replenish = timed
    stream("replenish", calls, NoTimer())
    del x.replenish
    med = {r: statistics.median(v) for r, v in ms.items()}
    line = {"workload": "c4_one_set_push_spare64", "points": POINTS, "spare_points": SPARE, "frames": list(HW), "window_len": S, "iters": 6,
            "precision": precision, "hip_graph": True, "max_lost": MAX_LOST, "grid": list(GRID), "thresh": THRESH, "passes": passes,
            "calls_per_pass": calls, "timed_calls_per_row": len(ms["plain"]),
            "protocol": "rows alternate pass by pass in one process; every call (the push and what follows it) between two HIP events; "
                        "median over the calls after the first two windows of each pass",
            "libctk_sha256": lib_sha()}
    for r in ROWS:
        line["ms_" + r] = round(med[r], 3)
        line["min_max_ms_" + r] = [round(min(ms[r]), 3), round(max(ms[r]), 3)]
    line["ratio_health_over_plain"] = round(med["health"] / med["plain"], 4)
    line["ratio_replenish_over_plain"] = round(med["replenish"] / med["plain"], 4)
    line["ratio_corners_over_plain"] = round(med["corners"] / med["plain"], 4)
    line["ratio_corners_over_replenish"] = round(med["corners"] / med["replenish"], 4)
    line["corners_released_added_per_call"] = [[len(r_), len(a_)] for r_, a_, _ in last["corners"][1]]
    line["replenish_host_ms_median"] = round(statistics.median(host_ms), 4)
    line["replenish_host_ms_min_max"] = [round(min(host_ms), 4), round(max(host_ms), 4)]
    outs, log = last["replenish"]
    line["replenish_released_added_per_call"] = [[len(r_), len(a_)] for r_, a_, _ in log]
    h_all, _, _, _ = compare(last["plain"][0], last["health"][0], [])
    r_all, r_untouched, r_before, first_change = compare(last["plain"][0], outs, log)
    line["health_equals_plain_bit_for_bit"] = h_all
    line["replenish_first_change_behind_call"] = first_change
    line["replenish_untouched_equal_plain_until_first_change"] = r_before
    line["replenish_untouched_equal_plain_all_calls"] = r_untouched
    line["replenish_equals_plain_all_points_all_calls"] = r_all
    line.update(health_line(stream, reps))
    line["range_fallbacks"] = int(sum(x_.model.range_fallbacks for x_ in stream.preds.values()))
    line["conditions_hold"] = bool(h_all and r_before)
    torch.cuda.empty_cache()
    return line


def synthetic_state(dev):
    """A stream state of the workload's shape with a random history, for the kernel traces: the launches do not depend on the bytes."""
    from cotracker_amd import ops
    g = torch.Generator().manual_seed(3)
    N = POINTS + SPARE
    sizes = [(HW[0] // 4 >> l, HW[1] // 4 >> l) for l in range(4)]
    gs = ops.StreamGroups(torch.zeros(1, N, 3, device=dev), S, STEP, 4.0, sizes)
    for h_, scale in zip(gs.hist, (300.0, 3.0, 3.0)):
        h_.copy_((torch.randn(h_.shape, generator=g) * scale).to(dev))
    gs.queries[:, 1:] = 100.0
    gs.committed, gs.next_ind = 3 * S, 3 * S - STEP
    return gs, torch.zeros(1, N, dtype=torch.int32, device=dev)


def trace_run(dev, kind, calls):
    gs, first32 = synthetic_state(dev)
    args = (S, GRID, THRESH, POINTS + SPARE, first32, (0.0, HW[1] - 1.0, 0.0, HW[0] - 1.0))
    torch.cuda.synchronize()
    for _ in range(calls):
        out = gs.health(*args) if kind == "health" else torch_health(gs, *args)
    torch.cuda.synchronize()
    print(json.dumps({"trace": kind, "calls": calls, "lost_sum": int(out[0].sum()), "cover_sum": int(out[2].sum())}))


def trace_summary(kind, dirs, calls):
    (da, db), (ka, kb) = dirs, calls
    a, b = kernel_rows(da), kernel_rows(db)
    per_call = {n: (b.get(n, 0) - a.get(n, 0)) / (kb - ka) for n in sorted(set(a) | set(b))}
    per_call = {n: round(v, 2) for n, v in per_call.items() if v}
    total = round(sum(per_call.values()), 2)
    line = {"trace_summary": kind, "workload": "c4_one_set_push_spare64", "evaluations": [ka, kb], "launches_per_evaluation": total,
            "launches_per_evaluation_by_name": per_call, "libctk_sha256": lib_sha()}
    if kind == "health":
        line["health_is_one_launch"] = bool(total == 1.0 and any("stream_health" in n for n in per_call))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3, help="stream passes per row")
    ap.add_argument("--calls", type=int, nargs="+", default=[8], help="calls per pass (two values with --trace-summary)")
    ap.add_argument("--reps", type=int, default=10, help="health / torch pairs timed after each call of the health stream")
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f32"])
    ap.add_argument("--trace", default=None, choices=("health", "torch"), help="run this many evaluations of one kind alone, for rocprofv3")
    ap.add_argument("--trace-summary", nargs=2, default=None, metavar=("OUT_A", "OUT_B"))
    ap.add_argument("--row", default="health", choices=("health", "torch"))
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    args = ap.parse_args()
    if args.trace_summary:
        line = trace_summary(args.row, args.trace_summary, args.calls)
    else:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        if args.trace:
            trace_run(dev, args.trace, args.calls[0])
            return
        line = bench_line(dev, args.precision, max(1, args.passes), max(4, args.calls[0]), max(2, args.reps))
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
    if line.get("conditions_hold") is False or line.get("health_is_one_launch") is False:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
