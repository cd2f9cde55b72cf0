#!/usr/bin/env python
"""Two structures aligned on the device (ops.fit_align / CoTrackerOnlinePredictor.align, one launch of ctk_fit_align), measured OUTSIDE
bench.py with the conventions of bench_stream_p3p.py:

    python tools/bench_align.py [--passes 3] [--calls 8] [--precision f16x3|f32] [--out profiles/align_bench.json]

Launch alone, at 1024 and at 8192 points, 256 hypotheses, 15 evaluations of each kind ALTERNATING, each between two HIP events after a
device synchronise, the first of each kind left out (14 timed):
  align  the ONE launch of ctk_fit_align on a planted pair (a random similarity, a fifth of the points moved, 0.5 % depth noise);
  p3p    the ONE launch of the parent commit's ctk_fit_p3p at the same size: the same points as the structure, their projections as the
         tracked frame, the same hypotheses;
  torch  the same question in batched torch: Umeyama by torch.linalg.svd over 256 sampled triples, every candidate scored over all
         points by the same two tolerances, the best one kept (no refit) -- what the launch replaces.  Its triples are drawn by
         torch.randint, not by the launch's seeded sampler (restating that generator in torch would time the restatement): the two
         rows score different candidates of the same kind and number, so their times compare and their counts need not agree.
The expectation, not a gate: one launch of ctk_fit_align is no slower than ctk_fit_p3p beyond the spread of single evaluations (it
scores the same list with a cheaper candidate).  The line says whether it is met and whether the single evaluations overlap.

Stream rows, the C4 shape on the online predictor (window 16, 384 x 512 model resolution, iters 6, window graph on), ONE query set of
1024 points, 1080 x 1920 uint8 frames pushed eight per call, IN ONE PROCESS, ALTERNATING pass by pass:
  plain  the push only;
  align  the push plus align() of two structures over the stream's slots (planted; the anchors pinned once).
What must hold: `align` returns the tracks of `plain` bit for bit (it reads nothing of the stream)."""

import argparse
import copy
import json
import math
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

ROWS = ("plain", "align")
KINDS = ("align", "p3p", "torch")
HYPOTHESES = 256
CAMERA = (1000.0, 1000.0, 959.5, 539.5)
TOL, DEPTH_TOL = 2.0, 0.1


def planted_pair(N, dev, seed=0):
    """b = s R a + t over N slots: points 3..12 deep in b's camera, 0.5 % depth noise in both sets, a fifth of the points moved."""
    g = torch.Generator().manual_seed(seed)
    fx, fy, cx, cy = CAMERA
    u = (torch.rand(N, generator=g) * 1840 + 40 - cx) / fx
    v = (torch.rand(N, generator=g) * 1000 + 40 - cy) / fy
    z = torch.rand(N, generator=g) * 9 + 3
    rays = torch.stack([u, v, torch.ones(N)], dim=1).double()
    b = rays * (z * (1 + 0.005 * torch.randn(N, generator=g)))[:, None]
    ya = rays * (z * (1 + 0.005 * torch.randn(N, generator=g)))[:, None]
    moved = torch.rand(N, generator=g) < 0.2
    ya = torch.where(moved[:, None], ya + torch.randn(N, 3, generator=g) * 0.4, ya)
    ang, s = 0.3, 1.7
    R = torch.tensor([[math.cos(ang), 0.0, math.sin(ang)], [0.0, 1.0, 0.0], [-math.sin(ang), 0.0, math.cos(ang)]], dtype=torch.float64)
    t_ = torch.tensor([0.5, -0.2, 0.8], dtype=torch.float64)
    a = (ya - t_) @ R / s
    ones = torch.ones(N, dtype=torch.int8)
    return a.float().to(dev), ones.to(dev), b.float().to(dev), ones.clone().to(dev)


def torch_umeyama(a, b, K, seed):
    """The torch chain: K sampled triples, Umeyama by one batched SVD, every candidate scored over all points -> (s, R, t, count)."""
    N = a.shape[0]
    g = torch.Generator(device=a.device).manual_seed(seed)
    idx = torch.randint(0, N, (K, 3), device=a.device, generator=g)
    X, Y = a[idx].double(), b[idx].double()
    mx, my = X.mean(dim=1, keepdim=True), Y.mean(dim=1, keepdim=True)
    Xc, Yc = X - mx, Y - my
    U, D, Vt = torch.linalg.svd(Yc.transpose(1, 2) @ Xc / 3.0)
    sign = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vt))
    Sg = torch.diag_embed(torch.stack([torch.ones_like(sign), torch.ones_like(sign), sign], dim=1))
    R = U @ Sg @ Vt
    s = (D * torch.diagonal(Sg, dim1=1, dim2=2)).sum(dim=1) / (Xc ** 2).sum(dim=(1, 2)).clamp_min(1e-30) * 3.0
    t_ = my[:, 0] - s[:, None] * (R @ mx.transpose(1, 2))[:, :, 0]
    Z = s[:, None, None] * (a.double()[None] @ R.transpose(1, 2)) + t_[:, None]
    Yd = b.double()[None]
    fx, fy = CAMERA[0], CAMERA[1]
    du, dv = fx * (Z[..., 0] / Z[..., 2] - Yd[..., 0] / Yd[..., 2]), fy * (Z[..., 1] / Z[..., 2] - Yd[..., 1] / Yd[..., 2])
    ok = (Z[..., 2] > 0) & (du * du + dv * dv <= TOL * TOL) & ((Z[..., 2] - Yd[..., 2]).abs() <= DEPTH_TOL * Yd[..., 2])
    count = ok.sum(dim=1)
    k = torch.argmax(count)
    return s[k], R[k], t_[k], count[k]


def alone_line(dev, reps):
    from cotracker_amd import ops
    line = {"alone_protocol": "the three kinds alternating, each evaluation between two HIP events after a device synchronise; the first "
                              "of each kind is left out", "alone_hypotheses": HYPOTHESES, "alone_evaluations_timed": reps - 1}
    fx, fy, cx, cy = CAMERA
    for N in (1024, 8192):
        a, va, b, vb = planted_pair(N, dev, seed=N)
        px = torch.stack([fx * b[:, 0] / b[:, 2] + cx, fy * b[:, 1] / b[:, 2] + cy], dim=1)
        tracks = torch.stack([px + 5.0, px], dim=0)[None].contiguous()  # [1,2,N,2]: frame 1 against frame 0
        visible = torch.ones(1, 2, N, dtype=torch.bool, device=dev)
        structure = (b / 1.0).contiguous()  # the tracked frame's own points: every candidate that stands is scored over the whole list

        def run(kind):
            if kind == "align":
                return int(ops.fit_align(a, va, b, vb, CAMERA, tol=TOL, depth_tol=DEPTH_TOL, hypotheses=HYPOTHESES)[4][0, 1])
            if kind == "p3p":
                return int(ops.fit_p3p(tracks, visible, CAMERA, structure, vb, lag=1, tol=TOL, hypotheses=HYPOTHESES)[3][0, 1, 1])
            return int(torch_umeyama(a, b, HYPOTHESES, 0)[3])
        ms, counted = {k: [] for k in KINDS}, {}
        for _ in range(reps):
            for kind in KINDS:
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if kind == "align":
                    out = ops.fit_align(a, va, b, vb, CAMERA, tol=TOL, depth_tol=DEPTH_TOL, hypotheses=HYPOTHESES)
                elif kind == "p3p":
                    out = ops.fit_p3p(tracks, visible, CAMERA, structure, vb, lag=1, tol=TOL, hypotheses=HYPOTHESES)
                else:
                    out = torch_umeyama(a, b, HYPOTHESES, 0)
                e1.record()
                e1.synchronize()
                ms[kind].append(e0.elapsed_time(e1))
                del out
        for kind in KINDS:
            counted[kind] = run(kind)
            v = ms[kind][1:]
            line[f"{kind}_{N}_gpu_ms_median"] = round(statistics.median(v), 4)
            line[f"{kind}_{N}_gpu_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
            line[f"{kind}_{N}_points_within_tol"] = counted[kind]
        x, y = line[f"align_{N}_gpu_ms_min_max"], line[f"p3p_{N}_gpu_ms_min_max"]
        line[f"ratio_align_over_p3p_{N}"] = round(line[f"align_{N}_gpu_ms_median"] / line[f"p3p_{N}_gpu_ms_median"], 4)
        line[f"ratio_align_over_torch_{N}"] = round(line[f"align_{N}_gpu_ms_median"] / line[f"torch_{N}_gpu_ms_median"], 4)
        line[f"align_vs_p3p_beyond_spread_{N}"] = bool(x[1] < y[0] or y[1] < x[0])  # (the single evaluations do not overlap)
        line[f"expectation_align_no_slower_than_p3p_{N}"] = bool(line[f"align_{N}_gpu_ms_median"] <= line[f"p3p_{N}_gpu_ms_median"] or
                                                                  not line[f"align_vs_p3p_beyond_spread_{N}"])
    return line


def make_rows(p, raw, dev):
    """One predictor per row (a row keeps its stream state, its buffers and its graph between passes)."""
    from cotracker_amd import ops
    preds, counts, held = {}, [], {}
    scale = torch.tensor([1.0, (RAW[1] - 1) / (HW[1] - 1), (RAW[0] - 1) / (HW[0] - 1)])

    def stream(row, calls, on_call):
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
                if row == "align" and i == 1:  # (the two structures are made once; this call is not timed)
                    Nm = x.model._gstream.N
                    a, va, b, vb = planted_pair(Nm, dev, seed=5)
                    held["a"] = ops.Structure(a, va, x.pin(x.model._gstream.committed - 2), CAMERA)
                    held["b"] = ops.Structure(b, vb, x.pin(), CAMERA)
                elif row == "align" and i >= 2:
                    res = x.align(held["a"], held["b"], hypotheses=HYPOTHESES)
            if res is not None:
                counts.append(res[4][:2].tolist())
            outs.append((out[0].clone(), out[1].clone()))
        x.finish()
        return outs
    stream.preds, stream.counts = preds, counts
    return stream


def bench_line(dev, precision, passes, calls, reps):
    p, raw = setup(dev, precision)
    stream = make_rows(p, raw, dev)
    for row in ROWS:  # warm every row: weights packed, graphs captured
        stream(row, 3, NoTimer())
    del stream.counts[:]
    ms, last = {r: [] for r in ROWS}, {}
    for _ in range(passes):
        for row in ROWS:
            last[row] = stream(row, calls, Timer(ms[row], 2))
    med = {r: statistics.median(v) for r, v in ms.items()}
    line = {"workload": "c4_one_set_push_u8_1080p", "points": POINTS, "frames": list(HW), "raw_frames": list(RAW), "window_len": S, "iters": 6,
            "precision": precision, "hip_graph": True, "hypotheses": HYPOTHESES, "camera": list(CAMERA), "tol": TOL, "depth_tol": DEPTH_TOL,
            "passes": passes, "calls_per_pass": calls, "timed_calls_per_row": len(ms["plain"]),
            "protocol": "rows alternate pass by pass in one process; every call (the push and what follows it) between two HIP events; "
                        "median over the calls after the first two windows of each pass",
            "libctk_sha256": lib_sha()}
    for r in ROWS:
        line["ms_" + r] = round(med[r], 3)
        line["min_max_ms_" + r] = [round(min(ms[r]), 3), round(max(ms[r]), 3)]
    spread = max(ms["plain"]) - min(ms["plain"])
    line["spread_plain_ms"] = round(spread, 3)
    line["ms_align_minus_plain"] = round(med["align"] - med["plain"], 3)
    line["align_minus_plain_exceeds_plain_spread"] = bool(med["align"] - med["plain"] > spread)
    line["align_points_fitted_and_within_tol"] = [min(c[0] for c in stream.counts), min(c[1] for c in stream.counts)]
    same = all(torch.equal(ta, tb) and torch.equal(va, vb) for (ta, va), (tb, vb) in zip(last["plain"], last["align"]))
    line["align_equals_plain_bit_for_bit"] = bool(same)
    line.update(alone_line(dev, reps))
    line["range_fallbacks"] = int(sum(x_.model.range_fallbacks for x_ in stream.preds.values()))
    line["conditions_hold"] = bool(same)
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3, help="stream passes per row")
    ap.add_argument("--calls", type=int, default=8, help="calls per pass")
    ap.add_argument("--reps", type=int, default=15, help="evaluations of each kind (the first is left out: 14 timed)")
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f32"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"), help="append the JSON line to this file")
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
