#!/usr/bin/env python
"""Planes of a live stream on the device (CoTrackerOnlinePredictor.follow_planes / overlay / rectify), measured OUTSIDE bench.py with the
conventions of bench_stream_objects.py:

    python tools/bench_stream_planes.py [--passes 3] [--calls 8] [--precision f16x3|f32] [--out profiles/stream_planes_bench.json]

The C4 shape on the online predictor (window 16, 384 x 512 model resolution, iters 6, window graph on), ONE query set of 1024
points, fed by push_frames with 1080 x 1920 uint8 channels-last frames, eight per call (sixteen for the first window):
  plain    the push only;
  overlay  the push plus overlay() of a 400 x 600 picture onto the eight frames just pushed, for one object boxed after the second
           window (the whole picture: every point belongs to it) -- inside the timed call;
  rectify  the push plus rectify() of the same quad into eight 400 x 600 pictures.
The rows run IN ONE PROCESS, ALTERNATING pass by pass; every call lies between two HIP events; ms_* is the median over the calls
after the first two windows of every pass, with the smallest and largest single call next to it: a ratio to `plain` is to be read
against that spread.  host_ms_in_overlay / host_ms_in_rectify is the wall clock the host itself spends inside the call, enqueueing
(no synchronise in it: if the device had to be waited for, it would show here).  How many frames of the overlay row had a fit is
reported (`overlay_frames_with_a_fit`): a frame without one costs the warp less, for every pixel is outside.  Then, between the calls of one stream and alternating, the stream time (HIP events)
over eight 1080p frames of
  fit         the one launch of ctk_fit_planes (anchor form, inverse);
  warp_keep   the one launch of ctk_warp_planes that draws a 400 x 600 picture under eight fixed perspective matrices, in place;
  warp_out    the one launch of ctk_warp_planes that resamples the eight frames into eight 400 x 600 pictures (rectify's);
  identity    ctk_warp_planes under the identity for eight 1080p pictures, next to ctk_warp_frames under the identity (frames_identity):
              what the per-pixel double arithmetic costs;
  torch       what a caller does without the kernels for the overlay: a float64 3 x 3 solve, F.grid_sample on a projective grid, a
              torch.where composite.

What must hold: `overlay` and `rectify` return the tracks of `plain` bit for bit (they only read the stream state).  No time is
gated: nobody has measured these kernels before."""

import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

from bench_stream_groups import NoTimer, S, Timer, grid, lib_sha  # noqa: E402
from bench_stream_motion import HW, POINTS, RAW, STEP, setup  # noqa: E402

ROWS = ("plain", "overlay", "rectify")
PICTURE = (400, 600)
CORNERS = [[620.0, 310.0], [1260.0, 350.0], [1230.0, 760.0], [650.0, 720.0]]
KINDS = ("fit", "warp_keep", "warp_out", "identity", "frames_identity", "torch")


def make_rows(p, raw, dev):
    """One predictor per row (a row keeps its stream state, its buffers and its graph between passes)."""
    preds, fits, host_ms = {}, [], {"overlay": [], "rectify": []}
    scale = torch.tensor([1.0, (RAW[1] - 1) / (HW[1] - 1), (RAW[0] - 1) / (HW[0] - 1)])
    picture = (torch.arange(PICTURE[0] * PICTURE[1] * 3, device=dev) % 251).to(torch.uint8).reshape(*PICTURE, 3)
    everything = torch.tensor([[0.0, 0.0, float(RAW[1]), float(RAW[0])]])

    def stream(row, calls, on_call, after_call=None):
        if row not in preds:
            preds[row] = copy.deepcopy(p)
        x = preds[row]
        x(torch.zeros(1, 1, 3, *RAW, device=dev), is_first_step=True, queries=(grid(32, 0.0) * scale)[None].to(dev))
        outs, chosen = [], None
        for i in range(calls):
            t0 = (i % 6) * STEP
            new = raw[t0:t0 + S] if i == 0 else raw[t0 + S - STEP:t0 + S]
            shown = new[-STEP:].clone() if row == "overlay" else new[-STEP:]  # (drawn in place: not into the ring of raw frames)
            with on_call(i):
                out = x.push_frames(new)
                h0 = time.perf_counter()
                if chosen is not None and row == "overlay":
                    x.overlay(shown, picture, CORNERS, chosen)
                if chosen is not None and row == "rectify":
                    x.rectify(shown, CORNERS, chosen, size=PICTURE)
                if chosen is not None and row in host_ms:  # (the host's own time in the call: nothing in it waits for the device)
                    host_ms[row].append((time.perf_counter() - h0) * 1e3)
            if chosen is not None and row == "overlay":
                fits.append(int((x.follow_planes(chosen, STEP, inverse=True)[2][:, 0, 1] > 0).sum()))
            if i == 1:  # (outside the timed calls: the median leaves the first two windows out)
                chosen = x.label_objects(everything)
            outs.append((out[0].clone(), out[1].clone()))
            if after_call is not None:
                after_call(x, i, chosen, shown)
        x.finish()
        return outs
    stream.preds, stream.fits, stream.picture, stream.host_ms = preds, fits, picture, host_ms
    return stream


def fixed_matrices(dev):
    """Eight perspective matrices frame pixel -> picture pixel: the quad of CORNERS drifting by a few pixels a frame."""
    from cotracker_amd import ops
    mats = []
    for j in range(STEP):
        moved = [[x + 3.0 * j + (2.0 * j if k in (1, 2) else 0.0), y + 1.5 * j - (1.0 * j if k in (2, 3) else 0.0)] for k, (x, y) in enumerate(CORNERS)]
        mats.append(torch.linalg.inv(ops.quad_matrix(moved, PICTURE)))
    return torch.stack(mats).to(dev)  # float64 [8,3,3]


def torch_overlay(frames, picture_f, forward64, base):
    """The overlay without the kernels: forward64 float64 [F,3,3] picture -> frame; base float32 [H,W,3] = (x, y, 1)."""
    inv = torch.linalg.solve(forward64, torch.eye(3, dtype=torch.float64, device=forward64.device).expand_as(forward64)).float()
    pos = torch.einsum("hwc,fdc->fhwd", base, inv)
    xy = pos[..., :2] / pos[..., 2:3]
    h, w = picture_f.shape[-2:]
    gx, gy = xy[..., 0] * (2.0 / (w - 1)) - 1.0, xy[..., 1] * (2.0 / (h - 1)) - 1.0
    inside = (pos[..., 2] > 0) & (gx.abs() <= 1.0) & (gy.abs() <= 1.0)
    samp = F.grid_sample(picture_f.expand(frames.shape[0], -1, -1, -1), torch.stack([gx, gy], dim=-1), mode="bilinear", align_corners=True)
    return torch.where(inside[..., None], samp.permute(0, 2, 3, 1).round().to(torch.uint8), frames)


def alone_line(stream, reps, dev):
    """Between the calls of one `plain` stream: the kinds alone, alternating."""
    from cotracker_amd import ops
    gpu_ms = {kind: [] for kind in KINDS}
    inv64 = fixed_matrices(dev)
    m_keep = inv64.float().contiguous()
    fwd64 = torch.linalg.inv(inv64.cpu()).to(dev)
    m_out = fwd64.float().contiguous()
    eye3 = torch.eye(3, device=dev).expand(STEP, 3, 3).contiguous()
    eye2 = torch.eye(2, 3, device=dev).expand(STEP, 2, 3).contiguous()
    picture = stream.picture
    picture_f = picture.permute(2, 0, 1)[None].float()
    ys, xs = torch.meshgrid(torch.arange(RAW[0], device=dev, dtype=torch.float32), torch.arange(RAW[1], device=dev, dtype=torch.float32),
                            indexing="ij")
    base = torch.stack([xs, ys, torch.ones_like(xs)], dim=-1)
    out_small = torch.empty(STEP, *PICTURE, 3, dtype=torch.uint8, device=dev)
    out_big = torch.empty(STEP, *RAW, 3, dtype=torch.uint8, device=dev)
    counts = []

    def after_call(x, i, chosen, shown):
        if i < 2:
            return
        done = x.model._gstream.committed
        (H, W), (ih, iw) = x._hw, x.interp_shape
        common = dict(N_out=x.N, scale=((W - 1) / (iw - 1), (H - 1) / (ih - 1)), thresh=0.6, first_row=x._emit_first_row(), group=0)
        frames = shown.clone()

        def run(kind):
            if kind == "fit":
                return x.model.stream_planes(done - STEP, STEP, labels=chosen.labels[None], planes=1, anchor=chosen.anchor, inverse=True, **common)
            if kind == "warp_keep":
                return ops.warp_planes(picture[None], m_keep, out=frames, border="keep")
            if kind == "warp_out":
                return ops.warp_planes(frames, m_out, size=PICTURE, out=out_small)
            if kind == "identity":
                return ops.warp_planes(frames, eye3, out=out_big)
            if kind == "frames_identity":
                return ops.warp_frames(frames, eye2, out=out_big)
            return torch_overlay(frames, picture_f, fwd64, base)
        for _ in range(reps):
            for kind in KINDS:
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                res = run(kind)
                b.record()
                b.synchronize()
                gpu_ms[kind].append(a.elapsed_time(b))
                if kind == "fit":
                    counts.extend(res[2][0, :, 0, :2].tolist())
    stream("plain", 5, NoTimer(), after_call)
    # the kernel draws what the torch chain draws, to within the rounding of float32 grids (reported, not gated)
    frames = torch.zeros(STEP, *RAW, 3, dtype=torch.uint8, device=dev)
    ours = ops.warp_planes(picture[None], m_keep, out=frames.clone(), border="keep")
    theirs = torch_overlay(frames, picture_f, fwd64, base)
    diff = (ours.int() - theirs.int()).abs()
    line = {"alone_protocol": "each kind over eight 1080p frames, alternating between the calls of one stream, each between two HIP events "
                              "after a device synchronise; the first of each kind is left out",
            "alone_frames": STEP, "alone_points": POINTS, "picture": list(PICTURE),
            "overlay_vs_torch_pixels_differing_by_more_than_1": int((diff > 1).any(dim=-1).sum()),
            "overlay_pixels_drawn": int((ours != frames).any(dim=-1).sum())}
    for kind, v in gpu_ms.items():
        v = v[1:]
        line[f"{kind}_gpu_ms_median"] = round(statistics.median(v), 4)
        line[f"{kind}_gpu_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    line["alone_evaluations_timed"] = len(gpu_ms["fit"]) - 1
    ours_ms = line["fit_gpu_ms_median"] + line["warp_keep_gpu_ms_median"]
    line["overlay_launches_gpu_ms"] = round(ours_ms, 4)
    line["ratio_overlay_launches_over_torch"] = round(ours_ms / line["torch_gpu_ms_median"], 4)
    line["ratio_identity_over_warp_frames"] = round(line["identity_gpu_ms_median"] / line["frames_identity_gpu_ms_median"], 4)
    line["fit_points_inliers_min"] = [min(v[0] for v in counts), min(v[1] for v in counts)]
    line["fit_points_inliers_max"] = [max(v[0] for v in counts), max(v[1] for v in counts)]
    return line


def bench_line(dev, precision, passes, calls, reps):
    p, raw = setup(dev, precision)
    stream = make_rows(p, raw, dev)
    for row in ROWS:  # warm every row: weights packed, graphs captured
        stream(row, 3, NoTimer())
    del stream.fits[:]
    for v in stream.host_ms.values():
        del v[:]
    ms, last = {r: [] for r in ROWS}, {}
    for _ in range(passes):
        for row in ROWS:
            last[row] = stream(row, calls, Timer(ms[row], 2))
    med = {r: statistics.median(v) for r, v in ms.items()}
    line = {"workload": "c4_one_set_push_u8_1080p", "points": POINTS, "frames": list(HW), "raw_frames": list(RAW), "window_len": S, "iters": 6,
            "precision": precision, "hip_graph": True, "hypotheses": 128, "planes": 1, "passes": passes,
            "calls_per_pass": calls, "timed_calls_per_row": len(ms["plain"]),
            "protocol": "rows alternate pass by pass in one process; every call (the push and what follows it) between two HIP events; "
                        "median over the calls after the first two windows of each pass",
            "libctk_sha256": lib_sha()}
    for r in ROWS:
        line["ms_" + r] = round(med[r], 3)
        line["min_max_ms_" + r] = [round(min(ms[r]), 3), round(max(ms[r]), 3)]
    for r in ROWS[1:]:
        line[f"ratio_{r}_over_plain"] = round(med[r] / med["plain"], 4)
        line[f"ms_{r}_minus_plain"] = round(med[r] - med["plain"], 3)
    for r in ROWS[1:]:  # what the host itself spends inside overlay() / rectify(), enqueueing: wall clock, no synchronise
        line[f"host_ms_in_{r}"] = round(statistics.median(stream.host_ms[r]), 3)
        line[f"host_ms_in_{r}_min_max"] = [round(min(stream.host_ms[r]), 3), round(max(stream.host_ms[r]), 3)]
    line["spread_plain_max_over_min"] = round(max(ms["plain"]) / min(ms["plain"]), 4)
    line["overlay_frames_with_a_fit"] = [min(stream.fits), max(stream.fits)] if stream.fits else None
    same = all(torch.equal(ta, tb) and torch.equal(va, vb) for r in ROWS[1:] for (ta, va), (tb, vb) in zip(last["plain"], last[r]))
    line["overlay_and_rectify_equal_plain_bit_for_bit"] = bool(same)
    line.update(alone_line(stream, reps, dev))
    line["range_fallbacks"] = int(sum(x_.model.range_fallbacks for x_ in stream.preds.values()))
    line["conditions_hold"] = bool(same)
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3, help="stream passes per row")
    ap.add_argument("--calls", type=int, default=8, help="calls per pass")
    ap.add_argument("--reps", type=int, default=5, help="evaluations of each kind timed after every call of one plain stream")
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f32"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_planes_bench.json"), help="append the JSON line to this file")
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
