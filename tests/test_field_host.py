"""The rules of ctk_track_field and ctk_warp_field without a GPU: co-tracker_amd/csrc/field_math.h built with g++ into a stand-alone
program (tests/host/field_host.cpp) against the numpy restatement of tests/field_reference.py on every byte and every float bit, the
consequences the rules promise (a zero field copies, a constant whole-pixel field is a shifted copy), the accuracy of the zeroth-order
weighting on a planted similarity against the float64 truth, and the same program once under -fsanitize=address,undefined."""
import os
import subprocess

import numpy as np
import pytest

import field_reference as R
from ctk_support import ROOT

SOURCE = os.path.join(ROOT, "tests", "host", "field_host.cpp")


def build(tmp, name, *flags):
    exe = os.path.join(str(tmp), name)
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-o", exe, SOURCE], check=True)
    return exe


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build(tmp_path_factory.mktemp("field"), "field_host", "-O2")


def run(exe, mode, blobs, tmp):
    src, dst = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(src, "wb") as f:
        for b in blobs:
            f.write(np.ascontiguousarray(b).tobytes())
    subprocess.run([exe, mode, src, dst], check=True)
    return open(dst, "rb").read()


def host_track(exe, tmp, coords, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1, size=(1, 1), cs=4,
               radius=2, to=-1, lag=0, anchor=None, sx=1.0, sy=1.0):
    coords = np.asarray(coords, dtype=np.float32)
    G, Rr, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    head = np.array([G, N, N_out, Rr, f0, F, size[0], size[1], cs, radius, to, lag, 0 if anchor is None else anchor[2],
                     visible is not None, first_row is not None, anchor is not None], dtype=np.int32)
    blobs = [head, np.array([sx, sy, thresh], dtype=np.float32), coords]
    blobs += [np.asarray(visible, dtype=np.uint8)] if visible is not None else [np.asarray(vis, dtype=np.float32), np.asarray(conf, dtype=np.float32)]
    if first_row is not None:
        blobs.append(np.asarray(first_row, dtype=np.int32))
    if anchor is not None:
        blobs += [np.asarray(anchor[0], dtype=np.float32), np.asarray(anchor[1], dtype=np.uint8)]
    raw = run(exe, "track", blobs, tmp)
    gh, gw = R.grid(size[0], cs), R.grid(size[1], cs)
    n = G * F * gh * gw
    assert len(raw) == n * 8 + n + G * F * 16
    return (np.frombuffer(raw, dtype=np.int32, count=n * 2).reshape(G, F, gh, gw, 2),
            np.frombuffer(raw, dtype=np.uint8, count=n, offset=n * 8).reshape(G, F, gh, gw),
            np.frombuffer(raw, dtype=np.int32, count=G * F * 4, offset=n * 9).reshape(G, F, 4))


def host_warp(exe, tmp, src, field, cs, border=R.FILL, fill=(0, 0, 0), layout=R.HWC):
    src, field = np.ascontiguousarray(src), np.ascontiguousarray(field, dtype=np.int32)
    F = field.shape[0]
    C = 1 if src.ndim == 3 else 3
    H, W = src.shape[1:3] if (src.ndim == 3 or layout == R.HWC) else src.shape[2:4]
    head = np.array([F, H, W, C, layout, border, cs, *fill, src.shape[0], 0], dtype=np.int32)
    raw = run(exe, "warp", [head, field, src], tmp)
    n = F * H * W
    assert len(raw) == n * C + n * 8
    dst = np.frombuffer(raw, dtype=np.uint8, count=n * C).reshape((F,) + src.shape[1:])
    return dst, np.frombuffer(raw, dtype=np.float32, count=n * 2, offset=n * C).reshape(F, H, W, 2)


def same(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def scene(seed, G, T, N, hw, p_visible=0.9, spread=1.0):
    """Random tracks that drift a few pixels a frame, some outside the picture."""
    rng = np.random.default_rng(seed)
    H, W = hw
    p0 = rng.uniform(-0.1, 1.1, (G, 1, N, 2)) * np.array([W, H]) * spread
    coords = (p0 + np.cumsum(rng.normal(0, 1.5, (G, T, N, 2)), axis=1)).astype(np.float32)
    visible = (rng.uniform(size=(G, T, N)) < p_visible).astype(np.uint8)
    return coords, visible


@pytest.mark.parametrize("cs,radius,hw", [(2, 1, (29, 37)), (4, 4, (45, 70)), (6, 1, (67, 130)), (4, 2, (33, 64)), (3, 3, (40, 41))])
def test_host_build_equals_the_restatement(host, tmp_path, cs, radius, hw):
    """All three "to" forms (a negative lag and an anchor with a reassigned slot among them), the visible tensor and logits, first_row,
    a ring (R < frames), sides that are and are not multiples of the cell."""
    G, T, N = 2, 7, 60
    coords, visible = scene(cs * 10 + radius, G, T, N, hw)
    rng = np.random.default_rng(cs)
    first_row = rng.integers(0, 4, (G, N)).astype(np.int32)
    first_row[:, 5], first_row[:, 6] = R.INT32_MAX, 6
    kw = dict(size=hw, cs=cs, radius=radius)
    for form in (dict(to=2, f0=0, F=T), dict(lag=2, f0=1, F=5), dict(lag=-1, f0=0, F=6)):
        for fr in (None, first_row):
            want = R.track_field(coords, visible=visible, first_row=fr, **form, **kw)
            assert same(host_track(host, tmp_path, coords, visible=visible, first_row=fr, **form, **kw), want), (form, fr is None)
            assert want[2][..., 0].max() > 0
    # logits, a scale, N_out, and a ring of 5 rows that holds frames 9..13: frame f in row f % 5
    vis, conf = rng.normal(1.0, 2.0, (G, 5, N)).astype(np.float32), rng.normal(1.0, 2.0, (G, 5, N)).astype(np.float32)
    ring = dict(vis=vis, conf=conf, thresh=0.6, N_out=41, sx=0.75, sy=1.25, f0=11, F=3, lag=2, **kw)
    want = R.track_field(coords[:, :5], **ring)
    assert same(host_track(host, tmp_path, coords[:, :5], **ring), want) and want[2][..., 0].min() > 0
    # an anchor taken on frame 3: slot 6 (first row 6) was reassigned after it and drops out, slot 7's anchor is not visible
    anchor = (coords[:, 3].copy(), visible[:, 3].copy(), 3)
    anchor[1][:, 7] = 0
    want = R.track_field(coords, visible=visible, first_row=first_row, anchor=anchor, f0=4, F=3, **kw)
    assert same(host_track(host, tmp_path, coords, visible=visible, first_row=first_row, anchor=anchor, f0=4, F=3, **kw), want)
    gone = first_row.copy()
    gone[:, 6] = 0
    assert not same(R.track_field(coords, visible=visible, first_row=gone, anchor=anchor, f0=4, F=3, **kw), want)  # (the slot mattered)


def test_few_pairs_bad_positions_and_holes(host, tmp_path):
    hw, kw = (45, 70), dict(size=(45, 70), cs=2, radius=1, to=1)
    gh, gw = R.grid(45, 2), R.grid(70, 2)
    for M in (0, 1, 2):
        coords = np.zeros((1, 2, 3, 2), dtype=np.float32)
        coords[0, 0, :, 0], coords[0, 0, :, 1] = (10.25, 50.5, 30.0), (8.0, 30.75, 20.0)
        coords[0, 1] = coords[0, 0] + np.array([[2.5, -1.25], [-3.0, 4.0], [0.5, 0.5]], dtype=np.float32)
        visible = np.zeros((1, 2, 3), dtype=np.uint8)
        visible[:, :, :M] = 1
        got, want = host_track(host, tmp_path, coords, visible=visible, **kw), R.track_field(coords, visible=visible, **kw)
        assert same(got, want)
        field, level, stats = want
        if M == 0:
            assert (field == 0).all() and (level == R.NO_LEVEL).all() and stats.tolist() == [[[0, 0, R.NO_LEVEL, 0]]]
        else:  # a radius of one cell of 4 pixels on an 18 x 13 node grid: most nodes are filled from levels >= 2
            assert stats[0, 0, 0] == M and stats[0, 0, 2] >= 2 and (level >= 2).sum() > gh * gw // 2 and (level == 0).any()
            assert stats[0, 0, 1] == (level == 0).sum() and stats[0, 0, 2] == level.max()
        if M == 1:  # one pair: its displacement everywhere, (2.5, -1.25) px in 1/256
            assert (field[..., 0] == 640).all() and (field[..., 1] == -320).all()
    # NaN, infinite and out-of-range positions are no pairs; points outside the picture count while they reach a node
    coords, visible = scene(7, 1, 2, 40, hw)
    bad = coords.copy()
    bad[0, 0, 0, 0], bad[0, 1, 1, 1], bad[0, 0, 2, 0], bad[0, 1, 3, 1], bad[0, 0, 4, 0] = np.nan, np.inf, -np.inf, 8192.5, -9000.0
    bad[0, :, 5], bad[0, :, 6] = (-20.0, -30.0), (8192.0, 8192.0)  # valid, far outside
    visible[0, :, :7] = 1
    got, want = host_track(host, tmp_path, bad, visible=visible, **kw), R.track_field(bad, visible=visible, **kw)
    assert same(got, want)
    dropped = visible.copy()
    dropped[0, :, :5] = 0
    assert same(want, R.track_field(bad, visible=dropped, **kw)) and want[2][0, 0, 0] == int((visible[0].min(axis=0) != 0).sum()) - 5
    # a hole in the middle of a dense set: levels >= 2 inside it, level 0 round it
    rng = np.random.default_rng(3)
    p = rng.uniform(0, 1, (400, 2)) * np.array([130, 67])
    p = p[~((np.abs(p[:, 0] - 65) < 30) & (np.abs(p[:, 1] - 33) < 22))]
    coords = np.stack([p, p + np.array([1.5, 0.25])]).astype(np.float32)[None]
    hole = dict(size=(67, 130), cs=2, radius=1, to=1, visible=np.ones(coords.shape[:3], dtype=np.uint8))
    got, want = host_track(host, tmp_path, coords, **hole), R.track_field(coords, **hole)
    assert same(got, want) and want[1][0, 0, 8, 16] >= 2 and want[2][0, 0, 2] >= 2 and (want[1] == 0).sum() > 100


def test_worst_case_magnitudes_stay_inside_int64(host, tmp_path):
    """8192 coincident points ON a node (x = 8192 px: node 128 of a c = 64 grid) with d = -2^18 (1/16 px): Wn = 2^33, S = -2^51,
    S * 16 = -2^55 -- the stated bounds, reached."""
    coords = np.zeros((1, 2, 8192, 2), dtype=np.float32)
    coords[0, 0, :, 0], coords[0, 1, :, 0] = 8192.0, -8192.0
    kw = dict(size=(8, 8200), cs=6, radius=1, to=1, visible=np.ones((1, 2, 8192), dtype=np.uint8))
    want = R.track_field(coords, **kw)
    assert same(host_track(host, tmp_path, coords, **kw), want)
    field, level, stats = want
    assert stats[0, 0].tolist() == [8192, 1, int(level.max()), 0] and level[0, 0, 0, 128] == 0 and level.max() >= 7
    assert (field[0, 0, ..., 0] == -(2 ** 22)).all() and (field[0, 0, ..., 1] == 0).all()
    P, d = R.pairs(coords, 0, 1, 0, kw["visible"], None, None, 0.0, None, 8192, 1.0, 1.0, None)
    assert R.node_sums(P, d, 2, 130, 6, 1)[0, 128].tolist() == [2 ** 33, -(2 ** 51), 0]


@pytest.mark.parametrize("cs", (2, 4, 6))
def test_resampling_equals_the_restatement_and_keeps_its_promises(host, tmp_path, cs):
    rng = np.random.default_rng(cs)
    H, W, F = 45, 70, 3
    gh, gw = R.grid(H, cs), R.grid(W, cs)
    field = rng.integers(-9 * 256, 9 * 256, (F, gh, gw, 2)).astype(np.int32)
    field[1] = rng.integers(-40, 40, (gh, gw, 2))
    field[2, ..., 0] += 60 * 256  # mostly outside
    for layout, shape in ((R.HWC, (F, H, W, 3)), (R.CHW, (F, 3, H, W)), (R.HWC, (F, H, W))):
        src = rng.integers(0, 256, shape, dtype=np.uint8)
        for border in (R.FILL, R.EDGE):
            dst, flow = host_warp(host, tmp_path, src, field, cs, border, (7, 200, 90), layout)
            assert np.array_equal(dst, R.warp_field(src, field, cs, border, (7, 200, 90), layout))
            assert np.array_equal(flow.view(np.int32), R.flow(field, H, W, cs).view(np.int32))
    # one source for several fields
    one = rng.integers(0, 256, (1, H, W), dtype=np.uint8)
    assert np.array_equal(host_warp(host, tmp_path, one, field, cs)[0], R.warp_field(one, field, cs))
    pic = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    zero = np.zeros((1, gh, gw, 2), dtype=np.int32)
    shift = zero.copy()
    shift[..., 0], shift[..., 1] = 4 * 256, -3 * 256  # out(x, y) = src(x + 4, y - 3)
    for warp in (lambda f, b: R.warp_field(pic, f, cs, b, (1, 2, 3)), lambda f, b: host_warp(host, tmp_path, pic, f, cs, b, (1, 2, 3))[0]):
        for border in (R.FILL, R.EDGE):
            assert np.array_equal(warp(zero, border), pic)  # a zero field is a byte copy
            out = warp(shift, border)
            assert np.array_equal(out[0, 3:, :W - 4], pic[0, :H - 3, 4:])
            if border == R.FILL:
                assert (out[0, :3] == (1, 2, 3)).all() and (out[0, :, W - 4:] == (1, 2, 3)).all()
            else:
                assert np.array_equal(out[0, 0, :W - 4], pic[0, 0, 4:]) and np.array_equal(out[0, 5, W - 4:], np.repeat(pic[0, 2, W - 1:], 4, axis=0))
    assert (R.flow(shift, H, W, cs) == np.array([4.0, -3.0], dtype=np.float32)).all()


def interior_error(field, move, hw, cs, radius):
    """max |field - truth| in pixels (Euclidean) over the nodes at least radius + 1 cells from the picture's border."""
    H, W = hw
    c = 1 << cs
    gh, gw = field.shape[:2]
    x, y = np.meshgrid(np.arange(gw) * c, np.arange(gh) * c)
    inside = (x >= (radius + 1) * c) & (x <= W - 1 - (radius + 1) * c) & (y >= (radius + 1) * c) & (y <= H - 1 - (radius + 1) * c)
    at = np.stack([x, y], axis=-1).astype(np.float64)
    err = np.linalg.norm(field.astype(np.float64) / 256.0 - (move(at) - at), axis=-1)
    assert inside.sum() > 100
    return float(err[inside].max())


def test_accuracy_on_a_planted_similarity(host, tmp_path):
    """A jittered 24 x 24 grid of points on a 480 x 270 picture under a similarity of 1.7 degrees and 2 % about the centre, c = 16,
    radius 2: the field at the nodes at least radius + 1 = 3 cells from the border against the float64 truth.  The bar is twice what
    the numpy restatement itself measures here: measured 0.1255 px, bar 0.2510 px (a zeroth-order weighting: the error is the local
    asymmetry of the points round a node times the gradient of the motion; the 1/16 px and 1/256 px quantisations are far below)."""
    coords, move = R.similarity_scene()
    kw = dict(size=(270, 480), cs=4, radius=2, to=1, visible=np.ones(coords.shape[:3], dtype=np.uint8))
    want = R.track_field(coords, **kw)
    measured = interior_error(want[0][0, 0], move, (270, 480), 4, 2)
    bar = 2.0 * 0.1255
    print(f"measured {measured:.4f} px, bar {bar:.4f} px")
    assert abs(measured - 0.1255) < 5e-4  # the recorded figure is the one the bar was set from
    got = host_track(host, tmp_path, coords, **kw)
    assert same(got, want) and (want[1] == 0).all()
    assert interior_error(got[0][0, 0], move, (270, 480), 4, 2) <= bar


def test_the_program_under_the_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined as a stand-alone host binary, run once on a case of each mode: it ends
    clean and gives the restatement's bytes."""
    exe = build(tmp_path, "field_host_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    coords, visible = scene(5, 2, 6, 300, (67, 130))
    kw = dict(size=(67, 130), cs=3, radius=2, lag=1, f0=0, F=6, visible=visible)
    want = R.track_field(coords, **kw)
    assert same(host_track(exe, tmp_path, coords, **kw), want)
    src = np.random.default_rng(0).integers(0, 256, (6, 67, 130, 3), dtype=np.uint8)
    dst, flow = host_warp(exe, tmp_path, src, want[0][0], 3, R.EDGE)
    assert np.array_equal(dst, R.warp_field(src, want[0][0], 3, R.EDGE)) and np.array_equal(flow, R.flow(want[0][0], 67, 130, 3))
