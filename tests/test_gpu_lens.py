"""ctk_lens_frames and ctk_lens_points on the GPU (csrc/lens.hip) against the numpy restatement of tests/lens_reference.py: every byte and
every float32 bit of the poisoned, fenced destinations, pitch padding included, with the inputs unchanged.  The shapes are the smallest
at which the kernels take each of their paths: one pixel, a row tail, whole dwords, a destination off by one byte, several tiles with
partial ones, one and several picture slices per grid z; points below, at and above a wave, strided, in place.  Then the ops layer and
the predictor on a pushed stream."""
import ctypes as C

import numpy as np
import pytest
import torch

import lens_reference as R
from ctk_support import HW, NAN_PATTERN, S, STEP, STRIDE, dev, frame_intact, nan_framed, recorded, t

pytestmark = pytest.mark.gpu

GUARD, POISON, FENCE = 64, 0x5A, 0xA5
ACTION_K = R.LENSES["action"][0]


def rows_view(buf, offset, F, rows, row_bytes, frame_stride, row_stride):
    """The pixel bytes of a strided surface inside the flat uint8 array buf as [F, rows, row_bytes] (rows: H, or 3 H planar)."""
    assert offset + (F - 1) * frame_stride + (rows - 1) * row_stride + row_bytes <= buf.size
    return np.lib.stride_tricks.as_strided(buf[offset:], shape=(F, rows, row_bytes), strides=(frame_stride, row_stride, 1))


def small_lens(k, f1080, hw, out_hw=None):
    """The lens k at the scale of a small picture (the focal length a 1080p one of f1080 has when shrunk to W pixels across); the ideal
    camera looks at the same field through out_hw pixels."""
    H, W = hw
    f = max(f1080 * W / 1920.0, 1.0)
    ideal = None
    if out_hw is not None:
        Ho, Wo = out_hw
        ideal = (max(f * Wo / W, 1.0), max(f * Ho / H, 1.0), (Wo - 1) / 2, (Ho - 1) / 2)
    return R.lens13(k, f, ((W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2), ideal)


def bind(cam, lens):
    for i in range(4):
        cam.sensor[i], cam.ideal[i] = lens[i], lens[4 + i]
    for i in range(5):
        cam.k[i] = lens[8 + i]
    cam.reserved = 0.0


def raw_frames(pics, lens, direction, size, border, fill, layout, src_pad=(0, 0), dst_pad=(0, 0), dst_off=0, tol=0.01):
    """The C-ABI call itself: pics uint8 [F,H,W,3] / [F,3,H,W] laid out with rows padded by pad[0] and frames by pad[1] elements, the
    destination poisoned, fenced and `dst_off` bytes off its 256-byte aligned allocation.  Checks every byte of the destination
    against the restatement (padding: still the poison), the fences and the source, and returns the resampled pictures."""
    from cotracker_amd import _lib as L
    F = pics.shape[0]
    H, W = pics.shape[1:3] if layout == R.HWC else pics.shape[2:4]
    Ho, Wo = (H, W) if size is None else size
    geo = []
    for (h, w), pad in (((H, W), src_pad), ((Ho, Wo), dst_pad)):
        rows, row_bytes = (h, 3 * w) if layout == R.HWC else (3 * h, w)
        rs = row_bytes + pad[0]
        geo.append((rows, row_bytes, rs, rows * rs + pad[1]))
    (srows, srb, srs, sfs), (drows, drb, drs, dfs) = geo
    rng = np.random.default_rng(F * H + W)
    src = rng.integers(0, 256, F * sfs, dtype=np.uint8)  # (what lies between the rows is noise: it must not be read)
    rows_view(src, 0, F, srows, srb, sfs, srs)[...] = pics.reshape(F, srows, srb)
    nd = (F - 1) * dfs + (drows - 1) * drs + drb
    want = np.full(GUARD + dst_off + nd + GUARD, FENCE, dtype=np.uint8)
    want[GUARD + dst_off:GUARD + dst_off + nd] = POISON
    src_d = t(src)
    whole = torch.empty(256 + want.size, dtype=torch.uint8, device=dev())
    base = (-(whole.data_ptr() + GUARD)) % 256  # the destination proper starts dst_off bytes behind a 256-byte boundary
    buf = whole[base:base + want.size]
    buf.copy_(t(want))
    a = L.Lens.FramesArgs()
    a.F, a.H, a.W, a.Ho, a.Wo, a.layout, a.border, a.direction, a.tol, a.reserved = F, H, W, Ho, Wo, layout, border, direction, tol, 0
    for k in range(3):
        a.fill[k] = fill[k]
    a.src_frame_stride, a.src_row_stride, a.dst_frame_stride, a.dst_row_stride = sfs, srs, dfs, drs
    bind(a.lens, lens)
    a.src, a.dst = src_d.data_ptr(), buf.data_ptr() + GUARD + dst_off
    res, rows_ = recorded(lambda: L.load().ctk_lens_frames(C.byref(a), torch.cuda.current_stream().cuda_stream))
    L.check(res, "ctk_lens_frames")
    torch.cuda.synchronize()
    assert rows_ == {"lens_frames": 1}
    ref = R.lens_frames(pics, lens, direction, size, border, fill, tol, layout)
    rows_view(want, GUARD + dst_off, F, drows, drb, dfs, drs)[...] = ref.reshape(F, drows, drb)
    got = buf.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert np.array_equal(src_d.cpu().numpy(), src)
    return ref


# H, W, output size, dst row padding per layout (HWC, CHW), dst frame padding, dst offset in bytes
SHAPES = [
    (1, 1, None, (0, 0), 0, 0),            # one pixel: the byte path, a row tail and nothing else
    (5, 7, None, (0, 0), 0, 0),            # rows of 21 / 7 bytes: one whole group and a tail of three pixels, bytes
    (16, 64, None, (0, 0), 4, 0),          # exactly one tile: whole dwords, no tail
    (17, 65, None, (1, 3), 8, 0),          # one pixel and one row more than a tile: four tiles, dwords plus a tail (rows of 196 / 68 bytes)
    (70, 130, None, (2, 2), 0, 0),         # 3 x 5 tiles, the last ones partial in x and in y; dwords plus a tail
    (16, 64, None, (0, 0), 4, 1),          # the one tile one byte off: the byte path
    (16, 64, None, (0, 0), 2, 0),          # aligned base and rows, but a frame stride that is no multiple of 4: bytes (for F > 1)
    (17, 65, (23, 40), (0, 0), 0, 0),      # another output size (whole dwords: 120 / 40 bytes a row)
    (16, 64, (70, 130), (2, 2), 4, 0),     # a larger output than the source
]


@pytest.mark.parametrize("direction", (R.TO_IDEAL, R.TO_SENSOR))
@pytest.mark.parametrize("border", (R.FILL, R.EDGE))
@pytest.mark.parametrize("layout", (R.HWC, R.CHW))
@pytest.mark.parametrize("H,W,size,row_pad,frame_pad,off", SHAPES)
def test_frames_kernel_against_the_restatement(H, W, size, row_pad, frame_pad, off, layout, border, direction):
    rng = np.random.default_rng(H * W + layout)
    fill = (17, 130, 251)
    outside = False
    for F in (1, 3):
        pics = rng.integers(0, 256, (F, H, W, 3) if layout == R.HWC else (F, 3, H, W), dtype=np.uint8)
        fold = 1920.0 / W * 0.5 * np.hypot(W, H) / 1.6  # the folding polynomial turns at a radius of 1.52: the corners lie at 1.6
        for k, f in ((ACTION_K, 1000.0), (R.LENSES["pincushion"][0], 1000.0), (R.FOLDING[0], fold)):
            lens = small_lens(k, f, (H, W), size)
            raw_frames(pics, lens, direction, size, border, fill, layout, src_pad=(3, 5), dst_pad=(row_pad[layout], frame_pad), dst_off=off)
            outside = outside or not R.source_positions(lens, direction, 0.01, *(size or (H, W)))[0].all()
        # the zero lens copies bit for bit (on equal sizes), from dense source rows too
        zero = R.lens13(R.ZERO, 37.5, ((W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2))
        out = raw_frames(pics, zero, direction, None, border, fill, layout, dst_pad=(row_pad[layout], frame_pad), dst_off=off)
        assert np.array_equal(out, pics)
    assert outside or min(H, W) < 16  # the folding lens leaves the corners of every picture that has corners without a source


def test_frames_slices_of_pictures():
    """How the pictures of a launch are dealt to grid z.  Eight pictures of 270 x 480 make 8 x 17 = 136 tiles: eight slices, one picture
    each.  Forty pictures of 64 x 64 make four tiles: forty slices.  At 1080p the 30 x 68 tiles alone fill the device and ONE slice
    walks all the pictures with the map it made once; every byte of every picture, both directions."""
    rng = np.random.default_rng(1)
    for (F, H, W), f in (((8, 270, 480), 250.0), ((40, 64, 64), 40.0)):
        pics = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
        raw_frames(pics, R.lens13(ACTION_K, f, ((W - 1) / 2, (H - 1) / 2)), R.TO_IDEAL, None, R.FILL, (1, 2, 3), R.HWC)
    pics = rng.integers(0, 256, (3, 1080, 1920, 3), dtype=np.uint8)
    raw_frames(pics, R.lens13(ACTION_K, 1000.0), R.TO_IDEAL, None, R.EDGE, (1, 2, 3), R.HWC)
    raw_frames(pics[:2].transpose(0, 3, 1, 2).copy(), R.lens13(ACTION_K, 1000.0), R.TO_SENSOR, None, R.FILL, (9, 8, 7), R.CHW)


def point_cases(rng, G, F, N, span=(2070.0, 1170.0)):
    p = rng.uniform((-150.0, -90.0), span, (G, F, N, 2)).astype(np.float32)
    flat = p.reshape(-1, 2)
    special = np.array([(np.nan, 5.0), (5.0, np.nan), (np.inf, 0.0), (0.0, -np.inf), (32769.0, 0.0), (3.0e38, 1.0), (32768.0, -32768.0),
                        (959.5, 539.5)], dtype=np.float32)
    n = min(len(special), len(flat) - 1) if len(flat) > 1 else 0
    flat[len(flat) - n:] = special[:n]
    return p


def raw_points(src, lens, direction, label=True, in_place=False, strides=None, tol=0.01):
    """The C-ABI call itself on a NaN-framed source and a poisoned, NaN-framed destination with strides of their own -> (dst, label) as
    numpy, after checking the frames, the gaps between the rows and the source."""
    from cotracker_amd import _lib as L
    G, F, N, _ = src.shape
    fs, gs = strides or (2 * N, 2 * N * F)
    flat = np.full((G - 1) * gs + (F - 1) * fs + 2 * N, np.float32(-7.5), dtype=np.float32)
    view = np.lib.stride_tricks.as_strided(flat, shape=(G, F, N, 2), strides=(4 * gs, 4 * fs, 8, 4))
    view[...] = src
    src_d, src_all = nan_framed(torch.from_numpy(flat), pattern=NAN_PATTERN, whole=True)
    before = src_all.clone()
    if in_place:
        dst_d, dst_all = src_d, src_all
    else:
        dst_d, dst_all = nan_framed(torch.full((flat.size,), -3.25), pattern=NAN_PATTERN, whole=True)
    lab = torch.full((G, F, N), 77, dtype=torch.int8, device=dev()) if label else None
    a = L.Lens.PointsArgs()
    a.G, a.F, a.N, a.direction, a.tol, a.reserved = G, F, N, direction, tol, 0
    a.src_group_stride = a.dst_group_stride = gs
    a.src_frame_stride = a.dst_frame_stride = fs
    bind(a.lens, lens)
    a.src, a.dst, a.label = src_d.data_ptr(), dst_d.data_ptr(), None if lab is None else lab.data_ptr()
    res, rows_ = recorded(lambda: L.load().ctk_lens_points(C.byref(a), torch.cuda.current_stream().cuda_stream))
    L.check(res, "ctk_lens_points")
    torch.cuda.synchronize()
    assert rows_ == {"lens_points": 1}
    assert frame_intact(dst_all, dst_d) and frame_intact(src_all, src_d)
    if not in_place:
        assert torch.equal(src_all.view(torch.int32), before.view(torch.int32))  # the input is only read
    got_flat = dst_d.cpu().numpy()
    got = np.lib.stride_tricks.as_strided(got_flat, shape=(G, F, N, 2), strides=(4 * gs, 4 * fs, 8, 4)).copy()
    # what lies between the rows kept its value
    touched = np.zeros(flat.size, dtype=bool)
    np.lib.stride_tricks.as_strided(touched, shape=(G, F, N, 2), strides=(gs, fs, 2, 1))[...] = True
    assert (got_flat[~touched] == (np.float32(-7.5) if in_place else np.float32(-3.25))).all()
    return got, None if lab is None else lab.cpu().numpy()


@pytest.mark.parametrize("direction", (R.TO_IDEAL, R.TO_SENSOR))
@pytest.mark.parametrize("N", (1, 63, 64, 65, 300))
def test_points_kernel_against_the_restatement(N, direction):
    rng = np.random.default_rng(N + direction)
    lenses = [R.lens13(k, f) for k, f in (R.LENSES["action"], R.LENSES["pincushion"], R.LENSES["mixed"], R.FOLDING)]
    zeros = 0
    for i, (G, F) in enumerate(((1, 1), (2, 3), (1, 3), (2, 1))):
        src = point_cases(rng, G, F, N)
        lens = lenses[i % len(lenses)] if N < 300 else lenses[3]
        want, wlab = R.lens_points(src, lens, direction)
        for kw in (dict(), dict(strides=(2 * N + 6, (2 * N + 6) * F + 10)), dict(in_place=True), dict(label=False),
                   dict(in_place=True, label=False, strides=(2 * N + 2, (2 * N + 2) * F))):
            got, lab = raw_points(src, lens, direction, **kw)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (G, F, kw)
            assert lab is None or np.array_equal(lab, wlab), (G, F, kw)
        zeros += int((wlab == 0).sum())
        if G * F * N > 8:
            assert (wlab == -1).sum() == 6 and (wlab == 1).sum() > 0
    if N == 300:
        assert zeros > 0  # the folding lens: positions in the enlarged corners have no image


def test_ops_layer():
    from cotracker_amd import ops
    rng = np.random.default_rng(3)
    k, f = R.LENSES["action"]
    H, W, Ho, Wo = 40, 64, 50, 72
    lens13 = small_lens(k, f, (H, W), (Ho, Wo))
    lens = ops.Lens(tuple(lens13[:4]), k, ideal=tuple(lens13[4:8]))
    pics = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    # frames: both layouts, both directions, a size, a cropped source (a view with a pitch) and an out with a pitch
    for to, direction in (("ideal", R.TO_IDEAL), ("sensor", R.TO_SENSOR)):
        out, rows = recorded(lambda: ops.lens_frames(t(pics), lens, to=to, size=(Ho, Wo), border="edge", fill=(1, 2, 3)))
        assert rows == {"lens_frames": 1} and out.dtype == torch.uint8 and tuple(out.shape) == (3, Ho, Wo, 3)
        assert np.array_equal(out.cpu().numpy(), R.lens_frames(pics, lens13, direction, (Ho, Wo), R.EDGE, (1, 2, 3)))
        chw = np.ascontiguousarray(pics.transpose(0, 3, 1, 2))
        big = torch.zeros(3, 3, Ho, Wo + 5, dtype=torch.uint8, device=dev())
        res = ops.lens_frames(t(chw), lens, to=to, size=(Ho, Wo), out=big[:, :, :, :Wo], fill=(9, 8, 7))
        assert res.data_ptr() == big.data_ptr()
        assert np.array_equal(res.cpu().numpy(), R.lens_frames(chw, lens13, direction, (Ho, Wo), R.FILL, (9, 8, 7), layout=R.CHW))
        assert not big[:, :, :, Wo:].any()
    same = ops.Lens(tuple(lens13[:4]), R.ZERO)
    src = t(pics)
    assert torch.equal(ops.lens_frames(src, same), src)  # the zero lens, a bit-for-bit copy
    with pytest.raises(RuntimeError, match="ctk_lens_frames"):  # in place: refused by the library
        ops.lens_frames(src, same, out=src[:])
    with pytest.raises(ValueError, match="out must be"):
        ops.lens_frames(src, same, out=src)
    with pytest.raises(ValueError, match="to must be"):
        ops.lens_frames(src, same, to="pinhole")
    with pytest.raises(ValueError, match="tol"):
        ops.lens_frames(src, same, tol=0.0)
    # points: every leading shape, labels, in place
    big13 = R.lens13(k, f)
    blens = ops.Lens(tuple(big13[:4]), k)
    for shape in ((7, 2), (5, 7, 2), (2, 5, 7, 2), (2, 1, 5, 7, 2)):
        p = point_cases(rng, 1, 1, int(np.prod(shape[:-1]))).reshape(shape)
        for to, direction in (("ideal", R.TO_IDEAL), ("sensor", R.TO_SENSOR)):
            want, wlab = R.lens_points(p, big13, direction)
            (got, lab), rows = recorded(lambda: ops.lens_points(t(p), blens, to=to, labels=True))
            assert rows == {"lens_points": 1} and tuple(lab.shape) == shape[:-1] and lab.dtype == torch.int8
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)) and np.array_equal(lab.cpu().numpy(), wlab)
            x = t(p)
            assert ops.lens_points(x, blens, to=to, out=x) is x and np.array_equal(x.cpu().numpy().view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError, match="contiguous"):
        ops.lens_points(t(p)[..., ::2, :], blens)


# ---- the predictor: a pushed stream that lives in ideal pixels -----------------------------------------------------------------------------
RAW = (96, 144)


def small_predictor():
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    from cotracker_amd.weights import fill_synthetic_
    from cotracker_amd.model import CoTrackerThreeOnline
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=S)
    model = CoTrackerThreeOnline(stride=STRIDE, corr_radius=3, window_len=S, model_resolution=HW).eval()
    fill_synthetic_(model, seed=5)
    model.hip_graph, model.batch_mode = True, "loop"
    p.model, p.interp_shape, p.step = model, HW, STEP
    return p.to(dev())


def test_stream_with_a_lens(monkeypatch):
    """Raw uint8 frames pushed into a predictor with the action lens give the tracks, bit for bit, of ops.lens_frames(raw, lens) pushed
    into one without; the zero lens gives the tracks of no lens; a push is one launch more and nothing else: no capture, no
    allocation after the first push.  to_sensor is ops.lens_points(to="sensor"), undistort is ops.lens_frames."""
    from cotracker_amd import ops
    from cotracker_amd.synthetic import synthetic_video
    T = S + 3 * STEP
    video = synthetic_video(T, *RAW, seed=11)[0].permute(0, 2, 3, 1).round().to(torch.uint8).contiguous().to(dev())
    g = torch.Generator().manual_seed(2)
    q = (torch.rand(1, 6, 3, generator=g) * torch.tensor([1.0, RAW[1] - 1.0, RAW[0] - 1.0])).to(dev())
    q[..., 0] = 0.0
    H, W = RAW
    cam = (W * 1000.0 / 1920.0, W * 1000.0 / 1920.0, (W - 1) / 2, (H - 1) / 2)
    lens, zero = ops.Lens(cam, ACTION_K), ops.Lens(cam, R.ZERO)
    captures = []
    orig = ops.WindowGraph._capture

    def counting(self, *a, **k):
        captures.append(1)
        return orig(self, *a, **k)
    monkeypatch.setattr(ops.WindowGraph, "_capture", counting)
    resampled, lens_frames = [], ops.lens_frames

    def counted(frames, *a, **k):
        resampled.append(int(frames.shape[0]))
        return lens_frames(frames, *a, **k)
    preds = {name: small_predictor() for name in ("none", "lens", "ideal", "zero")}
    preds["lens"].lens, preds["zero"].lens = lens, zero
    for p in preds.values():
        p(torch.zeros(1, 1, 3, H, W, device=dev()), is_first_step=True, queries=q)
    fixed = ops.lens_frames(video, lens)
    assert (fixed != video).any()
    monkeypatch.setattr(ops, "lens_frames", counted)  # (test_ops_layer shows that one call is one launch)
    outs, counts, where = {name: [] for name in preds}, {name: [] for name in preds}, {}
    for k, i in enumerate([0] + list(range(S, T, STEP))):
        n = S if k == 0 else STEP
        for name, p in preds.items():
            src = fixed if name == "ideal" else video
            c0, r0 = len(captures), len(resampled)
            res = p.push_frames(src[i:i + n])
            counts[name].append(len(captures) - c0)
            assert resampled[r0:] == ([n] if name in ("lens", "zero") else []), (name, k)  # one launch more per push, or none
            bufs = (p._push_buf.data_ptr(), None if p._lens_buf is None else p._lens_buf.data_ptr())
            assert where.setdefault(name, bufs) == bufs, (name, k)  # nothing is allocated again after the first push
            outs[name].append(res)
        with pytest.raises(RuntimeError, match="pushed stream is running"):
            preds["lens"].lens = None
    for name in preds:
        assert counts[name] == counts["none"], (name, counts)  # nothing is captured that a stream without a lens does not capture
    for a, b in (("lens", "ideal"), ("zero", "none")):
        for x, y in zip(outs[a], outs[b]):
            assert torch.equal(x[0].view(torch.int32), y[0].view(torch.int32)) and torch.equal(x[1], y[1]), (a, b)
    assert not torch.equal(outs["lens"][-1][0], outs["none"][-1][0])
    assert preds["none"]._lens_buf is None and tuple(preds["lens"]._lens_buf.shape) == (S, H, W, 3)
    p = preds["lens"]
    tracks = outs["lens"][-1][0]
    got, lab = p.to_sensor(tracks, labels=True)
    want, wlab = ops.lens_points(tracks.contiguous(), lens, to="sensor", labels=True)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(lab, wlab)
    ref, rlab = R.lens_points(tracks.cpu().numpy(), np.array(cam + cam + ACTION_K), R.TO_SENSOR)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32)) and np.array_equal(lab.cpu().numpy(), rlab)
    monkeypatch.setattr(ops, "lens_frames", lens_frames)
    assert torch.equal(p.undistort(video[:3]), fixed[:3]) and torch.equal(p.undistort(video[1]), fixed[1])
    for x in preds.values():
        x.finish()
