"""ctk_warp_frames and ctk_smooth_path on the GPU (csrc/warp.hip) against the numpy restatement of tests/warp_reference.py: every byte of
the poisoned, fenced destination, pitch padding included, and every float32 / float64 bit.  The shapes are the smallest at which the
kernel takes each of its paths: bytes with a row tail, whole dwords, dwords plus a tail, a destination off by one byte, several
tiles with partial ones at both edges, source rows of every alignment, a source box that fits the LDS and one that does not; then 64-bit offsets at 1080p, the ops layer on a planted sequence and the predictor on a pushed
ring stream."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_reference as MR
import warp_reference as R
from ctk_support import HW, S, STEP, STRIDE, dev, recorded, t

pytestmark = pytest.mark.gpu

GUARD, POISON, FENCE = 64, 0x5A, 0xA5
ONE = {"fit_motion": 1, "smooth_path": 1, "warp_frames": 1}


def rows_view(buf, offset, F, rows, row_bytes, frame_stride, row_stride):
    """The pixel bytes of a strided surface inside the flat uint8 array buf as [F, rows, row_bytes] (rows: H, or 3 H planar)."""
    assert offset + (F - 1) * frame_stride + (rows - 1) * row_stride + row_bytes <= buf.size
    return np.lib.stride_tricks.as_strided(buf[offset:], shape=(F, rows, row_bytes), strides=(frame_stride, row_stride, 1))


def dev_library():
    """The dev build of the library (make dev): it alone carries the direct form of the warp kernel, ctk_debug_warp_frames_direct."""
    import os
    from cotracker_amd import _lib as L
    lib = C.CDLL(os.path.join(os.path.dirname(L.LIB_PATH), "libctk_hip_dev.so"))
    lib.ctk_debug_warp_frames_direct.restype, lib.ctk_debug_warp_frames_direct.argtypes = C.c_int, [C.POINTER(L.Warp.Args), C.c_void_p]
    return lib


def raw_warp(pics, matrices, border, fill, layout, src_pad=(0, 0), dst_pad=(0, 0), dst_off=0, direct=False):
    """The C-ABI call itself: pics uint8 [F,H,W,3] / [F,3,H,W] laid out with rows padded by pad[0] and frames by pad[1] elements, the
    destination poisoned, fenced and `dst_off` bytes off its 256-byte aligned allocation.  Checks every byte of the destination
    against the restatement (padding: still the poison), the fences and the source, and returns the warped pictures."""
    from cotracker_amd import _lib as L
    F = pics.shape[0]
    H, W = pics.shape[1:3] if layout == R.HWC else pics.shape[2:4]
    rows, row_bytes = (H, 3 * W) if layout == R.HWC else (3 * H, W)
    geo = []
    for pad in (src_pad, dst_pad):
        rs = row_bytes + pad[0]
        geo.append((rs, rows * rs + pad[1]))
    (srs, sfs), (drs, dfs) = geo
    rng = np.random.default_rng(F * H + W)
    src = rng.integers(0, 256, F * sfs, dtype=np.uint8)  # (what lies between the rows is noise: it must not be read)
    rows_view(src, 0, F, rows, row_bytes, sfs, srs)[...] = pics.reshape(F, rows, row_bytes)
    nd = (F - 1) * dfs + (rows - 1) * drs + row_bytes
    want = np.full(GUARD + dst_off + nd + GUARD, FENCE, dtype=np.uint8)
    want[GUARD + dst_off:GUARD + dst_off + nd] = POISON
    src_d, m_d = t(src), t(np.ascontiguousarray(matrices, dtype=np.float32).reshape(F, 2, 3))
    whole = torch.empty(256 + want.size, dtype=torch.uint8, device=dev())
    base = (-(whole.data_ptr() + GUARD)) % 256  # the destination proper starts dst_off bytes behind a 256-byte boundary
    buf = whole[base:base + want.size]
    buf.copy_(t(want))
    assert (buf.data_ptr() + GUARD) % 256 == 0
    a = L.Warp.Args()
    a.F, a.H, a.W, a.layout, a.border, a.reserved = F, H, W, layout, border, 0
    for k in range(3):
        a.fill[k] = fill[k]
    a.src_frame_stride, a.src_row_stride, a.dst_frame_stride, a.dst_row_stride = sfs, srs, dfs, drs
    a.matrices, a.src, a.dst = m_d.data_ptr(), src_d.data_ptr(), buf.data_ptr() + GUARD + dst_off
    if direct:  # (the dev library has a recorder of its own: the launch is not counted here)
        L.check(dev_library().ctk_debug_warp_frames_direct(C.byref(a), torch.cuda.current_stream().cuda_stream), "ctk_debug_warp_frames_direct")
        torch.cuda.synchronize()
    else:
        res, rows_ = recorded(lambda: L.load().ctk_warp_frames(C.byref(a), torch.cuda.current_stream().cuda_stream))
        L.check(res, "ctk_warp_frames")
        torch.cuda.synchronize()
        assert rows_ == {"warp_frames": 1}
    ref = R.warp_frames(pics, matrices, border, fill, layout)
    rows_view(want, GUARD + dst_off, F, rows, row_bytes, dfs, drs)[...] = ref.reshape(F, rows, row_bytes)
    got = buf.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert np.array_equal(src_d.cpu().numpy(), src)
    return ref


def five_matrices(H, W):
    """The identity, a sub-pixel shift, 7 degrees with scale 1.1 about the centre, a shift that puts every tap outside, a NaN matrix."""
    m = np.stack([R.IDENTITY.reshape(2, 3), np.array([[1, 0, 0.37], [0, 1, -0.61]], dtype=np.float32),
                  R.similarity(np.deg2rad(7.0), 1.1, (0.0, 0.0), ((W - 1) / 2, (H - 1) / 2)),
                  np.array([[1, 0, W + 5], [0, 1, 0]], dtype=np.float32), R.IDENTITY.reshape(2, 3)]).astype(np.float32)
    m[4, 1, 1] = np.nan
    return m


def seven_matrices(H, W):
    """five_matrices, whose source box of a 64 x 16 tile fits the LDS (7 degrees, scale 1.1: about 75 x 27 pixels), then one whose box
    does not and takes the fallback to memory (scale 6: about 390 x 170 pixels a tile) and one that shrinks (scale 0.3)."""
    return np.concatenate([five_matrices(H, W), R.similarity(0.2, 6.0, (0.0, 0.0), ((W - 1) / 2, (H - 1) / 2))[None],
                           R.similarity(-0.1, 0.3, (1.5, 2.25), ((W - 1) / 2, (H - 1) / 2))[None]])


# H, W, dst row padding per layout (HWC, CHW), dst frame padding, dst offset in bytes
SHAPES = [
    (37, 53, (0, 0), 0, 0),      # rows of 159 / 53 bytes: the byte path, a row tail of one pixel
    (40, 64, (8, 8), 4, 0),      # padded rows of 200 / 72 bytes: whole dwords, no tail
    (40, 66, (2, 2), 8, 0),      # rows of 200 / 68 bytes: whole dwords plus a tail of two pixels
    (40, 64, (8, 8), 4, 1),      # the same surface one byte off: the byte path
    (70, 130, (2, 2), 0, 0),     # 3 x 5 tiles of 64 x 16, the last ones partial in x and in y; dwords plus a tail
    (40, 64, (8, 8), 2, 0),      # aligned base and rows, but a frame stride that is no multiple of 4: the byte path again
]


@pytest.mark.parametrize("border", (R.FILL, R.EDGE))
@pytest.mark.parametrize("layout", (R.HWC, R.CHW))
@pytest.mark.parametrize("H,W,row_pad,frame_pad,off", SHAPES)
def test_kernel_against_the_restatement(H, W, row_pad, frame_pad, off, layout, border):
    rng = np.random.default_rng(H * W + layout)
    pics = rng.integers(0, 256, (7, H, W, 3) if layout == R.HWC else (7, 3, H, W), dtype=np.uint8)
    m = seven_matrices(H, W)
    out = raw_warp(pics, m, border, (17, 130, 251), layout, src_pad=(3, 5), dst_pad=(row_pad[layout], frame_pad), dst_off=off)
    raw_warp(pics, m, border, (17, 130, 251), layout, src_pad=(0, 0), dst_pad=(row_pad[layout], frame_pad), dst_off=off)  # (dense source rows)
    assert np.array_equal(out[0], pics[0]) and np.array_equal(out[4], pics[4])  # the identity and the NaN matrix copy
    hwc = out if layout == R.HWC else out.transpose(0, 2, 3, 1)
    if border == R.FILL:
        assert (hwc[3] == (17, 130, 251)).all()
    else:
        src_hwc = pics if layout == R.HWC else pics.transpose(0, 2, 3, 1)
        assert np.array_equal(hwc[3], np.broadcast_to(src_hwc[3][:, -1:], hwc[3].shape))
    assert (out[1] != pics[1]).any() and (out[2] != pics[2]).any()


@pytest.mark.parametrize("border", (R.FILL, R.EDGE))
@pytest.mark.parametrize("layout", (R.HWC, R.CHW))
@pytest.mark.parametrize("H,W,row_pad,frame_pad,off", SHAPES)
def test_direct_dev_kernel_against_the_restatement(H, W, row_pad, frame_pad, off, layout, border):
    """The direct form (dev library only; DESIGN.md has the measurement that kept the staged one) gives the same bytes: the time
    recorded for it is the time of the same work."""
    rng = np.random.default_rng(H * W + layout + 50)
    pics = rng.integers(0, 256, (7, H, W, 3) if layout == R.HWC else (7, 3, H, W), dtype=np.uint8)
    raw_warp(pics, seven_matrices(H, W), border, (17, 130, 251), layout, src_pad=(3, 5), dst_pad=(row_pad[layout], frame_pad), dst_off=off,
             direct=True)


def test_64_bit_offsets_at_1080p():
    """Two 1080 x 1920 HWC pictures whose frame stride lies beyond the frame: the byte offset of the last row of picture 1 is the
    product of 64-bit factors.  One picture turns a little, the other shifts by whole pixels."""
    H, W = 1080, 1920
    rng = np.random.default_rng(7)
    pics = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    m = np.stack([R.similarity(0.01, 1.02, (3.25, -2.5), ((W - 1) / 2, (H - 1) / 2)), np.array([[1, 0, -7], [0, 1, 5]], dtype=np.float32)])
    out = raw_warp(pics, m, R.EDGE, (0, 0, 0), R.HWC, src_pad=(64, 4096), dst_pad=(0, 8192))
    assert np.array_equal(out[1, :H - 5, 7:], pics[1, 5:, :W - 7])


def raw_path(motion, state, alpha, post):
    """ctk_smooth_path on a poisoned, fenced `warp` and a fenced state -> (warp, state after) as numpy."""
    from cotracker_amd import _lib as L
    G, F = motion.shape[:2]
    w_whole = torch.full((G * F * 24 + 2 * GUARD,), FENCE, dtype=torch.uint8, device=dev())
    w_whole[GUARD:-GUARD] = POISON
    s_np = np.full(G * 48 + 2 * GUARD, FENCE, dtype=np.uint8)
    s_np[GUARD:-GUARD] = np.ascontiguousarray(state, dtype=np.float64).view(np.uint8).reshape(-1)
    s_whole = t(s_np)
    m_d = t(np.ascontiguousarray(motion, dtype=np.float32))
    p_d = None if post is None else t(np.ascontiguousarray(post, dtype=np.float32))
    a = L.Warp.PathArgs()
    a.G, a.F, a.alpha, a.reserved = G, F, alpha, 0
    a.motion, a.post, a.state, a.warp = m_d.data_ptr(), None if p_d is None else p_d.data_ptr(), s_whole.data_ptr() + GUARD, w_whole.data_ptr() + GUARD
    assert a.state % 8 == 0
    res, rows = recorded(lambda: L.load().ctk_smooth_path(C.byref(a), torch.cuda.current_stream().cuda_stream))
    L.check(res, "ctk_smooth_path")
    torch.cuda.synchronize()
    assert rows == {"smooth_path": 1}
    for whole in (w_whole, s_whole):
        assert bool((whole[:GUARD] == FENCE).all()) and bool((whole[-GUARD:] == FENCE).all())
    assert same_bits(m_d.cpu().numpy(), np.ascontiguousarray(motion, dtype=np.float32))
    return (w_whole[GUARD:-GUARD].cpu().numpy().view(np.float32).reshape(G, F, 2, 3), s_whole[GUARD:-GUARD].cpu().numpy().view(np.float64).reshape(G, 6))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("G,F", [(1, 1), (1, 9), (3, 1), (3, 9)])
@pytest.mark.parametrize("with_post", (False, True))
def test_smooth_path_against_the_restatement(G, F, with_post):
    rng = np.random.default_rng(G * 10 + F)
    motion = np.stack([[R.similarity(rng.uniform(-0.05, 0.05), rng.uniform(0.95, 1.05), rng.uniform(-6, 6, 2), (48, 32)) for _ in range(2 * F)]
                       for _ in range(G)])
    if F > 1:
        motion[0, 3, 1, 0], motion[G - 1, F + 1, 0, 2] = np.nan, np.inf  # count as the identity
    post = R.zoom_matrix(64, 96, 1.15) if with_post else None
    ident = np.tile(R.IDENTITY.astype(np.float64), (G, 1))
    for alpha in (0.1, 0.0, 1.0):
        w0, s0 = raw_path(motion[:, :F], ident, alpha, post)
        w1, s1 = raw_path(motion[:, F:], s0, alpha, post)  # the state carried across two calls
        want_w, want_s = R.smooth_path(motion, None, alpha, post)
        half_w, half_s = R.smooth_path(motion[:, :F], None, alpha, post)
        assert same_bits(w0, half_w) and same_bits(s0, half_s), alpha
        assert same_bits(np.concatenate([w0, w1], axis=1), want_w) and same_bits(s1, want_s), alpha
        assert np.isfinite(want_w).all()


def test_ops_layer_on_the_planted_sequence():
    from cotracker_amd import ops
    frames, tracks, off = R.planted(seed=4)
    T, N = tracks.shape[:2]
    fr, tr, vi = t(frames), t(tracks), torch.ones(T, N, dtype=torch.bool, device=dev())
    for model in ("translation", "similarity"):
        (out, warp, state), rows = recorded(lambda: ops.stabilize(fr, tr, vi, alpha=0.0, fill=(255, 0, 255), model=model, min_base=8.0))
        assert rows == ONE  # three launches, one each
        assert tuple(warp.shape) == (T, 2, 3) and tuple(state.shape) == (1, 6) and state.dtype == torch.float64
        w, o = warp.cpu().numpy(), out.cpu().numpy()
        seen = 0
        for f in range(T):
            d = off[0] - off[f]
            assert np.array_equal(w[f], np.array([[1, 0, d[0]], [0, 1, d[1]]], dtype=np.float32)), (model, f)
            inside = R.taps_inside(w[f], *frames.shape[1:3])
            assert np.array_equal(o[f][inside], frames[0][inside]), (model, f)  # frame 0 bit for bit wherever the taps lie inside
            seen += int(inside.sum())
        assert seen > T * frames.shape[1] * frames.shape[2] // 2
        assert np.array_equal(o, R.warp_frames(frames, w, R.FILL, (255, 0, 255)))
        assert np.array_equal(fr.cpu().numpy(), frames)
    # the pieces on their own: planar frames into a strided `out`, the edge border, a zoom, the state carried on
    motion = t(np.stack([R.similarity(0.02 * k, 1.0 + 0.01 * k, (k, -k), (32, 24)) for k in range(T)]))
    w_all, s_all = ops.smooth_path(motion, alpha=0.25, post=ops.zoom_matrix(48, 64, 1.2))
    w0, s0 = ops.smooth_path(motion[:3], alpha=0.25, post=ops.zoom_matrix(48, 64, 1.2))
    s_before = s0.data_ptr()
    w1, s1 = ops.smooth_path(motion[3:], s0, alpha=0.25, post=ops.zoom_matrix(48, 64, 1.2))
    assert s1 is s0 and s1.data_ptr() == s_before  # the state that comes back is the tensor that was updated in place
    want_w, want_s = R.smooth_path(motion.cpu().numpy()[None], None, 0.25, R.zoom_matrix(48, 64, 1.2))
    assert same_bits(torch.cat([w0, w1]).cpu().numpy(), want_w[0]) and same_bits(w_all.cpu().numpy(), want_w[0])
    assert same_bits(s1.cpu().numpy(), want_s) and same_bits(s_all.cpu().numpy(), want_s)
    chw = fr.permute(0, 3, 1, 2).contiguous()
    big = torch.full((T, 3, 48, 72), POISON, dtype=torch.uint8, device=dev())
    res = ops.warp_frames(chw, w_all, out=big[..., 4:68], border="edge")
    assert res.data_ptr() == big[..., 4:68].data_ptr()
    b = big.cpu().numpy()
    assert (b[..., :4] == POISON).all() and (b[..., 68:] == POISON).all()
    assert np.array_equal(b[..., 4:68], R.warp_frames(chw.cpu().numpy(), want_w[0], R.EDGE, (0, 0, 0), R.CHW))
    for bad in (dict(out=chw), dict(border="wrap"), dict(fill=(0, 0)), dict(fill=(0, 0, 256)), dict(layout="hwc"), dict(out=big)):
        with pytest.raises(ValueError):
            ops.warp_frames(chw, w_all, **bad)
    with pytest.raises(ValueError):
        ops.warp_frames(chw, w_all[:3])
    with pytest.raises(ValueError, match="overlaps"):  # refused before anything is launched
        ops.warp_frames(big[..., 0:64], w_all, out=big[..., 4:68])
    for bad in (dict(alpha=1.5), dict(alpha=float("nan")), dict(state=torch.zeros(2, 6, dtype=torch.float64, device=dev())),
                dict(state=torch.zeros(1, 6, device=dev())), dict(post=torch.zeros(3, 3)), dict(out=torch.zeros(T, 6, device=dev()))):
        with pytest.raises(ValueError):
            ops.smooth_path(motion, **bad)


# ---- the predictor ------------------------------------------------------------------------------------------------------------------
RAW = (100, 140)


def small_predictor(history, spare):
    from cotracker_amd.model import CoTrackerThreeOnline
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    from cotracker_amd.weights import fill_synthetic_
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=S)
    model = CoTrackerThreeOnline(stride=STRIDE, corr_radius=3, window_len=S, model_resolution=HW).eval()
    fill_synthetic_(model, seed=5)
    model.hip_graph, model.batch_mode = True, "loop"
    p.model, p.interp_shape, p.step = model, HW, STEP
    p.spare_points, p.history_frames = spare, history
    return p.to(dev())


def test_stabilize_on_a_push_stream(monkeypatch):
    """Ring + graph on, frames pushed as uint8.  stabilize reads the stream's own history and logits; what it is compared with is the
    restatement chain -- motion_reference.fit_motion on the history as recent() emits it, warp_reference.smooth_path with the state
    carried from call to call, warp_reference.warp_frames on the raw frames."""
    from cotracker_amd import ops
    from cotracker_amd.synthetic import synthetic_video
    K, G, N, spare = 32, 2, 6, 2
    T = S + 9 * STEP  # 44 frames: the ring of 32 rows has wrapped
    video = synthetic_video(T, *RAW, seed=11)[0].permute(0, 2, 3, 1).round().to(torch.uint8).contiguous().to(dev())
    video_np = video.cpu().numpy()
    g = torch.Generator().manual_seed(2)
    q = torch.rand(G, N, 3, generator=g) * torch.tensor([1.0, RAW[1] - 1.0, RAW[0] - 1.0])
    q[..., 0] = torch.tensor([0.0, 0.0, 2.0, 5.0, 9.0, 30.0])
    q = q.to(dev())
    captures = []
    orig = ops.WindowGraph._capture

    def counting(self, *a, **k):
        captures.append(1)
        return orig(self, *a, **k)
    monkeypatch.setattr(ops.WindowGraph, "_capture", counting)
    p, twin = small_predictor(K, spare), small_predictor(K, spare)
    for x in (p, twin):
        x(torch.zeros(1, 1, 3, *RAW, device=dev()), is_first_step=True, queries=q, add_support_grid=True)
    with pytest.raises(RuntimeError, match="no stream is running"):
        p.stabilize(video[:STEP])
    Nu = N + spare
    fit = dict(tol=4.0, min_base=4.0, hypotheses=64, seed=3)

    def want_motion(f0, F_, group):
        done = p.model._gstream.committed
        tr, vi = p.recent(min(done, K))
        base = done - tr.shape[1]
        ring_c, ring_v = np.zeros((G, K, Nu, 2), dtype=np.float32), np.zeros((G, K, Nu), dtype=np.uint8)
        for i in range(tr.shape[1]):
            ring_c[:, (base + i) % K], ring_v[:, (base + i) % K] = tr[:, i].cpu().numpy(), vi[:, i].cpu().numpy()
        first = None if p._first_row is None else np.clip(p._first_row.cpu().numpy(), 0, MR.INT32_MAX)
        return MR.fit_motion(ring_c, visible=ring_v, first_row=first, f0=f0, F=F_, tol=4.0, min_base=4.0, K=64, seed=3)[0][group:group + 1]

    def want(f0, F_, group, state, alpha, post=None, border=R.FILL, fill=(0, 0, 0)):
        motion = want_motion(f0, F_, group)
        if state is None:  # a fresh path locks onto frame f0: the motion into it is not part of the path
            motion[0, 0] = R.IDENTITY.reshape(2, 3)
        warp, state = R.smooth_path(motion, state, alpha, post)
        kept["moved"] = kept.get("moved", False) or post is None and bool((warp[0] != R.IDENTITY.reshape(2, 3)).any())
        return R.warp_frames(video_np[f0:f0 + F_], warp[0], border, fill), warp[0], state
    calls, kept = 0, {}
    for k, t0 in enumerate(range(0, T - S + 1, STEP)):
        new = video[:S] if k == 0 else video[t0 + S - STEP:t0 + S]
        c0 = len(captures)
        got = p.push_frames(new, add_support_grid=True)
        c1 = len(captures)
        ref = twin.push_frames(new, add_support_grid=True)
        assert len(captures) - c1 == c1 - c0, (k, c0, c1, len(captures))  # nothing is re-captured: the twin, which never asks, captures as often
        # the tracks of the stream are bit-identical with and without the stabilize calls in between
        assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(got[1], ref[1]), k
        done = p.model._gstream.committed
        if k == 3:  # the first call for group 0: locks onto frame done - 4
            (out, warp), rows = recorded(lambda: p.stabilize(video[done - STEP:done], alpha=0.2, **fit))
            assert rows == ONE and len(captures) == c1 + (c1 - c0)
            assert tuple(out.shape) == (STEP, *RAW, 3) and out.dtype == torch.uint8 and tuple(warp.shape) == (STEP, 2, 3)
            w_out, w_warp, state = want(done - STEP, STEP, 0, None, 0.2)
            assert np.array_equal(out.cpu().numpy(), w_out) and same_bits(warp.cpu().numpy(), w_warp)
            assert torch.equal(out[0], video[done - STEP]) and np.array_equal(w_warp[0], R.IDENTITY.reshape(2, 3))  # locked onto it
            kept["state"], kept["end"] = state, done
            calls += 1
        if k == 4:  # goes on where the last call ended; then both ranges in one call of 8 frames
            assert done - STEP == kept["end"]
            with pytest.raises(ValueError, match="reset=True"):  # another alpha
                p.stabilize(video[done - STEP:done], alpha=0.3, **fit)
            with pytest.raises(ValueError, match="overlaps"):  # a refused call leaves the path where it was: the next one goes on
                p.stabilize(video[done - STEP:done], alpha=0.2, out=video[done - STEP - 1:done - 1], **fit)
            (out, warp), rows = recorded(lambda: p.stabilize(video[done - STEP:done], alpha=0.2, **fit))
            assert rows == ONE
            w_out, w_warp, _ = want(done - STEP, STEP, 0, kept["state"], 0.2)
            assert np.array_equal(out.cpu().numpy(), w_out) and same_bits(warp.cpu().numpy(), w_warp)
            with pytest.raises(ValueError, match="reset=True"):  # the same frames again: not where the path ended
                p.stabilize(video[done - STEP:done], alpha=0.2, **fit)
            # two calls of 4 frames equal one call of 8 bit for bit (on one state of the history: the next push refines the newest rows)
            a4 = p.stabilize(video[done - 2 * STEP:done - STEP], first_frame=done - 2 * STEP, alpha=0.2, reset=True, **fit)
            b4 = p.stabilize(video[done - STEP:done], alpha=0.2, **fit)
            (out8, warp8), rows = recorded(lambda: p.stabilize(video[done - 2 * STEP:done], alpha=0.2, reset=True, **fit))
            assert rows == ONE
            assert torch.equal(out8, torch.cat([a4[0], b4[0]])) and same_bits(warp8.cpu().numpy(), torch.cat([a4[1], b4[1]]).cpu().numpy())
            w_out, w_warp, _ = want(done - 2 * STEP, 2 * STEP, 0, None, 0.2)
            assert np.array_equal(out8.cpu().numpy(), w_out) and same_bits(warp8.cpu().numpy(), w_warp)
            kept["end"] = done
            calls += 4
        if k == 6:  # a gap; then afresh: planar frames, one frame, another group, a zoom and the edge border
            assert done - STEP != kept["end"]
            with pytest.raises(ValueError, match="reset=True"):
                p.stabilize(video[done - STEP:done], alpha=0.2, **fit)
            (out, warp), rows = recorded(lambda: p.stabilize(video[done - STEP:done], alpha=0.2, reset=True, **fit))
            assert rows == ONE
            w_out, w_warp, _ = want(done - STEP, STEP, 0, None, 0.2)  # restarts from the identity
            assert np.array_equal(out.cpu().numpy(), w_out) and same_bits(warp.cpu().numpy(), w_warp)
            chw = video[done - 3:done].permute(0, 3, 1, 2).contiguous()
            into = torch.full_like(chw, POISON)
            res, warp = p.stabilize(chw, alpha=0.5, zoom=1.25, border="edge", group=1, out=into, **fit)  # (group 1: its first call)
            assert res is into
            w_out, w_warp, state1 = want(done - 3, 3, 1, None, 0.5, post=R.zoom_matrix(*RAW, 1.25), border=R.EDGE)
            assert np.array_equal(res.permute(0, 2, 3, 1).cpu().numpy(), w_out) and same_bits(warp.cpu().numpy(), w_warp)
            kept["end1"], kept["state1"] = done, state1
            calls += 2
        if k == 7:  # group 1 goes on with a single frame, while group 0's path has a gap of its own
            one, warp = p.stabilize(video[kept["end1"]], first_frame=kept["end1"], alpha=0.5, zoom=1.25, fill=(9, 8, 7), group=1, **fit)
            assert tuple(one.shape) == (*RAW, 3) and tuple(warp.shape) == (1, 2, 3)
            w_out, w_warp, _ = want(kept["end1"], 1, 1, kept["state1"], 0.5, post=R.zoom_matrix(*RAW, 1.25), fill=(9, 8, 7))
            assert np.array_equal(one.cpu().numpy(), w_out[0]) and same_bits(warp.cpu().numpy(), w_warp)
            with pytest.raises(ValueError, match="beyond what has been tracked"):
                p.stabilize(video[done - STEP:done], first_frame=done - 1, reset=True)
            calls += 1
        if k == 9:
            assert done > K  # the ring has wrapped: the oldest frame whose source it still holds, and one older
            p.stabilize(video[done - K + 1:done - K + 3], first_frame=done - K + 1, reset=True, **fit)
            with pytest.raises(ValueError, match="left the history"):
                p.stabilize(video[done - K:done - K + 2], first_frame=done - K, reset=True, **fit)
    assert calls == 8 and kept["moved"]  # (not vacuous: some camera motion was fitted and corrected)
    assert np.array_equal(video.cpu().numpy(), video_np)  # the pictures handed in are untouched
    # a new first step drops the paths: the next call locks on afresh, wherever it starts
    assert p.model._gstream._stab
    for x in (p, twin):
        x.finish()
    p(torch.zeros(1, 1, 3, *RAW, device=dev()), is_first_step=True, queries=q, add_support_grid=True)
    p.push_frames(video[:S], add_support_grid=True)
    assert not p.model._gstream._stab
    out, warp = p.stabilize(video[S - 2:S], alpha=0.2, **fit)
    w_out, w_warp, _ = want(S - 2, 2, 0, None, 0.2)
    assert np.array_equal(out.cpu().numpy(), w_out) and same_bits(warp.cpu().numpy(), w_warp)
    p.finish()
