"""ctk_fit_planes and ctk_warp_planes on the GPU (csrc/planes.hip, csrc/warp_planes.hip) against the numpy restatement of
tests/planes_reference.py: every byte of poisoned, fenced outputs, the float32 matrices bit for bit.  The shapes are the smallest at
which the kernels take each of their paths: exactly four slots, five, one wave, one more, two chunks with the second nearly empty,
several, the full LDS list; one round, several, all sixteen; one, several and a partial last pass of hypotheses; tiles cut at both
edges, staged and direct taps, whole-dword and byte stores."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_reference as R
import objects_reference as O
import planes_reference as PR
from ctk_support import HW, S, STEP, STRIDE, dev, recorded, t

pytestmark = pytest.mark.gpu

GUARD, POISON, FENCE = 64, 0x5A, 0xA5
NAMES = ("homography", "label", "stats", "box")


def fenced(nbytes):
    """A poisoned output of nbytes between two fences: -> (whole buffer, the output's view)."""
    buf = torch.full((nbytes + 2 * GUARD,), FENCE, dtype=torch.uint8, device=dev())
    buf[GUARD:GUARD + nbytes] = POISON
    return buf, buf[GUARD:GUARD + nbytes]


def raw_fit(coords, *, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1, to=None, lag=None, anchor=None,
            labels=None, L=1, inverse=0, min_points=8, tol=2.0, K=128, min_base=16.0, seed=0, scale=(1.0, 1.0)):
    """The C-ABI call itself on poisoned, fenced outputs -> (homography, label, stats, box) as numpy; the fences are checked here."""
    from cotracker_amd import _lib as L_
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    given = (visible, vis, conf, first_row, None if anchor is None else anchor[0], None if anchor is None else anchor[1],
             None if labels is None else np.asarray(labels, dtype=np.int8))
    keep = [t(coords)] + [None if x is None else t(np.ascontiguousarray(x)) for x in given]
    a = L_.Planes.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.F = G, N, N_out, R_, f0, F
    a.to, a.lag, a.anchor_frame = -1 if to is None else to, 0 if lag is None else lag, 0 if anchor is None else anchor[2]
    a.L, a.min_points, a.inverse, a.K, a.seed = L, min_points, inverse, K, seed
    a.tol, a.min_base, a.sx, a.sy, a.thresh, a.reserved = tol, min_base, scale[0], scale[1], thresh, 0
    (a.hist_coords, a.visible, a.hist_vis, a.hist_conf, a.first_row, a.anchor_coords, a.anchor_visible,
     a.labels) = (None if x is None else x.data_ptr() for x in keep)
    outs = [fenced(G * F * L * 36), fenced(G * F * N_out), fenced(G * F * L * 16), fenced(G * F * L * 16)]
    a.homography, a.label, a.stats, a.box = (o[1].data_ptr() for o in outs)
    n = C.c_size_t(99)
    L_.check(L_.load().ctk_fit_planes_workspace_bytes(C.byref(a), C.byref(n)), "ctk_fit_planes_workspace_bytes")
    assert n.value == 0
    L_.check(L_.load().ctk_fit_planes(C.byref(a), None, 0, torch.cuda.current_stream().cuda_stream), "ctk_fit_planes")
    torch.cuda.synchronize()
    for whole, _ in outs:  # the bytes next to each output
        assert bool((whole[:GUARD] == FENCE).all()) and bool((whole[-GUARD:] == FENCE).all())
    m, la, s, b = (o[1].cpu().numpy() for o in outs)
    return (m.view(np.float32).reshape(G, F, L, 3, 3), la.view(np.int8).reshape(G, F, N_out), s.view(np.int32).reshape(G, F, L, 4),
            b.view(np.int32).reshape(G, F, L, 4))


def same(got, want):
    for g_, w_, name in zip(got, want, NAMES):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        eq = (g_.view(np.int32) if g_.dtype == np.float32 else g_) == (w_.view(np.int32) if w_.dtype == np.float32 else w_)
        assert eq.all(), (name, np.argwhere(~eq)[:5].tolist(), g_[~eq][:5], w_[~eq][:5])


def both(coords, **kw):
    """Every byte of the four poisoned outputs equals the restatement's (no value of which is the poison pattern)."""
    got, want = raw_fit(coords, **kw), PR.fit_planes(coords, **kw)
    same(got, want)
    return want


# N_out, G, F, L, K, inverse, labels given, form ("lag": linear rows; "ring": R < frames, f - lag and f straddle the wrap; "to"; "anchor":
# a ring that has dropped the anchor's frame, and a slot released after it), logits
CASES = [
    (4, 1, 1, 1, 1, 0, False, "lag", False),
    (5, 2, 3, 1, 128, 1, False, "ring", True),
    (64, 1, 3, 3, 128, 0, True, "to", False),
    (65, 2, 2, 3, 300, 1, True, "anchor", False),
    (257, 1, 3, 16, 128, 0, True, "ring", True),
    (257, 2, 2, 1, 1, 1, True, "lag", False),
    (1024, 1, 2, 3, 300, 0, True, "anchor", False),
    (1024, 1, 2, 1, 128, 1, False, "to", True),
    (1024, 2, 1, 16, 128, 1, True, "lag", False),
    (3600, 1, 1, 3, 8, 0, True, "lag", False),  # 63.3 KiB of dynamic LDS next to the static part: just below 64 KiB
]


@pytest.mark.parametrize("N_out,G,F,L,K,inverse,labelled,form,logits", CASES)
def test_fit_against_the_restatement(N_out, G, F, L, K, inverse, labelled, form, logits):
    N, T = N_out + 3, 14  # the last 3 slots of a group are never read
    coords, visible, who = PR.planes_scene(N_out + K + L, G, T, N, planes=min(L, 3))
    first = O.spoil(coords, N_out) if N_out > 5 else np.zeros((G, N), dtype=np.int32)
    if N_out <= 5:
        visible[:] = 1
    labels = None
    if labelled:
        labels = who.astype(np.int8)
        labels[0, :4] = (-1, 20, 16, L)  # no round's
    kw = dict(first_row=first, N_out=N_out, F=F, labels=labels, L=L, inverse=inverse, min_points=4, K=K, seed=K + 7, min_base=6.0,
              scale=(1.37, 0.81), tol=2.0)
    if form == "lag":
        kw.update(f0=T - F - 1, lag=2)
    elif form == "to":
        kw.update(f0=T - F, to=T - 6)
    elif form == "ring":  # 12 rows after 14 frames hold frames 2 .. 13, frame 12 in row 0
        coords, visible = R.fold(coords, 12, T), R.fold(visible, 12, T)
        kw.update(f0=T - F, lag=3)
        assert (kw["f0"] - 3) % 12 > (T - 1) % 12
    else:  # the anchor was taken on frame 1, which the ring of 12 rows has dropped; slot 7 was released and reassigned after it
        anchor = (coords[:, 1].copy(), visible[:, 1].copy(), 1)
        first[-1, 7] = 2
        coords, visible = R.fold(coords, 12, T), R.fold(visible, 12, T)
        kw.update(f0=T - F, anchor=anchor)
    if logits:  # away from the threshold: products of 0.98 or below 0.02 against 0.6, so that expf cannot decide
        rng = np.random.default_rng(K)
        kw.update(vis=np.where(visible != 0, 5.0, -5.0).astype(np.float32) + rng.uniform(-1, 1, visible.shape).astype(np.float32),
                  conf=np.full(visible.shape, 6.0, dtype=np.float32), thresh=0.6)
    else:
        kw.update(visible=visible)
    m, lab, st, bx = both(coords, **kw)
    if N_out > 5:
        assert (lab[0, :, 4] == -1).all()
    if form == "anchor":
        assert (lab[-1, :, 7] == -1).all()
    if N_out >= 64 and K >= 128:
        assert (st[:, :, :min(L, 3), 1] >= 4).all() and (lab == 0).any() and (st[..., 3] == 0).all()
        if labelled:
            assert (lab[0, :, :4][lab[0, :, :4] >= 0] == PR.NONE).all()


def test_full_lds_list():
    """N_out = 8192: 144 KiB of dynamic LDS, 32 chunks."""
    N = 8192 + 3
    coords, visible, who = PR.planes_scene(1, 1, 2, N, planes=3, hw=(2000, 4000))
    m, lab, st, bx = both(coords, visible=visible, N_out=8192, f0=1, F=1, lag=1, L=3, K=8, seed=3, min_base=32.0, labels=who.astype(np.int8))
    assert st[0, 0, :, 0].min() > 1500 and st[0, 0, :, 1].sum() > 3000 and (st[0, 0, :, 2] >= 0).all()


def test_few_correspondences_and_lists_that_fit_nothing():
    """Frames with 0, 1, 2, 3, 4 and 12 correspondences; a collinear list; a list with too few inliers for min_points."""
    N = 12
    coords, _, _ = PR.planes_scene(9, 2, 7, N, planes=1)
    visible = np.zeros((2, 7, N), dtype=np.uint8)
    visible[:, 0] = 1
    for f, count in enumerate((12, 4, 3, 2, 1, 0), start=1):
        visible[:, f, :count] = 1
    kw = dict(visible=visible, K=64, seed=1, f0=0, F=7, to=0, min_base=4.0, min_points=4)
    m, lab, st, bx = both(coords, **kw)
    assert st[0, :, 0, 0].tolist() == [12, 12, 4, 3, 2, 1, 0] and (st[:, 3:, 0, 1] == 0).all() and (st[:, 3:, 0, 2] == -1).all()
    assert (lab[:, 6] == -1).all() and st[1, 1, 0, 1] >= 4
    both(coords, **{**kw, "inverse": 1})
    both(coords, **{**kw, "min_points": 13})
    x = np.arange(40, dtype=np.float32) * 7.0
    line = np.stack([x, 2.0 * x + 3.0], axis=1)
    flat = np.stack([line, line + 5.0])[None]
    m, lab, st, bx = both(flat, visible=np.ones((1, 2, 40), dtype=np.uint8), f0=1, F=1, lag=1, K=128, seed=2, min_points=4, min_base=0.0)
    assert st[0, 0, 0].tolist() == [40, 0, -1, 0]


# ---- the warp -------------------------------------------------------------------------------------------------------------------------
def raw_warp(src, matrices, dst, *, border, fill=(7, 200, 90), layout=PR.HWC, pad=0, offset=0, one_source=False):
    """ctk_warp_planes on a fenced destination whose rows carry `pad` poisoned bytes and which starts `offset` bytes into its
    allocation.  src, dst: numpy pictures in `layout` ([F,H,W,3], [F,3,H,W] or [F,H,W]); dst holds what is there before the call ->
    the destination after the call, with the padding (checked here to be untouched, like the fences)."""
    from cotracker_amd import _lib as L_
    mask = src.ndim == 3
    Cn = 1 if mask else 3
    planar = layout == PR.CHW and not mask
    Fn = dst.shape[0]
    (Hs, Ws), (H, W) = (src.shape[-2:] if planar or mask else src.shape[1:3]), (dst.shape[-2:] if planar or mask else dst.shape[1:3])
    rows, row_elems = (Cn * H, W) if planar else (H, Cn * W)
    pitch = row_elems + pad
    nbytes = Fn * rows * pitch
    whole, view = fenced(nbytes + offset)
    view = view[offset:]
    grid = view.view(Fn, rows, pitch)
    grid[:, :, :row_elems] = t(np.ascontiguousarray(dst)).reshape(Fn, rows, row_elems)
    before = whole.clone()
    s = t(np.ascontiguousarray(src))
    a = L_.Planes.WarpArgs()
    a.F, a.H, a.W, a.Hs, a.Ws, a.C, a.layout, a.border, a.reserved = Fn, H, W, Hs, Ws, Cn, layout, border, 0
    for k in range(3):
        a.fill[k] = fill[k]
    srows, srow_elems = (Cn * Hs, Ws) if planar else (Hs, Cn * Ws)
    a.src_frame_stride, a.src_row_stride = (0 if one_source else srows * srow_elems), srow_elems
    a.dst_frame_stride, a.dst_row_stride = rows * pitch, pitch
    mats = t(np.ascontiguousarray(matrices, dtype=np.float32).reshape(Fn, 3, 3))
    a.matrices, a.src, a.dst = mats.data_ptr(), s.data_ptr(), view.data_ptr()
    L_.check(L_.load().ctk_warp_planes(C.byref(a), torch.cuda.current_stream().cuda_stream), "ctk_warp_planes")
    torch.cuda.synchronize()
    assert bool((whole[:GUARD + offset] == before[:GUARD + offset]).all()) and bool((whole[-GUARD:] == FENCE).all())
    assert bool((grid[:, :, row_elems:] == POISON).all())  # the pitch padding keeps its value
    return grid[:, :, :row_elems].cpu().numpy().reshape(dst.shape)


def pictures(seed, Fn, H, W, layout, mask=False):
    pics = np.stack([PR.WR.texture(seed + j, H, W) for j in range(Fn)])
    if mask:
        return np.ascontiguousarray(pics[..., 0])
    return np.ascontiguousarray(pics if layout == PR.HWC else pics.transpose(0, 3, 1, 2))


WARPS = {
    "perspective": [[0.9, 0.05, 1.3], [-0.04, 1.1, 0.7], [0.002, 0.001, 1.0]],
    "horizon": [[1.0, 0.2, -3.0], [0.1, 0.9, 2.0], [0.0, -0.05, 1.0]],     # Z = 0 on y = 20
    "zero": np.zeros((3, 3)),
    "nan": [[1.0, 0.0, 0.0], [0.0, np.nan, 0.0], [0.0, 0.0, 1.0]],
    "strong": [[3.5, 0.2, 1.0], [0.1, 3.0, 2.0], [0.001, 0.0005, 1.0]],    # a tile's source box is far larger than 16 KiB
    "far": [[40000.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]],
}


@pytest.mark.parametrize("layout,mask", ((PR.HWC, False), (PR.CHW, False), (PR.HWC, True)))
@pytest.mark.parametrize("size", ((1, 1), (3, 5), (70, 130)))
def test_warp_shapes_layouts_and_borders(size, layout, mask):
    """dst 1 x 1, 3 x 5 and 70 x 130 (tile edges in both directions) from sources of another size; HWC, CHW and C = 1; dense aligned
    rows (whole dwords) and padded rows at an odd address (bytes); one source for all pictures; the three borders; every matrix."""
    H, W = size
    Hs, Ws = (23, 31) if H < 70 else (200, 260)
    Fn = len(WARPS)
    src = pictures(1, Fn, Hs, Ws, layout, mask)
    dst = pictures(50, Fn, H, W, layout, mask)
    mats = np.stack([np.asarray(m, dtype=np.float32) for m in WARPS.values()])
    for border in (PR.FILL, PR.EDGE, PR.KEEP):
        want = PR.warp_planes(src, mats, dst, border=border, fill=(7, 200, 90), layout=layout)
        for pad, offset in ((0, 0), (5, 3)):
            got = raw_warp(src, mats, dst, border=border, layout=layout, pad=pad, offset=offset)
            assert np.array_equal(got, want), (border, pad, np.argwhere(got != want)[:5].tolist())
        if border == PR.KEEP:
            assert np.array_equal(want[2], dst[2]) and np.array_equal(want[3], dst[3])  # zero and NaN matrices: nothing is written
            assert H < 70 or (want[0] != dst[0]).any()
    one = PR.warp_planes(src[:1], mats, dst, border=PR.EDGE, fill=(7, 200, 90), layout=layout)
    assert np.array_equal(raw_warp(src[:1], mats, dst, border=PR.EDGE, layout=layout, pad=4, one_source=True), one)


def test_warp_identity_and_integer_translation():
    src = pictures(3, 2, 70, 130, PR.HWC)
    eye = np.tile(np.eye(3, dtype=np.float32), (2, 1, 1))
    for pad, offset in ((0, 0), (3, 1)):
        got = raw_warp(src, eye, np.zeros_like(src), border=PR.FILL, pad=pad, offset=offset)
        assert np.array_equal(got, src)  # bit for bit
    shift = eye.copy()
    shift[:, 0, 2], shift[:, 1, 2] = 9.0, -4.0
    got = raw_warp(src, shift, np.zeros_like(src), border=PR.FILL, fill=(1, 2, 3))
    want = np.empty_like(src)
    want[...] = (1, 2, 3)
    want[:, 4:, :130 - 9] = src[:, :70 - 4, 9:]
    assert np.array_equal(got, want) and np.array_equal(got, PR.warp_planes(src, shift, np.zeros_like(src), fill=(1, 2, 3)))


def test_warp_keep_draws_a_small_picture_inside_one_tile():
    """KEEP in place: a 5 x 7 picture lands strictly inside one 64 x 16 tile whose four corners are all outside the picture's quad.  Its
    bytes are written and every other byte of the frames is untouched."""
    frames = pictures(8, 2, 32, 128, PR.HWC)
    pic = pictures(20, 1, 5, 7, PR.HWC)
    m = np.tile(np.eye(3, dtype=np.float32), (2, 1, 1))
    m[0, 0, 2], m[0, 1, 2] = -20.0, -4.0          # the picture's pixel (0, 0) at frame pixel (20, 4): tile (0, 0)
    m[1, 0, 2], m[1, 1, 2] = -(64.0 + 30.5), -(16.0 + 6.25)  # tile (1, 1), between pixels
    want = PR.warp_planes(pic, m, frames, border=PR.KEEP)
    for pad, offset in ((0, 0), (2, 1)):
        got = raw_warp(pic, m, frames, border=PR.KEEP, pad=pad, offset=offset, one_source=True)
        assert np.array_equal(got, want)
    changed = (want != frames).any(axis=-1)
    assert np.array_equal(want[0, 4:8, 20:26], pic[0, :4, :6]) and changed[0].sum() > 0  # a tap column and row short of the picture
    outside = np.ones_like(changed)
    outside[0, 4:8, 20:26] = False
    outside[1, 22:27, 94:101] = False
    assert not changed[outside].any() and changed[1, 23:26, 95:100].any()


# ---- the ops layer --------------------------------------------------------------------------------------------------------------------
def test_the_ops_layer(monkeypatch):
    from cotracker_amd import _lib as L_
    from cotracker_amd import ops
    coords, visible, who = PR.planes_scene(21, 2, 6, 90, planes=3)
    tr, vi = t(coords), t(visible)
    kw = dict(hypotheses=300, seed=9, scale=(1.37, 0.81), min_points=5, min_base=6.0)
    ref = dict(K=300, seed=9, scale=(1.37, 0.81), min_points=5, min_base=6.0)
    want = PR.fit_planes(coords, visible=visible, f0=0, F=6, lag=1, **ref)  # no labels, the default lag (the result is padded), twice
    for _ in range(2):
        same(tuple(x.cpu().numpy() for x in ops.fit_planes(tr, vi, **kw)), want)
    labels = who.astype(np.int8)
    res, rows = recorded(lambda: ops.fit_planes(tr, vi, labels=t(labels), planes=3, to=1, inverse=True, frames=(2, 3), **kw))
    assert rows == {"fit_planes": 1}
    same(tuple(x.cpu().numpy() for x in res), PR.fit_planes(coords, visible=visible, labels=labels, f0=2, F=3, to=1, L=3, inverse=1, **ref))
    first = np.zeros(90, dtype=np.int64)
    first[:3] = (2, 2 ** 40, 0)
    anchor = ops.FieldAnchor(t(coords[1:, 0]), t(visible[1:, 0]), 0)
    got = ops.fit_planes(tr[1], vi[1].bool(), labels=t(labels[1]), planes=4, anchor=anchor, first_row=torch.from_numpy(first), frames=(1, 5), **kw)
    same(tuple(x.cpu().numpy() for x in got),
         PR.fit_planes(coords[1:], visible=visible[1:], labels=labels[1:], anchor=(coords[1:, 0], visible[1:, 0], 0), f0=1, F=5, L=4,
                       first_row=np.clip(first, 0, R.INT32_MAX)[None], **ref))
    lib, seen = L_.load(), []
    for name in L_.SYMBOLS:
        if name != "ctk_error_string":
            def counted(*a, _fn=getattr(lib, name), _name=name):
                seen.append(_name)
                return _fn(*a)
            monkeypatch.setattr(lib, name, counted)
    ops.fit_planes(tr, vi, **kw)
    assert seen == ["ctk_fit_planes_workspace_bytes", "ctk_fit_planes"]
    for bad in (dict(lag=0), dict(hypotheses=0), dict(seed=-1), dict(planes=0), dict(planes=17), dict(planes=2), dict(min_points=0),
                dict(to=6), dict(to=-1), dict(to=1, anchor=anchor), dict(frames=(5, 2)), dict(labels=t(labels).to(torch.int32), planes=3),
                dict(anchor=anchor)):  # (planes = 2 without labels; the anchor holds one group, the tracks two)
        with pytest.raises(ValueError):
            ops.fit_planes(tr, vi, **bad)
    with pytest.raises(RuntimeError, match="ctk_fit_planes"):  # the C-ABI's own refusal, through the query
        ops.fit_planes(tr, vi, tol=0.0)


def test_ops_warp_overlay_and_rectify():
    """ops.warp_planes reads strides off the tensors; ops.overlay draws a picture in place where numpy says, from the device's own
    matrices; ops.rectify shows the quad upright."""
    from cotracker_amd import ops
    src = pictures(5, 3, 40, 56, PR.HWC)
    mats = np.stack([np.asarray(WARPS[k], dtype=np.float32) for k in ("perspective", "horizon", "strong")])
    big = t(np.zeros((3, 48, 64, 3), dtype=np.uint8))
    view = big[:, 2:42, 3:59]  # a crop: rows with a pitch of their own
    view.copy_(t(src))
    res, rows = recorded(lambda: ops.warp_planes(view, t(mats), size=(30, 50), border="edge"))
    assert rows == {"warp_planes": 1} and tuple(res.shape) == (3, 30, 50, 3)
    assert np.array_equal(res.cpu().numpy(), PR.warp_planes(src, mats, np.zeros((3, 30, 50, 3), dtype=np.uint8), border=PR.EDGE))
    chw = np.ascontiguousarray(src.transpose(0, 3, 1, 2))
    out = torch.full((3, 3, 30, 50), 9, dtype=torch.uint8, device=dev())
    assert ops.warp_planes(t(chw[:1]), t(mats), out=out, border="keep") is out  # one picture for every matrix
    assert np.array_equal(out.cpu().numpy(), PR.warp_planes(chw[:1], mats, np.full((3, 3, 30, 50), 9, dtype=np.uint8), border=PR.KEEP, layout=PR.CHW))
    mask = t(np.ascontiguousarray(src[..., 0]))
    assert np.array_equal(ops.warp_planes(mask, t(mats), fill=200).cpu().numpy(),
                          PR.warp_planes(src[..., 0], mats, np.zeros((3, 40, 56), dtype=np.uint8), fill=(200,)))
    for bad in (dict(border="wrap"), dict(border="keep"), dict(fill=(1, 2)), dict(out=view), dict(size=(0, 5))):
        with pytest.raises((ValueError, RuntimeError)):
            ops.warp_planes(view, t(mats), **bad)
    # a plane of 200 points under a slowly changing homography; a picture pinned onto a quad of frame 1
    coords, visible, _ = PR.planes_scene(4, 1, 5, 200, planes=1)
    visible[:] = 1
    visible[0, 3] = 0  # frame 3 has no correspondences: no fit, the frame is returned unchanged
    frames = pictures(30, 4, 270, 480, PR.HWC)
    pic = pictures(40, 1, 33, 47, PR.HWC)[0]
    corners = [[100.0, 60.0], [300.0, 70.0], [290.0, 200.0], [110.0, 190.0]]
    fit = dict(hypotheses=64, seed=5, min_base=8.0)
    fr = t(frames)
    res, rows = recorded(lambda: ops.overlay(fr, t(pic), corners, t(coords), t(visible), src_frame=1, first_frame=1, **fit))
    assert res is fr and rows == {"fit_planes": 1, "warp_planes": 1}
    hom, _, stats, _ = ops.fit_planes(t(coords), t(visible), to=1, inverse=True, frames=(1, 4), **fit)
    assert stats[0, :, 0, 1].tolist()[2] == 0 and stats[0, 0, 0, 1] == 200 and int(stats[0, 3, 0, 1]) >= 140
    quad = PR.quad_matrix(corners, (33, 47))
    assert np.allclose(quad, ops.quad_matrix(corners, (33, 47)).numpy(), rtol=1e-12, atol=1e-12)
    m = np.linalg.inv(ops.quad_matrix(corners, (33, 47)).numpy())[None] @ hom[0, :, 0].cpu().numpy().astype(np.float64)
    m[2] = 0.0
    mats32 = ops.plane_matrices(hom[0, :, 0], stats[0, :, 0], ops.quad_matrix(corners, (33, 47)), inverse=True)
    # the constant is kept on the device per quad: the same tensor again, the same matrices from it, and a second overlay of the same
    # quad solves nothing on the host
    const = ops.quad_constant(corners, (33, 47), dev(), inverse=True)
    assert const is ops.quad_constant([list(c) for c in corners], (33, 47), dev(), inverse=True) and const.is_cuda and const.dtype == torch.float64
    assert const is not ops.quad_constant(corners, (33, 47), dev(), inverse=False) and const is not ops.quad_constant(corners, (33, 48), dev(), inverse=True)
    assert torch.equal(ops.plane_matrices(hom[0, :, 0], stats[0, :, 0], const, inverse=True), mats32)
    solved = []
    solve = ops.quad_matrix
    ops.quad_matrix = lambda *a_, **k_: solved.append(1) or solve(*a_, **k_)
    try:
        again = ops.overlay(t(frames), t(pic), corners, t(coords), t(visible), src_frame=1, first_frame=1, **fit)
    finally:
        ops.quad_matrix = solve
    assert not solved and torch.equal(again, fr)
    assert np.allclose(mats32.cpu().numpy(), m, rtol=1e-5, atol=1e-6) and not mats32[2].any()
    want = PR.warp_planes(pic[None], mats32.cpu().numpy(), frames, border=PR.KEEP)
    got = fr.cpu().numpy()
    assert np.array_equal(got, want) and np.array_equal(got[2], frames[2])
    drawn = (got != frames).any(axis=-1)
    assert drawn[0].sum() > 15000 and drawn[3].sum() > 15000 and not drawn[0, :50].any()  # the quad covers about 200 x 130 pixels
    # on frame 1 itself the picture's corner pixels land on the corners (one tap short at the right and the bottom)
    ys, xs = np.nonzero(drawn[0])
    assert abs(xs.min() - 100) <= 2 and abs(xs.max() - 300) <= 6 and abs(ys.min() - 60) <= 2 and abs(ys.max() - 200) <= 6
    # rectify: the forward matrices; the drawn picture comes back upright
    res, rows = recorded(lambda: ops.rectify(fr, corners, t(coords), t(visible), src_frame=1, size=(33, 47), first_frame=1, **fit))
    assert rows == {"fit_planes": 1, "warp_planes": 1} and tuple(res.shape) == (4, 33, 47, 3)
    fwd, _, fst, _ = ops.fit_planes(t(coords), t(visible), to=1, frames=(1, 4), **fit)
    mf = ops.plane_matrices(fwd[0, :, 0], fst[0, :, 0], ops.quad_matrix(corners, (33, 47)), inverse=False)
    assert np.array_equal(res.cpu().numpy(), PR.warp_planes(got, mf.cpu().numpy(), np.zeros((4, 33, 47, 3), dtype=np.uint8)))
    inner = res.cpu().numpy()[:, 2:-2, 2:-2].astype(np.int32) - pic[None, 2:-2, 2:-2].astype(np.int32)
    assert np.abs(inner[0]).mean() < 25 and np.abs(inner[3]).mean() < 25  # resampled twice: close to the picture, not equal


# ---- the predictor --------------------------------------------------------------------------------------------------------------------
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


def test_follow_overlay_rectify_on_a_push_stream(monkeypatch):
    """Ring + graph on, frames pushed as uint8.  follow_planes, overlay and rectify read the stream's own history and logits; what they
    are compared with is ops.fit_planes on the tracks as recent() emits them and ops.warp_planes of the same matrices.  The stream's
    tracks are bit-identical to a twin's that never asks, nothing is re-captured, each entry point makes one launch per kernel."""
    from cotracker_amd import ops
    from cotracker_amd.synthetic import synthetic_video
    K, G, N, spare, g = 16, 2, 12, 2, 1
    T = S + 5 * STEP
    video = synthetic_video(T, *RAW, seed=11)[0].permute(0, 2, 3, 1).round().to(torch.uint8).contiguous().to(dev())
    gen = torch.Generator().manual_seed(2)
    q = torch.rand(G, N, 3, generator=gen) * torch.tensor([0.0, RAW[1] - 1.0, RAW[0] - 1.0])
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
        p.follow_planes(None)
    Nu = N + spare
    fit = dict(tol=8.0, min_base=1.0, hypotheses=64, min_points=4, seed=3)
    boxes = torch.tensor([[-50.0, -50.0, 70.0, 150.0], [50.0, -50.0, 200.0, 150.0], [500.0, 500.0, 600.0, 600.0]])  # left, right, nothing
    corners = [[20.0, 15.0], [90.0, 20.0], [85.0, 70.0], [25.0, 75.0]]
    picture = torch.from_numpy(PR.WR.texture(7, 9, 11)).to(dev())

    def history():
        """-> (tracks [done,Nu,2], visible [done,Nu]) of group g, zeros where the ring has dropped the frame."""
        done = p.model._gstream.committed
        tr, vi = p.recent(min(done, K))
        full_t, full_v = torch.zeros(done, Nu, 2, device=dev()), torch.zeros(done, Nu, dtype=torch.bool, device=dev())
        full_t[done - tr.shape[1]:], full_v[done - tr.shape[1]:] = tr[g], vi[g]
        return full_t, full_v
    chosen, anchor_row, checked, fitted, drawn = None, None, 0, 0, 0
    follow = p.follow_planes
    for k, t0 in enumerate(range(0, T - S + 1, STEP)):
        new = video[:S] if k == 0 else video[t0 + S - STEP:t0 + S]
        c0 = len(captures)
        got = p.push_frames(new, add_support_grid=True)
        c1 = len(captures)
        ref = twin.push_frames(new, add_support_grid=True)
        assert len(captures) - c1 == c1 - c0, (k, c0, c1, len(captures))  # nothing is re-captured: the twin, which never asks, captures as often
        assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(got[1], ref[1]), k
        done = p.model._gstream.committed
        first = None if p._first_row is None else p._first_row[g]
        if k == 3:
            at = done - 3
            full_t, full_v = history()
            chosen = p.label_objects(boxes, at, group=g)
            anchor_row = ops.FieldAnchor(full_t[at][None].contiguous(), full_v[at][None].contiguous(), at)
        if k in (4, 5):
            full_t, full_v = history()
            for inverse in (False, True):
                res, rows = recorded(lambda: p.follow_planes(chosen, inverse=inverse, **fit))
                assert rows == {"fit_planes": 1} and len(captures) == c1 + (c1 - c0)
                assert [tuple(x.shape) for x in res] == [(STEP, 3, 3, 3), (STEP, Nu), (STEP, 3, 4), (STEP, 3, 4)]
                m, la, st, bx = ops.fit_planes(full_t, full_v, labels=chosen.labels[:Nu].contiguous(), planes=3, anchor=anchor_row,
                                               inverse=inverse, frames=(done - STEP, STEP), first_row=first, **fit)
                assert torch.equal(res[0].view(torch.int32), m[0].view(torch.int32)) and torch.equal(res[1], la[0])
                assert torch.equal(res[2], st[0]) and torch.equal(res[3], bx[0].float() / 16.0) and res[3].dtype == torch.float32
                assert int(st[0, :, :, 0].sum()) > 0
                checked += 1
            # overlay() and rectify() take no fit parameters; on synthetic weights the defaults find no plane, so the test's bounds reach
            # them through follow_planes, which both call.  The object with the most fitted frames carries the picture.
            monkeypatch.setattr(p, "follow_planes", lambda *a, **kw: follow(*a, **{**fit, **kw}))
            index = int((p.follow_planes(chosen, inverse=True)[2][:, :, 1] > 0).sum(dim=0).argmax())
            # overlay: in place, two launches; equal to warp_planes of the same matrices; a frame without a fit is returned unchanged
            frames = video[done - STEP:done].clone()
            before = frames.clone()
            res, rows = recorded(lambda: p.overlay(frames, picture, corners, chosen, index=index))
            assert res is frames and rows == {"fit_planes": 1, "warp_planes": 1} and len(captures) == c1 + (c1 - c0)
            hom, _, st, _ = p.follow_planes(chosen, inverse=True)
            mats = ops.plane_matrices(hom[:, index], st[:, index], ops.quad_matrix(corners, (9, 11)), inverse=True)
            want = ops.warp_planes(picture[None], mats, out=before.clone(), border="keep")
            assert torch.equal(frames, want)
            none = st[:, index, 1] == 0
            fitted += int((~none).sum())
            drawn += int((frames != before).any(dim=-1).sum())
            print(f"push {k}: overlay of object {index}: {int((~none).sum())} of {STEP} frames have a fit, {int((frames != before).any(dim=-1).sum())} pixels drawn")
            assert torch.equal(frames[none], before[none]) and bool(((mats == 0).flatten(1).all(dim=1) == none).all())
            same_frames = p.overlay(before.clone(), picture, corners, chosen, index=2)  # object 2 has no point: no fit on any frame
            assert torch.equal(same_frames, before)
            one = p.overlay(before[-1].clone(), picture[..., 0].contiguous(), corners, chosen)  # one frame, a [h,w] picture
            assert tuple(one.shape) == (RAW[0], RAW[1], 3)
            # rectify: a new tensor through the forward matrices
            res, rows = recorded(lambda: p.rectify(before, corners, chosen, index=index, size=(24, 32), border="edge"))
            assert rows == {"fit_planes": 1, "warp_planes": 1} and tuple(res.shape) == (STEP, 24, 32, 3) and len(captures) == c1 + (c1 - c0)
            hom, _, st, _ = p.follow_planes(chosen)
            fwd = ops.plane_matrices(hom[:, index], st[:, index], ops.quad_matrix(corners, (24, 32)), inverse=False)
            assert torch.equal(res, ops.warp_planes(before, fwd, size=(24, 32), border="edge"))
            single = p.rectify(before[-1], corners, chosen, index=index, size=(24, 32), border="edge")  # one frame in, one picture out
            assert tuple(single.shape) == (24, 32, 3) and torch.equal(single, res[-1])
            given = torch.zeros(24, 32, 3, dtype=torch.uint8, device=dev())
            assert torch.equal(p.rectify(before[-1], corners, chosen, index=index, size=(24, 32), border="edge", out=given), res[-1])
            assert torch.equal(given, res[-1])
            with pytest.raises(ValueError, match="beyond what has been tracked"):
                p.follow_planes(chosen, 2, first_frame=done - 1)
            with pytest.raises(ValueError, match="index"):
                p.overlay(frames, picture, corners, chosen, index=3)
    assert checked == 4 and fitted > 0  # (not vacuous: some frame had a fit, so its matrix was not the zero matrix)
    print(f"frames with a fit {fitted}, pixels drawn {drawn}")
    with pytest.raises(ValueError, match="ObjectSet"):
        p.follow_planes(None)
    for x in (p, twin):
        x.finish()
