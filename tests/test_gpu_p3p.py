"""ctk_fit_p3p on the GPU (csrc/p3p.hip) against the numpy restatement of tests/p3p_reference.py: every byte of poisoned, fenced
outputs, the float32 poses and errors bit for bit, the inputs unchanged.  The shapes are p3p_reference.cases(): the smallest at which
the kernel takes each of its paths -- a fit list of exactly min_points entries and of one less, one chunk less one slot, one chunk, one
chunk and one slot, several chunks, the list cap (bit 3) and the largest N_out; 1 hypothesis, one less than / exactly / one more than
what a wave (64) and a workgroup (256) make at a time, 1024; the three source forms across a ring wrap; logits; first rows; G = 2 and
F = 3; spoiled positions, structure points and validity bytes; collinear and repeated triples; a frame on which every sampled
candidate is skipped; ties between candidates; the frame that is the source frame itself.  The last tests hold the host layers to the
raw call."""
import ctypes as C

import numpy as np
import pytest
import torch

import p3p_reference as P3
import resection_reference as RR
from ctk_support import STEP, S, dev, recorded, t
from test_gpu_resection import RAW, bits, fenced, same, small_predictor, GUARD, FENCE

pytestmark = pytest.mark.gpu


def raw_fit(coords, cam, structure, valid, *, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1,
            to=None, lag=None, anchor=None, tol=2.0, hypotheses=256, seed=0, min_points=16, scale=(1.0, 1.0)):
    """The C-ABI call itself on poisoned, fenced outputs -> (pose, label, error, stats) as numpy; the fences and the inputs are checked
    here."""
    from cotracker_amd import _lib as L_
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out
    given = (visible, vis, conf, first_row, None if anchor is None else anchor[0], None if anchor is None else anchor[1],
             np.asarray(structure, dtype=np.float32), np.asarray(valid, dtype=np.int8))
    keep = [t(coords)] + [None if x is None else t(np.ascontiguousarray(x)) for x in given]
    before = [None if x is None else x.clone() for x in keep]
    a = L_.P3p.Args()
    a.G, a.N, a.N_out, a.R, a.f0, a.F = G, N, N_out, R_, f0, F
    a.to, a.lag, a.anchor_frame = -1 if to is None else to, 0 if lag is None else lag, 0 if anchor is None else anchor[2]
    a.min_points, a.hypotheses, a.seed = min_points, hypotheses, seed
    a.fx, a.fy, a.cx, a.cy = cam
    a.sx, a.sy, a.thresh, a.tol = scale[0], scale[1], thresh, tol
    (a.hist_coords, a.visible, a.hist_vis, a.hist_conf, a.first_row, a.anchor_coords, a.anchor_visible, a.structure,
     a.valid) = (None if x is None else x.data_ptr() for x in keep)
    outs = [fenced(G * F * 48), fenced(G * F * N_out), fenced(G * F * N_out * 4), fenced(G * F * 16)]
    a.pose, a.label, a.error, a.stats = (o[1].data_ptr() for o in outs)
    n = C.c_size_t(99)
    L_.check(L_.load().ctk_fit_p3p_workspace_bytes(C.byref(a), C.byref(n)), "ctk_fit_p3p_workspace_bytes")
    assert n.value == 0
    L_.check(L_.load().ctk_fit_p3p(C.byref(a), None, 0, torch.cuda.current_stream().cuda_stream), "ctk_fit_p3p")
    torch.cuda.synchronize()
    for whole, _ in outs:  # the bytes next to each output
        assert bool((whole[:GUARD] == FENCE).all()) and bool((whole[-GUARD:] == FENCE).all())
    for x, b in zip(keep, before):  # the kernel only reads its inputs, the structure among them
        assert x is None or torch.equal(x.view(torch.uint8), b.view(torch.uint8))
    po, la, er, st = (o[1].cpu().numpy() for o in outs)
    return (po.view(np.float32).reshape(G, F, 3, 4), la.view(np.int8).reshape(G, F, N_out), er.view(np.float32).reshape(G, F, N_out),
            st.view(np.int32).reshape(G, F, 4))


CASES = {name: (args, kw) for name, args, kw in P3.cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_against_the_restatement(name):
    """Every byte of the four poisoned outputs equals the restatement's (no value of which is the poison pattern)."""
    args, kw = CASES[name]
    same(raw_fit(*args, **kw), P3.fit_p3p(*args, **kw))


def test_the_ops_layer():
    """ops.fit_p3p: one launch that equals the raw call, `out`, one group without its axis, the anchor form, and the refusals."""
    from cotracker_amd import ops
    G, T, N = 2, 6, 150
    sc = RR.scene(5, G, T, N, src=1)
    coords, visible, cam = sc["coords"], sc["visible"], sc["cam"]
    valid = (~sc["mover"]).astype(np.int8)
    fit = dict(tol=2.0, hypotheses=64, seed=4, min_points=10)
    want = raw_fit(coords, cam, sc["structure"], valid, visible=visible, f0=0, F=T, to=1, **fit)
    same(want, P3.fit_p3p(coords, cam, sc["structure"], valid, visible=visible, f0=0, F=T, to=1, **fit))
    k = want[3][:, :, 2]  # every row has a fit -- no seed is needed --, and the source frame itself is exact
    assert (k >= 0).all() and (want[3][:, 1, 3] == 32).all() and (k[:, 1] == 64).all()
    tr, vi, st, va = t(coords), t(visible).bool(), t(sc["structure"]), t(valid)
    got, rows = recorded(lambda: ops.fit_p3p(tr, vi, cam, st, va, to=1, **fit))
    assert rows == {"fit_p3p": 1}
    same([g_.cpu().numpy() for g_ in got], want)
    assert [tuple(g_.shape) for g_ in got] == [(G, T, 3, 4), (G, T, N), (G, T, N), (G, T, 4)]
    out = tuple(torch.empty_like(g_) for g_ in got)
    again = ops.fit_p3p(tr, vi, cam, st, va.bool(), to=1, out=out, **fit)
    assert all(a_ is b_ for a_, b_ in zip(again, out))
    same([g_.cpu().numpy() for g_ in again], want)
    one = ops.fit_p3p(tr[0], vi[0], list(cam), st[0], va[0].to(torch.uint8), to=1, **fit)
    same([g_.cpu().numpy() for g_ in one], [w[:1] for w in want])
    anchor = ops.FieldAnchor(tr[:, 1].contiguous(), vi[:, 1].contiguous(), 1)
    anchored = ops.fit_p3p(tr, vi, cam, st, va, anchor=anchor, **fit)  # the same source, as an anchor
    same([g_.cpu().numpy() for g_ in anchored], want)
    for bad in (dict(min_points=5), dict(hypotheses=0), dict(hypotheses=1025), dict(tol=0.0), dict(tol=float("nan")), dict(to=None, lag=0),
                dict(anchor=anchor), dict(to=T), dict(out=out[:3])):
        with pytest.raises(ValueError):
            ops.fit_p3p(tr, vi, cam, st, va, **{**dict(to=1), **fit, **bad})
    for bad_cam in ((0.0, 1.0, 2.0, 3.0), (1.0, float("nan"), 2.0, 3.0), (1.0, 2.0, 3.0), t(np.array(cam))):
        with pytest.raises(ValueError, match="intrinsics"):
            ops.fit_p3p(tr, vi, bad_cam, st, va, to=1)
    for s_, v_ in ((st.double(), va), (st[:, :5], va), (st, va.float()), (st, va[:, :5]), (st.cpu(), va)):
        with pytest.raises(ValueError):
            ops.fit_p3p(tr, vi, cam, s_, v_, to=1)


def test_resect_on_a_push_stream(monkeypatch):
    """Ring + graph on, frames pushed as uint8.  resect() is ONE launch on the stream's own history and logits and equals ops.fit_p3p on
    the tracks as recent() emits them; on the structure's own frame it gives exactly (I | 0); its poses go into extend() as they
    stand.  The stream's tracks are bit-identical to a twin's that never asks, nothing is re-captured, and the stream's state is not
    re-allocated.  A v2 predictor raises."""
    from cotracker_amd import ops
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    from cotracker_amd.synthetic import synthetic_video
    K, G, N, spare, g = 16, 2, 24, 2, 1
    T = S + 4 * STEP
    cam = (120.0, 118.0, 70.0, 50.0)
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
        p.resect(None)
    Nu = N + spare
    # synthetic weights track nothing real: the bounds are wide, so that some frames have a fit
    two_view = dict(tol=6.0, min_base=1.0, hypotheses=64, min_points=8, seed=3)
    fit = dict(tol=8.0, hypotheses=65, min_points=6, seed=3)
    lag, checked, fitted, on_anchor, extended = 3, 0, 0, 0, 0
    state, structures = None, []
    for k, t0 in enumerate(range(0, T - S + 1, STEP)):
        new = video[:S] if k == 0 else video[t0 + S - STEP:t0 + S]
        c0 = len(captures)
        got = p.push_frames(new, add_support_grid=True)
        c1 = len(captures)
        ref = twin.push_frames(new, add_support_grid=True)
        assert len(captures) - c1 == c1 - c0, (k, c0, c1, len(captures))  # nothing is re-captured: the twin, which never asks, captures as often
        assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(got[1], ref[1]), k
        gs = p.model._gstream
        done = gs.committed
        ptrs = tuple(h_.data_ptr() for h_ in gs.hist) + (gs.queries.data_ptr(),)
        assert state is None or state == ptrs  # the stream's state stays where it is
        state = ptrs
        first = None if p._first_row is None else p._first_row[g]
        if k < 2:
            continue
        tr, vi = p.recent(min(done, K))
        full_t, full_v = torch.zeros(done, Nu, 2, device=dev()), torch.zeros(done, Nu, dtype=torch.bool, device=dev())
        full_t[done - tr.shape[1]:], full_v[done - tr.shape[1]:] = tr[g], vi[g]
        at = done - 2
        s = p.reconstruct(cam, at, lag=lag, max_depth=1e6, group=g, **two_view)
        anchor_row = ops.FieldAnchor(full_t[at][None].contiguous(), full_v[at][None].contiguous(), at)
        structures.append((s, anchor_row))
        for s_, row_ in structures:
            res, rows = recorded(lambda: p.resect(s_, **fit))
            assert rows == {"fit_p3p": 1} and len(captures) == c1 + (c1 - c0)  # ONE launch, no capture
            assert [tuple(x.shape) for x in res] == [(STEP, 3, 4), (STEP, Nu), (STEP, Nu), (STEP, 4)]
            mu = s_.valid[:Nu].contiguous()
            want = ops.fit_p3p(full_t, full_v, cam, s_.points[:Nu].contiguous(), mu, anchor=row_, first_row=first, **fit)
            for a_, b_ in zip(res, want):
                assert torch.equal(bits(a_), bits(b_[0, done - STEP:]))
            fitted += int((res[3][:, 2] >= 0).sum())
            checked += 1
            if s_.anchor.frame >= done - STEP and int(s_.valid.sum()) >= 6:  # the structure's own frame is among the rows
                j = s_.anchor.frame - (done - STEP)
                if int(((res[1][j] >= 0)).sum()) >= 6:
                    assert torch.equal(res[0][j], torch.eye(3, 4, device=dev())) and int(res[3][j, 3]) == 32 and int(res[3][j, 2]) == 65
                    on_anchor += 1
                    longer = p.extend(s_, poses=(res[0], res[3]), tol=8.0, min_views=2)  # resect()'s poses, as they stand
                    assert isinstance(longer, ops.Structure) and tuple(longer.points.shape) == (gs.N, 3)
                    assert tuple(p.world_pose(longer, res[0]).shape) == (STEP, 3, 4) and len(captures) == c1 + (c1 - c0)
                    extended += 1
        with pytest.raises(ValueError, match="beyond what has been tracked"):
            p.resect(structures[0][0], 2, first_frame=done - 1)
        with pytest.raises(ValueError, match="ops.Structure"):
            p.resect(None)
    assert checked == 6 and fitted > 0 and on_anchor > 0 and extended > 0  # (not vacuous)
    same_tracks = twin.recent(4)
    mine = p.recent(4)
    assert torch.equal(mine[0].view(torch.int32), same_tracks[0].view(torch.int32)) and torch.equal(mine[1], same_tracks[1])
    for x in (p, twin):
        x.finish()
    p2 = CoTrackerOnlinePredictor(checkpoint=None, v2=True, window_len=8)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.resect(None)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.model.stream_p3p(0, 1, cam, None, None)
