"""corr_mlp.fc2 folded into the input projection (include/ctk.h, ctk_model_weights "folded form"), on the GPU (-m gpu).

The window calls run fc1 straight into the folded input xf and ONE projection with K = 1632; the stage operators keep the unfolded
launches.  Both are compared here with ONE float64 evaluation of the unfolded formulas (oracle/window_fp64.py):

  tokens        after the projection, from the folded window path (ops.window_tokens) and from the unfolded operators
                (ops.corr_embed + ops.assemble_tokens + the projection as ops.gemm), at the smallest shapes where the folded path
                can go wrong.  The folded path's maximum error must stay within 2 x the unfolded path's on the same inputs -- the
                margin is for a different rounding order and nothing else.  Both errors go to profiles/fold_input_errors.json.
  merged GEMM   ops.gemm at K = 1632, N = 384, per-frame bias rows, SH input, against float64: within 2 x the error of the same call
                at K = 1120 (the first 1120 columns of the same operands), at M = 32 800 (persistent kernel + 64 x 64 tail) and
                M = 300 (64 x 64 kernel only).
  graph         a replayed folded window equals the direct launches bit for bit, and two replays are identical.
  full window   six iterations (S = 8, N = 300) against the float64 window, under the bars of tests/test_gpu_window_stages.py.

Measured on MI355X (max |error| of the tokens, folded / unfolded, |token| <= 3.6; profiles/fold_input_errors.json has every case):
split-half 3.9e-7 / 3.8e-7 (S=8, N=70, whole, chunked and as two shared groups), 5.6e-7 / 5.7e-7 (S=16, N=520), 5.1e-7 / 3.8e-7 (joint
B=2); exact f32 8.0e-7 / 5.3e-7 and 8.7e-7 / 8.4e-7.  Merged GEMM, K=1632 / K=1120: 5.8e-6 / 4.2e-6 (M=32 800), 4.3e-6 / 3.8e-6 (M=300).
Six iterations: 8.7e-5 px, 6.8e-6 / 6.0e-6 logit (split-half); 1.3e-4 px, 6.9e-6 / 6.1e-6 (exact f32).  The module takes 4 s."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import test_gpu_window_stages as WS  # noqa: E402  (inputs, checker and the bars of the window-stage tests: imported, not restated)
from ctk_support import ROOT, dev, recorded, same_bits  # noqa: E402
from ctk_support import precision_param as precision  # noqa: E402,F401
from oracle import window_fp64 as W  # noqa: E402  (checker only)

ERRORS = {}


def record(case, precision, **numbers):
    ERRORS.setdefault(case, {})[precision] = numbers
    with open(os.path.join(ROOT, "profiles", "fold_input_errors.json"), "w") as f:
        json.dump({"what": "max |tokens - float64| after the input projection: folded window path vs unfolded operators "
                           "(tests/test_gpu_fold_input.py)", "cases": ERRORS}, f, indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------
# inputs: one video = pyramid, support, moving tracks (the generators of the window-stage tests)
# ------------------------------------------------------------------------------------------
class Video:
    def __init__(self, S, N, seed):
        from cotracker_amd import ops
        self.S, self.N = S, N
        self.pyr = ops.build_pyramid(WS.features(S, seed=seed))
        self.pyr64 = [f.permute(0, 3, 1, 2).double().contiguous() for f in self.pyr]
        qc, qf, coords, vis, conf = WS.make_tracks(S, N, seed=seed + 1)
        self.qc, self.qf = qc.to(dev()), qf.to(dev())
        self.coords, self.vis, self.conf = coords.to(dev()), vis.to(dev()), conf.to(dev())
        self.sup = [ops.sample_support(self.pyr[l], self.qf.float(), (self.qc / 2 ** l).contiguous()) for l in range(4)]

    def window(self, **kw):
        from cotracker_amd import ops
        return ops.Window(self.pyr, self.sup, self.coords.clone(), self.vis.clone(), self.conf.clone(), WS.SCALE_XY, **kw)

    def tokens64(self, sl=slice(None)):
        """The float64 tokens [n,S,384] of the tracks `sl`: the unfolded formulas, once."""
        p = WS.model()["p64"]
        sup64 = [s_[:, sl] for s_ in WS.Case.sup64_of(self.sup, None)]
        c, v, f = self.coords[:, sl], self.vis[:, sl], self.conf[:, sl]
        with torch.no_grad():
            x = W.tokens(c, v, f, W.corr_embeds(self.pyr64, sup64, c, p), p, WS.RES, WS.STRIDE)
            return F.linear(x, p["updateformer.input_transform.weight"], p["updateformer.input_transform.bias"])


_videos = {}


def video(S, N, seed):
    if (S, N, seed) not in _videos:
        _videos[S, N, seed] = Video(S, N, seed)
    return _videos[S, N, seed]


def pw_of(precision):
    return WS.model()["m"].packed(dev(), precision)


def unfolded_tokens(wins, pw, points_per_chunk=None, shared=False):
    """The unfolded operators: corr_embed -> assemble_tokens -> input projection (the stage struct's own weight tensors)."""
    from cotracker_amd import ops
    S, N = wins[0].S, wins[0].N
    if len(wins) == 1:
        if points_per_chunk is not None:
            wins[0].args.points_per_chunk = points_per_chunk
        x = ops.corr_embed(wins[0], pw)
    else:
        x = ops.corr_embed_batch(wins, pw, points_per_chunk=points_per_chunk, shared=shared)
    for b, w_ in enumerate(wins):
        ops.assemble_tokens(w_, x[b * N * S:(b + 1) * N * S])
    st = pw.struct_for(S)
    held = {t_.data_ptr(): t_ for t_ in pw.keep}
    return ops.gemm(x, held[st.in_w], bias_rows=pw._bias_t[S, False], packed=held[st.in_p] if st.in_p else None)


def tokens_case(name, precision, wins, refs, points_per_chunk=None, shared=False):
    """wins: the B windows of one call; refs: their float64 tokens [N,S,384] each."""
    from cotracker_amd import ops
    S, N, B = wins[0].S, wins[0].N, len(wins)
    pw = pw_of(precision)
    start = [[t_.clone() for t_ in w_.state] for w_ in wins]
    folded = ops.window_tokens(wins, pw, points_per_chunk=points_per_chunk, shared=shared)
    unfolded = unfolded_tokens(wins, pw, points_per_chunk, shared)
    torch.cuda.synchronize()
    for w_, s_ in zip(wins, start):
        assert all(torch.equal(a, b) for a, b in zip(w_.state, s_)), "ops.window_tokens changed the window state"
    ref = torch.cat(refs, dim=0)
    wf = WS.check(folded.reshape(B * N, S, -1), ref)
    wu = WS.check(unfolded.reshape(B * N, S, -1), ref)
    scale = float(ref.abs().max())
    record(name, precision, S=S, N=N, B=B, points_per_chunk=points_per_chunk, shared=shared, folded_max_err=wf[0], unfolded_max_err=wu[0],
           ratio=wf[0] / wu[0] if wu[0] > 0 else None, tokens_max_abs=scale)
    print(f"{name} [{precision}]: tokens max |err| folded {wf[0]:.3e} (track {wf[1]}, frame {wf[2]}, column {wf[3]}), "
          f"unfolded {wu[0]:.3e}; max |token| {scale:.3f}")
    assert wu[0] < 1e-3 * scale, "the unfolded reference path itself is off: the comparison would mean nothing"
    assert wf[0] <= 2.0 * wu[0], (f"{name}: folded tokens max |error| {wf[0]:.3e} > 2 x the unfolded path's {wu[0]:.3e} "
                                  f"(worst at track {wf[1]}, frame {wf[2]}, column {wf[3]})")


# S, N, points_per_chunk: 560 ragged rows on the 64 x 64 kernels; a chunk cut inside a tile; 8 320 rows -- the smallest count at
# which the level-batched fc1 reaches the persistent kernel (4 x 33 x 2 = 264 tiles >= 256 CUs), with a ragged last tile
SINGLE = {"s8_n70": (8, 70, None), "s8_n70_chunk32": (8, 70, 32), "s16_n520": (16, 520, None)}


@pytest.mark.parametrize("name", list(SINGLE))
def test_tokens_single_window(name, precision):
    S, N, ppc = SINGLE[name]
    v = video(S, N, seed=300 + S)
    tokens_case(name, precision, [v.window()], [v.tokens64()], points_per_chunk=ppc)


def test_fc1_of_8320_rows_runs_on_the_persistent_kernel():
    """What makes s16_n520 the threshold case: the folded window's fc1 is ONE persistent launch there, the projection stays on
    the 64 x 64 kernel, and no fc2 launch is left."""
    from cotracker_amd import ops
    v = video(16, 520, seed=316)
    _, rows = recorded(lambda: ops.window_tokens([v.window()], pw_of("f16x3")))
    assert rows.get("gemm_sh_pp192_k2432_n384") == 1 and rows.get("gemm_sh_64_k1632_n384") == 1, rows
    assert not [k for k in rows if k.endswith("_k384_n256") or "_k1120_" in k], rows


def test_two_stream_overlap_gives_the_same_bits():
    """CTK_OPT_OVERLAP bit 0 on the folded path: fc1 of a point piece on the auxiliary stream beside the next piece's sampler, joined
    before the projection -- the same launches on the same inputs.  1 030 points: two pieces, the second one ragged."""
    from cotracker_amd import _lib as L, ops
    v = video(8, 1030, seed=708)
    pw = pw_of("f16x3")
    plain = ops.window_tokens([v.window()], pw)
    with L.option(L.OPT_OVERLAP, 1):
        piped = ops.window_tokens([v.window()], pw)
    torch.cuda.synchronize()
    assert same_bits(plain, piped)
    assert float(plain.abs().max()) > 0.1


def test_tokens_joint_two_videos_chunk_straddles(precision):
    S, N = 8, 70
    a, b = video(S, N, seed=308), video(S, N, seed=408)
    tokens_case("joint_b2_chunk100", precision, [a.window(), b.window()], [a.tokens64(), b.tokens64()], points_per_chunk=100)


def test_tokens_shared_groups(precision):
    """Two query groups of 35 tracks over one video (CTK_BATCH_SHARED_FMAPS): the 70 tracks of the single-window case, regrouped."""
    from cotracker_amd import ops
    S, N, G = 8, 70, 2
    v = video(S, N, seed=308)
    h = N // G
    coords = torch.stack([v.coords[:, g * h:(g + 1) * h] for g in range(G)]).contiguous()
    vis = torch.stack([v.vis[:, g * h:(g + 1) * h] for g in range(G)]).contiguous()
    conf = torch.stack([v.conf[:, g * h:(g + 1) * h] for g in range(G)]).contiguous()
    wins = ops.group_windows(v.pyr, v.sup, coords, vis, conf, WS.SCALE_XY)
    tokens_case("shared_g2", precision, wins, [v.tokens64(slice(g * h, (g + 1) * h)) for g in range(G)], shared=True)


# ------------------------------------------------------------------------------------------
# the merged GEMM's shape against the shape it replaces
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,kernels", [(32800, {"gemm_sh_pp192_k%d_n384", "gemm_sh_64_k%d_n384"}), (300, {"gemm_sh_64_k%d_n384"})])
def test_merged_gemm_shape(M, kernels):
    from cotracker_amd import _lib as L, ops
    g = torch.Generator().manual_seed(1632 + M)
    A = torch.randn(M, L.XF_LD, generator=g).to(dev())
    Wt = (torch.randn(L.HID, L.XF_LD, generator=g) / 40).to(dev())
    rows = torch.randn(16, L.HID, generator=g).to(dev())
    err = {}
    for K in (L.XF_LD, L.X_LD):
        a, w = A[:, :K].contiguous(), Wt[:, :K].contiguous()
        out, ran = recorded(lambda: ops.gemm(ops.split_rows(a), w, bias_rows=rows, packed=ops.pack_weight(w)))
        torch.cuda.synchronize()
        ref = a.double() @ w.double().t() + rows.double().repeat((M + 15) // 16, 1)[:M]
        err[K] = float((out.double() - ref).abs().max())
        assert {k for k in ran if k.startswith("gemm_")} == {k % K for k in kernels}, ran
    print(f"M={M}: max |err| K=1632 {err[L.XF_LD]:.3e}, K=1120 {err[L.X_LD]:.3e}")
    assert err[L.XF_LD] <= 2.0 * err[L.X_LD], err


# ------------------------------------------------------------------------------------------
# graph replay of a folded window
# ------------------------------------------------------------------------------------------
def test_graph_replay_is_the_direct_launches():
    from cotracker_amd import ops
    v = video(16, 128, seed=516)
    pw = pw_of("f16x3")
    direct = v.window(iters=2)
    ops.forward_window(direct, pw)
    win = v.window(iters=2)
    start = [t_.clone() for t_ in win.state]
    graph = ops.WindowGraph(win, pw)
    replays = []
    for _ in range(2):
        for t_, s_ in zip(win.state, start):
            t_.copy_(s_)
        graph.launch()
        torch.cuda.synchronize()
        replays.append([t_.clone() for t_ in win.state])
    for k, d, r0, r1 in zip(("coords", "vis", "conf"), direct.state, *replays):
        assert same_bits(r0, d), f"{k}: graph replay differs from the direct launches"
        assert same_bits(r0, r1), f"{k}: two replays differ"
    assert float((direct.state[0] - start[0]).abs().max()) > 1e-3  # the window moved the tracks


# ------------------------------------------------------------------------------------------
# a full window on the folded path
# ------------------------------------------------------------------------------------------
def test_six_iterations_against_float64(precision):
    """S = 8, N = 300: the `small` case of the window-stage tests, its cached float64 run and its bars for six iterations."""
    from cotracker_amd import ops
    cs = WS.get_case("small")
    st = cs.state()
    _, rows = recorded(lambda: ops.forward_window(cs.window(st, iters=6), cs.pw(precision)))
    torch.cuda.synchronize()
    assert not [k for k in rows if k.endswith("_k384_n256") or "_k1120_" in k], f"an unfolded launch on the window path: {rows}"
    w = WS.compare_state(st, cs.free_run64(), px_scale=float(WS.STRIDE))
    print(f"six iterations [{precision}]: coords {w['coords'][0]:.3e} px, vis {w['vis'][0]:.3e}, conf {w['conf'][0]:.3e}")
    WS.expect("six iterations on the folded path, coords (px at model resolution)", w["coords"], WS.BAR["px"])
    WS.expect("six iterations on the folded path, vis logit", w["vis"], WS.BAR["logit"])
    WS.expect("six iterations on the folded path, conf logit", w["conf"], WS.BAR["logit"])
