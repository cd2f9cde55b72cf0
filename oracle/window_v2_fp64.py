"""One CoTracker2 update window, stage by stage, in plain torch -- on any device and in any floating dtype.

THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE (see oracle/cotracker_oracle.py).  It restates CoTracker2.forward_window
(cotracker.py:86-173) one function per stage, with torch ops only, so that the same text runs in float64 on the GPU -- the
reference tests/test_gpu_window_v2_stages.py holds every HIP stage of ctk_forward_window_v2 to, at the full window size -- and in
float32 / float64 on the CPU, where tests/test_window_v2_fp64_reference.py pins it against the goldens of the unmodified reference.
It imports nothing of the library; what it shares with the CoTracker3 text (oracle/window_fp64.py: the coordinate rule `_grid`,
the lattice, Mlp, AttnBlock, CrossAttnBlock) it imports from there.  Device and dtype are those of the tensors it is given.

Layouts are the reference's without its batch axis (one window = one video):
  pyr[l]      [S,C,H,W]   CorrBlock pyramid of the window's frames, NOT normalised (blocks.py:300-307)
  coords      [S,N,2]     (x, y) in level-0 feature units
  track_feat  [S,N,128]   = the CorrBlock targets; already multiplied by the attention mask (cotracker.py:346)
  vis, track_mask [S,N];  mask [N] (or [S,N]) bool, the attention mask: False = a point that is not tracked yet
  pos         [N,456]     pos_emb at the first frame's coordinates
  fcorrs      [N,S,196]   column = 49 * level + 7 * (x tap) + (y tap)                (blocks.py:309-340)
  x           [N,S,456]   cat(flow 2 | pe 128 | fcorrs 196 | track_feat 128 | track_mask | vis) + pos + time embedding
  delta       [N,S,130]   (dx, dy, 128 feature deltas)

Position arithmetic (where a tap lands, the argument of the flow embedding's sin / cos) runs in the dtype of the coordinates it
is given, as window_fp64._grid explains; values run in the dtype of the features / parameters.

`faults` arguments (and `on_volume`) exist for the negative controls of the GPU stage tests: each plants ONE small, named fault
in this reference (never in a kernel) so that a test can show its bar would notice the same fault in the kernel.
"""
import math

import torch
import torch.nn.functional as F

from .window_fp64 import HID, TAPS, VIRT, _grid, cast_params, cross_block, lattice, self_block  # noqa: F401

LEVELS, LATENT, IN_DIM = 4, 128, 456
NEG = -torch.finfo(torch.float32).max  # -FLT_MAX: what (~mask) * max_neg_value puts on a masked logit (cotracker.py:571-572)


def pyramid(f0):
    """CorrBlock.__init__ (blocks.py:300-307): f0 [S,C,H,W] -> [f0, three times avg_pool2d(2, stride=2)]."""
    pyr = [f0]
    for _ in range(LEVELS - 1):
        pyr.append(F.avg_pool2d(pyr[-1], 2, stride=2))
    return pyr


def pos(p, coords0):
    """sampled_pos_emb (cotracker.py:126-130; sample_features4d, model_utils.py:258-290): pos_emb [1,456,H,W] at the first
    frame's coordinates [N,2] -> [N,456]."""
    pe = p["pos_emb"]
    H, W = pe.shape[-2:]
    grid = torch.stack([_grid(coords0[:, 0], W, pe.dtype), _grid(coords0[:, 1], H, pe.dtype)], dim=-1)[None, :, None]  # [1,N,1,2]
    return F.grid_sample(pe, grid, mode="bilinear", align_corners=True, padding_mode="border")[0, :, :, 0].t()


def corrblock(pyr, track_feat, coords, chunk=None, on_volume=None, faults=None):
    """CorrBlock.corr + CorrBlock.sample (blocks.py:309-362) -> fcorrs [N,S,196].  Per level the FULL volume
    <track_feat[s,n], pyr_l[s,:,y,x]> / sqrt(128) is formed and sampled at coords / 2^l + lattice with grid_sample
    (align_corners=True, border).  chunk: points at a time (the float64 level-0 volume of 6400 points x 8 frames over a
    96 x 128 map is 5 GB).  on_volume(level, n0, n1, vol [S,n1-n0,H,W]) -> vol or None: lets a test look at, or plant a fault
    in, every volume on its way to the sampler.  faults: {"drop_tap": (level, tap)} -- that tap of that level contributes 0."""
    faults = faults or {}
    S, N = coords.shape[:2]
    chunk = chunk or N
    out = pyr[0].new_empty(N, S, LEVELS * TAPS)
    for l, f in enumerate(pyr):
        H, W = f.shape[-2:]
        for n0 in range(0, N, chunk):
            n1 = min(N, n0 + chunk)
            vol = torch.einsum("snc,schw->snhw", track_feat[:, n0:n1].to(f.dtype), f) / math.sqrt(f.shape[1])
            if on_volume is not None:
                alt = on_volume(l, n0, n1, vol)
                vol = vol if alt is None else alt
            pts = coords[:, n0:n1, None] / 2 ** l + lattice(coords)[None, None]              # [S,n,49,2], in coords' dtype
            grid = torch.stack([_grid(pts[..., 0], W, f.dtype), _grid(pts[..., 1], H, f.dtype)], dim=-1)
            smp = F.grid_sample(vol.reshape(S * (n1 - n0), 1, H, W), grid.reshape(S * (n1 - n0), 7, 7, 2), mode="bilinear",
                                align_corners=True, padding_mode="border").reshape(S, n1 - n0, TAPS)
            if faults.get("drop_tap", (None,))[0] == l:
                smp[..., faults["drop_tap"][1]] = 0
            out[n0:n1, :, l * TAPS:(l + 1) * TAPS] = smp.permute(1, 0, 2)
    return out


def flow_embedding(flows, dtype, faults=None):
    """get_2d_embedding(flows, 64, cat_coords=True) (embeddings.py:87-120): flows [...,2] -> [...,130] = (flows | pe_x 64 | pe_y 64),
    sin on the even and cos on the odd columns of each half.  The product flows * div (div = arange(0, 64, 2) * 1000 / 64) is
    taken in the dtype of `flows`, sin / cos in `dtype`.  faults: {"swap_xy": True} exchanges pe_x and pe_y."""
    div = torch.arange(0, 64, 2, device=flows.device, dtype=flows.dtype) * (1000.0 / 64)
    halves = []
    for a in range(2):
        arg = (flows[..., a:a + 1] * div).to(dtype)
        halves.append(torch.stack([torch.sin(arg), torch.cos(arg)], dim=-1).reshape(*flows.shape[:-1], 64))
    if (faults or {}).get("swap_xy"):
        halves.reverse()
    return torch.cat([flows.to(dtype)] + halves, dim=-1)


def assemble(coords, fcorrs, track_feat, track_mask, vis, pos_, faults=None):
    """transformer_input + sampled_pos_emb (cotracker.py:139-151 without the time embedding: what ctk_v2_assemble writes)
    -> [N,S,456].  faults: {"swap_xy": True} (flow_embedding)."""
    dt = fcorrs.dtype
    emb = flow_embedding((coords - coords[0:1]).permute(1, 0, 2), dt, faults)                 # [N,S,130]
    x = torch.cat([emb, fcorrs, track_feat.to(dt).permute(1, 0, 2), track_mask.to(dt).t()[..., None], vis.to(dt).t()[..., None]], dim=-1)
    return x + pos_[:, None]


def time_embed(p, S, faults=None):
    """self.time_emb (cotracker.py:57-59, 151) -> [S,456].  faults: {"swap_time": t} exchanges the rows of frames t and t + 1."""
    te = p["time_emb"][0]
    assert te.shape == (S, IN_DIM), te.shape
    if "swap_time" in (faults or {}):
        t = faults["swap_time"]
        te = te.clone()
        te[[t, t + 1]] = te[[t + 1, t]]
    return te


def tokens(coords, fcorrs, track_feat, track_mask, vis, pos_, p, faults=None):
    """x = transformer_input + sampled_pos_emb + time_emb (cotracker.py:139-151) -> [N,S,456]."""
    return assemble(coords, fcorrs, track_feat, track_mask, vis, pos_, faults) + time_embed(p, coords.shape[0], faults)


def _bias(mask, queries, dtype):
    """The attn_bias of CrossAttnBlock.forward (cotracker.py:560-572) for mask [S,n] bool: over QUERIES when n is the number of
    queries -- every logit of a masked query gets -FLT_MAX, so that row attends uniformly -- and over KEYS otherwise."""
    b = (~mask).to(dtype) * NEG
    return b[:, None, :, None] if mask.shape[1] == queries else b[:, None, None, :]


def update_former(x, p, mask=None, depth=6, each_depth=False, faults=None, u="updateformer."):
    """EfficientUpdateFormer.forward (cotracker.py:483-531) as CoTracker2 builds it (:46-56: 6 + 6 layers, one flow_head of 130
    outputs) with the attention mask: x [N,S,456] (time embedding included), mask [N] or [S,N] bool -> delta [N,S,130].
    each_depth: [delta after 1 layer, after 2, ...], i.e. what a former of that many layers returns.
    faults: {"v2p_unmask": (layer, head, k0, k1)} -- that head of that virtual<-points layer ignores the key mask on keys k0..k1-1;
            {"p2v_unmask": layer} -- that points<-virtual layer leaves the masked queries unmasked."""
    faults = faults or {}
    t = F.linear(x, p[u + "input_transform.weight"], p[u + "input_transform.bias"])
    N, S, _ = t.shape
    if mask is not None:
        mask = mask.to(torch.bool)
        mask = mask[None].expand(S, N) if mask.dim() == 1 else mask
    t = torch.cat([t, p[u + "virual_tracks"].reshape(VIRT, 1, HID).to(t.dtype).expand(VIRT, S, HID)], dim=0)  # [N+64,S,384]
    head = lambda tok: F.linear(tok, p[u + "flow_head.weight"], p[u + "flow_head.bias"])  # noqa: E731
    outs = []
    for i in range(depth):
        t = self_block(t, p, f"{u}time_blocks.{i}.")
        s = t.permute(1, 0, 2)                                                                # [S,N+64,384]
        pt, vt = s[:, :N], s[:, N:]
        kb = qb = None
        if mask is not None:
            kb, qb = _bias(mask, VIRT, t.dtype), _bias(mask, N, t.dtype)
            f = faults.get("v2p_unmask")
            if f is not None and f[0] == i and kb.shape[-1] == N:
                kb = kb.expand(S, 8, 1, N).clone()
                kb[:, f[1], :, f[2]:f[3]] = 0
            if faults.get("p2v_unmask") == i:
                qb = None
        vt = cross_block(vt, pt, p, f"{u}space_virtual2point_blocks.{i}.", mask=kb)
        vt = self_block(vt, p, f"{u}space_virtual_blocks.{i}.")
        pt = cross_block(pt, vt, p, f"{u}space_point2virtual_blocks.{i}.", mask=qb)
        t = torch.cat([pt, vt], dim=1).permute(1, 0, 2)
        if each_depth:
            outs.append(head(t[:N]))
    return outs if each_depth else head(t[:N])


def apply_delta(coords, delta, p, faults=None):
    """cotracker.py:159-167: -> (coords + delta[..., :2] as [S,N,2], GroupNorm(1, 128) of delta[..., 2:] as [N,S,128]).
    faults: {"unbiased": True} divides the variance by 127."""
    d = delta[..., 2:]
    mu = d.mean(dim=-1, keepdim=True)
    var = d.var(dim=-1, keepdim=True, unbiased=bool((faults or {}).get("unbiased")))
    normed = (d - mu) / torch.sqrt(var + 1e-5) * p["norm.weight"] + p["norm.bias"]
    return coords.to(delta.dtype) + delta[..., :2].permute(1, 0, 2), normed


def updater(normed, track_feat, p, faults=None):
    """track_feat_updater(norm(delta_feats)) + track_feat (cotracker.py:167; Linear + erf GELU, :80): normed [N,S,128],
    track_feat [S,N,128] -> [S,N,128].  faults: {"tanh_gelu": True}."""
    h = F.linear(normed, p["track_feat_updater.0.weight"], p["track_feat_updater.0.bias"])
    h = F.gelu(h, approximate="tanh" if (faults or {}).get("tanh_gelu") else "none")
    return h.permute(1, 0, 2) + track_feat.to(h.dtype)


def vis_head(track_feat, p):
    """vis_predictor (cotracker.py:81-83, 172): [S,N,128] -> logits [S,N]."""
    return F.linear(track_feat, p["vis_predictor.0.weight"], p["vis_predictor.0.bias"])[..., 0]


def iterate(state, pyr, pos_, vis, track_mask, mask, p, chunk=None, trace=None, faults=None):
    """One update iteration (cotracker.py:133-170): state = (coords [S,N,2], track_feat [S,N,128]) -> the new state in the
    pyramid's dtype.  A float32 state is sampled at the reference's float32 tap positions (_grid), everything else is exact.
    trace: a list that receives dict(fcorrs, x, delta, coords, track_feat) of this iteration."""
    coords, track_feat = state
    fcorrs = corrblock(pyr, track_feat, coords, chunk, faults=faults)
    x = tokens(coords, fcorrs, track_feat, track_mask, vis, pos_, p, faults)
    delta = update_former(x, p, mask, faults=faults)
    new_coords, normed = apply_delta(coords, delta, p, faults)
    new_feat = updater(normed, track_feat, p, faults)
    if trace is not None:
        trace.append(dict(fcorrs=fcorrs, x=x, delta=delta, coords=new_coords, track_feat=new_feat))
    return new_coords, new_feat


def forward_window(pyr, coords, track_feat, vis, track_mask, mask, p, iters, chunk=None, trace=None):
    """CoTracker2.forward_window (cotracker.py:86-173): `iters` iterations from (coords, track_feat) -> (coords of the last
    iteration in level-0 units, visibility logits [S,N], track_feat).  trace: see `iterate`."""
    pos_ = pos(p, coords[0])
    state = (coords, track_feat)
    for _ in range(iters):
        state = iterate(state, pyr, pos_, vis, track_mask, mask, p, chunk, trace)
    return state[0], vis_head(state[1].to(pyr[0].dtype), p), state[1]
