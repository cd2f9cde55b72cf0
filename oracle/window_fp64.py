"""One CoTracker3 update window, stage by stage, in plain torch -- on any device and in any floating dtype.

THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE (see oracle/cotracker_oracle.py).  It restates
CoTrackerThreeOnline.forward_window (cotracker3_online.py:171-264) one function per stage, with torch ops only
(F.grid_sample, einsum, F.linear, F.layer_norm, F.gelu, softmax), so that the same text runs in float64 on the GPU --
the reference tests/test_gpu_window_stages.py holds every HIP stage to, at the full window size -- and in float32 /
float64 on the CPU, where tests/test_window_fp64_reference.py pins it against the goldens of the unmodified reference.
It imports nothing of the library: no cotracker_amd._lib, no ops, no HIP kernel of this project.  Device and dtype are
those of the tensors it is given; constants are built with them.

Layouts are the reference's without its batch axis (one window = one video):
  pyr[l]      [S,C,H,W]   feature pyramid of the window's frames (of the whole video for `support`)
  support[l]  [49,N,C]    support features of the query, first lattice index = x  (cotracker3_online.py:94-128)
  coords      [S,N,2]     (x, y) in level-0 feature units;  vis / conf [S,N] logits
  volume      [S,N,2401]  column = (tap of the frame's patch) * 49 + (tap of the support patch)
  x           [N,S,1110]  columns [vis, conf, corr_emb(4 x 256), posenc(84)]   (cotracker3_online.py:212-248)
  delta       [N,S,4]     (dx, dy, dvis, dconf)                                 (cotracker.py:526-531)

`faults` arguments exist for the negative controls of the GPU stage tests: they plant ONE small, named fault in this
reference (never in a kernel) so that a test can show its bar would notice the same fault in the kernel.
"""
import math

import torch
import torch.nn.functional as F

R = 3            # corr_radius
TAPS = 49        # (2 R + 1)^2
HID, HEADS, VIRT = 384, 8, 64


def cast_params(p, device, dtype):
    """The update path's parameters (state_dict entries without the encoder) on `device` in `dtype`."""
    return {k: v.detach().to(device=device, dtype=dtype) for k, v in p.items() if not k.startswith("fnet.")}


def lattice(like):
    """get_support_points (cotracker3_online.py:94-111): the 49 (dx, dy) offsets, dx-major."""
    d = torch.arange(-R, R + 1, device=like.device, dtype=like.dtype)
    dx, dy = torch.meshgrid(d, d, indexing="ij")
    return torch.stack([dx, dy], dim=-1).reshape(TAPS, 2)


def _grid(c, size, dtype):
    """Pixel coordinate -> grid_sample's [-1, 1] (align_corners=True), for sampling values in `dtype`.

    The reference maps coordinates in the dtype of the coordinate tensor, float32 (model_utils.py:242-251: multiply by
    2 / (size - 1), subtract 1; ATen then takes ((g + 1) / 2) * (size - 1) back), and where a tap lands is part of what the
    model computes: at x ~ 100 that rounding moves a tap by up to 4e-6 px, more than the value bars of the stage tests.  So the
    position arithmetic here runs in the dtype of `c` -- float32 state from the kernels gives the reference's tap positions,
    float64 state gives exact ones -- and only the interpolation runs in `dtype`."""
    g = c * (2.0 / max(size - 1, 1)) - 1.0
    if c.dtype == dtype:
        return g
    u = ((g + 1.0) / 2.0) * (size - 1)
    return u.to(dtype) * (2.0 / max(size - 1, 1)) - 1.0


def support(pyr, qframes, qcoords):
    """get_track_feat (cotracker3_online.py:113-128) on every level: pyr[l] [T,C,H,W], qframes [N] (integer valued),
    qcoords [N,2] level-0 units -> list of [49,N,C].  Trilinear (t, y, x) sampling with border padding."""
    out = []
    for l, f in enumerate(pyr):
        T, C, H, W = f.shape
        pts = qcoords[None] / 2 ** l + lattice(qcoords)[:, None]                            # [49,N,2], in qcoords' dtype
        t = qframes.to(qcoords.dtype)[None].expand(TAPS, -1)
        grid = torch.stack([_grid(pts[..., 0], W, f.dtype), _grid(pts[..., 1], H, f.dtype), _grid(t, T, f.dtype)],
                           dim=-1)[None, :, :, None]                                        # [1,49,N,1,3]
        s = F.grid_sample(f.permute(1, 0, 2, 3)[None], grid, mode="bilinear", align_corners=True, padding_mode="border")
        out.append(s[0, :, :, :, 0].permute(1, 2, 0))                                       # [C,49,N] -> [49,N,C]
    return out


def patches(pyr_l, coords_l):
    """get_correlation_feat (cotracker3_online.py:130-143): pyr_l [S,C,H,W], coords_l [S,N,2] in THIS level's units
    -> [S,N,49,C]."""
    S, C, H, W = pyr_l.shape
    pts = coords_l[:, :, None] + lattice(coords_l)[None, None]                              # [S,N,49,2], in coords' dtype
    grid = torch.stack([_grid(pts[..., 0], W, pyr_l.dtype), _grid(pts[..., 1], H, pyr_l.dtype)], dim=-1)
    return F.grid_sample(pyr_l, grid, mode="bilinear", align_corners=True, padding_mode="border").permute(0, 2, 3, 1)


def volume(pyr_l, support_l, coords_l):
    """The 49 x 49 correlation of one level (cotracker3_online.py:193-207): pyr_l [S,C,H,W], support_l [49,N,C],
    coords_l [S,N,2] in this level's units -> [S,N,2401]."""
    S, N = coords_l.shape[:2]
    return torch.einsum("tnpc,qnc->tnpq", patches(pyr_l, coords_l), support_l).reshape(S, N, TAPS * TAPS)


def mlp(x, p, pre, tanh=True):
    """Mlp.forward (blocks.py:70-76)."""
    h = F.gelu(F.linear(x, p[pre + "fc1.weight"], p[pre + "fc1.bias"]), approximate="tanh" if tanh else "none")
    return F.linear(h, p[pre + "fc2.weight"], p[pre + "fc2.bias"])


def corr_embed(vol, p):
    """corr_mlp on the rows of a volume (cotracker3_online.py:208): [...,2401] -> [...,256]; erf GELU."""
    return mlp(vol, p, "corr_mlp.", tanh=False)


def posenc(x, lo=0, hi=10):
    """posenc (cotracker3_online.py:19-39): [...,D] -> [...,D + 2 D (hi - lo)]."""
    scales = 2.0 ** torch.arange(lo, hi, device=x.device, dtype=x.dtype)
    xb = (x[..., None, :] * scales[:, None]).reshape(*x.shape[:-1], -1)
    return torch.cat([x, torch.sin(torch.cat([xb, xb + 0.5 * math.pi], dim=-1))], dim=-1)


def posenc_tokens(coords, vis, conf, res=(384, 512), stride=4):
    """The columns of x that are not correlation (cotracker3_online.py:212-241): coords [S,N,2], vis / conf [S,N]
    -> (vis_conf [N,S,2], rel_pos [N,S,84])."""
    z = torch.zeros_like(coords[:1])
    scale = torch.tensor([res[1], res[0]], device=coords.device, dtype=coords.dtype) / stride
    fwd = torch.cat([coords[:-1] - coords[1:], z], dim=0) / scale
    bwd = torch.cat([z, coords[1:] - coords[:-1]], dim=0) / scale
    pe = posenc(torch.cat([fwd, bwd], dim=-1))
    return torch.stack([vis, conf], dim=-1).permute(1, 0, 2), pe.permute(1, 0, 2)


def time_embed(p, S):
    """interpolate_time_embed (cotracker3_online.py:145-156) -> [S,1110]."""
    te = p["time_emb"]
    if S != te.shape[1]:
        te = F.interpolate(te.permute(0, 2, 1), size=S, mode="linear").permute(0, 2, 1)
    return te[0]


def tokens(coords, vis, conf, emb, p, res=(384, 512), stride=4):
    """x [N,S,1110] = cat(vis, conf, emb [S,N,1024], posenc) + time embedding (cotracker3_online.py:212-248)."""
    dt = emb.dtype
    vc, pe = posenc_tokens(coords.to(dt), vis.to(dt), conf.to(dt), res, stride)
    return torch.cat([vc, emb.permute(1, 0, 2), pe], dim=-1) + time_embed(p, coords.shape[0])


def attention(x, ctx, p, pre, drop_keys=None, mask=None):
    """Attention.forward (blocks.py:379-398): x [B,N1,384], ctx [B,N2,384].  drop_keys = (head, k0, k1): a planted fault --
    that head ignores keys k0..k1-1.  mask: attn_bias (blocks.py:392-394), added to the scaled logits; anything that
    broadcasts to [B,8,N1,N2] (CoTracker2 only, oracle/window_v2_fp64.py)."""
    B, N1, C = x.shape
    d = C // HEADS
    q = F.linear(x, p[pre + "to_q.weight"], p[pre + "to_q.bias"]).reshape(B, N1, HEADS, d).permute(0, 2, 1, 3)
    k, v = F.linear(ctx, p[pre + "to_kv.weight"], p[pre + "to_kv.bias"]).chunk(2, dim=-1)
    k = k.reshape(B, -1, HEADS, d).permute(0, 2, 1, 3)
    v = v.reshape(B, -1, HEADS, d).permute(0, 2, 1, 3)
    s = (q @ k.transpose(-2, -1)) * d ** -0.5
    if mask is not None:
        s = s + mask
    if drop_keys is not None:
        h, k0, k1 = drop_keys
        s[:, h, :, k0:k1] = -math.inf
    o = (s.softmax(dim=-1) @ v).transpose(1, 2).reshape(B, N1, C)
    return F.linear(o, p[pre + "to_out.weight"], p[pre + "to_out.bias"])


def self_block(x, p, pre):
    """AttnBlock.forward (blocks.py:426-438)."""
    n = F.layer_norm(x, (HID,), eps=1e-6)
    x = x + attention(n, n, p, pre + "attn.")
    return x + mlp(F.layer_norm(x, (HID,), eps=1e-6), p, pre + "mlp.")


def cross_block(x, ctx, p, pre, drop_keys=None, mask=None):
    """CrossAttnBlock.forward (cotracker.py:559-577); mask: the additive attn_bias of `attention`."""
    c = F.layer_norm(ctx, (HID,), p[pre + "norm_context.weight"], p[pre + "norm_context.bias"], eps=1e-5)
    x = x + attention(F.layer_norm(x, (HID,), eps=1e-6), c, p, pre + "cross_attn.", drop_keys, mask)
    return x + mlp(F.layer_norm(x, (HID,), eps=1e-6), p, pre + "mlp.")


def heads(t, p, u="updateformer."):
    """flow_head and vis_conf_head (cotracker.py:526-531): tokens [N,S,384] -> [N,S,4]."""
    return torch.cat([F.linear(t, p[u + "flow_head.weight"], p[u + "flow_head.bias"]),
                      F.linear(t, p[u + "vis_conf_head.weight"], p[u + "vis_conf_head.bias"])], dim=-1)


def update_former(x, p, depth=3, each_depth=False, faults=None, u="updateformer."):
    """EfficientUpdateFormer.forward (cotracker.py:483-531): x [N,S,1110] (time embedding included) -> delta [N,S,4].
    each_depth: return [delta after 1 layer, after 2, ...] -- the heads applied to the tokens after every depth, i.e. what a
    former of that many layers returns.  faults: {"v2p_keys": (layer, head, k0, k1)} drops those keys of virtual<-points."""
    faults = faults or {}
    t = F.linear(x, p[u + "input_transform.weight"], p[u + "input_transform.bias"])
    N, S, _ = t.shape
    t = torch.cat([t, p[u + "virual_tracks"].reshape(VIRT, 1, HID).to(t.dtype).expand(VIRT, S, HID)], dim=0)  # [N+64,S,384]
    outs = []
    for i in range(depth):
        t = self_block(t, p, f"{u}time_blocks.{i}.")                       # attention over time, one batch entry per track
        s = t.permute(1, 0, 2)                                            # [S,N+64,384]: attention over tracks, per frame
        pt, vt = s[:, :N], s[:, N:]
        dk = faults.get("v2p_keys")
        vt = cross_block(vt, pt, p, f"{u}space_virtual2point_blocks.{i}.", dk[1:] if dk is not None and dk[0] == i else None)
        vt = self_block(vt, p, f"{u}space_virtual_blocks.{i}.")
        pt = cross_block(pt, vt, p, f"{u}space_point2virtual_blocks.{i}.")
        t = torch.cat([pt, vt], dim=1).permute(1, 0, 2)
        if each_depth:
            outs.append(heads(t[:N], p, u))
    return outs if each_depth else heads(t[:N], p, u)


def corr_embeds(pyr, sup, coords, p, chunk=None, on_volume=None):
    """The correlation stage of one iteration (cotracker3_online.py:190-210): -> emb [S,N,1024].  chunk: points at a time (the
    float64 volume of 6400 points is 2 GB per level).  on_volume(level, n0, n1, vol [S,n1-n0,2401]) -> vol or None: lets a test
    look at, or plant a fault in, every volume on its way to corr_mlp."""
    S, N = coords.shape[:2]
    chunk = chunk or N
    emb = pyr[0].new_empty(S, N, 4 * 256)
    for l in range(len(pyr)):
        for n0 in range(0, N, chunk):
            n1 = min(N, n0 + chunk)
            vol = volume(pyr[l], sup[l][:, n0:n1], coords[:, n0:n1] / 2 ** l)
            if on_volume is not None:
                alt = on_volume(l, n0, n1, vol)
                vol = vol if alt is None else alt
            emb[:, n0:n1, l * 256:(l + 1) * 256] = corr_embed(vol, p)
    return emb


def iterate(state, pyr, sup, p, res=(384, 512), stride=4, chunk=None, depth=3):
    """One update iteration (cotracker3_online.py:187-262): state = (coords [S,N,2], vis [S,N], conf [S,N]) -> new state in the
    pyramid's dtype.  A float32 state is sampled at the reference's float32 tap positions (_grid), everything else is exact."""
    coords, vis, conf = state
    emb = corr_embeds(pyr, sup, coords, p, chunk)
    d = update_former(tokens(coords, vis, conf, emb, p, res, stride), p, depth).permute(1, 0, 2)   # [S,N,4]
    return coords.to(d.dtype) + d[..., :2], vis.to(d.dtype) + d[..., 2], conf.to(d.dtype) + d[..., 3]


def forward_window(pyr, coords, sup, vis, conf, p, iters, res=(384, 512), stride=4, chunk=None, trace=None):
    """CoTrackerThreeOnline.forward_window (cotracker3_online.py:171-264): `iters` iterations from (coords, vis, conf);
    returns the last state, coords in level-0 units (x stride = pixels).  trace: a list that receives every iterate."""
    state = (coords, vis, conf)
    for _ in range(iters):
        state = iterate(state, pyr, sup, p, res, stride, chunk)
        if trace is not None:
            trace.append(state)
    return state
