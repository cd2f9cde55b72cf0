"""CoTracker2 / CoTracker2.1 on the MI355X primitives.

Host-side mirror of ``CoTracker2`` (cotracker/models/core/cotracker/cotracker.py:29-384): same constructor kwargs,
attributes, ``forward`` signature / 3-tuple return, online-state methods and the same 321 ``state_dict`` keys
(``time_emb``, ``pos_emb``, ``fnet.*``, ``updateformer.*`` with 6 time + 6 space layers and a 130-wide ``flow_head``,
``norm.*``, ``track_feat_updater.0.*``, ``vis_predictor.0.*``), so reference checkpoints load unchanged.
"""
import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .encoder import BasicEncoder
from .model import OnlineState, TrackerBase, _Lin, _online_attr, _UpdateFormerParams, sincos_time_embed

IN_LD, OUT_LD, DEPTH_V2 = 480, 192, 6  # input_dim 456 / output_dim 130 padded for the GEMM tiles


def sincos_pos_embed_2d(dim: int, h: int, w: int) -> torch.Tensor:
    """get_2d_sincos_pos_embed (embeddings.py:11-55) -> [1, dim, h, w]: first half encodes the x (column) index,
    second half the y (row) index, each as [sin(pos*omega), cos(pos*omega)] with omega_k = 10000^(-k/(dim/4))."""
    def emb1d(d, pos):
        omega = torch.arange(d // 2, dtype=torch.double) / (d / 2.0)
        omega = 1.0 / 10000 ** omega
        out = torch.einsum("m,d->md", pos.reshape(-1).double(), omega)
        return torch.cat([torch.sin(out), torch.cos(out)], dim=1)
    gw, gh = torch.meshgrid(torch.arange(w, dtype=torch.float), torch.arange(h, dtype=torch.float), indexing="xy")
    emb = torch.cat([emb1d(dim // 2, gw), emb1d(dim // 2, gh)], dim=1).float()  # (h*w, dim): grid[0] = x index
    return emb.reshape(1, h, w, dim).permute(0, 3, 1, 2).contiguous()


class _Affine128(nn.Module):  # nn.GroupNorm(1, 128) parameters (cotracker.py:79)
    def __init__(self, dim=128):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))


# ------------------------------------------------------------------------------------------
# device-side packed weights (ctk_former_weights of include/ctk.h)
# ------------------------------------------------------------------------------------------
class PackedWeightsV2:
    def __init__(self, model: "CoTracker2", device, precision: str = "f16x3"):
        if precision not in ("f16x3", "f32"):
            raise ValueError("precision must be 'f16x3' (split-half MFMA, default) or 'f32' (exact-f32 MFMA)")
        self.precision, self.device = precision, device
        split = precision == "f16x3"
        sd = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in model.state_dict().items()}
        self.keep = []

        def hold(t):
            t = t.contiguous()
            self.keep.append(t)
            return t.data_ptr()

        def pack(t):
            if not split:
                return None
            blob = ops.pack_weight(t.contiguous())
            self.keep.append(blob)
            return blob.data_ptr()

        u = "updateformer."
        fw = L.FormerWeights()
        fw.depth, fw.in_dim, fw.in_ld, fw.out_dim, fw.out_ld = DEPTH_V2, model.input_dim, IN_LD, model.latent_dim + 2, OUT_LD
        in_w = torch.zeros(384, IN_LD, device=device)
        in_w[:, : model.input_dim] = sd[u + "input_transform.weight"]
        fw.in_w, fw.in_p = hold(in_w), pack(in_w)
        fw.in_b = hold(sd[u + "input_transform.bias"])
        # time embedding folded into per-frame bias rows: W (x + e_t) + b = W x + (W e_t + b)   (cotracker.py:150,484)
        te = sd["time_emb"][0].double()
        bias_t = (te @ sd[u + "input_transform.weight"].double().t() + sd[u + "input_transform.bias"].double()).float()
        fw.in_bias_t = hold(bias_t)
        fw.virtual_tokens = hold(sd[u + "virual_tracks"].reshape(64, 384))
        head_w = torch.zeros(OUT_LD, 384, device=device)
        head_w[: model.latent_dim + 2] = sd[u + "flow_head.weight"]
        head_b = torch.zeros(OUT_LD, device=device)
        head_b[: model.latent_dim + 2] = sd[u + "flow_head.bias"]
        # flow_head (384 -> 128 feature delta + 2 coordinates) always runs on the exact-f32 MFMA kernel (head_p = null): its output
        # re-enters the track features six times per window, and with split-half products this ONE Linear took the visibility logit
        # of the BASELINE-scale run from 5.1e-5 to 1.04e-4 against the reference (bar 1e-4; round-6 bisect, profiles/
        # r06_v2_flow_head_bisect.txt: track_feat_updater in f32 changes nothing).  It is 0.3 % of the update's flops.
        fw.head_w, fw.head_p, fw.head_b = hold(head_w), None, hold(head_b)

        def block(prefix, attn_name, cross):
            b = L.BlockWeights()
            a = f"{prefix}{attn_name}."
            b.wq, b.bq = hold(sd[a + "to_q.weight"]), hold(sd[a + "to_q.bias"])
            b.wkv, b.bkv = hold(sd[a + "to_kv.weight"]), hold(sd[a + "to_kv.bias"])
            b.wo, b.bo = hold(sd[a + "to_out.weight"]), hold(sd[a + "to_out.bias"])
            b.w1, b.b1 = hold(sd[prefix + "mlp.fc1.weight"]), hold(sd[prefix + "mlp.fc1.bias"])
            b.w2, b.b2 = hold(sd[prefix + "mlp.fc2.weight"]), hold(sd[prefix + "mlp.fc2.bias"])
            b.wq_p, b.wkv_p, b.wo_p = pack(sd[a + "to_q.weight"]), pack(sd[a + "to_kv.weight"]), pack(sd[a + "to_out.weight"])
            b.w1_p, b.w2_p = pack(sd[prefix + "mlp.fc1.weight"]), pack(sd[prefix + "mlp.fc2.weight"])
            if cross:
                b.ctx_gamma, b.ctx_beta = hold(sd[prefix + "norm_context.weight"]), hold(sd[prefix + "norm_context.bias"])
            return b

        Arr = L.BlockWeights * DEPTH_V2
        self.arrays = [Arr(*[block(f"{u}{name}.{i}.", attn, cross) for i in range(DEPTH_V2)])
                       for name, attn, cross in (("time_blocks", "attn", False), ("space_virtual2point_blocks", "cross_attn", True),
                                                 ("space_virtual_blocks", "attn", False), ("space_point2virtual_blocks", "cross_attn", True))]
        fw.time_blocks, fw.virtual2point, fw.virtual_self, fw.point2virtual = self.arrays
        self.former = fw
        self.split = split
        self.pos_hwc = sd["pos_emb"][0].permute(1, 2, 0).contiguous()  # [H/4, W/4, 456]
        self.norm_w, self.norm_b = sd["norm.weight"].contiguous(), sd["norm.bias"].contiguous()
        self.upd_w, self.upd_b = sd["track_feat_updater.0.weight"].contiguous(), sd["track_feat_updater.0.bias"].contiguous()
        self.upd_p = ops.pack_weight(self.upd_w) if split else None
        self.vis_w, self.vis_b = sd["vis_predictor.0.weight"].reshape(128).contiguous(), sd["vis_predictor.0.bias"].contiguous()
        st = L.V2Weights()  # ctk_v2_weights of the one-call window driver (ctk_forward_window_v2)
        st.former = fw
        st.pos_hwc, st.pos_h, st.pos_w = self.pos_hwc.data_ptr(), self.pos_hwc.shape[0], self.pos_hwc.shape[1]
        st.norm_w, st.norm_b = self.norm_w.data_ptr(), self.norm_b.data_ptr()
        st.upd_w, st.upd_b = self.upd_w.data_ptr(), self.upd_b.data_ptr()
        st.upd_p = self.upd_p.data_ptr() if self.upd_p is not None else None
        st.vis_w, st.vis_b = self.vis_w.data_ptr(), self.vis_b.data_ptr()
        self.struct = st


class CoTracker2(TrackerBase):
    """Constructor mirrors cotracker.py:30-84.  The attributes that are not reference kwargs (precision, hip_graph, the f16 range
    guard, ...) are TrackerBase's; the HIP encoder runs without the final L2 normalisation CoTracker3 applies."""

    PACKED_WEIGHTS = PackedWeightsV2
    online_ind = _online_attr("ind")
    online_track_feat = _online_attr("track_feat")
    online_coords_predicted = _online_attr("coords_predicted")
    online_vis_predicted = _online_attr("vis_predicted")

    def __init__(self, window_len=8, stride=4, add_space_attn=True, num_virtual_tracks=64, model_resolution=(384, 512)):
        super().__init__()
        if num_virtual_tracks != 64 or not add_space_attn:
            raise NotImplementedError("HIP path is specialised to 64 virtual tracks with space attention on")
        self.window_len = window_len
        self.stride = stride
        self.hidden_dim = 256
        self.latent_dim = 128
        self.add_space_attn = add_space_attn
        self.num_virtual_tracks = num_virtual_tracks
        self.model_resolution = model_resolution
        self.input_dim = 456
        self.fnet = BasicEncoder(input_dim=3, output_dim=self.latent_dim, stride=stride)
        self.updateformer = _UpdateFormerParams(self.input_dim, 384, 6, num_virtual_tracks,
                                                flow_out=self.latent_dim + 2, vis_conf_head=False)
        self.register_buffer("time_emb", sincos_time_embed(self.input_dim, window_len))
        self.register_buffer("pos_emb", sincos_pos_embed_2d(self.input_dim, model_resolution[0] // stride,
                                                           model_resolution[1] // stride))
        self.norm = _Affine128(self.latent_dim)
        self.track_feat_updater = nn.Sequential(_Lin(self.latent_dim, self.latent_dim))  # + nn.GELU() (no parameters)
        self.vis_predictor = nn.Sequential(_Lin(self.latent_dim, 1))

    @TrackerBase.batch_mode.setter
    def batch_mode(self, mode):  # B > 1 is a loop over the videos; the joint batch mode of the CoTracker3 models is not available here
        if mode == "joint":
            raise NotImplementedError("CoTracker2 (model_v2.py) stays on the loop; batch_mode=\"joint\" on a v2 model is not implemented")
        if mode != "loop":
            raise ValueError(f"batch_mode must be 'loop' or 'joint', got {mode!r}")

    @TrackerBase.stream_groups.setter
    def stream_groups(self, on):  # streaming takes one query set per video here: the device stream state is the CoTracker3 online model's
        if on:
            raise NotImplementedError("CoTracker2 (model_v2.py) streams one query set per video; stream_groups on a v2 model is not implemented")

    @TrackerBase.stream_slots.setter
    def stream_slots(self, on):  # slots live in the device stream state, which is the CoTracker3 online model's
        if on:
            raise NotImplementedError("CoTracker2 (model_v2.py) takes the queries of a stream at its first call; stream_slots on a v2 model is not implemented")

    @TrackerBase.stream_history_frames.setter
    def stream_history_frames(self, K):  # the ring history lives in the device stream state, which is the CoTracker3 online model's
        if K is not None:
            raise NotImplementedError("CoTracker2 (model_v2.py) returns the tracks of the whole stream; stream_history_frames on a v2 model is not implemented")

    def stream_assign(self, *args, **kwargs):  # slots and the resident pyramid belong to the CoTracker3 online model's stream state
        raise NotImplementedError("CoTracker2 (model_v2.py) takes the queries of a stream at its first call; stream_assign on a v2 model is not implemented")

    def stream_health(self, *args, **kwargs):  # the history it judges is the CoTracker3 online model's device stream state
        raise NotImplementedError("CoTracker2 (model_v2.py) keeps no stream state on the device; stream_health on a v2 model is not implemented")

    def stream_draw(self, *args, **kwargs):  # the history it draws is the CoTracker3 online model's device stream state
        raise NotImplementedError("CoTracker2 (model_v2.py) keeps no stream state on the device; stream_draw on a v2 model is not implemented")

    def stream_motion(self, *args, **kwargs):  # the history it fits is the CoTracker3 online model's device stream state
        raise NotImplementedError("CoTracker2 (model_v2.py) keeps no stream state on the device; stream_motion on a v2 model is not implemented")

    def stream_stabilize(self, *args, **kwargs):  # the history it steadies by is the CoTracker3 online model's device stream state
        raise NotImplementedError("CoTracker2 (model_v2.py) keeps no stream state on the device; stream_stabilize on a v2 model is not implemented")

    def stream_field(self, *args, **kwargs):  # the history it interpolates is the CoTracker3 online model's device stream state
        raise NotImplementedError("CoTracker2 (model_v2.py) keeps no stream state on the device; stream_field on a v2 model is not implemented")

    def stream_objects(self, *args, **kwargs):  # the history it fits is the CoTracker3 online model's device stream state
        raise NotImplementedError("CoTracker2 (model_v2.py) keeps no stream state on the device; stream_objects on a v2 model is not implemented")

    def stream_planes(self, *args, **kwargs):  # the history it fits is the CoTracker3 online model's device stream state
        raise NotImplementedError("CoTracker2 (model_v2.py) keeps no stream state on the device; stream_planes on a v2 model is not implemented")

    def stream_epipolar(self, *args, **kwargs):  # the history it fits is the CoTracker3 online model's device stream state
        raise NotImplementedError("CoTracker2 (model_v2.py) keeps no stream state on the device; stream_epipolar on a v2 model is not implemented")

    def stream_pose(self, *args, **kwargs):  # the history it reads is the CoTracker3 online model's device stream state
        raise NotImplementedError("CoTracker2 (model_v2.py) keeps no stream state on the device; stream_pose on a v2 model is not implemented")

    def stream_focal(self, *args, **kwargs):  # the history it reads is the CoTracker3 online model's device stream state
        raise NotImplementedError("CoTracker2 (model_v2.py) keeps no stream state on the device; stream_focal on a v2 model is not implemented")

    def stream_resection(self, *args, **kwargs):  # the history it reads is the CoTracker3 online model's device stream state
        raise NotImplementedError("CoTracker2 (model_v2.py) keeps no stream state on the device; stream_resection on a v2 model is not implemented")

    def stream_p3p(self, *args, **kwargs):  # the history it reads is the CoTracker3 online model's device stream state
        raise NotImplementedError("CoTracker2 (model_v2.py) keeps no stream state on the device; stream_p3p on a v2 model is not implemented")

    def stream_align(self, *args, **kwargs):  # the slots it aligns over are the CoTracker3 online model's device stream state
        raise NotImplementedError("CoTracker2 (model_v2.py) keeps no stream state on the device; stream_align on a v2 model is not implemented")

    def stream_structure(self, *args, **kwargs):  # the history it reads is the CoTracker3 online model's device stream state
        raise NotImplementedError("CoTracker2 (model_v2.py) keeps no stream state on the device; stream_structure on a v2 model is not implemented")

    def stream_push(self, *args, **kwargs):  # the resident pyramid it advances belongs to the CoTracker3 online model's stream state
        raise NotImplementedError("CoTracker2 (model_v2.py) is fed overlapping chunks through forward(); stream_push on a v2 model is not implemented")

    def init_video_online_processing(self):  # cotracker.py:187-191
        self._resolve_deferred_range_check()  # the last chunk of the previous stream (graph streaming defers its check by one call)
        self._online = [OnlineState()]  # (B > 1: replicated by the first call)

    @torch.no_grad()
    def forward(self, video, queries, iters=4, is_train=False, is_online=False):
        """CoTracker2.forward (cotracker.py:193-384): returns (coords [B,T,N,2] px, vis [B,T,N] post-sigmoid, None).
        A query-group call (video [1,...], queries [G,N,3], G > 1; TrackerBase.__init__) encodes the video once and runs the G
        query sets one after the other on those features (this model has no joint mode): [G,T,N,.] results, bit-identical to G
        separate calls.  Sliding only."""
        self._check_call(video, is_train)
        B, T = video.shape[:2]
        G = queries.shape[0]
        assert self.window_len >= 2 and (G == B or (B == 1 and G > 1))
        if G != B:
            if is_online:
                raise NotImplementedError("streaming (is_online=True) takes one query set per video: a query-group call (video "
                                          f"[1,...], queries [{G},...]) is available in sliding mode only")
            f0 = []  # encoded once for the call (a range-guard re-run included)

            def make_gens(group):
                if not f0:
                    f0.append(self._encode(video[0]))
                return [self._video_gen(video[0], queries[g], None, f0[0]) for g in group]
            return self._track(video, iters, make_gens, units=G)
        states = self._online_states(B, T) if is_online else None
        return self._track(video, iters, lambda group: [self._video_gen(video[b], queries[b], states[b] if is_online else None)
                                                        for b in group], states)

    def forward_window(self, pyr, coords, track_feat, vis, track_mask, point_mask, iters, pw):
        """CoTracker2.forward_window (cotracker.py:86-173) for one batch element: ONE C call (ctk_forward_window_v2).
        pyr: 4 x [S,H_l,W_l,128] (NOT normalised), coords [S,N,2] feature units, track_feat [S,N,128] (already masked),
        vis [S,N], track_mask [S,N] float 0/1, point_mask [N] uint8.  Returns (coords [S,N,2] feature units, vis logits [S,N])."""
        return self._run_windows([(pyr, coords, track_feat, vis, track_mask, point_mask)], iters, pw, False)[0]

    def _window(self, req, iters):
        return ops.V2Window(*req, iters)

    def _window_graph(self, wins, pw, joint):
        return ops.V2WindowGraph(wins[0], pw)

    def _run_windows(self, reqs, iters, pw, graphed):
        """The window of one request (forward_window's arguments): one direct call, or -- streaming -- one replay of the hipGraph the
        whole window (iters x (5 + ~390) launches) was captured into; its results are handed out as clones."""
        (req,) = reqs  # (no joint batch mode: every group is one video)
        if graphed:
            return [tuple(t_.clone() for t_ in res) for res in self._graphed_windows(reqs, iters, pw)]
        pyr, coords, track_feat, vis, track_mask, point_mask = req
        win = self._window((pyr, coords.clone(), track_feat.clone(), vis.contiguous(), track_mask, point_mask), iters)
        ops.forward_window_v2(win, pw)
        return [win.result()]

    def _encode(self, frames):
        """frames [T,3,H,W] in 0..255 -> NHWC level-0 features [T,H/4,W/4,128], NOT normalised (cotracker.py:273-275)."""
        if self.encoder_backend == "hip":
            return self._hip_encode(frames, self.encoder_chunk, normalize=False)
        return self.fnet(2 * (frames.float() / 255.0) - 1.0).float().permute(0, 2, 3, 1).contiguous()

    def _video_gen(self, video, queries, st, f0=None):
        """One video's host code as a generator (see TrackerBase._track): yields forward_window's arguments per window, receives
        (coords, vis logits), returns (coords_pred, vis_pred).  st: this video's OnlineState (streaming) or None (sliding).
        f0: the video's level-0 features when the caller has encoded them already (a query-group call)."""
        is_online = st is not None
        T, N = video.shape[0], queries.shape[0]
        S, step, dev = self.window_len, self.window_len // 2, video.device
        queries = queries.float()
        qframes = queries[:, 0].long()
        qcoords = (queries[:, 1:3] / self.stride).contiguous()
        coords_pred = torch.zeros(T, N, 2, device=dev)
        vis_pred = torch.zeros(T, N, device=dev)
        if is_online and st.coords_predicted is not None:
            coords_pred, vis_pred = self._pad_history(T, step, st.coords_predicted, st.vis_predicted)
        # encoder; padding the video with its last frame (:264-270) == repeating the last feature map (fnet is per-frame)
        pad = (S - T) if is_online else (S - T % S) % S
        if f0 is None:
            f0 = self._encode(video)  # NHWC, not normalised
        if pad > 0:
            f0 = torch.cat([f0, f0[-1:].expand(pad, -1, -1, -1)], dim=0).contiguous()
        pyr = ops.build_pyramid(f0, 4)  # CorrBlock pyramid (blocks.py:300-307) for every frame at once
        # get_track_feat (:175-185): trilinear sample at (t, x, y) = the centre tap of the support sampler
        frames_rel = (qframes - st.ind if is_online else qframes).float().contiguous()
        tf0 = ops.sample_support(f0, frames_rel, qcoords)[:, 24].contiguous()  # [N,128]
        track_feat = tf0[None].expand(S, N, 128)
        if is_online:  # :286-295
            left = 0 if st.ind == 0 else st.ind + step
            right = st.ind + S
            smask = ((qframes >= left) & (qframes < right)).float()[None, :, None]
            acc = torch.zeros(S, N, 128, device=dev) if st.track_feat is None else st.track_feat
            st.track_feat = track_feat = acc + track_feat * smask
        num_windows = (T - S + step - 1) // step + 1
        indices = [st.ind] if is_online else range(0, step * num_windows, step)
        coords_init = qcoords[None].expand(S, N, 2).contiguous()
        vis_init = torch.full((S, N), 10.0, device=dev)
        for ind in indices:
            overlap = S - step
            if ind > 0:
                coords_init, vis_init = self._carry_over(qframes, ind, S, step, (coords_pred, vis_pred), (coords_init, vis_init))
            amask = qframes < ind + S                                                        # attention_mask, :331-333
            tmask = qframes[None, :] <= torch.arange(ind, ind + S, device=dev)[:, None]      # track_mask, :338-344
            if ind > 0:
                tmask = tmask.clone()
                tmask[:overlap] = False
            win_pyr = pyr if is_online else [p_[ind:ind + S] for p_ in pyr]
            coords, vis = yield (win_pyr, coords_init, (track_feat * amask.float()[None, :, None]).contiguous(), vis_init,
                                 tmask.float().contiguous(), amask.to(torch.uint8).contiguous())
            S_trim = T if is_online else min(T - ind, S)
            coords_pred[ind:ind + S] = (coords * float(self.stride))[:S_trim]
            vis_pred[ind:ind + S] = vis[:S_trim]
        if is_online:
            st.ind += step
            st.coords_predicted, st.vis_predicted = coords_pred, vis_pred
        return coords_pred, vis_pred  # (visibility LOGITS: the shared tail applies the sigmoid, cotracker.py:373)
