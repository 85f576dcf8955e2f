"""HomoModelBuilder / track_proj: the deep-homography head wired onto the HIP kernels.

    HomoModelBuilder.forward(data) -> dict   <- .../Oneline_DLTv1/models/homo_model_builder.py:115-217
    track_proj(model, data, tmp_mask)        <- hdn/models/model_builder_e2e_unconstrained_v2.py:161-217

Per pair the HIP path is: PreShareFeature(template), PreShareFeature(search) -> [PyTorch-ROCm ResNet-34
+ avgpool + fc -> 8 corner offsets] -> fused DLT + projective warp -> PreShareFeature(warped) -> L1 scores.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import homography as G
from .share_feature import PreShareFeature
from .trunk import ACT_SCALE_LOG2, resnet34_homo, resnet50_homo


def avgpool_fc(x, fc, in_domain=0):
    """fc(avgpool(x).flatten(1)) as one launch (hdn_avgpool_fc_f32); x [B,C,H,W] float32, NCHW-contiguous or channels-last; in_domain = 1: x is the
    trunk's scaled-domain output (x_real * 2^-8): the pooled means are multiplied by 2^8 (exact) before the fully connected layer."""
    from . import _lib

    dev = _lib.require_device(x, fc.weight)
    B, C, H, W = x.shape
    nhwc = 0 if x.is_contiguous() else 1
    if nhwc and not x.is_contiguous(memory_format=torch.channels_last):
        x, nhwc = x.contiguous(), 0
    w = fc.weight.detach().contiguous()
    out = torch.empty((B, w.shape[0]), dtype=torch.float32, device=dev)
    _lib.launch("avgpool_fc", dev, _lib.load().hdn_avgpool_fc_f32, _lib.ptr(x), _lib.ptr(w), _lib.opt(fc.bias), _lib.ptr(out),
                B, C, H * W, w.shape[0], nhwc, int(in_domain))
    return out


def _regress(net, feats):
    fast = getattr(net, "_hdn_fast_trunk", None)
    if fast is not None and not net.training:
        inp = feats.contiguous(memory_format=torch.channels_last) if getattr(net, "_hdn_fast_nhwc", False) else feats
        # the tail of the optimised trunk: AdaptiveAvgPool2d(1) + Linear(512, 8) in one launch — which also takes the trunk's output straight from its
        # scaled activation domain (hdn_amd.trunk.ACT_SCALE_LOG2) when the folded copy runs in it
        tail = (feats.is_cuda and feats.dtype == torch.float32 and isinstance(net.avgpool, nn.AdaptiveAvgPool2d) and net.avgpool.output_size in (1, (1, 1))
                and isinstance(net.fc, nn.Linear) and net.fc.out_features <= 16 and net.fc.weight.dtype == torch.float32)
        dom = int(getattr(fast, "act_domain", 0))
        if tail and dom and hasattr(fast, "forward_scaled"):
            return avgpool_fc(fast.forward_scaled(inp).detach(), net.fc, in_domain=1)
        x = fast(inp)
        if tail:
            return avgpool_fc(x.detach(), net.fc, in_domain=dom)     # (dom: a folded trunk without forward_scaled, e.g. the reference's ResNet)
        if dom and not hasattr(fast, "forward_scaled"):
            x = x * float(1 << ACT_SCALE_LOG2)
    else:
        x = net.backbone(feats)
    x = net.avgpool(x)
    x = x.view(x.size(0), -1)
    return net.fc(x)


_TRUNK_HOOK, _TRUNK_ARGS = "_hdn_trunk_reload_hook", "_hdn_trunk_fold_args"


def _refold_trunk(net, incompatible_keys=None):
    """load_state_dict post-hook of optimize_trunk: the folded trunk is rebuilt from the module's new weights and copied INTO the tensors of the
    attached copy (same storage: a captured hipGraph keeps pointing at them); a copy whose tensors no longer match is replaced instead."""
    from .trunk import fold_for_inference

    args, old = net.__dict__.get(_TRUNK_ARGS), net.__dict__.get("_hdn_fast_trunk")
    if args is None or old is None:
        return
    with torch.no_grad():
        fresh = fold_for_inference(net.backbone, *args)
        dst = dict(list(old.named_parameters()) + list(old.named_buffers()))
        src = dict(list(fresh.named_parameters()) + list(fresh.named_buffers()))
        if dst.keys() == src.keys() and all(dst[k].shape == v.shape and dst[k].dtype == v.dtype for k, v in src.items()):
            for k, v in src.items():
                dst[k].copy_(v)
        else:
            object.__setattr__(net, "_hdn_fast_trunk", fresh)


def optimize_trunk(net, enable: bool = True, channels_last: bool = False, fused_stem: bool = None, fused_epilogue: bool = None):
    """Attach the BN-folded trunk to any module with a `.backbone` (also the reference's HomoModelBuilder).

    Measured at B=64 on MI355X (tools/experiments/exp_trunk.py, fresh process each): as-is 2.92 ms, folded 2.47 ms; with
    torch.backends.cudnn.benchmark = True (MIOpen find mode, set before the first forward): 2.76 / 2.28 ms, and
    folded + channels_last 2.06 ms.  Without find mode channels_last does not pay (2.96 ms), hence the default.

    The folded copy is a snapshot, so a load_state_dict post-hook is registered on `net` (once; enable=False removes it): after
    `net.load_state_dict(...)`, or a load_state_dict of a module that contains `net`, the trunk is folded again and written into the attached
    copy's own tensors, so the next forward sees the new weights and a hipGraph captured before the reload stays valid.  Only when the new fold
    has other tensors (another architecture under the same attribute) is the copy replaced; a graph captured before that must be captured again.
    Weights edited in place (`.data`) are not seen: call optimize_trunk again."""
    from .trunk import fold_for_inference, trunk_block_kinds

    if enable:
        trunk_block_kinds(net.backbone)        # BasicBlock / Bottleneck layouts only: ValueError for anything else
    on_gpu = next(net.backbone.parameters()).is_cuda
    if fused_stem is None:  # the fused first stage / block epilogues need the HIP library and weights on a GPU
        fused_stem = on_gpu
    if fused_epilogue is None:
        fused_epilogue = on_gpu
    object.__setattr__(net, "_hdn_fast_trunk", fold_for_inference(net.backbone, channels_last, fused_stem, fused_epilogue) if enable else None)
    # the fused stem reads NCHW and writes the layout the rest of the trunk runs in: no input conversion then
    object.__setattr__(net, "_hdn_fast_nhwc", bool(enable and channels_last and not fused_stem))
    hook = net.__dict__.get(_TRUNK_HOOK)
    if enable:
        object.__setattr__(net, _TRUNK_ARGS, (channels_last, fused_stem, fused_epilogue))
        if hook is None:
            object.__setattr__(net, _TRUNK_HOOK, net.register_load_state_dict_post_hook(_refold_trunk))
    else:
        if hook is not None:
            hook.remove()
        net.__dict__.pop(_TRUNK_HOOK, None)
        net.__dict__.pop(_TRUNK_ARGS, None)


def _share(net, x):
    return net.ShareFeature(x)


def _check_data(data):
    for k in ("org_imgs", "input_tensors", "h4p", "patch_indices"):
        if k not in data:
            raise KeyError(f"data['{k}'] missing (homo_model_builder.py:116-119)")
    org, inp = data["org_imgs"], data["input_tensors"]
    if org.dim() != 4 or org.shape[1] != 2 or inp.shape != org.shape:
        raise ValueError(f"org_imgs / input_tensors must both be [B,2,H,W] full patches, got {tuple(org.shape)} / {tuple(inp.shape)}")
    B, _, H, W = org.shape
    if tuple(data["patch_indices"].shape) != (B, H * W):
        raise ValueError("patch_indices must be the [B, H*W] full-patch index (get_img_info.py:88-92)")
    return B, H, W


def homo_stages(net, data, cached_patch_1=None):
    """ShareFeature x2 -> trunk -> fused DLT+warp -> ShareFeature.  Returns the intermediates.

    `cached_patch_1`: ShareFeature(template) is constant for a whole sequence; pass it to skip
    one of the three ShareFeature launches.
    """
    B, H, W = _check_data(data)
    org, inp, h4p = data["org_imgs"], data["input_tensors"], data["h4p"]
    with torch.no_grad():
        if cached_patch_1 is None:
            # one launch for both channels: [B,2,H,W] viewed as 2B single-channel images
            both = _share(net, inp.reshape(B * 2, 1, H, W)).reshape(B, 2, H, W)
            p1, p2 = both[:, :1], both[:, 1:]
            feats = both
        else:
            p1 = cached_patch_1
            p2 = _share(net, inp[:, 1:].contiguous())
            feats = torch.cat((p1, p2), dim=1)
        x = _regress(net, feats)
        H_mat, pred = G.dlt_warp(h4p, x, org[:, :1])
        pf = _share(net, pred)
    return {"x": x, "H_mat": H_mat, "pred_I2": pred, "patch_1": p1, "patch_2": p2, "pred_feat": pf}


def track_proj(net, data, tmp_mask=None, cached_patch_1=None):
    """(H_mat [B,3,3], similarity_norm, similarity_norm_simi) as ModelBuilder.track_proj returns them.

    `net` is the HomoModelBuilder (the reference passes self.hm_net's sub-modules); tmp_mask is accepted and
    unused, as in the reference.
    """
    st = homo_stages(net, data, cached_patch_1)
    # model_builder…:213-216 — sample 0 / channel 0 only, divided by the literal 127*127
    inv = 1.0 / (127 * 127)
    score, score_simi = G.l1_score2(st["patch_2"][0, 0], st["pred_feat"][0, 0], st["patch_1"][0, 0], inv)
    return st["H_mat"], score, score_simi


def track_proj_pair(net, template, search, h4p, patch_1, per_sample: bool = False):
    """track_proj for the tracker's per-frame call, where the two crops are separate tensors and ShareFeature(template) is cached
    (SURVEY §3d): the same stages as homo_stages(..., cached_patch_1) without building the [B,2,H,W] pair first (one concatenation
    and one strided copy per call less - launches that are pure latency at B = 1).
    template / search: [B,1,H,W] contiguous fp32; patch_1 = ShareFeature(template).
    per_sample: the two scores of EVERY sample ([B] each) instead of sample 0's (the reference's `[0][0]`): B independent sequences."""
    if template.shape != search.shape or template.dim() != 4 or template.shape[1] != 1:
        raise ValueError(f"template / search must both be [B,1,H,W], got {tuple(template.shape)} / {tuple(search.shape)}")
    with torch.no_grad():
        p2 = _share(net, search.contiguous())
        x = _regress(net, torch.cat((patch_1, p2), dim=1))
        H_mat, pred = G.dlt_warp(h4p, x, template.contiguous())
        pf = _share(net, pred)
    if per_sample:
        score, score_simi = G.l1_score2_batch(p2, pf, patch_1, 1.0 / (127 * 127))
    else:
        score, score_simi = G.l1_score2(p2[0, 0], pf[0, 0], patch_1[0, 0], 1.0 / (127 * 127))
    return H_mat, score, score_simi


class HomoModelBuilder(nn.Module):
    """Same sub-module names as the reference (ShareFeature, backbone, avgpool, fc) so snapshots load."""

    def __init__(self, pretrained: bool = False, backbone: str = "resnet34"):
        super().__init__()
        # `pretrained` fetched ImageNet weights over the network in the reference (backbone/__init__.py:39-49);
        # there is no network here, weights come from the tracker snapshot (hdn/utils/model_load.py).
        # `backbone`: cfg.BACKBONE_HOMO.TYPE of the reference (homo_model_builder.py:97-112), the two trunks it can build with a head
        if backbone not in ("resnet34", "resnet50"):
            raise ValueError(f"backbone must be 'resnet34' or 'resnet50', got {backbone!r}")
        self.ShareFeature = PreShareFeature()
        self.backbone = resnet34_homo() if backbone == "resnet34" else resnet50_homo()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(512 if backbone == "resnet34" else 2048, 8)

    def track_proj(self, data, tmp_mask=None, cached_patch_1=None):
        return track_proj(self, data, tmp_mask, cached_patch_1)

    def optimize_for_inference(self, enable: bool = True, channels_last: bool = False, fused_stem: bool = None, fused_epilogue: bool = None):
        """Build (or drop) the BN-folded copy of the trunk used by eval-mode forwards (§8f rank 4).
        Call it after the weights are loaded and the module is on its device; call again if they change."""
        optimize_trunk(self, enable, channels_last, fused_stem, fused_epilogue)
        return self

    def forward(self, data):
        """Inference-mode forward with the reference's output keys (homo_model_builder.py:212-215).

        if_pos / if_unsup default to ones as in the reference (:125-132; the 'search_windowx' typo at :122 means the window is
        always ones there too).  With per-sample flags (the training set's, unconstrained_v2_dataset.py:310-312) the
        negative-sample branch (:172-205) runs: the triplet term over the samples with if_pos * if_unsup == 1 only, normalised
        by their count, and homo_neg_loss = mean L2 norm of the predicted offsets of the if_pos == 0 samples.  Losses are
        computed without autograd (this package is the inference path).
        """
        st = homo_stages(self, data)
        p1, p2, pf, pred, x = st["patch_1"], st["patch_2"], st["pred_feat"], st["pred_I2"], st["x"]
        B = x.shape[0]
        homo_neg_loss = torch.zeros((), device=x.device)
        with torch.no_grad():
            n_pos = B * p1.shape[2] * p1.shape[3]          # default flags [B,1,127,127] of ones: nonzero() has one row per pixel
            if "if_pos" in data or "if_unsup" in data:
                ones = torch.ones((B, 1, 127, 127), dtype=torch.float32, device=x.device)
                if_pos, if_unsup = data.get("if_pos", ones).to(x.device), data.get("if_unsup", ones).to(x.device)
                neg_ids = if_pos.eq(0).nonzero().squeeze(1)
                pos_ids = (if_pos * if_unsup).eq(1).nonzero().squeeze(1)
                n_pos = pos_ids.shape[0]
                if neg_ids.shape[0] != 0:
                    p1, p2, pf = p1[pos_ids], p2[pos_ids], pf[pos_ids]
                    homo_neg_loss = torch.sum(torch.norm(x[neg_ids, :], p=2, dim=1)) / neg_ids.shape[0]
            # TripletMarginLoss(margin=1, p=1, reduce=False): pairwise L1 over the last dim, eps 1e-6
            d_ap = ((p2 - pf) + 1e-6).abs().sum(-1)
            d_an = ((p2 - p1) + 1e-6).abs().sum(-1)
            loss_mat = (d_ap - d_an + 1.0).clamp_min(0.0)
            feature_loss = (loss_mat.sum() / n_pos / (127 * 127)).reshape(1)
        p2 = st["patch_2"]
        pf = st["pred_feat"]
        return {
            "feature_loss": feature_loss,
            "pred_I2_d": pred[:1],
            "x": x,
            "H_mat": st["H_mat"],
            "patch_2_res_d": p2[:1],
            "pred_I2_CnnFeature_d": pf[:1],
            "homo_neg_loss": homo_neg_loss,
        }

    def _host_free_constants(self, B, H, W, dev):
        """(M_tile, M_tile_inv, batch_inds) of training_forward(host_free=True) as device buffers, built once per (B, H, W, device) - outside any
        capture, since building them uploads.  The inverse of the literal of :139-142 is written down: [[1/63.5, 0, -1], [0, 1/63.5, -1], [0, 0, 1]]."""
        cache = self.__dict__.setdefault("_hdn_host_free_constants", {})
        key = (B, H, W, str(dev))
        if key not in cache:
            if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"HomoModelBuilder.training_forward(host_free=True): the constants of (B, H, W) = {(B, H, W)} are not on {dev} "
                                   "yet and building them uploads; run one forward outside the capture first (the warm-up does)")
            M = torch.tensor([[63.5, 0.0, 63.5], [0.0, 63.5, 63.5], [0.0, 0.0, 1.0]], device=dev)
            M_inv = torch.tensor([[1.0 / 63.5, 0.0, -1.0], [0.0, 1.0 / 63.5, -1.0], [0.0, 0.0, 1.0]], device=dev)
            batch_inds = torch.arange(0, B * H * W, H * W, device=dev).unsqueeze(1).expand(B, H * W).reshape(-1)
            cache[key] = (M.unsqueeze(0).expand(B, 3, 3).contiguous(), M_inv.unsqueeze(0).expand(B, 3, 3).contiguous(), batch_inds)
        return cache[key]

    def _training_forward_host_free(self, data):
        """training_forward(host_free=True): see there."""
        from . import _lib
        from .triplet import triplet_l1_mean

        sf = self.ShareFeature
        B, H, W = _check_data(data)
        for k in ("if_pos", "if_unsup"):
            if k not in data:
                raise KeyError(f"data['{k}'] missing: host_free=True decides the sample sets on the device and needs both flags as [B] float")
            if tuple(data[k].shape) != (B,):
                raise ValueError(f"data['{k}'] must be [{B}] (one flag per sample), got {list(data[k].shape)}")
        org, inp, h4p, patch_inds = data["org_imgs"], data["input_tensors"], data["h4p"], data["patch_indices"]
        if_pos, if_unsup = data["if_pos"], data["if_unsup"]
        dev = _lib.require_device(inp, if_pos, if_unsup)        # a flag on the host would be an upload
        p1 = sf(inp[:, :1].contiguous())
        p2 = sf(inp[:, 1:].contiguous())
        x = self.backbone(torch.cat((p1, p2), dim=1))
        x = self.fc(self.avgpool(x).view(x.size(0), -1))
        H_mat = G.DLT_solve(h4p, x).squeeze(1)
        M_tile, M_tile_inv, batch_inds = self._host_free_constants(B, H, W, dev)
        pred = G.transform(H, W, M_tile_inv, H_mat, M_tile, org[:, :1], patch_inds, batch_inds)
        pf = sf(pred)
        value, counts = triplet_l1_mean(p2, pf, p1, if_pos, if_unsup, rule=1, denom=127 * 127, margin=1.0, eps=1e-6)
        # homo_neg_loss (:176-178) without x[neg_ids]: the other samples' offsets are replaced (not multiplied) by 0 before the norm, whose
        # gradient at 0 is 0, so a NaN in them reaches nothing; gated on n_neg, where the reference tests neg_ids.shape[0]
        n_neg = counts[1]
        x_neg = torch.where(if_pos.eq(0).unsqueeze(1), x, torch.zeros_like(x))
        neg_sum = torch.sum(torch.norm(x_neg, p=2, dim=1))
        homo_neg_loss = torch.where(n_neg > 0, neg_sum / n_neg.clamp(min=1).to(torch.float32), torch.zeros_like(neg_sum))
        return {
            "feature_loss": value.unsqueeze(0),
            "pred_I2_d": pred[:1],
            "x": x,
            "H_mat": H_mat,
            "patch_2_res_d": p2[:1],
            "pred_I2_CnnFeature_d": pf[:1],
            "homo_neg_loss": homo_neg_loss,
        }

    def training_forward(self, data, host_free: bool = False):
        """The reference's training forward (homo_model_builder.py:154-215) on the differentiable HIP operators; the returned dict has forward()'s
        keys and every loss carries the graph to the regressor and to ShareFeature.

        host_free=True: the same forward with nothing read by or uploaded from the host, so that it can be captured in a graph.  data['if_pos']
        and data['if_unsup'] are required, float [B] on the device.  feature_loss is hdn_amd.triplet_l1_mean(patch_2, pred_feat, patch_1, if_pos,
        if_unsup, rule=1) (the sets and the divisor are decided in the kernel; 0 with no selected sample, where the reference divides by zero),
        homo_neg_loss a masked expression on x [B,8] gated with torch.where on the kernel's n_neg, and M, its inverse (written down, no
        torch.inverse and its error check) and batch_inds are device buffers built once per (B, H, W, device), outside any capture.

        In the reference's order: ShareFeature on each of the two channels (two calls, as :154-155: in train() mode each normalises with its own
        batch statistics and updates the running buffers), the module's own backbone / avgpool / fc (never the folded inference trunk),
        hdn_amd.DLT_solve and hdn_amd.transform (M = [[63.5, 0, 63.5], [0, 63.5, 63.5], [0, 0, 1]], the literal of :139-142), ShareFeature(pred_I2).
        The flags are handled as forward() handles them.  The triplet term is one triplet_l1(patch_2, pred_feat, patch_1, ids=pos_ids,
        differentiable=True): the x[pos_ids] copies of :185-187 are not made, and the gradients come back full size with zero rows for the
        samples left out.  feature_loss = sum / n_pos / (127 * 127).

        Raises when ShareFeature would detach (eval() mode with hip_train False: the fused inference kernel), rather than return a loss that is
        cut off from the regressor."""
        from .triplet import triplet_l1

        sf = self.ShareFeature
        if not sf.training and not getattr(sf, "hip_train", False):
            raise RuntimeError("HomoModelBuilder.training_forward: ShareFeature is in eval() mode with hip_train False, where it runs the fused "
                               "inference kernel and detaches; call .train(), or set ShareFeature.hip_train = True to keep the running statistics "
                               "and the graph")
        if host_free:
            return self._training_forward_host_free(data)
        B, H, W = _check_data(data)
        org, inp, h4p, patch_inds = data["org_imgs"], data["input_tensors"], data["h4p"], data["patch_indices"]
        dev = inp.device
        p1 = sf(inp[:, :1].contiguous())
        p2 = sf(inp[:, 1:].contiguous())
        x = self.backbone(torch.cat((p1, p2), dim=1))
        x = self.fc(self.avgpool(x).view(x.size(0), -1))
        H_mat = G.DLT_solve(h4p, x).squeeze(1)
        M = torch.tensor([[63.5, 0.0, 63.5], [0.0, 63.5, 63.5], [0.0, 0.0, 1.0]], device=dev)
        M_tile, M_tile_inv = M.unsqueeze(0).expand(B, 3, 3), torch.inverse(M).unsqueeze(0).expand(B, 3, 3)
        batch_inds = torch.arange(0, B * H * W, H * W, device=dev).unsqueeze(1).expand(B, H * W).reshape(-1)
        pred = G.transform(H, W, M_tile_inv, H_mat, M_tile, org[:, :1], patch_inds, batch_inds)
        pf = sf(pred)
        homo_neg_loss = torch.zeros((), device=dev)
        n_pos, ids = B * H * W, None                          # default flags [B,1,127,127] of ones: nonzero() has one row per pixel
        if "if_pos" in data or "if_unsup" in data:
            ones = torch.ones((B, 1, 127, 127), dtype=torch.float32, device=dev)
            if_pos, if_unsup = data.get("if_pos", ones).to(dev), data.get("if_unsup", ones).to(dev)
            neg_ids = if_pos.eq(0).nonzero().squeeze(1)
            pos_ids = (if_pos * if_unsup).eq(1).nonzero().squeeze(1)
            n_pos = pos_ids.shape[0]
            if neg_ids.shape[0] != 0:
                ids = pos_ids
                homo_neg_loss = torch.sum(torch.norm(x[neg_ids, :], p=2, dim=1)) / neg_ids.shape[0]
        loss_mat = triplet_l1(p2, pf, p1, margin=1.0, eps=1e-6, ids=ids, differentiable=True)
        feature_loss = (torch.sum(loss_mat) / n_pos / (127 * 127)).unsqueeze(0)
        return {
            "feature_loss": feature_loss,
            "pred_I2_d": pred[:1],
            "x": x,
            "H_mat": H_mat,
            "patch_2_res_d": p2[:1],
            "pred_I2_CnnFeature_d": pf[:1],
            "homo_neg_loss": homo_neg_loss,
        }
