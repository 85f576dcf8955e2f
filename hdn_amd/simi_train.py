"""The similarity model's training forward composed from the package's operators, with nothing read by or uploaded from the host.

    simi_training_forward(model, data, cfg=SimiTrainConfig())   <- hdn/models/model_builder_e2e_unconstrained_v2.py:361-563 (ModelBuilder.forward)

The reference's forward (what tools/train.py trains) reads six nonzero() / len() results on the host, uploads a dozen constants per call and calls
torch.inverse, so the step cannot be captured in a graph.  Here the same statements, in the reference's order, are: the model's own networks,
polar_pick (:377), the model's log-polar sampler and heads (:379-388), similarity_warps (:390-415), affine_sample for the two warps of search_hm
(:407-408), the channel means of get_simi_data / get_homo_data with their constants h4p and patch_indices cached on the device, three ShareFeature
calls (:421-427), triplet_l1_mean(rule=0) for sim_loss (:430-440), hm_net.training_forward(homo_data, host_free=True) (:450-455),
supervised_losses (:457-478), corner_losses (:441-444, :481-523) and training_outputs (:526-562).  The sample sets are decided in the kernels from
if_pos and if_unsup; torch.where on the kernels' counts stands where the reference tests a length.

Not computed: the third stn_with_theta of :418 (the warped search_window).  Its result is read by nobody: get_homo_data passes it on as
data['search_window'], and homo_model_builder.py:122 tests the key 'search_windowx', so the window is always ones there.

install() does not bind this function; a training loop calls it in place of model(data).  There is no CPU fallback: every tensor of `data` must
already be on the model's device (the reference's .cuda() calls are uploads).
"""
from __future__ import annotations

import dataclasses

import torch

from . import _lib
from .affine import affine_sample
from .corner import training_outputs, corner_losses
from .losses import supervised_losses
from .simi_geometry import polar_pick, similarity_warps
from .triplet import triplet_l1_mean

DATA_KEYS = ("template", "template_lp", "search", "label_cls", "label_loc_c", "label_cls_lp", "label_loc_lp", "template_poly", "search_poly",
             "search_hm", "template_hm", "if_pos", "if_unsup", "temp_cx", "temp_cy")
_PATCH = 127                                                   # the literal of get_homo_data / get_simi_data (:275-276, :324-325)


@dataclasses.dataclass(frozen=True)
class SimiTrainConfig:
    """What ModelBuilder.forward reads from cfg, with the shipped values.  Only the two loss weights and `adjust` (cfg.ADJUST.ADJUST: whether the
    necks run) may differ from them: the rest is either a literal elsewhere in the reference's forward (127, 255) or selects a branch that is not
    restated (OBJ, MODEL_TYPE, WEIGHTED_MAP_LP: True); validate() raises ValueError for anything else."""
    stride: int = 8                                            # POINT.STRIDE
    stride_lp: int = 8                                         # POINT.STRIDE_LP
    exemplar_size: int = 127                                   # TRAIN.EXEMPLAR_SIZE = TRACK.EXEMPLAR_SIZE
    instance_size: int = 255                                   # TRACK.INSTANCE_SIZE
    output_size_lp: int = 13                                   # TRAIN.OUTPUT_SIZE_LP
    cls_weight: float = 1.0                                    # TRAIN.CLS_WEIGHT
    loc_weight: float = 1.0                                    # TRAIN.LOC_WEIGHT
    obj: str = "ALL"                                           # TRAIN.OBJ
    model_type: str = "E2E"                                    # TRAIN.MODEL_TYPE
    weighted_map_lp: bool = False                              # TRAIN.WEIGHTED_MAP_LP
    adjust: bool = True                                        # ADJUST.ADJUST

    def validate(self):
        shipped = SimiTrainConfig()
        for f in dataclasses.fields(self):
            if f.name in ("cls_weight", "loc_weight", "adjust"):
                continue
            if getattr(self, f.name) != getattr(shipped, f.name) or type(getattr(self, f.name)) is not type(getattr(shipped, f.name)):
                raise ValueError(f"SimiTrainConfig.{f.name} = {getattr(self, f.name)!r}: simi_training_forward restates the shipped value "
                                 f"{getattr(shipped, f.name)!r} only")
        for k in ("cls_weight", "loc_weight"):
            v = getattr(self, k)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
                raise ValueError(f"SimiTrainConfig.{k} must be a number, got {v!r}")
        if not isinstance(self.adjust, bool):
            raise ValueError(f"SimiTrainConfig.adjust must be a bool, got {self.adjust!r}")
        return self


_CONSTANTS = {}


def homo_constants(B, dev):
    """(h4p [B,8], patch_indices [B,127*127]) of get_homo_data (:283-295) as device buffers, built once per (B, device) - outside any capture,
    since building them uploads: the four corners (0,0), (0,127), (127,127), (127,0) and the row-major index of the full patch."""
    key = (int(B), str(dev))
    if key not in _CONSTANTS:
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"simi_training_forward: the constants of batch size {B} are not on {dev} yet and building them uploads; run one "
                               "forward outside the capture first (the warm-up does)")
        h4p = torch.tensor([0, 0, 0, _PATCH, _PATCH, _PATCH, _PATCH, 0], dtype=torch.float32, device=dev).unsqueeze(0).repeat(B, 1)
        patch_indices = torch.arange(_PATCH * _PATCH, dtype=torch.float32, device=dev).unsqueeze(0).repeat(B, 1)
        _CONSTANTS[key] = (h4p, patch_indices)
    return _CONSTANTS[key]


def _f32(t):
    return t if t.dtype == torch.float32 else t.float()        # on the device: a cast kernel, not an upload


def _check_model(model, cfg):
    need = ["feature_extractor", "head", "head_lp", "logpolar_instance", "hm_net"] + (["neck", "neck_lp"] if cfg.adjust else [])
    for k in need:
        if getattr(model, k, None) is None:
            raise AttributeError(f"simi_training_forward: the model has no `{k}` (the reference's ModelBuilder attribute)")
    sf = getattr(model.hm_net, "ShareFeature", None)
    if sf is None:
        raise AttributeError("simi_training_forward: model.hm_net has no `ShareFeature`")
    if not (callable(getattr(model.hm_net, "training_forward", None)) or callable(model.hm_net)):
        raise AttributeError("simi_training_forward: model.hm_net has neither `training_forward` nor the reference's `forward`")
    if hasattr(sf, "hip_train") and not sf.training and not sf.hip_train:
        raise RuntimeError("simi_training_forward: hm_net.ShareFeature is in eval() mode with hip_train False, where it runs the fused inference "
                           "kernel and detaches; call .train(), or set ShareFeature.hip_train = True to keep the running statistics and the graph")
    return sf


def simi_training_forward(model, data, cfg: SimiTrainConfig = SimiTrainConfig(), return_counts: bool = False):
    """ModelBuilder.forward (model_builder_e2e_unconstrained_v2.py:361-563) on the package's operators -> the reference's fourteen outputs
    (hdn_amd.corner.OUTPUT_KEYS, 0-d tensors; total_loss carries the graph to every parameter the reference's reaches).

    model: any object with the reference's attribute names - feature_extractor, neck, head, neck_lp, head_lp, logpolar_instance, hm_net (the necks
    may be absent when cfg.adjust is False); hm_net has ShareFeature and either training_forward (hdn_amd.HomoModelBuilder: called with
    host_free=True) or the reference's forward (which reads nonzero() on the host: the result is the same, the capture is lost).
    data: the reference's batch (DATA_KEYS), every tensor on the device; if_pos, if_unsup, temp_cx, temp_cy [B].
    return_counts=True: (outputs, counts) with counts = {'corner': int32 [6] (n_sup, n_sup_pos, n_sup_neg, n_unsup, n_unsup_pos, n_neg),
    'sim': int32 [2] (n_sel, n_neg)} on the device.

    With no unsupervised-positive sample sim_loss and cor_err_sim are 0 with zero gradients; with no selected sample in the homography estimator
    its feature_loss is 0, where the reference divides by zero.  The third stn_with_theta of :418 is not computed: nobody reads its result
    (homo_model_builder.py:122 tests the key 'search_windowx').  Once the constants of this batch size are on the device (one call outside any
    capture) nothing is read by or uploaded from the host: forward and backward can be captured in one graph."""
    if not isinstance(cfg, SimiTrainConfig):
        raise TypeError(f"cfg must be a SimiTrainConfig, got {type(cfg).__name__}")
    cfg.validate()
    sf = _check_model(model, cfg)
    for k in DATA_KEYS:
        if k not in data:
            raise KeyError(f"data['{k}'] missing (model_builder_e2e_unconstrained_v2.py:337-355)")
    template, template_lp, search = data["template"], data["template_lp"], data["search"]
    search_hm, template_hm = data["search_hm"], data["template_hm"]
    dev = _lib.require_device(template, template_lp, search, search_hm, template_hm)
    for k in DATA_KEYS:
        if data[k].device != dev:
            raise _lib.HdnHipError(f"data['{k}'] lives on {data[k].device}, the images on {dev}; nothing is uploaded here and there is no CPU fallback")
    if_pos, if_unsup, temp_cx, temp_cy = (_f32(data[k]) for k in ("if_pos", "if_unsup", "temp_cx", "temp_cy"))
    template_poly, search_poly = _f32(data["template_poly"]), _f32(data["search_poly"])
    B = int(search.shape[0])
    for k, v in (("if_pos", if_pos), ("if_unsup", if_unsup), ("temp_cx", temp_cx), ("temp_cy", temp_cy)):
        if tuple(v.shape) != (B,):
            raise ValueError(f"data['{k}'] must be [{B}], got {list(v.shape)}")
    if tuple(search_hm.shape[2:]) != (cfg.instance_size,) * 2 or tuple(template_hm.shape[2:]) != (cfg.exemplar_size,) * 2:
        raise ValueError(f"search_hm must be [B,C,{cfg.instance_size},{cfg.instance_size}] and template_hm [B,C,{cfg.exemplar_size},"
                         f"{cfg.exemplar_size}], got {list(search_hm.shape)} and {list(template_hm.shape)}")

    # :361-388 the networks, the pick between them and the log-polar sampler
    zf = model.feature_extractor(template)
    zf_lp = model.feature_extractor(template_lp)
    xf = model.feature_extractor(search)
    if cfg.adjust:
        zf, xf = model.neck(zf), model.neck(xf)
    cls, loc = model.head(zf, xf)
    polar = polar_pick(cls.detach(), loc, stride=cfg.stride)                           # :377, the `* STRIDE` folded in; the class map only chooses
    x_lp, _ = model.logpolar_instance(search, polar)
    xf_lp = model.feature_extractor(x_lp)
    if cfg.adjust:
        zf_lp, xf_lp = model.neck_lp(zf_lp), model.neck_lp(xf_lp)
    cls_lp, loc_lp = model.head_lp(zf_lp, xf_lp)
    if cls_lp.shape[-1] != cfg.output_size_lp:
        raise ValueError(f"head_lp returned a {cls_lp.shape[-1]} x {cls_lp.shape[-2]} map, cfg.output_size_lp is {cfg.output_size_lp}")

    # :390-418 scale and rotation, the four warp matrices and the two point sets; the two warps of search_hm
    g = similarity_warps(cls_lp.detach(), loc_lp, polar, temp_cx, temp_cy, search_poly, stride=cfg.stride, stride_lp=cfg.stride_lp,
                         map_size=cfg.exemplar_size, in_sz=cfg.instance_size, out_sz=cfg.exemplar_size)
    grid_size = (B, 1, cfg.exemplar_size, cfg.exemplar_size)
    warped_search_ori = affine_sample(search_hm, g["affine_m"], grid_size, differentiable=True)
    search_hm_simi_ori = affine_sample(search_hm, g["affine_m_c_aug"], grid_size, differentiable=True)
    template_mean = torch.mean(_f32(template_hm), 1, keepdim=True)                     # get_simi_data = get_homo_data's mean: computed once
    search_hm_simi = torch.mean(search_hm_simi_ori, 1, keepdim=True)
    warped_search_mean = torch.mean(warped_search_ori, 1, keepdim=True)

    # :421-440 ShareFeature x 3 and the similarity triplet term over the unsupervised positives
    tmp_f = sf(template_mean)
    sear_f = sf(search_hm_simi)
    pre_sear_f = sf(warped_search_mean)
    sim_loss, sim_counts = triplet_l1_mean(tmp_f, pre_sear_f, sear_f, if_pos, if_unsup, rule=0, denom=_PATCH * _PATCH, margin=1.0, eps=1e-6)

    # :447-455 the homography estimator on (template_hm, warped search) (MODEL_TYPE 'E2E')
    h4p, patch_indices = homo_constants(B, dev)
    org_imgs = torch.cat([template_mean, warped_search_mean], dim=1)
    homo_data = {"org_imgs": org_imgs, "input_tensors": org_imgs, "h4p": h4p, "patch_indices": patch_indices, "if_pos": if_pos,
                 "if_unsup": if_unsup}
    hm_train = getattr(model.hm_net, "training_forward", None)
    batch_out = hm_train(homo_data, host_free=True) if callable(hm_train) else model.hm_net(homo_data)
    loss_feature = batch_out["feature_loss"].mean()

    # :457-562 the supervised head losses, the corner supervision, the dictionary
    head = supervised_losses(cls, loc, cls_lp, loc_lp, data["label_cls"], data["label_loc_c"], data["label_cls_lp"], data["label_loc_lp"],
                             if_unsup=if_unsup)
    cor = corner_losses(batch_out["H_mat"], g["pred_points"], template_poly, batch_out["x"], if_pos, if_unsup,
                        aug_sear_points=g["aug_sear_points"])
    outputs = training_outputs(head, cor, sim_loss, loss_feature, cfg.cls_weight, cfg.loc_weight)
    if return_counts:
        return outputs, {"corner": cor["counts"], "sim": sim_counts}
    return outputs
