"""Rebind the reference's hot-path symbols to the HIP implementations.

    import hdn_amd.install as hi; hi.install()     # after the reference packages are importable

so that tools/test.py / tools/demo.py of the reference run unchanged.  Each rebinding site is the module
attribute the reference resolves at call time:

    hdn.core.xcorr.xcorr_depthwise{,_circular}           definitions
    hdn.models.head.ban.xcorr_depthwise                  ban.py:10 (from-import binding used at ban.py:76)
    hdn.models.head.ban_lp.xcorr_depthwise_circular      ban_lp.py:10 (used at ban_lp.py:38)
    ...Oneline_DLTv1.utils.{DLT_solve,transform,transformer}
    ...models.homo_model_builder.{DLT_solve,transform}   homo_model_builder.py:13
    hdn.models.model_builder_e2e_unconstrained_v2.{DLT_solve,Homo_STN}   :29-30
    ...preprocess.head['PreShareFeature']                registry used by get_pre(), preprocess/__init__.py:18-26
    ModelBuilder.track_proj                              replaced by the fused version (install(trunk=True): which also attaches the folded HIP trunk
                                                         to self.hm_net at its first eval-mode call on a GPU)
    hdn.models.logpolar.STN_Polar (+ its from-import in model_builder…:24)   device-resident log-polar sampler
    MultiBAN.forward / MultiCircBAN.forward              one correlation launch per head + cached template branch
    ModelBuilder.track_new_lp                            same ops, the zero `polar` argument cached on the device (:145: a pageable
                                                         host->device copy per frame, which a hipGraph capture cannot hold)
    ModelBuilder.template                                unchanged, then drops the heads' cached template-branch features
    ModelBuilder.stn_with_theta                          (install(train=True), while AFFINE_STN_TRAIN_BOUND) the differentiable HIP affine sampler
    {model_builder_e2e_unconstrained_v2, homo_model_builder}.triplet_loss   (install(train=True), while TRIPLET_TRAIN_BOUND) TripletMarginLossL1
    model_builder_e2e_unconstrained_v2.{select_xr_focal_fuse_smooth_l1_loss_top_k, select_l1_loss_c, select_cross_entropy_loss, select_l1_loss,
        kalyo_l1_loss}                                   (install(train=True), while SUP_LOSS_TRAIN_BOUND) the drop-ins of hdn_amd/losses.py
    model_builder_e2e_unconstrained_v2.{lp_pick, combine_affine_c0_v2, combine_affine_lt0}   :27-28 (install(train=True), while
        hdn.models.logpolar.Polar_Pick.get_polar_from_two_para_loc       SIMI_GEOMETRY_TRAIN_BOUND) the drop-ins of hdn_amd/simi_geometry.py
    DepthwiseXCorr.forward / DepthwiseXCorrCirc.forward  (install(train=True), while HEAD_CONV_TRAIN_BOUND) in .train() mode the two 3x3 convolutions
                                                         on hdn_amd.conv3x3_valid (hdn_amd/conv_train.py) and, while HEAD_BN_TRAIN_BOUND, their
                                                         BatchNorm + ReLU on hdn_amd.batchnorm_relu_train; the class's own forward otherwise
    hdn.tracker.tracker_builder.TRACKS['hdnTrackerHomoProje2e']   (install(tracker=True)) the device-resident tracker loop

Training under install(train=True): every statement of the reference's training forwards that resolves to a drop-in is differentiable on the device -
xcorr_depthwise{,_circular} (hdn_amd/xcorr.py), DLT_solve / transform / transformer (hdn_amd/homography.py) and, with train=True, STN_Polar
(STN_PolarTrain, hdn_amd/logpolar.py; without train=True the STN_Polar drop-in raises on a grad-carrying input rather than detach) and
PreShareFeature (PreShareFeatureTrain, hdn_amd/share_feature.py: batch statistics and the backward on HIP, and an eval mode that carries the graph) and
ModelBuilder.stn_with_theta (hdn_amd/affine.py: the affine sampler of :407, :408, :418, forward and backward on HIP) and the module attribute
`triplet_loss` of both model builders (hdn_amd/triplet.py: the L1 triplet rows of :438 and homo_model_builder.py:197).  The rebound head
forwards defer to the classes' own forward in .train() mode.  What still needs uninstall(): anything that calls the fused inference paths with
autograd expected - the fused track_proj, dlt_warp, the fused heads in eval mode, xcorr_fast / xcorr_slow, xcorr_depthwise_multi (they detach).
"""
from __future__ import annotations

import importlib
import types
import weakref

import torch

from . import affine, conv_train, heads, homo_model, homography, logpolar, losses, share_feature, simi_geometry, triplet, xcorr

_DLT = "homo_estimator.Deep_homography.Oneline_DLTv1"

REBINDINGS = (
    ("hdn.core.xcorr", "xcorr_depthwise", xcorr.xcorr_depthwise),
    ("hdn.core.xcorr", "xcorr_depthwise_circular", xcorr.xcorr_depthwise_circular),
    ("hdn.core.xcorr", "xcorr_fast", xcorr.xcorr_fast),
    ("hdn.core.xcorr", "xcorr_slow", xcorr.xcorr_slow),
    ("hdn.models.head.ban", "xcorr_fast", xcorr.xcorr_fast),
    ("hdn.models.head.ban", "xcorr_depthwise", xcorr.xcorr_depthwise),
    ("hdn.models.head.ban_lp", "xcorr_depthwise", xcorr.xcorr_depthwise),
    ("hdn.models.head.ban_lp", "xcorr_depthwise_circular", xcorr.xcorr_depthwise_circular),
    (_DLT + ".utils", "DLT_solve", homography.DLT_solve),
    (_DLT + ".utils", "transform", homography.transform),
    (_DLT + ".utils", "transformer", homography.transformer),
    (_DLT + ".models.homo_model_builder", "DLT_solve", homography.DLT_solve),
    (_DLT + ".models.homo_model_builder", "transform", homography.transform),
    ("hdn.models.model_builder_e2e_unconstrained_v2", "DLT_solve", homography.DLT_solve),
    ("hdn.models.model_builder_e2e_unconstrained_v2", "Homo_STN", homography.transform),
    # class rebinding: ModelBuilder.__init__ instantiates it (model_builder…:42), so install() must run first
    ("hdn.models.logpolar", "STN_Polar", logpolar.STN_Polar),
    ("hdn.models.model_builder_e2e_unconstrained_v2", "STN_Polar", logpolar.STN_Polar),
)


def _track_proj_method(self, data, tmp_mask):
    """ModelBuilder.track_proj with the fused stages; self.hm_net supplies ShareFeature/backbone/avgpool/fc."""
    return homo_model.track_proj(self.hm_net, data, tmp_mask)


_trunk_nets = []   # weak references to the hm_nets _track_proj_trunk_method attached a folded trunk to; uninstall() detaches them


def _maybe_attach_trunk(net) -> bool:
    """Attach the folded HIP trunk to `net` (hm_net) if it has none, is in eval mode and holds CUDA float32 weights; was it attached now?"""
    if getattr(net, "_hdn_fast_trunk", None) is not None or net.training or getattr(net, "_hdn_trunk_refused", False):
        return False
    p = next(net.backbone.parameters())
    if not p.is_cuda or p.dtype != torch.float32:
        return False
    try:
        homo_model.optimize_trunk(net, channels_last=True)
    except ValueError as e:          # a trunk the fold does not know: say so once, keep the model's own backbone
        import warnings
        warnings.warn(f"hdn_amd: install(trunk=True) leaves hm_net.backbone as it is ({e})")
        object.__setattr__(net, "_hdn_trunk_refused", True)
        return False
    _trunk_nets.append(weakref.ref(net))
    return True


def _track_proj_trunk_method(self, data, tmp_mask):
    """_track_proj_method of install(trunk=True): the folded HIP trunk is attached to self.hm_net at the first call that can use it."""
    _maybe_attach_trunk(self.hm_net)
    return homo_model.track_proj(self.hm_net, data, tmp_mask)


def _track_new_lp_method(self, x, delta=[0, 0]):
    """ModelBuilder.track_new_lp (model_builder_e2e_unconstrained_v2.py:144-158), statement for statement, except that the
    all-zero `polar` lives on the device instead of being built on the host and uploaded every frame."""
    polar = getattr(self, "_hdn_polar0", None)
    if polar is None or polar.device != x.device or polar.shape[0] != x.shape[0]:
        polar = torch.zeros((x.shape[0], 2), dtype=torch.float32, device=x.device)
        object.__setattr__(self, "_hdn_polar0", polar)
    x_lp, grid = self.logpolar_instance(x, polar, delta)
    xf_lp = self.feature_extractor(x_lp)
    if hasattr(self, "neck_lp"):          # cfg.ADJUST.ADJUST (the constructor creates the necks under the same condition, :45-49)
        xf_lp = self.neck_lp(xf_lp)
    cls_lp, loc_lp = self.head_lp(self.zf_lp, xf_lp)
    return {"x_lp": x_lp, "cls_lp": cls_lp, "loc_lp": loc_lp, "grid": grid}


def _make_template_method(orig):
    def template(self, z):
        out = orig(self, z)
        for name in ("head", "head_lp"):
            if hasattr(self, name):
                heads.invalidate_template_cache(getattr(self, name))
        return out
    template._hdn_wraps = orig
    return template


# Does install(train=True) bind PreShareFeatureTrain at preprocess.head['PreShareFeature']?  Set by the outcome of tools/share_feature_train_bench.py
# (profiles/share_feature_train.json): True only while the HIP path is faster than the stock nn.Sequential on the step's six calls at B = 32.
SHARE_FEATURE_TRAIN_BOUND = True

# Does install(train=True) bind hdn_amd.affine.stn_with_theta at ModelBuilder.stn_with_theta?  Set by the outcome of tools/affine_stn_train_bench.py
# (profiles/affine_stn_train.json): True only while the HIP path is faster than F.affine_grid + F.grid_sample on the step's three calls at B = 32.
AFFINE_STN_TRAIN_BOUND = True

# Does install(train=True) bind a hdn_amd.triplet.TripletMarginLossL1 at the two `triplet_loss` module attributes?  Set by the outcome of
# tools/triplet_train_bench.py (profiles/triplet_train.json): True only while the HIP loss is faster than x[ids] x 3 + nn.TripletMarginLoss on the
# step's two sites at B = 32.
TRIPLET_TRAIN_BOUND = True

# the modules whose attribute `triplet_loss` is the reference's nn.TripletMarginLoss(margin=1.0, p=1, reduce=False, size_average=False)
TRIPLET_SITES = ("hdn.models.model_builder_e2e_unconstrained_v2", _DLT + ".models.homo_model_builder")

# Does install(train=True) bind the five loss drop-ins of hdn_amd.losses at the names model_builder_e2e_unconstrained_v2 imports from
# hdn.models.loss?  Set by the outcome of tools/sup_loss_train_bench.py (profiles/sup_loss_train.json): True only while the reference's formulation
# of :457-478 with the drop-ins inside is faster, forward and backward at B = 32, than with its own PyTorch functions.
SUP_LOSS_TRAIN_BOUND = True

SUP_LOSS_SITE = "hdn.models.model_builder_e2e_unconstrained_v2"
SUP_LOSS_NAMES = ("select_xr_focal_fuse_smooth_l1_loss_top_k", "select_l1_loss_c", "select_cross_entropy_loss", "select_l1_loss", "kalyo_l1_loss")

# Does install(train=True) bind the drop-ins of hdn_amd.simi_geometry at the three names model_builder_e2e_unconstrained_v2 imports (:27-28: lp_pick,
# combine_affine_c0_v2, combine_affine_lt0) and at Polar_Pick.get_polar_from_two_para_loc?  Set by the outcome of tools/simi_geometry_train_bench.py
# (profiles/simi_geometry_train.json, "ahead"): True only while the reference's lines :377, :390-415 with the drop-ins inside are faster, forward and
# backward at B = 32, than with their own PyTorch functions.
SIMI_GEOMETRY_TRAIN_BOUND = True

SIMI_GEOMETRY_SITE = "hdn.models.model_builder_e2e_unconstrained_v2"
SIMI_GEOMETRY_NAMES = ("lp_pick", "combine_affine_c0_v2", "combine_affine_lt0")
POLAR_PICK_SITE = ("hdn.models.logpolar", "Polar_Pick", "get_polar_from_two_para_loc")

# Does install(train=True) rebind DepthwiseXCorr.forward / DepthwiseXCorrCirc.forward to the dispatcher that, in .train() mode, runs
# hdn_amd.conv_train.depthwise_xcorr_train_forward (the two 3x3 convolutions of a head branch, forward, dgrad and wgrad on HIP)?  Set by the outcome of
# tools/head_conv_train_bench.py (profiles/head_conv_train.json): True only while the HIP path is faster than PyTorch-ROCm autograd through nn.Conv2d
# on the step's 24 convolutions at B = 32, beyond both sides' spread.
HEAD_CONV_TRAIN_BOUND = True

# Does that training forward also run a head branch's BatchNorm2d (batch statistics) + ReLU as one hdn_amd.bn_train.batchnorm_relu_train, channels-last
# in and NCHW out, in place of the modules, the layout copies around the correlation and the copy behind the inplace ReLU?  It has no rebinding site of
# its own: hdn_amd.conv_train._branch reads it at every call, inside the forward that HEAD_CONV_TRAIN_BOUND binds.  Set by the outcome of
# tools/head_bn_train_bench.py (profiles/head_bn_train.json, "ahead"): True only while the HIP path is faster than the stock modules and copies on the
# step's 24 sites at B = 32, beyond both sides' spread.
HEAD_BN_TRAIN_BOUND = False

# (module, class, the module attribute its forward resolves the correlation by)
HEAD_CONV_SITES = (("hdn.models.head.ban", "DepthwiseXCorr", "xcorr_depthwise"), ("hdn.models.head.ban_lp", "DepthwiseXCorrCirc", "xcorr_depthwise_circular"))


def _make_head_branch_forward(orig, module, xcorr_name):
    """The dispatcher bound at a head branch's forward: .train() mode runs the HIP training forward with the correlation `module` resolves NOW (the
    rebindings above included), any other mode the class's saved forward."""
    def forward(self, kernel, search):
        if self.training:
            return conv_train.depthwise_xcorr_train_forward(self, kernel, search, getattr(module, xcorr_name))
        return orig(self, kernel, search)
    forward._hdn_wraps = orig
    return forward


_MISSING = object()
_saved = []  # (owner, attribute or dict key, original value, is_dict_item) in application order; undone by uninstall()


def _rebind(owner, attr, value, item=False):
    if item:
        _saved.append((owner, attr, owner.get(attr, _MISSING), True))
        owner[attr] = value
    else:
        _saved.append((owner, attr, owner.__dict__.get(attr, _MISSING) if isinstance(owner, type) else getattr(owner, attr, _MISSING), False))
        setattr(owner, attr, value)


def uninstall() -> int:
    """Undo every rebinding install() made (most recent first): the reference runs on its own PyTorch ops again, e.g. for code that expects autograd
    through the fused inference paths (the fused track_proj, dlt_warp, the eval-mode heads and xcorr_fast carry no autograd graph).  Folded trunks
    that install(trunk=True) attached are detached (optimize_trunk(net, enable=False)).  Returns the number of rebindings undone."""
    n = 0
    while _trunk_nets:
        net = _trunk_nets.pop()()
        if net is not None:
            homo_model.optimize_trunk(net, enable=False)
    while _saved:
        owner, attr, orig, item = _saved.pop()
        if item:
            if orig is _MISSING:
                owner.pop(attr, None)
            else:
                owner[attr] = orig
        elif orig is _MISSING:
            try:
                delattr(owner, attr)
            except AttributeError:
                pass
        else:
            setattr(owner, attr, orig)
        n += 1
    return n


def install(strict: bool = False, modules: dict = None, tracker: bool = False, trunk: bool = False, train: bool = False) -> list:
    """Apply the rebindings.  tracker=True also registers hdn_amd.tracker.DeviceTrackerHomo under
    TRACKS['hdnTrackerHomoProje2e'] (hdn/tracker/tracker_builder.py:12-19), so build_tracker(model) of tools/test.py:72 /
    tools/demo.py returns the device-resident loop (frames uploaded once, crops / warps / decodes as kernels, one host read per
    frame) instead of the host-side one.  `modules` (name -> module) lets tests supply stand-in modules; by default the
    real reference modules are imported.  trunk=True: the rebound ModelBuilder.track_proj attaches the BatchNorm-folded HIP trunk
    (hdn_amd.homo_model.optimize_trunk(self.hm_net, channels_last=True)) at its first eval-mode call with CUDA float32 weights, for users of the
    rebindings without the device tracker; off by default.  train=True: the two STN_Polar sites are bound to hdn_amd.logpolar.STN_PolarTrain (the same
    module with differentiable=True) and, while SHARE_FEATURE_TRAIN_BOUND, preprocess.head['PreShareFeature'] to hdn_amd.share_feature.PreShareFeatureTrain
    (hip_train=True) and, while AFFINE_STN_TRAIN_BOUND, ModelBuilder.stn_with_theta to hdn_amd.affine.stn_with_theta and, while TRIPLET_TRAIN_BOUND,
    the attribute `triplet_loss` of the two TRIPLET_SITES modules to a hdn_amd.triplet.TripletMarginLossL1 of the same margin and eps (only where it
    is an nn.TripletMarginLoss with p = 1, swap False and reduction 'none') and, while SUP_LOSS_TRAIN_BOUND, the five SUP_LOSS_NAMES that
    model_builder_e2e_unconstrained_v2 imports from hdn.models.loss to the drop-ins of hdn_amd.losses (only where the attribute exists;
    select_xr_focal_fuse_smooth_l1_loss and select_l1_loss_lp, the WEIGHTED_MAP_LP: True branch, stay the reference's), so that the reference's
    training forward runs on the drop-ins and, while SIMI_GEOMETRY_TRAIN_BOUND, the three SIMI_GEOMETRY_NAMES that the same module imports and
    Polar_Pick.get_polar_from_two_para_loc to the drop-ins of hdn_amd.simi_geometry (only where the attribute exists; the method keeps the one it
    replaces for a points table that is not the analytic one) and, while HEAD_CONV_TRAIN_BOUND, DepthwiseXCorr.forward and DepthwiseXCorrCirc.forward
    (HEAD_CONV_SITES) to a dispatcher that runs hdn_amd.conv_train.depthwise_xcorr_train_forward in .train() mode and the class's own forward
    otherwise (inside it, while HEAD_BN_TRAIN_BOUND, a branch's BatchNorm + ReLU run as hdn_amd.batchnorm_relu_train); everything else is unchanged.  Returns the list of (module, attribute) pairs that were rebound;
    with strict=True a site that cannot be imported raises instead of being skipped.  uninstall() reverses it."""
    done = []

    def get(name):
        if modules is not None:
            return modules.get(name)
        try:
            return importlib.import_module(name)
        except Exception:
            if strict:
                raise
            return None

    for mod_name, attr, fn in REBINDINGS:
        m = get(mod_name)
        if m is None:
            continue
        if not hasattr(m, attr) and strict:
            raise AttributeError(f"{mod_name}.{attr} not found: reference layout changed?")
        _rebind(m, attr, logpolar.STN_PolarTrain if train and fn is logpolar.STN_Polar else fn)
        done.append((mod_name, attr))

    pre = get(_DLT + ".preprocess")
    if pre is not None and isinstance(getattr(pre, "head", None), dict):
        sf = share_feature.PreShareFeatureTrain if train and SHARE_FEATURE_TRAIN_BOUND else share_feature.PreShareFeature
        _rebind(pre.head, "PreShareFeature", sf, item=True)
        done.append((_DLT + ".preprocess", "head['PreShareFeature']"))

    # heads: keep the reference's classes (and their weights), swap the schedule of forward()
    for mod_name, cls_name, circ in (("hdn.models.head.ban", "MultiBAN", False), ("hdn.models.head.ban_lp", "MultiCircBAN", True)):
        m = get(mod_name)
        if m is not None and hasattr(m, cls_name):
            klass = getattr(m, cls_name)
            if "_hdn_orig_forward" not in klass.__dict__ and "forward" in klass.__dict__:
                _rebind(klass, "_hdn_orig_forward", klass.__dict__["forward"])  # training-mode calls are deferred to it
            _rebind(klass, "forward", (lambda c: lambda self, z_fs, x_fs: heads.fused_forward(self, z_fs, x_fs, c))(circ))
            done.append((mod_name, cls_name + ".forward"))

    if train and HEAD_CONV_TRAIN_BOUND:
        for mod_name, cls_name, xcorr_name in HEAD_CONV_SITES:
            m = get(mod_name)
            klass = getattr(m, cls_name, None) if m is not None else None
            if isinstance(klass, type) and "forward" in klass.__dict__ and not hasattr(klass.__dict__["forward"], "_hdn_wraps"):
                _rebind(klass, "forward", _make_head_branch_forward(klass.__dict__["forward"], m, xcorr_name))
                done.append((mod_name, cls_name + ".forward"))

    mb = get("hdn.models.model_builder_e2e_unconstrained_v2")
    if mb is not None and hasattr(mb, "ModelBuilder"):
        _rebind(mb.ModelBuilder, "track_proj", _track_proj_trunk_method if trunk else _track_proj_method)
        done.append(("hdn.models.model_builder_e2e_unconstrained_v2", "ModelBuilder.track_proj"))
        if "track_new_lp" in mb.ModelBuilder.__dict__:
            _rebind(mb.ModelBuilder, "track_new_lp", _track_new_lp_method)
            done.append(("hdn.models.model_builder_e2e_unconstrained_v2", "ModelBuilder.track_new_lp"))
        orig_t = mb.ModelBuilder.__dict__.get("template")
        if orig_t is not None and not hasattr(orig_t, "_hdn_wraps"):
            _rebind(mb.ModelBuilder, "template", _make_template_method(orig_t))
            done.append(("hdn.models.model_builder_e2e_unconstrained_v2", "ModelBuilder.template"))
        if train and AFFINE_STN_TRAIN_BOUND and "stn_with_theta" in mb.ModelBuilder.__dict__:
            _rebind(mb.ModelBuilder, "stn_with_theta", affine.stn_with_theta)
            done.append(("hdn.models.model_builder_e2e_unconstrained_v2", "ModelBuilder.stn_with_theta"))

    if train and TRIPLET_TRAIN_BOUND:
        for mod_name in TRIPLET_SITES:
            m = get(mod_name)
            loss = getattr(m, "triplet_loss", None) if m is not None else None
            # only the loss the kernel restates: L1 distances, no distance swap, one value per row
            if isinstance(loss, torch.nn.TripletMarginLoss) and loss.p == 1 and not loss.swap and loss.reduction == "none":
                _rebind(m, "triplet_loss", triplet.TripletMarginLossL1(margin=loss.margin, eps=loss.eps))
                done.append((mod_name, "triplet_loss"))

    if train and SUP_LOSS_TRAIN_BOUND:
        m = get(SUP_LOSS_SITE)
        for name in SUP_LOSS_NAMES:
            if m is not None and hasattr(m, name):
                _rebind(m, name, losses.DROP_INS[name])
                done.append((SUP_LOSS_SITE, name))

    if train and SIMI_GEOMETRY_TRAIN_BOUND:
        m = get(SIMI_GEOMETRY_SITE)
        for name in SIMI_GEOMETRY_NAMES:
            if m is not None and hasattr(m, name):
                _rebind(m, name, simi_geometry.DROP_INS[name])
                done.append((SIMI_GEOMETRY_SITE, name))
        mod_name, cls_name, meth = POLAR_PICK_SITE
        klass = getattr(get(mod_name), cls_name, None)
        if isinstance(klass, type) and meth in klass.__dict__:
            _rebind(klass, meth, simi_geometry.make_get_polar(klass.__dict__[meth]))
            done.append((mod_name, cls_name + "." + meth))

    if tracker:
        tb = get("hdn.tracker.tracker_builder")
        if tb is None or not isinstance(getattr(tb, "TRACKS", None), dict):
            if strict:
                raise AttributeError("hdn.tracker.tracker_builder.TRACKS not found: reference layout changed?")
        else:
            from .tracker import DeviceTrackerHomo
            _rebind(tb.TRACKS, "hdnTrackerHomoProje2e", DeviceTrackerHomo, item=True)
            done.append(("hdn.tracker.tracker_builder", "TRACKS['hdnTrackerHomoProje2e']"))
            from .simi_tracker import DeviceTrackerSimi
            _rebind(tb.TRACKS, "hdnTracker", DeviceTrackerSimi, item=True)
            done.append(("hdn.tracker.tracker_builder", "TRACKS['hdnTracker']"))
    return done
