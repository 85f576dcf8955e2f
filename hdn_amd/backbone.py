"""The similarity branch's backbone and necks at inference: PyTorch-ROCm (MIOpen) keeps the convolutions, this module removes the
launches around them.

The reference runs `ResNet-50 (stride 8, dilated) -> AdjustAllLayer` twice per frame (hdn/models/model_builder_e2e_unconstrained_v2.py
:131-158: 255-px search crop, 127-px log-polar crop) as eval-mode `conv -> BatchNorm -> ReLU` chains
(hdn/models/backbone/resnet_atrous.py:60-108 Bottleneck.forward, :186-199 ResNet.forward; hdn/models/neck/neck.py:11-51).  At the
tracker's B = 1 every one of those elementwise modules is a launch of its own: per frame 108 BatchNorm, 95 ReLU and 31 residual-add
launches, 1.1 ms of the 3.4 ms frame (profiles/round4_sequence.txt), none of them doing more than a few microseconds of work.

    optimize_similarity_model(model)      # model.backbone / model.neck / model.neck_lp, in place and reversible (restore_...)

  * every eval-mode BatchNorm is folded into the convolution in front of it (weights scaled in float64, rounded once);
  * a Bottleneck becomes  conv -> hdn_bias_relu_f32 -> conv -> hdn_bias_relu_f32 -> conv -> hdn_bias_relu_f32(+ residual):
    three convolutions + three in-place HIP passes instead of three convolutions + seven library launches; a downsample branch is
    one bias-free convolution whose folded shift rides in the last pass's bias;
  * a neck level is one biased 1x1 convolution.

The modules keep their classes' names and parameters (state_dict unchanged): the object gets a subclass whose forward() uses the
folded copy for CUDA float32 inputs in eval mode and the original forward() for anything else (training, CPU tensors).  The
folded copy follows `load_state_dict` (of the module or of any parent: a post-hook re-folds INTO the existing buffers, so a hipGraph
captured around them sees the new weights too); weights edited in place some other way need optimize_similarity_model again.  A switched
module deep-copies and moves like any other, but pickling the MODULE object (torch.save(model), not state_dict) needs
restore_similarity_model first, because the subclass exists only in this process.
hdn_amd.tracker.DeviceTrackerHomo applies it to the model it is given (HDN_FOLD_BACKBONE=0 keeps the modules as they are).

    optimize_similarity_model(model, hip=True)      # or HDN_HIP_BACKBONE=1 (default off)

puts the convolutions themselves on the library's two-fp16-piece matrix-core kernels where it has one (HipBottleneck, HipAtrousResNet, hip_necks below):
every 1x1 convolution on hdn_conv1x1_f32, every stride-1 3x3 convolution with padding == dilation in {1, 2, 4} on hdn_conv3x3d_f32, channels-last between
the maxpool and the necks' outputs.  Convolutions without a kernel (the 7x7 stem; the stride-2, padding-0 first block of layer2 with its strided 3x3 skip)
stay on MIOpen as above.  hip_plan(net) names the kernel of every convolution without building anything.

    optimize_similarity_model(model, hip=2)         # or HDN_HIP_BACKBONE=2 (default off)

is level 2 of the same form, with no library convolution left: the two padding-0 3x3 convolutions of layer2's first block on hdn_conv3x3v_f32 and
conv1 + bn1 + ReLU + maxpool as ONE launch of hdn_simi_stem_f32 (HipAtrousResNetFull).  Level 1 is unchanged by it.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .ops import SIMI_STEM_MAX_SIDE, bias_relu_, conv1x1, conv3x3d, conv3x3v, fold_conv_bn, pack_conv1x1, pack_conv3x3d, pack_simi_stem, simi_stem


def _epilogue(y, bias, residual=None):
    """y = relu(y + bias[c] (+ residual)) in place: one HIP pass (hdn_bias_relu_f32) for device tensors; CPU tensors (the CPU tests
    of the folding against the reference's modules) take the same arithmetic in torch ops."""
    if y.is_cuda:
        return bias_relu_(y, bias, residual)
    y.add_(bias.view(1, -1, 1, 1))
    if residual is not None:
        y.add_(residual)
    return torch.relu_(y)


class _FoldedConv(nn.Module):
    """A convolution with a BatchNorm folded in.  raw(x): without the shift (the caller's epilogue adds it); act(x): relu(conv + shift);
    forward(x): conv + shift (the necks).  (The 1x1 convolutions as hipBLASLt GEMMs with the shift and the ReLU in the GEMM's epilogue
    were measured and dropped: 2-13 us faster per shape in isolation, but under the frame's hipGraph the library picked 60-120-us
    kernels for some of them: profiles/round4_experiments.txt item 9.)"""

    def __init__(self, conv, bn):
        super().__init__()
        w, b = fold_conv_bn(conv, bn)
        self.register_buffer("weight", w)
        self.register_buffer("bias", b)
        self.stride, self.padding, self.dilation = conv.stride, conv.padding, conv.dilation

    def raw(self, x):
        return F.conv2d(x, self.weight, None, self.stride, self.padding, self.dilation)

    def act(self, x):
        return _epilogue(self.raw(x), self.bias)

    def forward(self, x):
        return F.conv2d(x, self.weight, self.bias, self.stride, self.padding, self.dilation)


def _conv_bn_pair(seq):
    """(conv, bn) of a `Sequential(Conv2d, BatchNorm2d)` (the reference's downsample branches and neck levels), else None."""
    if isinstance(seq, nn.Sequential) and len(seq) == 2 and isinstance(seq[0], nn.Conv2d) and isinstance(seq[1], nn.BatchNorm2d):
        return seq[0], seq[1]
    return None


class FusedBottleneck(nn.Module):
    """Bottleneck.forward (resnet_atrous.py:87-108) of a block whose BatchNorms are folded, with `+ shift -> ReLU` and
    `+ shift + residual -> ReLU` as one in-place pass each.  Takes any module with that block's attributes."""

    def __init__(self, blk):
        super().__init__()
        for name in ("conv1", "bn1", "conv2", "bn2", "conv3", "bn3"):
            if not hasattr(blk, name):
                raise ValueError(f"not a Bottleneck: no {name}")
        self.c1, self.c2, self.c3 = _FoldedConv(blk.conv1, blk.bn1), _FoldedConv(blk.conv2, blk.bn2), _FoldedConv(blk.conv3, blk.bn3)
        down = getattr(blk, "downsample", None)
        if down is None:
            self.cd = None
            self.register_buffer("b3", self.c3.bias.clone())
        else:
            pair = _conv_bn_pair(down)
            if pair is None:
                raise ValueError("Bottleneck.downsample is not Sequential(Conv2d, BatchNorm2d)")
            self.cd = _FoldedConv(*pair)
            self.register_buffer("b3", self.c3.bias + self.cd.bias)      # (b3 + b_downsample) once: differs from the unfused sum by rounding

    def forward(self, x):
        y = self.c2.act(self.c1.act(x))
        idt = x if self.cd is None else self.cd.raw(x)
        return _epilogue(self.c3.raw(y), self.b3, idt)


class FusedAtrousResNet(nn.Module):
    """ResNet.forward (resnet_atrous.py:186-199) with folded BatchNorms and FusedBottleneck blocks: conv1 -> shift + ReLU -> maxpool
    -> layer1..4 -> the `used_layers` selection ([stem, p1, p2, p3, p4]; a single level is returned bare, as the reference does)."""

    block = FusedBottleneck

    def __init__(self, net):
        super().__init__()
        for name in ("conv1", "bn1", "maxpool", "layer1", "layer2", "used_layers"):
            if not hasattr(net, name):
                raise ValueError(f"not the reference's ResNet layout: no {name}")
        self.c1 = _FoldedConv(net.conv1, net.bn1)
        self.maxpool = net.maxpool
        self.layers = nn.ModuleList()
        for name in ("layer1", "layer2", "layer3", "layer4"):
            layer = getattr(net, name, None)
            if isinstance(layer, nn.Sequential):
                self.layers.append(nn.Sequential(*[self.block(b) for b in layer]))
            elif layer is None or callable(layer):
                self.layers.append(nn.Identity())       # (`lambda x: x` for an unused stage, resnet_atrous.py:134-141)
            else:
                raise ValueError(f"{name}: expected a Sequential of blocks")
        self.used_layers = list(net.used_layers)

    def stem(self, x):
        """(the stem's own output: level 0 of `used_layers`, or None where it is never written out; layer1's input)"""
        x_ = self.c1.act(x)
        return x_, self.maxpool(x_)

    def forward(self, x):
        x_, p = self.stem(x)
        out = [x_]
        for layer in self.layers:
            p = layer(p)
            out.append(p)
        out = [out[i] for i in self.used_layers]
        return out[0] if len(out) == 1 else out


def fold_sequentials(module: nn.Module, hip: bool = False) -> nn.Module:
    """A deep copy of `module` in which every `Sequential(Conv2d, BatchNorm2d)` is one biased convolution (the necks: AdjustLayer.downsample,
    neck.py:14-17); everything else — the crop of AdjustLayer.forward, the level loop of AdjustAllLayer.forward — stays the module's own.
    hip: levels with a kernel become _HipConv (hip_necks)."""
    import copy

    m = copy.deepcopy(module)

    def walk(parent):
        for name, child in list(parent.named_children()):
            pair = _conv_bn_pair(child)
            if pair is not None:
                setattr(parent, name, (_HipConv if hip and hip_conv_kind(pair[0]) != "miopen" else _FoldedConv)(*pair))
            else:
                walk(child)

    walk(m)
    return m


# --------------------------------------------------------------------------------------------------------- the opt-in HIP form (hip=True)
def hip_conv_kind(conv, level: int = 1) -> str:
    """The kernel a folded convolution of the backbone / necks runs on in the HIP form: "conv1x1" (hdn_conv1x1_f32: 1x1, stride 1 or 2, no padding),
    "conv3x3d" (hdn_conv3x3d_f32: 3x3, stride 1, padding == dilation in {1, 2, 4}) — both with channel counts that are multiples of 32 — or "miopen"
    (F.conv2d + hdn_bias_relu_f32, as in the folded form).  level 2 adds "conv3x3v" (hdn_conv3x3v_f32: 3x3, stride 1 or 2, padding 0, dilation 1)."""
    if not isinstance(conv, nn.Conv2d) or conv.groups != 1 or conv.in_channels % 32 or conv.out_channels % 32 or conv.padding_mode != "zeros":
        return "miopen"
    k, st, pad, dil = conv.kernel_size, conv.stride, conv.padding, conv.dilation
    if k == (1, 1) and st in ((1, 1), (2, 2)) and pad == (0, 0):
        return "conv1x1"
    if k == (3, 3) and st == (1, 1) and dil in ((1, 1), (2, 2), (4, 4)) and pad == dil:
        return "conv3x3d"
    if level >= 2 and k == (3, 3) and st in ((1, 1), (2, 2)) and dil == (1, 1) and pad == (0, 0):
        return "conv3x3v"
    return "miopen"


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def simi_stem_ok(net) -> bool:
    """Does hdn_simi_stem_f32 serve this network's first stage?  conv1 = Conv2d(3, 64, 7, stride 2, padding 0, groups 1), maxpool = MaxPool2d(3, 2, 1)
    without dilation or ceil mode, and the stem's own output is not returned (0 not in used_layers)."""
    c, mp = getattr(net, "conv1", None), getattr(net, "maxpool", None)
    if not isinstance(c, nn.Conv2d) or not isinstance(mp, nn.MaxPool2d) or 0 in list(getattr(net, "used_layers", [0])):
        return False
    conv_ok = (c.in_channels == 3 and c.out_channels == 64 and c.kernel_size == (7, 7) and c.stride == (2, 2) and c.padding == (0, 0)
               and c.dilation == (1, 1) and c.groups == 1 and c.padding_mode == "zeros")
    pool_ok = (_pair(mp.kernel_size) == (3, 3) and _pair(mp.stride) == (2, 2) and _pair(mp.padding) == (1, 1) and _pair(mp.dilation) == (1, 1)
               and not mp.ceil_mode and not mp.return_indices)
    return conv_ok and pool_ok


def hip_plan(net, level: int = 1) -> dict:
    """{"layerN.M.conv1" / ".conv2" / ".conv3" / ".downsample": hip_conv_kind} for every block of a network of the reference's ResNet layout (reads
    the structure only: no weights are folded or packed, no device is needed).  level 2 adds "stem": "simi_stem" (hdn_simi_stem_f32) or "miopen"."""
    plan = {}
    if level >= 2:
        plan["stem"] = "simi_stem" if simi_stem_ok(net) else "miopen"
    for name in ("layer1", "layer2", "layer3", "layer4"):
        layer = getattr(net, name, None)
        if not isinstance(layer, nn.Sequential):
            continue
        for i, blk in enumerate(layer):
            for cn in ("conv1", "conv2", "conv3"):
                plan[f"{name}.{i}.{cn}"] = hip_conv_kind(getattr(blk, cn, None), level)
            pair = _conv_bn_pair(getattr(blk, "downsample", None))
            if pair is not None:
                plan[f"{name}.{i}.downsample"] = hip_conv_kind(pair[0], level)
    return plan


class _HipConv(nn.Module):
    """A convolution with a BatchNorm folded in, on the kernel hip_conv_kind names: the packed stream (a non-persistent buffer, so it moves with .to()
    and a reload re-packs into the same storage) instead of the fp32 weights; a "miopen" one keeps the folded weights and F.conv2d.  Channels-last in
    and out.  run(x, bias, residual, relu): [relu](conv(x) [+ bias] [+ residual]).  level: hip_conv_kind's (2: "conv3x3v", on the "conv3x3d" stream)."""

    def __init__(self, conv, bn, level=1):
        super().__init__()
        w, b = fold_conv_bn(conv, bn)
        self.kind = hip_conv_kind(conv, level)
        self.stride, self.padding, self.dilation = conv.stride, conv.padding, conv.dilation
        self.register_buffer("bias", b)
        if self.kind == "miopen":
            self.register_buffer("weight", w.contiguous(memory_format=torch.channels_last))
            self.register_buffer("packed", None, persistent=False)
        else:
            self.register_buffer("weight", None)
            self.register_buffer("packed", (pack_conv1x1 if self.kind == "conv1x1" else pack_conv3x3d)(w).to(w.device), persistent=False)

    def run(self, x, bias=None, residual=None, relu=True):
        if self.kind == "conv1x1":
            return conv1x1(x, self.packed, self.bias if bias is None else bias, residual, stride=self.stride[0], relu=relu)
        if self.kind == "conv3x3d" and residual is None:
            return conv3x3d(x, self.packed, bias, dilation=self.dilation[0], relu=relu)
        if self.kind == "conv3x3v" and residual is None:
            return conv3x3v(x, self.packed, bias, stride=self.stride[0], relu=relu)
        if self.kind != "miopen":
            raise ValueError("hdn_conv3x3d_f32 / hdn_conv3x3v_f32 take no residual")
        y = F.conv2d(x, self.weight, None, self.stride, self.padding, self.dilation).contiguous(memory_format=torch.channels_last)
        if relu:
            return bias_relu_(y, bias, residual)
        if residual is not None:
            raise ValueError("a residual without the ReLU has no fused pass")
        return y if bias is None else y.add_(bias.view(1, -1, 1, 1))

    def forward(self, x):
        """conv + shift, NCHW-agnostic in, channels-last out (a neck level)."""
        if not x.is_contiguous(memory_format=torch.channels_last):
            x = x.contiguous(memory_format=torch.channels_last)
        return self.run(x, self.bias, relu=False)


class HipBottleneck(nn.Module):
    """Bottleneck.forward (resnet_atrous.py:87-108) of a block whose BatchNorms are folded, channels-last inside: conv1 + shift + ReLU and conv3 + shift +
    residual + ReLU as one hdn_conv1x1_f32 launch each (as hdn_amd.trunk.FusedBottleneck fuses them), conv2 + shift + ReLU as one hdn_conv3x3d_f32 launch;
    a 1x1 downsample branch is a hdn_conv1x1_f32 launch with its own shift, a 3x3 one a bias-free hdn_conv3x3d_f32 launch whose shift rides in the last
    bias (b3).  A convolution without a kernel (hip_conv_kind: "miopen") runs bias-free on F.conv2d with one hdn_bias_relu_f32 pass behind it.
    level 2: a padding-0 3x3 conv2 / skip runs on hdn_conv3x3v_f32 the same way (conv2 with its shift and ReLU, the skip bias-free)."""

    def __init__(self, blk, level=1):
        super().__init__()
        for name in ("conv1", "bn1", "conv2", "bn2", "conv3", "bn3"):
            if not hasattr(blk, name):
                raise ValueError(f"not a Bottleneck: no {name}")
        self.c1, self.c2, self.c3 = _HipConv(blk.conv1, blk.bn1, level), _HipConv(blk.conv2, blk.bn2, level), _HipConv(blk.conv3, blk.bn3, level)
        down = getattr(blk, "downsample", None)
        if down is None:
            self.cd = None
            self.register_buffer("b3", self.c3.bias.clone())
        else:
            pair = _conv_bn_pair(down)
            if pair is None:
                raise ValueError("Bottleneck.downsample is not Sequential(Conv2d, BatchNorm2d)")
            self.cd = _HipConv(*pair, level)
            # a 1x1 branch adds its own shift in its launch; any other hands it to the last pass: (b3 + b_downsample) once
            self.register_buffer("b3", self.c3.bias.clone() if self.cd.kind == "conv1x1" else self.c3.bias + self.cd.bias)

    def forward(self, x):
        y = self.c2.run(self.c1.run(x, self.c1.bias), self.c2.bias)
        if self.cd is None:
            idt = x
        elif self.cd.kind == "conv1x1":
            idt = self.cd.run(x, self.cd.bias, relu=False)
        else:
            idt = self.cd.run(x, None, relu=False)
        return self.c3.run(y, self.b3, idt)


class HipAtrousResNet(FusedAtrousResNet):
    """FusedAtrousResNet with HipBottleneck blocks: the 7x7 stem and the maxpool as there (MIOpen + hdn_bias_relu_f32), the activation converted to
    channels-last once behind the maxpool; the feature levels come out channels-last (the necks take them as they are)."""

    block = HipBottleneck

    def stem(self, x):
        x_, p = super().stem(x)
        return x_, p.contiguous(memory_format=torch.channels_last)


def _bottleneck_level2(blk):
    return HipBottleneck(blk, level=2)


class HipAtrousResNetFull(HipAtrousResNet):
    """Level 2 of the HIP form: HipBottleneck blocks at level 2 (no "miopen" convolution left in the reference's layout) and, where simi_stem_ok(net),
    conv1 + shift + ReLU + maxpool as one hdn_simi_stem_f32 launch on the NCHW input, channels-last out: the packed stream is a non-persistent buffer
    (`stem_packed`; state_dict keys unchanged, a reload re-packs into the same storage), the folded shift is c1.bias.  A network the fused stem does not
    serve — and an input that is not square with a side of 7 .. ops.SIMI_STEM_MAX_SIDE — runs the level-1 stem."""

    block = staticmethod(_bottleneck_level2)

    def __init__(self, net):
        super().__init__(net)
        self.fused_stem = simi_stem_ok(net)
        self.register_buffer("stem_packed", pack_simi_stem(self.c1.weight).to(self.c1.weight.device) if self.fused_stem else None, persistent=False)

    def stem(self, x):
        if not (self.fused_stem and x.dim() == 4 and x.shape[2] == x.shape[3] and 7 <= x.shape[2] <= SIMI_STEM_MAX_SIDE):
            return super().stem(x)
        return None, simi_stem(x.contiguous(), self.stem_packed, self.c1.bias)       # (simi_stem_ok: 0 is not in used_layers)


_BACKBONE_FORMS = (FusedAtrousResNet, HipAtrousResNet, HipAtrousResNetFull)       # by level


class _HipNeck(nn.Module):
    """A neck whose Sequential(Conv2d, BatchNorm2d) levels are _HipConv (hdn_conv1x1_f32, relu = 0); what the module's own forward returns (after
    its crop) is made NCHW-contiguous, so that everything downstream sees the layout it sees without the switch."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, feats):
        out = self.inner(feats)
        if torch.is_tensor(out):
            return out.contiguous()
        return type(out)(o.contiguous() if torch.is_tensor(o) else o for o in out)


def hip_necks(module: nn.Module) -> nn.Module:
    """fold_sequentials with the folded levels on hdn_conv1x1_f32 (a level whose convolution has no kernel stays a _FoldedConv)."""
    return _HipNeck(fold_sequentials(module, hip=True))


# ---------------------------------------------------------------------------------------------------------------- in-place switch
_FUSED, _ORIG_CLASS, _HOOK, _BUILD = "_hdn_fused", "_hdn_orig_class", "_hdn_reload_hook", "_hdn_fused_builder"


def _use_fused(mod, x) -> bool:
    fused = mod.__dict__.get(_FUSED)
    x0 = x[0] if isinstance(x, (list, tuple)) else x
    return (fused is not None and not mod.training and torch.is_tensor(x0) and x0.is_cuda and x0.dtype == torch.float32
            and next(fused.buffers()).device == x0.device)


def _refold(mod, incompatible_keys=None):
    """load_state_dict post-hook: the folded copy is recomputed from the module's new weights and written INTO the existing folded buffers
    (same storage: captured hipGraphs keep pointing at them).  Round-4 ADVICE: without it the folded weights silently stayed the old
    snapshot's while state_dict() reported the new one."""
    fused, build = mod.__dict__.get(_FUSED), mod.__dict__.get(_BUILD)
    if fused is None or build is None:
        return
    with torch.no_grad():
        fresh = build(mod)
        dst = dict(fused.named_buffers())
        for name, buf in fresh.named_buffers():
            dst[name].copy_(buf.to(dst[name].device))


def _attach(mod: nn.Module, fused: nn.Module, build=None):
    """mod(x) -> fused(x) for CUDA float32 inputs in eval mode, the class's own forward otherwise; parameters, buffers and state_dict of
    `mod` are untouched (the folded copy is not a registered sub-module).  build(mod) -> a fresh folded copy (for the reload hook)."""
    base = mod.__dict__.get(_ORIG_CLASS, type(mod))

    def forward(self, *args, **kw):
        if len(args) == 1 and not kw and _use_fused(self, args[0]):
            return self.__dict__[_FUSED](args[0])
        return base.forward(self, *args, **kw)

    object.__setattr__(mod, _FUSED, fused.eval())
    object.__setattr__(mod, _ORIG_CLASS, base)
    object.__setattr__(mod, _BUILD, build)
    object.__setattr__(mod, _HOOK, mod.register_load_state_dict_post_hook(_refold) if build is not None else None)
    mod.__class__ = type(base.__name__, (base,), {"forward": forward, "__module__": base.__module__})


def _detach(mod: nn.Module):
    base = mod.__dict__.get(_ORIG_CLASS)
    if base is not None:
        mod.__class__ = base
        hook = mod.__dict__.pop(_HOOK, None)
        if hook is not None:
            hook.remove()
        mod.__dict__.pop(_BUILD, None)
        del mod.__dict__[_ORIG_CLASS], mod.__dict__[_FUSED]


def _original_view(mod):
    """`mod` with its own class for the duration of a re-fold (the builders read attributes only, but fold_sequentials deep-copies: the
    copy must not carry the switched class, whose folded attributes are plain dictionary entries)."""
    import copy

    m = copy.copy(mod)
    m.__dict__ = {k: v for k, v in mod.__dict__.items() if k not in (_FUSED, _ORIG_CLASS, _HOOK, _BUILD)}
    m.__class__ = mod.__dict__.get(_ORIG_CLASS, type(mod))
    return m


def _build_backbone(mod, hip=False):
    dev = next(mod.parameters()).device
    return _BACKBONE_FORMS[int(hip)](_original_view(mod)).to(dev)


def _build_neck(mod, hip=False):
    return hip_necks(_original_view(mod)) if hip else fold_sequentials(_original_view(mod))


def optimize_similarity_model(model, strict: bool = False, hip=None) -> list:
    """Fold / fuse model.backbone, model.neck, model.neck_lp (the reference's ModelBuilder attributes, model_builder…v2.py:44-60) where
    their structure is the reference's; returns the names that were switched.  strict: raise where the structure is not recognised
    instead of leaving that module as it is.  Eval mode only (BatchNorm statistics are frozen into the weights).
    hip (None: HDN_HIP_BACKBONE, default off): the convolutions on hdn_conv1x1_f32 / hdn_conv3x3d_f32 where they have a kernel (HipAtrousResNet,
    hip_necks); the reload hook re-packs into the same buffers.  hip=2 (HDN_HIP_BACKBONE=2): level 2, the rest of the convolutions on hdn_conv3x3v_f32 and
    the stem on hdn_simi_stem_f32 (HipAtrousResNetFull); True / 1 is level 1, False / 0 is off."""
    import functools

    hip = hip_level() if hip is None else (2 if (hip is not True and hip == 2) else int(bool(hip)))
    build_bb, build_nk = functools.partial(_build_backbone, hip=hip), functools.partial(_build_neck, hip=hip)
    done = []
    with torch.no_grad():
        bb = getattr(model, "backbone", None)
        if isinstance(bb, nn.Module):
            try:
                _detach(bb)
                _attach(bb, _BACKBONE_FORMS[hip](bb), build=build_bb)
                done.append("backbone")
            except ValueError:
                if strict:
                    raise
        for name in ("neck", "neck_lp"):
            nk = getattr(model, name, None)
            if isinstance(nk, nn.Module):
                _detach(nk)
                folded = hip_necks(nk) if hip else fold_sequentials(nk)
                if any(isinstance(m, (_FoldedConv, _HipConv)) for m in folded.modules()):
                    _attach(nk, folded, build=build_nk)
                    done.append(name)
                elif strict:
                    raise ValueError(f"{name}: no Sequential(Conv2d, BatchNorm2d) found")
    return done


def restore_similarity_model(model):
    for name in ("backbone", "neck", "neck_lp"):
        m = getattr(model, name, None)
        if isinstance(m, nn.Module):
            _detach(m)


def enabled() -> bool:
    return os.environ.get("HDN_FOLD_BACKBONE", "1") not in ("", "0")


def hip_enabled() -> bool:
    """HDN_HIP_BACKBONE (default off): optimize_similarity_model's `hip` when the caller does not say."""
    return os.environ.get("HDN_HIP_BACKBONE", "0") not in ("", "0")


def hip_level() -> int:
    """HDN_HIP_BACKBONE as a level: 0 off (unset, "", "0"), 2 for "2", 1 for anything else."""
    v = os.environ.get("HDN_HIP_BACKBONE", "0")
    return 0 if v in ("", "0") else 2 if v.strip() == "2" else 1
