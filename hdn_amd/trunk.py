"""The homography regressor trunk: a 2-channel-input ResNet-34 (or ResNet-50: Bottleneck, resnet50_homo) with BatchNorm folded and its blocks on HIP.

Reference: homo_estimator/Deep_homography/Oneline_DLTv1/backbone/resnet.py:137-194 with
BasicBlock x [3,4,6,3], conv1 = Conv2d(2,64,7,2,3), used_layers=[4] (returns layer4 only).
Parameter names match the reference (conv1, bn1, layerN.M.{conv1,bn1,conv2,bn2,downsample.0,downsample.1})
so its state_dict loads unchanged.  This is a dense MFMA-bound contraction and legitimately a library job
(SURVEY.md §8f rank 4); it is plumbing here, not one of the hand-written kernels.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
# the launch wrappers and packers live in hdn_amd.ops; every name is kept importable from here
from .ops import (ACT_SCALE_LOG2, MATRIX_CORE_CHANNELS, S2_CHANNELS, SIMI_STEM_MAX_SIDE, SPLIT_PIECES, V2_MIN_BATCH, _MC_SIDE,  # noqa: F401
                  LazyAct, _c_pack, _host_f32, bias_relu_, chain_conv, conv1x1, conv3x3_bias_relu, conv3x3d, conv3x3s2, conv3x3s2_ds, conv3x3v,
                  fold_conv_bn, pack_conv1x1, pack_conv3x3, pack_conv3x3_v2, pack_conv3x3d, pack_conv3x3s2, pack_conv3x3s2_ds, pack_conv3x3s2_ds_v2,
                  pack_simi_stem, pack_stem_mfma, simi_stem)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.bn2(self.conv2(y))
        y += idt
        return self.relu(y)


class Bottleneck(nn.Module):
    """backbone/resnet.py:97-133: 1x1 -> 3x3 (stride here) -> 1x1 x 4 channels, the ResNet-50 block."""

    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.relu(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        y += idt
        return self.relu(y)


class HomoResNet(nn.Module):
    def __init__(self, layers=(3, 4, 6, 3), in_channels=2, block=None):
        super().__init__()
        self.block = BasicBlock if block is None else block
        self.inplanes = 64
        self.conv1 = nn.Conv2d(in_channels, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._stage(64, layers[0], 1)
        self.layer2 = self._stage(128, layers[1], 2)
        self.layer3 = self._stage(256, layers[2], 2)
        self.layer4 = self._stage(512, layers[3], 2)
        for m in self.modules():  # resnet.py:154-159
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()

    def _stage(self, planes, blocks, stride):
        blk, out = self.block, planes * self.block.expansion
        down = None
        if stride != 1 or self.inplanes != out:
            down = nn.Sequential(nn.Conv2d(self.inplanes, out, 1, stride, bias=False), nn.BatchNorm2d(out))
        mods = [blk(self.inplanes, planes, stride, down)]
        self.inplanes = out
        mods += [blk(out, planes) for _ in range(1, blocks)]
        return nn.Sequential(*mods)

    act_domain = 0       # 1 on a folded copy whose stages all run in the scaled domain (fold_for_inference): activations are x * 2^-ACT_SCALE_LOG2 inside

    def forward_scaled(self, x):
        """The trunk's output in ITS activation domain (x 2^-8 when act_domain == 1: what hdn_avgpool_fc_f32 takes with in_domain = 1)."""
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return x.finish() if isinstance(x, LazyAct) else x       # (the chained small-batch form of the folded trunk: FusedBasicBlock)

    def forward(self, x):
        x = self.forward_scaled(x)
        return x.mul_(float(1 << ACT_SCALE_LOG2)) if self.act_domain else x      # (a fresh tensor of this forward: in place is safe; exact)


_scale_checked = False


def check_act_scale():
    """The library's compile-time activation scale (hdn_act_scale_log2) against ACT_SCALE_LOG2, until it has matched once: a library built with
    another HDN_ACT_SCALE_LOG2 would take this module's pre-scaled biases and give wrong offsets with no error.  RuntimeError on a mismatch."""
    global _scale_checked
    if _scale_checked:
        return
    got = int(_lib.load().hdn_act_scale_log2())
    if got != ACT_SCALE_LOG2:
        raise RuntimeError(f"libhdn_hip.so was built with HDN_ACT_SCALE_LOG2 = {got}, hdn_amd.trunk scales activations by 2^-{ACT_SCALE_LOG2}: "
                           "rebuild the library, or fold with HDN_TRUNK_SCALED_DOMAIN=0")
    _scale_checked = True


def resnet34_homo():
    return HomoResNet((3, 4, 6, 3))


def resnet50_homo(layers=(3, 4, 6, 3)):
    """backbone/resnet.py:223-231 with conv1 = Conv2d(2, 64, 7, 2, 3) (backbone/__init__.py:28-35): Bottleneck x [3, 4, 6, 3], a [B, 2048, 4, 4]
    output at 127-px crops; the same parameter names as the reference (layerN.M.{conv1,bn1,conv2,bn2,conv3,bn3,downsample.0,downsample.1})."""
    return HomoResNet(layers, block=Bottleneck)


# hdn_trunk_stem_mfma_f32 from this batch on (measured, rocprofv3 kernel time, MI355X, matrix cores / vector pipe: B = 1 8.8 / 12.0 us with cold caches,
# 8: 10.6 / 12.8, 16: 10.8 / 18.9, 32: 12.5 / 31.9, 64: 17.4 / 53.0); HDN_STEM_MFMA_MIN_BATCH: A/B switch
STEM_MFMA_MIN_BATCH = int(os.environ.get("HDN_STEM_MFMA_MIN_BATCH", "1"))


class FusedStem(nn.Module):
    """conv1 + folded bn1 + relu + maxpool of the trunk as ONE HIP kernel (hdn_trunk_stem_f32): the 64-channel 64 x 64 conv output
    never goes through HBM.  Built from a folded conv (weight [64,2,7,7], bias [64]); eval / no-grad only; CUDA tensors only."""

    def __init__(self, conv: nn.Conv2d, channels_last: bool, out_domain: int = 0):
        super().__init__()
        self.out_domain = int(out_domain)        # 1: the output is relu(...) * 2^-ACT_SCALE_LOG2 (the scaled domain of a fully fused trunk)
        if tuple(conv.weight.shape) != (64, 2, 7, 7) or conv.stride != (2, 2) or conv.padding != (3, 3) or conv.bias is None:
            raise ValueError("FusedStem replaces Conv2d(2, 64, 7, 2, 3) with a folded bias")
        self.register_buffer("wT", conv.weight.detach().permute(1, 2, 3, 0).contiguous())  # [ci][ky][kx][co]
        self.register_buffer("b", conv.bias.detach().clone())
        self.register_buffer("wfrag", pack_stem_mfma(conv.weight).to(conv.weight.device))                           # the matrix-core form's weights (28 KB)
        self.channels_last = bool(channels_last)
        self.mfma_disabled = False                                                           # A/B switch (tools/experiments, tests)

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != 2 or x.dtype != self.wT.dtype:
            raise ValueError("FusedStem takes float32 [B,2,H,W]")
        B, _, H, W = x.shape
        if W < 2 or W > 128:  # outside the kernel's range: the same arithmetic through the library
            y = F.conv2d(x, self.wT.permute(3, 0, 1, 2), self.b, stride=2, padding=3)
            y = F.max_pool2d(F.relu(y), 3, 2, 1)
            return y.mul_(2.0 ** -ACT_SCALE_LOG2) if self.out_domain else y
        dev = _lib.require_device(x, self.wT, self.b)
        if self.wfrag.device != dev:
            raise _lib.HdnHipError(f"FusedStem weights on {self.wfrag.device}, input on {dev}")
        xs = x.detach().contiguous()  # NCHW
        Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
        out = torch.empty((B, 64, Hp, Wp), dtype=x.dtype, device=dev,
                          memory_format=torch.channels_last if self.channels_last else torch.contiguous_format)
        if self.channels_last and H == 127 and W == 127 and B >= STEM_MFMA_MIN_BATCH and not self.mfma_disabled:
            _lib.launch("trunk_stem_mfma", dev, _lib.load().hdn_trunk_stem_mfma_f32, _lib.ptr(xs), _lib.ptr(self.wfrag), _lib.ptr(self.b), _lib.ptr(out),
                        B, H, W, self.out_domain)
            return out
        _lib.launch("trunk_stem", dev, _lib.load().hdn_trunk_stem_f32, _lib.ptr(xs), _lib.ptr(self.wT), _lib.ptr(self.b), _lib.ptr(out), B, H, W,
                    1 if self.channels_last else 0)
        return out.mul_(2.0 ** -ACT_SCALE_LOG2) if self.out_domain else out


# Batches up to this run the blocks CHAINED (hdn_conv3x3_chain_f32): at the tracker's B = 1 every launch is a dependent step of ~5 us
# and the launches that only add the K slices up were half of the trunk's 70
CHAIN_MAX_BATCH = 16


class FusedBasicBlock(nn.Module):
    """BasicBlock.forward (backbone/resnet.py:78-94) of the BN-folded trunk with its elementwise tail fused.  Stride-1 3x3
    convolutions of MATRIX_CORE_CHANNELS run, bias / residual / ReLU included, as ONE launch of the split-fp16 matrix-core kernel
    (hdn_conv3x3_bias_relu_f32, channels-last only); every other convolution runs bias-free on MIOpen with `relu(y + b1)` /
    `relu(y + b2 + residual)` as one HIP pass each (hdn_bias_relu_f32).  A folded downsample branch contributes its bias to b2 and
    its raw convolution as the residual.  GPU / eval only."""

    def __init__(self, blk: "BasicBlock", matrix_core: bool = False, act_domain: int = 0):
        super().__init__()
        self.act_domain = int(act_domain)     # 1: input, output and residuals are x * 2^-ACT_SCALE_LOG2 in memory (a fully fused trunk's interior)

        for c in (blk.conv1, blk.conv2) + ((blk.downsample,) if blk.downsample is not None else ()):
            if not isinstance(c, nn.Conv2d) or c.bias is None:
                raise ValueError("FusedBasicBlock takes a block whose BatchNorms were folded into biased convolutions")
        self.stride = blk.conv1.stride
        self.w1 = nn.Parameter(blk.conv1.weight.detach().clone(), requires_grad=False)
        self.w2 = nn.Parameter(blk.conv2.weight.detach().clone(), requires_grad=False)
        self.register_buffer("b1", blk.conv1.bias.detach().clone())
        b2 = blk.conv2.bias.detach().clone()
        if blk.downsample is not None:
            self.wd = nn.Parameter(blk.downsample.weight.detach().clone(), requires_grad=False)
            self.ds_stride = blk.downsample.stride
            b2 = b2 + blk.downsample.bias.detach()     # (b2 + bd) once, instead of per element: differs from the unfused sum by rounding
        else:
            self.wd = None
        self.register_buffer("b2", b2)
        if self.act_domain:      # the biases of the scaled domain (exact: a power of two); b1 / b2 stay the real ones
            self.register_buffer("b1d", self.b1 * 2.0 ** -ACT_SCALE_LOG2, persistent=False)
            self.register_buffer("b2d", self.b2 * 2.0 ** -ACT_SCALE_LOG2, persistent=False)
        # packed split-fp16 weights for the matrix-core kernel (stride 1, C -> C only)
        dev = self.w1.device
        cin, cout = self.w1.shape[1], self.w1.shape[0]
        use1 = matrix_core and self.stride == (1, 1) and cin == cout and cout in MATRIX_CORE_CHANNELS
        use2 = matrix_core and cout in MATRIX_CORE_CHANNELS
        use_s2 = (matrix_core and self.stride == (2, 2) and self.wd is not None and cout == 2 * cin and cout in MATRIX_CORE_CHANNELS
                  and self.ds_stride == (2, 2))
        self.register_buffer("p1", pack_conv3x3(self.w1).to(dev) if use1 else None)
        self.register_buffer("p2", pack_conv3x3(self.w2).to(dev) if use2 else None)
        self.register_buffer("p1s2", pack_conv3x3s2_ds(self.w1, self.wd).to(dev) if use_s2 else None)
        # the large-batch packing of the same weights (pack_conv3x3_v2 / pack_conv3x3s2_ds_v2): buffers like p1 / p2 / p1s2, so that
        # .to() / .cuda() move them with the module and no host round trip happens at the first batch of V2_MIN_BATCH or more
        # (which a stream capture could not hold); non-persistent: state_dict stays the reference's
        self.register_buffer("p1v2", pack_conv3x3_v2(self.w1).to(dev) if use1 else None, persistent=False)
        self.register_buffer("p2v2", pack_conv3x3_v2(self.w2).to(dev) if use2 else None, persistent=False)
        self.register_buffer("p1s2v2", pack_conv3x3s2_ds_v2(self.w1, self.wd).to(dev) if use_s2 else None, persistent=False)

    def _packed_v2(self, which, batch):
        """which: 1 / 2 = the block's stride-1 convolutions, "s2" = the stride-2 convolution + downsample branch."""
        if batch < V2_MIN_BATCH or FusedBasicBlock.v2_disabled or (which == "s2" and FusedBasicBlock.v2_s2_disabled):
            return None
        return {1: self.p1v2, 2: self.p2v2, "s2": self.p1s2v2}[which]

    v2_disabled = False        # A/B switch (tests, tools/experiments)
    v2_s2_disabled = False     # ... of the stride-2 stages' large-batch form alone

    def forward(self, x):
        def shape_ok(t):   # the kernel's shapes: square, side tied to the channel count (127-px crops), channels-last
            return t.is_contiguous(memory_format=torch.channels_last) and t.shape[2] == t.shape[3] == _MC_SIDE.get(t.shape[1], -1)

        chained = self._chained(x)
        if chained is not None:
            return chained
        dom = self.act_domain
        b1, b2 = (self.b1d, self.b2d) if dom else (self.b1, self.b2)
        if isinstance(x, LazyAct):
            x = x.finish()
        if (self.p1s2 is not None and x.is_contiguous(memory_format=torch.channels_last)
                and x.shape[2] == x.shape[3] == 2 * _MC_SIDE.get(2 * x.shape[1], -1)):
            y, idt = conv3x3s2_ds(x, self.p1s2, b1, wpacked_v2=self._packed_v2("s2", x.shape[0]), act_domain=dom)   # stride-2 convolution + the downsample branch from one staged input
        else:
            if self.p1 is not None and shape_ok(x):
                y = conv3x3_bias_relu(x, self.p1, b1, wpacked_v2=self._packed_v2(1, x.shape[0]), act_domain=dom)
            else:
                y = bias_relu_(F.conv2d(x, self.w1, None, self.stride, 1), b1)       # (linear + ReLU: the same in either domain, with the domain's bias)
            idt = x if self.wd is None else F.conv2d(x, self.wd, None, self.ds_stride)
        if self.p2 is not None and shape_ok(y) and idt.is_contiguous(memory_format=torch.channels_last):
            return conv3x3_bias_relu(y, self.p2, b2, idt, wpacked_v2=self._packed_v2(2, y.shape[0]), act_domain=dom)
        return bias_relu_(F.conv2d(y, self.w2, None, 1, 1), b2, idt)

    chain_disabled = False     # A/B switch for every block at once (tests, tools/experiments)

    def _chained(self, x):
        """The block as two chained launches (None: not this input).  A LazyAct in: the previous block's output, finished while conv1
        stages it (and written out once, as this block's residual); a LazyAct out."""
        lazy = isinstance(x, LazyAct)
        if self.p2 is None or getattr(self, "_hdn_no_chain", False) or FusedBasicBlock.chain_disabled:
            return None
        B, C, S, S2 = x.shape
        if not lazy and not (x.is_cuda and x.dtype == torch.float32 and B <= CHAIN_MAX_BATCH and x.is_contiguous(memory_format=torch.channels_last)):
            return None
        dom = self.act_domain
        b1, b2 = (self.b1d, self.b2d) if dom else (self.b1, self.b2)
        if self.p1s2 is not None and S == S2 == 2 * _MC_SIDE.get(2 * C, -1):
            s1, sd, _ = chain_conv(x, self.p1s2, 2, act_domain=dom)
            s2, _, _ = chain_conv(LazyAct(s1, b1), self.p2, act_domain=dom)
            return LazyAct(s2, b2, sd)
        if self.p1 is not None and self.wd is None and S == S2 == _MC_SIDE.get(C, -1):
            s1, _, idt = chain_conv(x, self.p1, 1, want_x=True, act_domain=dom)
            s2, _, _ = chain_conv(LazyAct(s1, b1), self.p2, act_domain=dom)
            return LazyAct(s2, b2, idt if lazy else x)
        return None


class FusedBottleneck(nn.Module):
    """Bottleneck.forward (backbone/resnet.py:113-133) of the BN-folded homography trunk: conv1 1x1 + bias + ReLU, conv2 3x3 + bias + ReLU,
    conv3 1x1 + bias + residual + ReLU, the residual being the input or the folded downsample branch (1x1 / stride, bias, no ReLU).  The 1x1
    convolutions are one hdn_conv1x1_f32 launch each (channels-last; an NCHW input is converted once).  conv2 runs on the split-fp16 matrix-core
    kernels where it has one: hdn_conv3x3_bias_relu_f32 for stride 1 (MATRIX_CORE_CHANNELS at their side: 13 of the 16 blocks of a ResNet-50) and
    hdn_conv3x3s2_f32 for stride 2 / padding 1 (S2_CHANNELS at twice their side: the first block of layer2 / 3 / 4), so a folded ResNet-50 trunk at
    127-px crops makes no MIOpen call.  Any other conv2 runs bias-free on MIOpen followed by one hdn_bias_relu_f32 pass, as FusedBasicBlock does for
    shapes without a kernel.  GPU / eval only."""

    def __init__(self, blk: "Bottleneck", matrix_core: bool = False, act_domain: int = 0):
        super().__init__()
        self.act_domain = int(act_domain)
        convs = (blk.conv1, blk.conv2, blk.conv3) + ((blk.downsample,) if blk.downsample is not None else ())
        for c in convs:
            if not isinstance(c, nn.Conv2d) or c.bias is None:
                raise ValueError("FusedBottleneck takes a block whose BatchNorms were folded into biased convolutions")
        dev = blk.conv1.weight.device
        self.stride = blk.conv2.stride
        self.w2 = nn.Parameter(blk.conv2.weight.detach().clone(), requires_grad=False)
        # packed weights are buffers: .to() / .cuda() move them with the module, no host round trip inside a forward (or a stream capture);
        # non-persistent, like FusedBasicBlock's large-batch streams
        self.register_buffer("p1", pack_conv1x1(blk.conv1.weight).to(dev), persistent=False)
        self.register_buffer("p3", pack_conv1x1(blk.conv3.weight).to(dev), persistent=False)
        self.register_buffer("pd", pack_conv1x1(blk.downsample.weight).to(dev) if blk.downsample is not None else None, persistent=False)
        self.ds_stride = blk.downsample.stride[0] if blk.downsample is not None else 1
        planes = self.w2.shape[0]
        use2 = matrix_core and self.stride == (1, 1) and self.w2.shape[1] == planes and planes in MATRIX_CORE_CHANNELS
        self.register_buffer("p2", pack_conv3x3(self.w2).to(dev) if use2 else None, persistent=False)
        self.register_buffer("p2v2", pack_conv3x3_v2(self.w2).to(dev) if use2 else None, persistent=False)
        use_s2 = matrix_core and self.stride == (2, 2) and blk.conv2.padding == (1, 1) and self.w2.shape[1] == planes and planes in S2_CHANNELS
        self.register_buffer("p2s2", pack_conv3x3s2(self.w2).to(dev) if use_s2 else None, persistent=False)
        for name, c in (("b1", blk.conv1), ("b2", blk.conv2), ("b3", blk.conv3), ("bd", blk.downsample)):
            b = c.bias.detach().clone() if c is not None else None
            self.register_buffer(name, b)
            if self.act_domain:       # the biases of the scaled domain (exact: a power of two); b1 .. bd stay the real ones
                self.register_buffer(name + "d", b * 2.0 ** -ACT_SCALE_LOG2 if b is not None else None, persistent=False)

    def forward(self, x):
        cl = torch.channels_last
        dom = self.act_domain
        b1, b2, b3, bd = (self.b1d, self.b2d, self.b3d, self.bdd) if dom else (self.b1, self.b2, self.b3, self.bd)
        if isinstance(x, LazyAct):
            x = x.finish()
        if not x.is_contiguous(memory_format=cl):
            x = x.contiguous(memory_format=cl)
        y = conv1x1(x, self.p1, b1, relu=True, act_domain=dom)
        C, S = y.shape[1], y.shape[2]
        if self.p2 is not None and S == y.shape[3] == _MC_SIDE.get(C, -1):
            v2 = self.p2v2 if (y.shape[0] >= V2_MIN_BATCH and not FusedBasicBlock.v2_disabled) else None
            y = conv3x3_bias_relu(y, self.p2, b2, wpacked_v2=v2, act_domain=dom)
        elif self.p2s2 is not None and S == y.shape[3] == 2 * _MC_SIDE[C]:
            y = conv3x3s2(y, self.p2s2, b2, act_domain=dom)
        else:
            y = bias_relu_(F.conv2d(y, self.w2, None, self.stride, 1).contiguous(memory_format=cl), b2)   # (linear + ReLU: either domain, its bias)
        idt = x if self.pd is None else conv1x1(x, self.pd, bd, stride=self.ds_stride, relu=False, act_domain=dom)
        return conv1x1(y, self.p3, b3, residual=idt, relu=True, act_domain=dom)


def _is_conv(m, k):
    return isinstance(m, nn.Conv2d) and m.kernel_size == (k, k) and m.groups == 1 and m.dilation == (1, 1)


def block_kind(blk) -> str:
    """"basic" (BasicBlock: conv1 / bn1 / conv2 / bn2, both 3x3) or "bottleneck" (conv1 1x1 / conv2 3x3 / conv3 1x1 with bn1 .. bn3), matched by
    attribute layout (so the reference's own classes pass); the downsample branch is None or Sequential(Conv2d 1x1, BatchNorm2d).  Anything else:
    ValueError (the fold and the fused blocks would silently drop what they do not know)."""
    bn = lambda m: isinstance(m, nn.BatchNorm2d)
    ds = getattr(blk, "downsample", None)
    ds_ok = ds is None or (isinstance(ds, nn.Sequential) and len(ds) == 2 and _is_conv(ds[0], 1) and ds[0].padding == (0, 0) and bn(ds[1]))
    names = {n for n, _ in blk.named_children()}
    known = {"conv1", "bn1", "conv2", "bn2", "relu", "downsample"}
    if (ds_ok and names <= known | {"conv3", "bn3"} and _is_conv(getattr(blk, "conv1", None), 3) and _is_conv(getattr(blk, "conv2", None), 3)
            and bn(getattr(blk, "bn1", None)) and bn(getattr(blk, "bn2", None)) and getattr(blk, "conv3", None) is None and getattr(blk, "bn3", None) is None):
        return "basic"
    if (ds_ok and names <= known | {"conv3", "bn3"} and _is_conv(getattr(blk, "conv1", None), 1) and _is_conv(getattr(blk, "conv2", None), 3)
            and _is_conv(getattr(blk, "conv3", None), 1) and all(bn(getattr(blk, n, None)) for n in ("bn1", "bn2", "bn3"))
            and blk.conv1.stride == (1, 1) and blk.conv3.stride == (1, 1)):
        return "bottleneck"
    raise ValueError(f"{type(blk).__name__}: neither a BasicBlock nor a Bottleneck by its attributes ({sorted(names)}); the trunk fold does not take it")


def trunk_block_kinds(net) -> list:
    """block_kind of every block of layer1 .. layer4 (ValueError for a trunk without them or with an unknown block)."""
    kinds = []
    for name in ("layer1", "layer2", "layer3", "layer4"):
        layer = getattr(net, name, None)
        if not isinstance(layer, nn.Sequential):
            raise ValueError(f"trunk has no {name} Sequential")
        kinds += [block_kind(blk) for blk in layer]
    return kinds


def fold_for_inference(net: HomoResNet, channels_last: bool = True, fused_stem: bool = False, fused_epilogue: bool = False,
                       matrix_core: bool = None) -> nn.Module:
    """A copy of `net` with every eval-mode BatchNorm folded into the preceding convolution (weights scaled in
    float64, rounded once) and, optionally, NHWC weights for MIOpen's channels-last kernels.  Measured on MI355X at
    B=64: 2.92 ms (as-is) -> 2.47 ms (folded) -> 2.11 ms (folded + NHWC); outputs agree with the un-folded CPU
    trunk to ~1.5e-6 relative either way (tools/experiments/exp_trunk.py).  The copy does not track later weight changes.
    fused_stem: replace conv1 / relu / maxpool by FusedStem (GPU only, W <= 128).
    fused_epilogue: replace every BasicBlock by FusedBasicBlock (GPU only): 83 elementwise launches per forward -> 32; every Bottleneck by
    FusedBottleneck (its 1x1 convolutions on hdn_conv1x1_f32).  A block that is neither (block_kind) raises ValueError.
    matrix_core (default: fused_epilogue and channels_last): the stride-1 3x3 convolutions of MATRIX_CORE_CHANNELS as one launch of
    the split-fp16 matrix-core kernel each, epilogue included (and a Bottleneck's stride-2 ones: hdn_conv3x3s2_f32).
    With every stage fused the interior runs in the scaled activation domain; the library's scale constant is checked first (check_act_scale)."""
    import copy

    trunk_block_kinds(net)
    net = copy.deepcopy(net).eval()

    def fuse(conv, bn):
        out = nn.Conv2d(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding, bias=True)
        out = out.to(conv.weight.device)
        out.weight.data, out.bias.data = fold_conv_bn(conv, bn)
        return out

    net.conv1, net.bn1 = fuse(net.conv1, net.bn1), nn.Identity()
    for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
        for blk in layer:
            blk.conv1, blk.bn1 = fuse(blk.conv1, blk.bn1), nn.Identity()
            blk.conv2, blk.bn2 = fuse(blk.conv2, blk.bn2), nn.Identity()
            if hasattr(blk, "conv3"):                                       # a Bottleneck (trunk_block_kinds above)
                blk.conv3, blk.bn3 = fuse(blk.conv3, blk.bn3), nn.Identity()
            if blk.downsample is not None:
                blk.downsample = fuse(blk.downsample[0], blk.downsample[1])
    for p in net.parameters():
        p.requires_grad_(False)
    if channels_last:
        net = net.to(memory_format=torch.channels_last)
    mc = bool(channels_last) if matrix_core is None else bool(matrix_core)
    # every stage fused and on the matrix cores: the interior runs in the scaled activation domain (ACT_SCALE_LOG2 above)
    dom = 1 if (fused_epilogue and fused_stem and mc and channels_last and os.environ.get("HDN_TRUNK_SCALED_DOMAIN", "1") not in ("", "0")) else 0
    if dom:
        check_act_scale()
    if fused_epilogue:
        for name in ("layer1", "layer2", "layer3", "layer4"):
            setattr(net, name, nn.Sequential(*[(FusedBottleneck if hasattr(blk, "conv3") else FusedBasicBlock)(blk, mc, act_domain=dom)
                                               for blk in getattr(net, name)]))
        if channels_last:
            net = net.to(memory_format=torch.channels_last)
    if fused_stem:  # conv1 (+ folded bn1) + relu + maxpool in one HIP kernel; the stages behind it stay on MIOpen
        net.conv1 = FusedStem(net.conv1, channels_last, out_domain=dom)
        net.relu, net.maxpool = nn.Identity(), nn.Identity()
    net.act_domain = dom
    return net
