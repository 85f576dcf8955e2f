"""BatchNorm2d on batch statistics followed by ReLU, in training, on HIP (hdn/models/head/ban.py:55-64, ban_lp.py:17-26: the pair between a head
branch's 3x3 convolution and its correlation):

    forward(...) / backward(...)         raw wrappers of hdn_bn_relu_train_fwd_f32 / hdn_bn_relu_train_bwd_f32
    batchnorm_relu_train(c, weight, ...) autograd Function: reads channels-last (what conv3x3_valid returns), writes NCHW (what the correlation takes);
                                         its backward reads the NCHW gradient and writes channels-last (what _Conv3x3Valid.backward takes)
    qualifies(bn, x)                     is `bn` a BatchNorm2d the kernels restate?

Nothing is allocated outside torch's caching allocator, nothing is uploaded and nothing is read back: forward and backward can be captured into a
hipGraph, and the running buffers advance on every replay.  There is no CPU fallback (_lib.require_device).
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib

launches = {"forward": 0, "backward": 0}   # calls made, for tests ("launches only what is asked")

CL = torch.channels_last


def _cl(t):
    """t [B, C, H, W] with channels-last strides (the NHWC image dense in memory), copied if it is not."""
    return t if t.is_contiguous(memory_format=CL) and t.stride(1) == 1 else t.contiguous(memory_format=CL)


def _in_layout(t, nchw):
    if nchw:
        return t if t.is_contiguous() else t.contiguous()
    return _cl(t)


def _dims(c):
    if c.dim() != 4:
        raise ValueError("batchnorm_relu_train: c [B, C, H, W]")
    B, C, H, W = (int(s) for s in c.shape)
    if B * H * W < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(c.shape)}")
    return B, H * W, C


def _empty(shape, dev, nchw):
    return torch.empty(shape, dtype=torch.float32, device=dev, memory_format=torch.contiguous_format if nchw else CL)


def forward(c, weight, bias, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, relu=True, out_nchw=True, out=None, stats=None):
    """(y, stats) of hdn_bn_relu_train_fwd_f32: c channels-last [B, C, H, W]; y contiguous NCHW (out_nchw) or channels-last; stats = mean[C], invstd[C].
    The running buffers, when given, are updated in place."""
    dev = _lib.require_device(c, weight, bias, *[t for t in (running_mean, running_var) if t is not None])
    B, P, C = _dims(c)
    lib = _lib.load()
    ws, nws = _lib.workspace("batchnorm_relu_train", lib.hdn_bn_relu_train_workspace_bytes(B, P, C), dev)
    y = _empty(tuple(c.shape), dev, out_nchw) if out is None else out
    stats = torch.empty(2 * C, dtype=torch.float32, device=dev) if stats is None else stats
    launches["forward"] += 1
    _lib.launch("bn_relu_train_fwd", dev, lib.hdn_bn_relu_train_fwd_f32, _lib.ptr(c), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(y), _lib.ptr(stats),
                _lib.opt(running_mean), _lib.opt(running_var), float(momentum), float(eps), _lib.opt(ws), nws, B, P, C, int(bool(relu)), int(bool(out_nchw)))
    return y, stats


def backward(dy, c, weight, bias, stats, relu=True, dy_nchw=True, need=(True, True, True)):
    """(dc, dgamma, dbeta) of hdn_bn_relu_train_bwd_f32, None where `need` says so; dc channels-last."""
    dev = _lib.require_device(dy, c, weight, bias, stats)
    B, P, C = _dims(c)
    lib = _lib.load()
    ws, nws = _lib.workspace("batchnorm_relu_train backward", lib.hdn_bn_relu_train_workspace_bytes(B, P, C), dev)
    dc = _empty(tuple(c.shape), dev, False) if need[0] else None
    dgamma = torch.empty(C, dtype=torch.float32, device=dev) if need[1] else None
    dbeta = torch.empty(C, dtype=torch.float32, device=dev) if need[2] else None
    launches["backward"] += 1
    _lib.launch("bn_relu_train_bwd", dev, lib.hdn_bn_relu_train_bwd_f32, _lib.ptr(dy), _lib.ptr(c), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(stats),
                _lib.opt(dc), _lib.opt(dgamma), _lib.opt(dbeta), _lib.opt(ws), nws, B, P, C, int(bool(relu)), int(bool(dy_nchw)))
    return dc, dgamma, dbeta


class _BatchNormReluTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, c, weight, bias, running_mean, running_var, momentum, eps, relu, out_nchw):
        c = _cl(c)
        w, b = weight.contiguous(), bias.contiguous()
        y, stats = forward(c, w, b, running_mean, running_var, momentum, eps, relu, out_nchw)
        ctx.save_for_backward(c, w, b, stats)
        ctx.relu, ctx.out_nchw = bool(relu), bool(out_nchw)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        c, w, b, stats = ctx.saved_tensors
        need = tuple(ctx.needs_input_grad[:3])
        if not any(need):
            return (None, ) * 9
        dc, dgamma, dbeta = backward(_in_layout(dy, ctx.out_nchw), c, w, b, stats, ctx.relu, ctx.out_nchw, need)
        return (dc, dgamma, dbeta) + (None, ) * 6


def batchnorm_relu_train(c, weight, bias, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, relu=True, out_nchw=True):
    """F.relu(F.batch_norm(c, running_mean, running_var, weight, bias, training=True, momentum, eps)) (without the ReLU: relu=False), differentiable
    once, on HIP.  c [B, C, H, W] float32 on the device (made channels-last if it is not), C a multiple of 32, at most 2048.  Returns a contiguous
    NCHW tensor (out_nchw) or a channels-last one.  running_mean / running_var: both None, or updated in place."""
    tensors = [t for t in (running_mean, running_var) if t is not None]
    _lib.require_device(c, weight, bias, *tensors)
    if len(tensors) == 1:
        raise ValueError("batchnorm_relu_train: running_mean and running_var, both or neither")
    _dims(c)
    return _BatchNormReluTrain.apply(c, weight, bias, running_mean, running_var, momentum, eps, relu, out_nchw)


def qualifies(bn, x=None) -> bool:
    """Is `bn` a BatchNorm2d batchnorm_relu_train restates: affine, fp32 on the device, a momentum (no cumulative average), num_features a multiple
    of 32 and at most 2048, tracking running statistics or holding none at all (and x, when given, an fp32 [B, C, H, W] map on the same device)?"""
    ok = restates(bn) and bn.weight.is_cuda
    if ok and x is not None:
        ok = x.dim() == 4 and x.dtype == torch.float32 and x.device == bn.weight.device and x.shape[1] == bn.num_features
    return bool(ok)


def restates(bn) -> bool:
    """qualifies() without the device: every condition on the module itself."""
    if not isinstance(bn, torch.nn.BatchNorm2d) or not bn.affine or bn.weight is None or bn.bias is None:
        return False
    tracked = bn.track_running_stats and bn.running_mean is not None and bn.running_var is not None
    untracked = not bn.track_running_stats and bn.running_mean is None and bn.running_var is None
    ok = (bn.weight.dtype == torch.float32 and bn.bias.dtype == torch.float32 and bn.momentum is not None
          and bn.num_features % 32 == 0 and bn.num_features <= 2048 and (tracked or untracked))
    if ok and tracked:
        ok = bn.running_mean.dtype == torch.float32 and bn.running_var.dtype == torch.float32
    return bool(ok)
