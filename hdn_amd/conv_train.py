"""The heads' 3x3 convolutions in training (hdn/models/head/ban.py:55-64, ban_lp.py:17-26: Conv2d(CI, CO, 3, bias=False), stride 1, padding 0) on HIP:

    conv3x3_valid(x, weight)                 autograd Function: forward hdn_conv3x3v_f32, backward hdn_conv3x3v_dgrad_f32 / hdn_conv3x3v_wgrad_f32
    depthwise_xcorr_train_forward(...)       DepthwiseXCorr.forward / DepthwiseXCorrCirc.forward (ban.py:73-78, ban_lp.py:35-40) with the two 3x3
                                             convolutions on conv3x3_valid and, while install.HEAD_BN_TRAIN_BOUND, their BatchNorm + ReLU on
                                             bn_train.batchnorm_relu_train; the correlation and the 1x1 tail are the modules' own

The weight streams are rebuilt ON THE DEVICE by hdn_pack_conv3x3d_dev_f32 at every call: a replayed optimizer step changes the weight's bytes in place,
which no version counter sees, so nothing about a weight is cached but the BUFFER its stream is written to.  After the first call of a shape nothing is
allocated outside torch's caching allocator, nothing is uploaded and nothing is read back: forward and backward can be captured into a hipGraph.
There is no CPU fallback (_lib.require_device).
"""
from __future__ import annotations

import torch

from . import _lib, bn_train

_cache = {}   # (device index, what, CO, CI[, B, S]) -> persistent device buffer (packed streams, the exponent, the packer's counter)
launches = {"pack": 0, "forward": 0, "scale": 0, "dgrad": 0, "wgrad": 0}   # calls made, for tests ("launches only what is asked")


def _buffer(dev, key, nbytes, dtype=torch.uint8):
    k = (dev.index, ) + key
    buf = _cache.get(k)
    if buf is None:
        n = nbytes if dtype == torch.uint8 else nbytes // 4
        buf = _cache[k] = torch.zeros(n, dtype=dtype, device=dev)
    return buf


def bad_weight_count(dev) -> int:
    """How many weights the device packer has met on `dev` that the host packers would have refused (|w| >= 65,504 or NaN) since the last call of
    this function.  Reads the device: not inside a capture."""
    c = _buffer(torch.device(dev), ("bad", ), 4, torch.int32)
    n = int(c.item())
    c.zero_()
    return n


def pack_dev(weight, mode, out=None, count=True):
    """The stream of hdn_conv3x3v_f32 (mode 0) or hdn_conv3x3v_dgrad_f32 (mode 1) from weight [CO, CI, 3, 3] on the device, written into the cached
    buffer of (device, mode, CO, CI) (or `out`)."""
    dev = _lib.require_device(weight)
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or not weight.is_contiguous():
        raise ValueError("pack_dev: contiguous float32 [CO, CI, 3, 3]")
    CO, CI = int(weight.shape[0]), int(weight.shape[1])
    lib = _lib.load()
    nbytes = lib.hdn_pack_conv3x3d_bytes(CO, CI)
    if nbytes < 0:
        _lib.check(int(nbytes), "pack_dev")
    if out is None:
        out = _buffer(dev, ("stream", int(mode), CO, CI), nbytes)
    bad = _buffer(dev, ("bad", ), 4, torch.int32) if count else None
    launches["pack"] += 1
    _lib.launch("pack_conv3x3d_dev", dev, lib.hdn_pack_conv3x3d_dev_f32, _lib.ptr(weight), CO, CI, int(mode), _lib.ptr(out), nbytes, _lib.opt(bad))
    return out


def grad_scale(g, out=None):
    """The int32 device scalar e with amax|g| 2^e in [2^14, 2^15) (hdn_grad_scale_f32)."""
    dev = _lib.require_device(g)
    if out is None:
        out = torch.empty(1, dtype=torch.int32, device=dev)
    launches["scale"] += 1
    _lib.launch("grad_scale", dev, _lib.load().hdn_grad_scale_f32, _lib.ptr(g), g.numel(), _lib.ptr(out))
    return out


def _cl(t):
    """t [B, C, H, W] with channels-last strides (the NHWC image dense in memory), copied if it is not."""
    return t if t.is_contiguous(memory_format=torch.channels_last) and t.stride(1) == 1 else t.contiguous(memory_format=torch.channels_last)


def _empty_cl(shape, dev):
    return torch.empty(shape, dtype=torch.float32, device=dev, memory_format=torch.channels_last)


def _dims(x, weight):
    if x.dim() != 4 or x.shape[2] != x.shape[3] or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or weight.shape[1] != x.shape[1]:
        raise ValueError("conv3x3_valid: x [B, CI, S, S] and weight [CO, CI, 3, 3]")
    return int(x.shape[0]), int(x.shape[2]), int(x.shape[1]), int(weight.shape[0])


def forward(x, weight):
    """hdn_conv3x3v_f32(stride 1, no bias, no ReLU) on the stream packed from `weight` now; x channels-last [B, CI, S, S] -> channels-last [B, CO, S-2, S-2]."""
    dev = _lib.require_device(x, weight)
    B, S, CI, CO = _dims(x, weight)
    lib = _lib.load()
    ws, nws = _lib.workspace("conv3x3_valid", lib.hdn_conv3x3v_workspace_bytes(B, S, CI, CO, 1), dev)
    wp = pack_dev(weight, 0)
    out = _empty_cl((B, CO, S - 2, S - 2), dev)
    launches["forward"] += 1
    _lib.launch("conv3x3v", dev, lib.hdn_conv3x3v_f32, _lib.ptr(x), _lib.ptr(wp), None, _lib.ptr(out), _lib.opt(ws), nws, B, S, CI, CO, 1, 0, 0)
    return out


def dgrad(dy, weight, exp, S, out=None):
    """gx [B, CI, S, S] (channels-last; written to `out` when given) from dy [B, CO, S-2, S-2] (channels-last), the plain weight and dy's exponent."""
    dev = _lib.require_device(dy, weight)
    CO, CI, B = int(weight.shape[0]), int(weight.shape[1]), int(dy.shape[0])
    lib = _lib.load()
    ws, nws = _lib.workspace("conv3x3_valid dgrad", lib.hdn_conv3x3v_dgrad_workspace_bytes(B, S, CI, CO), dev)
    wt = pack_dev(weight, 1)
    gx = _empty_cl((B, CI, S, S), dev) if out is None else out
    launches["dgrad"] += 1
    _lib.launch("conv3x3v_dgrad", dev, lib.hdn_conv3x3v_dgrad_f32, _lib.ptr(dy), _lib.ptr(wt), _lib.ptr(exp), _lib.ptr(gx), _lib.opt(ws), nws, B, S, CI, CO)
    return gx


def wgrad(x, dy, exp, out=None):
    """gw [CO, CI, 3, 3] from x [B, CI, S, S] and dy [B, CO, S-2, S-2] (both channels-last) and dy's exponent."""
    dev = _lib.require_device(x, dy)
    B, CI, S = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    CO = int(dy.shape[1])
    lib = _lib.load()
    ws, nws = _lib.workspace("conv3x3_valid wgrad", lib.hdn_conv3x3v_wgrad_workspace_bytes(B, S, CI, CO), dev)
    gw = torch.empty((CO, CI, 3, 3), dtype=torch.float32, device=dev) if out is None else out
    launches["wgrad"] += 1
    _lib.launch("conv3x3v_wgrad", dev, lib.hdn_conv3x3v_wgrad_f32, _lib.ptr(x), _lib.ptr(dy), _lib.ptr(exp), _lib.ptr(gw), _lib.opt(ws), nws, B, S, CI, CO)
    return gw


class _Conv3x3Valid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        x = _cl(x)
        w = weight.contiguous()
        ctx.save_for_backward(x, w)
        return forward(x, w)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad
        if not (need_x or need_w):
            return None, None
        dy = _cl(dy)
        exp = grad_scale(dy)
        gx = dgrad(dy, w, exp, int(x.shape[2])) if need_x else None
        gw = wgrad(x, dy, exp) if need_w else None
        return gx, gw


def conv3x3_valid(x, weight):
    """F.conv2d(x, weight) for a 3x3 weight (stride 1, padding 0, no bias), differentiable, on HIP.  x [B, CI, S, S] float32 on the device (made
    channels-last if it is not), weight [CO, CI, 3, 3]; CI and CO multiples of 32.  Returns channels-last [B, CO, S-2, S-2]."""
    _lib.require_device(x, weight)
    _dims(x, weight)
    return _Conv3x3Valid.apply(x, weight)


def qualifies(conv, x=None) -> bool:
    """Is `conv` the convolution conv3x3_valid restates: Conv2d 3x3, stride 1, padding 0, dilation 1, groups 1, no bias, fp32 on the device, channels
    multiples of 32 (and x, when given, a square fp32 map on the same device)?"""
    if not isinstance(conv, torch.nn.Conv2d):
        return False
    w = conv.weight
    ok = (conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.dilation == (1, 1) and conv.groups == 1
          and conv.bias is None and conv.padding_mode == "zeros" and w.dtype == torch.float32 and w.is_cuda
          and conv.in_channels % 32 == 0 and conv.out_channels % 32 == 0)
    if ok and x is not None:
        ok = x.dim() == 4 and x.dtype == torch.float32 and x.device == w.device and x.shape[2] == x.shape[3] and x.shape[2] >= 3
    return ok


def _branch(seq, x):
    """seq = Sequential(Conv2d, BatchNorm2d, ReLU): the convolution through conv3x3_valid when it qualifies; then, while install.HEAD_BN_TRAIN_BOUND
    (read now) and the sequential is exactly that triple with a BatchNorm2d in training mode that bn_train.qualifies, BatchNorm + ReLU as one
    batchnorm_relu_train on the module's own parameters and buffers (channels-last in, contiguous NCHW out; num_batches_tracked advanced on the
    device); else the sequential's own remaining modules."""
    if not (isinstance(seq, torch.nn.Sequential) and len(seq) >= 1 and qualifies(seq[0], x)):
        return seq(x)
    y = conv3x3_valid(x, seq[0].weight)
    from . import install   # (install imports this module)
    # (seq[1].training: a BatchNorm2d frozen by its own .eval() inside a .train() parent normalises by its running statistics and leaves them alone)
    if (install.HEAD_BN_TRAIN_BOUND and len(seq) == 3 and isinstance(seq[2], torch.nn.ReLU) and seq[1].training
            and bn_train.qualifies(seq[1], y)):
        bn = seq[1]
        y = bn_train.batchnorm_relu_train(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, relu=True, out_nchw=True)
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
        return y
    for m in list(seq)[1:]:
        y = m(y)
    return y


def depthwise_xcorr_train_forward(self, kernel, search, xcorr):
    """DepthwiseXCorr.forward (ban.py:73-78) / DepthwiseXCorrCirc.forward (ban_lp.py:35-40) for .train() mode; `xcorr` = the correlation the class's
    module resolves (xcorr_depthwise / xcorr_depthwise_circular)."""
    kernel = _branch(self.conv_kernel, kernel)
    search = _branch(self.conv_search, search)
    feature = xcorr(search, kernel)
    return self.head(feature)
