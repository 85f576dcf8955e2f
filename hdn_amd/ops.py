"""The Python side of the split-fp16 matrix-core kernels: the weight packers (csrc/pack.hip, host code) and one launch wrapper per entry point of
include/hdn_hip.h that the homography trunk (hdn_amd.trunk), the similarity backbone (hdn_amd.backbone) and the heads (hdn_amd.heads) share.

A wrapper checks what the C side cannot know (device, layout, that a packed stream belongs to the shape), allocates the output and the workspace from
torch's caching allocator and launches on torch's current stream.  There is no fallback: a shape without a kernel is a ValueError.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib

# The matrix-core kernels split an activation as x * 2^-8 (csrc/mfma_split.h: finite and fp32-accurate to |x| < 1.67e7).  A fully fused trunk pays that
# multiply ONCE: its first stage writes relu(conv) * 2^-8, every block runs with act_domain = 1 (activations already scaled in memory, biases handed over
# scaled: exact), and the exit multiplies by 2^8 (hdn_avgpool_fc_f32's in_domain, or HomoResNet.forward).
ACT_SCALE_LOG2 = 8
SPLIT_PIECES = 2
V2_MIN_BATCH = 24      # below: the chained / K-sliced form of conv3x3_kernel (CHAIN_MAX_BATCH = 16 pairs and the sizes between)
# channel counts whose stride-1 3x3 convolutions run on hdn_conv3x3_bias_relu_f32 instead of MIOpen (measured per shape at
# B = 64, profiles/round3_conv3x3.txt: the kernel is kept only where it wins)
MATRIX_CORE_CHANNELS = (64, 128, 256, 512)
_MC_SIDE = {64: 32, 128: 16, 256: 8, 512: 4}
S2_CHANNELS = (128, 256, 512)       # ... whose stride-2 C -> C convolutions (a Bottleneck's conv2) run on hdn_conv3x3s2_f32, input side 2 * _MC_SIDE[C]
SIMI_STEM_MAX_SIDE = 255      # hdn_simi_stem_f32's documented limit (csrc/simi_stem.hip: MAX_S)


def fold_conv_bn(conv: nn.Conv2d, bn: nn.BatchNorm2d):
    """(weight, bias) of the convolution that equals eval-mode bn(conv(x)): w' = w * gamma / sqrt(var + eps), b' = beta - mean * (that
    factor) (+ the convolution's own bias through it), computed in float64 and rounded once."""
    if not isinstance(conv, nn.Conv2d) or not isinstance(bn, nn.BatchNorm2d) or conv.groups != 1:
        raise ValueError("fold_conv_bn takes a dense Conv2d and the BatchNorm2d behind it")
    if bn.running_var is None or bn.running_mean is None:
        raise ValueError("fold_conv_bn needs running statistics (track_running_stats)")
    var, mean = bn.running_var.double(), bn.running_mean.double()
    gamma = bn.weight.double() if bn.weight is not None else torch.ones_like(var)
    beta = bn.bias.double() if bn.bias is not None else torch.zeros_like(var)
    s = gamma / torch.sqrt(var + bn.eps)
    w = (conv.weight.double() * s.view(-1, 1, 1, 1)).to(conv.weight.dtype)
    b0 = conv.bias.double() if conv.bias is not None else torch.zeros_like(var)
    b = (beta + (b0 - mean) * s).to(conv.weight.dtype)
    if conv.weight.is_contiguous(memory_format=torch.channels_last) and not conv.weight.is_contiguous():
        w = w.contiguous(memory_format=torch.channels_last)
    return w.detach(), b.detach()


# ------------------------------------------------------------------------------------------------------------------------------ packers
def _c_pack(what, n_bytes, call):
    """Run one of the library's packers (csrc/pack.hip, host code): -> int16 CPU tensor holding the opaque stream."""
    if n_bytes < 0:
        raise ValueError(f"{what}: no matrix-core kernel takes weights of this shape")
    out = torch.empty(n_bytes // 2, dtype=torch.int16)
    rc = call(out.data_ptr(), n_bytes)
    if rc == -3:                                   # HDN_E_LIMIT
        raise ValueError(f"{what}: weights beyond the fp16 range (|w| >= 65,504) or NaN")
    _lib.check(rc, what)
    return out


def _host_f32(t):
    return t.detach().to(device="cpu", dtype=torch.float32).contiguous()


def _pack(name, takes, weights, shapes, *dims, c_name=None):
    """`weights` (any device / dtype; of `shapes`, else a ValueError that says what the packer `takes`) through the pair hdn_<name>_bytes(dims) /
    hdn_<name>_f32(weights..., dims, out, n) -> _c_pack's stream."""
    if [tuple(w.shape) for w in weights] != shapes:
        raise ValueError(f"{name} takes {takes} weights, got {', '.join(str(tuple(w.shape)) for w in weights)}")
    lib, c = _lib.load(), "hdn_" + (c_name or name)
    host = [_host_f32(w) for w in weights]       # (alive until the packer has read them: a device tensor's host copy is a temporary)
    return _c_pack(name, getattr(lib, c + "_bytes")(*dims), lambda o, n: getattr(lib, c + "_f32")(*[w.data_ptr() for w in host], *dims, o, n))


def pack_stem_mfma(weight):
    """[64, 2, 7, 7] fp32 weights (BatchNorm folded in) -> the stream hdn_trunk_stem_mfma_f32 takes (hdn_pack_stem_mfma_f32; the layout is
    the library's: csrc/pack.hip)."""
    return _pack("pack_stem_mfma", "[64, 2, 7, 7]", [weight], [(64, 2, 7, 7)])


def pack_conv3x3(weight):
    """[C, C, 3, 3] fp32 weights of a stride-1 convolution -> the stream hdn_conv3x3_bias_relu_f32 / hdn_conv3x3_chain_f32 take
    (hdn_pack_conv3x3_f32).  The side S is implied by C in the trunk (64 -> 32, 128 -> 16, 256 -> 8, 512 -> 4)."""
    C = weight.shape[0]
    return _pack("pack_conv3x3", "[C, C, 3, 3]", [weight], [(C, C, 3, 3)], C)


def pack_conv3x3_v2(weight):
    """[C, C, 3, 3] fp32 weights -> the stream of hdn_conv3x3_v2_f32 (hdn_pack_conv3x3_v2_f32)."""
    C = weight.shape[0]
    return _pack("pack_conv3x3_v2", "[C, C, 3, 3]", [weight], [(C, C, 3, 3)], C)


def _pack_s2_ds(name, weight, ds_weight, c_name=None):
    CI = weight.shape[1]
    return _pack(name, "[2C, C, 3, 3] and [2C, C, 1, 1]", [weight, ds_weight], [(2 * CI, CI, 3, 3), (2 * CI, CI, 1, 1)], CI, c_name=c_name)


def pack_conv3x3s2_ds(weight, ds_weight):
    """[2C, C, 3, 3] weights of the stride-2 convolution + [2C, C, 1, 1] weights of the block's downsample branch -> the stream of
    hdn_conv3x3s2_ds_f32 (hdn_pack_conv3x3s2_ds_f32)."""
    return _pack_s2_ds("pack_conv3x3s2_ds", weight, ds_weight)


def pack_conv3x3s2_ds_v2(weight, ds_weight):
    """The same two weight tensors -> the stream of hdn_conv3x3s2_v2_f32 (hdn_pack_conv3x3s2_v2_f32)."""
    return _pack_s2_ds("pack_conv3x3s2_ds_v2", weight, ds_weight, c_name="pack_conv3x3s2_v2")


def pack_conv1x1(weight):
    """[CO, CI, 1, 1] (or [CO, CI]) fp32 weights, BatchNorm folded in -> the stream hdn_conv1x1_f32 takes (hdn_pack_conv1x1_f32)."""
    CO, CI = weight.shape[0], weight.shape[1]
    if tuple(weight.shape) not in ((CO, CI), (CO, CI, 1, 1)):
        raise ValueError(f"pack_conv1x1 takes [CO, CI, 1, 1] weights, got {tuple(weight.shape)}")
    return _pack("pack_conv1x1", "[CO, CI]", [weight.reshape(CO, CI)], [(CO, CI)], CO, CI)


def pack_conv3x3s2(weight):
    """[C, C, 3, 3] fp32 weights of a Bottleneck's stride-2 convolution, BatchNorm folded in, C = 128 / 256 / 512 -> the stream hdn_conv3x3s2_f32
    takes (hdn_pack_conv3x3s2_f32)."""
    C = weight.shape[0]
    return _pack("pack_conv3x3s2", "[C, C, 3, 3]", [weight], [(C, C, 3, 3)], C)


def pack_conv3x3d(weight):
    """[CO, CI, 3, 3] fp32 weights of a stride-1 convolution with padding == dilation (any of 1 / 2 / 4: the stream is the same), BatchNorm folded in,
    CO and CI multiples of 32 -> the stream hdn_conv3x3d_f32 takes (hdn_pack_conv3x3d_f32)."""
    CO, CI = weight.shape[0], weight.shape[1]
    return _pack("pack_conv3x3d", "[CO, CI, 3, 3]", [weight], [(CO, CI, 3, 3)], CO, CI)


def pack_simi_stem(weight):
    """[64, 3, 7, 7] fp32 weights of the similarity backbone's conv1, BatchNorm folded in -> the stream hdn_simi_stem_f32 takes (hdn_pack_simi_stem_f32)."""
    return _pack("pack_simi_stem", "[64, 3, 7, 7]", [weight], [(64, 3, 7, 7)])


def _pack_w1(w1):
    """[G, H, H] fp32 (row = output channel) -> the stream hdn_head_tail_f32 takes (hdn_pack_head_tail_f32, csrc/pack.hip), on w1's device."""
    G, H = w1.shape[0], w1.shape[1]
    return _pack("pack_head_tail", "[G, H, H]", [w1], [(G, H, H)], G, H).to(w1.device)


def _pack_conv_search(ws):
    """n folded conv_search weights [CO, 256, 3, 3] fp32 -> the stream hdn_head_conv3x3_f32 takes (hdn_pack_head_conv3x3_f32), on their device."""
    host = [_host_f32(t) for t in ws]
    n, CO = len(host), host[0].shape[0]
    if any(tuple(t.shape) != (CO, 256, 3, 3) for t in host):
        raise ValueError("conv_search weights must be [CO, 256, 3, 3]")
    lib, ptrs = _lib.load(), _lib.ptr_array(host)
    return _c_pack("pack_head_conv3x3", lib.hdn_pack_head_conv3x3_bytes(n, CO),
                   lambda o, nb: lib.hdn_pack_head_conv3x3_f32(ptrs, n, CO, o, nb)).to(ws[0].device)


# ------------------------------------------------------------------------------------------------------------------------- launch helpers
_CL = torch.channels_last


def _square_cl(x):
    """Is x a square, channels-last, float32 [B,C,S,S]?"""
    return x.dim() == 4 and x.dtype == torch.float32 and x.shape[2] == x.shape[3] and x.is_contiguous(memory_format=_CL)


def _stream_ok(wpacked, dev, numel):
    """Is `wpacked` a packer's stream (int16) of `numel` elements on `dev`?"""
    return wpacked.dtype == torch.int16 and wpacked.device == dev and wpacked.numel() == numel


def _empty_cl(shape, dev):
    return torch.empty(shape, dtype=torch.float32, device=dev, memory_format=_CL)


# ------------------------------------------------------------------------------------------------------------------------------ wrappers
def bias_relu_(y, bias, residual=None):
    """In place: y = relu(y + bias[c] (+ residual)) through hdn_bias_relu_f32; y / residual [B,C,H,W] float32, both NCHW-contiguous
    or both channels-last."""
    dev = _lib.require_device(y, bias) if residual is None else _lib.require_device(y, bias, residual)
    if y.dim() != 4 or bias.numel() != y.shape[1] or (residual is not None and residual.shape != y.shape):
        raise ValueError(f"bias_relu_: y [B,C,H,W], bias [C], residual like y; got {tuple(y.shape)}, {tuple(bias.shape)}")
    B, C, H, W = y.shape
    if y.is_contiguous():   # (a [B,C,1,1] tensor is both: NCHW arithmetic is right for it)
        nhwc = 0
    elif y.is_contiguous(memory_format=_CL):
        nhwc = 1
    else:
        raise ValueError("bias_relu_: y must be NCHW-contiguous or channels-last")
    if residual is not None and not (residual.is_contiguous(memory_format=_CL) if nhwc else residual.is_contiguous()):
        residual = residual.contiguous(memory_format=_CL if nhwc else torch.contiguous_format)
    _lib.launch("bias_relu", dev, _lib.load().hdn_bias_relu_f32, _lib.ptr(y), _lib.ptr(bias), _lib.opt(residual), B, C, H * W, nhwc)
    return y


def conv3x3_bias_relu(x, wpacked, bias, residual=None, wpacked_v2=None, act_domain=0):
    """relu(conv3x3(x) + bias (+ residual)) through hdn_conv3x3_bias_relu_f32 — or, given `wpacked_v2` (pack_conv3x3_v2) and a batch of
    V2_MIN_BATCH or more, through hdn_conv3x3_v2_f32; x / residual channels-last [B,C,S,S] float32.  act_domain = 1: x, residual and the result are
    x_real * 2^-8 in memory and `bias` is bias * 2^-8 (include/hdn_hip.h, "Activation domain")."""
    dev = _lib.require_device(x, bias) if residual is None else _lib.require_device(x, bias, residual)
    B, C, S, _ = x.shape
    if not _square_cl(x) or (residual is not None and (residual.shape != x.shape or not residual.is_contiguous(memory_format=_CL))):
        raise ValueError("conv3x3_bias_relu: square channels-last inputs of equal shape")
    if not _stream_ok(wpacked, dev, 9 * SPLIT_PIECES * C * C) or bias.numel() != C:
        raise ValueError("conv3x3_bias_relu: weights must come from pack_conv3x3 for this channel count, on the input's device")
    lib = _lib.load()
    v2 = wpacked_v2 is not None and B >= V2_MIN_BATCH
    if v2 and not _stream_ok(wpacked_v2, dev, 9 * SPLIT_PIECES * C * C):
        raise ValueError("conv3x3_bias_relu: wpacked_v2 must come from pack_conv3x3_v2 for this channel count, on the input's device")
    ws, nws = _lib.workspace("conv3x3_bias_relu", lib.hdn_conv3x3_v2_workspace_bytes(B, S, C) if v2 else lib.hdn_conv3x3_workspace_bytes(B, S, C, 1), dev)
    out = torch.empty_like(x, memory_format=_CL)
    _lib.launch("conv3x3_bias_relu", dev, lib.hdn_conv3x3_v2_f32 if v2 else lib.hdn_conv3x3_bias_relu_f32, _lib.ptr(x), _lib.ptr(wpacked_v2 if v2 else wpacked),
                _lib.ptr(bias), _lib.opt(residual), _lib.ptr(out), _lib.opt(ws), nws, B, S, C, int(act_domain))
    return out


def conv3x3s2_ds(x, wpacked, bias, wpacked_v2=None, act_domain=0):
    """(relu(conv3x3/s2(x) + bias), conv1x1/s2(x)) through hdn_conv3x3s2_ds_f32 - or, given `wpacked_v2` (pack_conv3x3s2_ds_v2) and a batch of
    V2_MIN_BATCH or more, through hdn_conv3x3s2_v2_f32; x channels-last [B,C,2S,2S] -> two [B,2C,S,S]."""
    dev = _lib.require_device(x, bias)
    B, CI, H, _ = x.shape
    if not _square_cl(x) or H % 2:
        raise ValueError("conv3x3s2_ds: square, even-sided channels-last input")
    S, CO = H // 2, 2 * CI
    v2 = wpacked_v2 is not None and B >= V2_MIN_BATCH
    if v2 and (not _stream_ok(wpacked_v2, dev, SPLIT_PIECES * 10 * CI * CO) or bias.numel() != CO):
        raise ValueError("conv3x3s2_ds: v2 weights must come from pack_conv3x3s2_ds_v2 for this channel count, on the input's device")
    if not v2 and (not _stream_ok(wpacked, dev, SPLIT_PIECES * 3 * 4 * CI * CO) or bias.numel() != CO):
        raise ValueError("conv3x3s2_ds: weights must come from pack_conv3x3s2_ds for this channel count, on the input's device")
    lib = _lib.load()
    out, out_ds = _empty_cl((B, CO, S, S), dev), _empty_cl((B, CO, S, S), dev)
    if v2:
        _lib.launch("conv3x3s2_v2", dev, lib.hdn_conv3x3s2_v2_f32, _lib.ptr(x), _lib.ptr(wpacked_v2), _lib.ptr(bias), _lib.ptr(out), _lib.ptr(out_ds),
                    B, S, CI, int(act_domain))
    else:
        ws, nws = _lib.workspace("conv3x3s2_ds", lib.hdn_conv3x3_workspace_bytes(B, S, CI, 2), dev)
        _lib.launch("conv3x3s2_ds", dev, lib.hdn_conv3x3s2_ds_f32, _lib.ptr(x), _lib.ptr(wpacked), _lib.ptr(bias), _lib.ptr(out), _lib.ptr(out_ds),
                    _lib.opt(ws), nws, B, S, CI, int(act_domain))
    return out, out_ds


class LazyAct:
    """An activation of the chained trunk that was never written out: relu(sum of `slices` [z,B,S,S,C] + bias[c] (+ res)), finished by
    the convolution that reads it (or by finish()).  res: None, a channels-last activation [B,C,S,S], or raw slices [zr,B,S,S,C]
    (the downsample branch)."""

    __slots__ = ("slices", "bias", "res")

    def __init__(self, slices, bias, res=None):
        if slices.dim() != 5 or slices.shape[2] != slices.shape[3] or not slices.is_contiguous() or bias.numel() != slices.shape[4]:
            raise ValueError(f"LazyAct: slices [z,B,S,S,C] contiguous with a bias of C elements, got {tuple(slices.shape)}, {tuple(bias.shape)}")
        self.slices, self.bias, self.res = slices, bias, res

    @property
    def shape(self):
        z, B, S, _, C = self.slices.shape
        return (B, C, S, S)

    def res_args(self):
        """(pointer, slice count) of the residual for the C ABI: a channels-last activation counts as one slice."""
        r = self.res
        if r is None:
            return None, 0
        z, B, S, _, C = self.slices.shape
        if r.dim() == 5:
            ok = tuple(r.shape[1:]) == (B, S, S, C) and r.is_contiguous()
        else:
            ok = tuple(r.shape) == (B, C, S, S) and r.is_contiguous(memory_format=_CL)
        if not ok or r.dtype != torch.float32 or r.device != self.slices.device:
            raise ValueError(f"LazyAct residual must be a channels-last [B,C,S,S] activation or [z,B,S,S,C] slices matching {tuple(self.slices.shape)}")
        return _lib.ptr(r), (r.shape[0] if r.dim() == 5 else 1)

    def finish(self):
        """The activation itself, channels-last [B,C,S,S] (hdn_conv3x3_finish_f32)."""
        z, B, S, _, C = self.slices.shape
        dev = self.slices.device
        out = _empty_cl((B, C, S, S), dev)
        rp, rz = self.res_args()
        _lib.launch("conv3x3_finish", dev, _lib.load().hdn_conv3x3_finish_f32, _lib.ptr(self.slices), z, _lib.ptr(self.bias), rp, rz, _lib.ptr(out), B, S, C)
        return out


def chain_conv(x, wpacked, stride=1, want_x=False, act_domain=0):
    """One convolution of the chained trunk (hdn_conv3x3_chain_f32): x a channels-last activation [B,CI,SI,SI] or a LazyAct; returns
    (slices [z,B,S,S,CO], downsample slices or None (stride 2), the finished input as an activation or None (want_x, LazyAct input))."""
    lazy = isinstance(x, LazyAct)
    B, CI, SI, SI2 = x.shape
    src = x.slices if lazy else x
    dev = _lib.require_device(src)
    if SI != SI2 or SI % stride or (not lazy and not x.is_contiguous(memory_format=_CL)):
        raise ValueError("chain_conv: square channels-last input")
    S, CO = SI // stride, CI * stride
    T = 4 if stride == 2 else 3
    if not _stream_ok(wpacked, dev, SPLIT_PIECES * 3 * T * CI * CO):
        raise ValueError("chain_conv: weights must come from pack_conv3x3 / pack_conv3x3s2_ds for this channel count")
    lib = _lib.load()
    z = lib.hdn_conv3x3_chain_slices(B, S, CI, stride)
    if z < 0:
        _lib.check(int(z), "conv3x3_chain")
    out = torch.empty((z, B, S, S, CO), dtype=torch.float32, device=dev)
    out_ds = torch.empty_like(out) if stride == 2 else None
    x_out = _empty_cl((B, CI, SI, SI), dev) if (lazy and want_x) else None
    rp, rz = x.res_args() if lazy else (None, 0)
    _lib.launch("conv3x3_chain", dev, lib.hdn_conv3x3_chain_f32, _lib.ptr(src), src.shape[0] if lazy else 0, _lib.opt(x.bias if lazy else None), rp, rz,
                _lib.opt(x_out), _lib.ptr(wpacked), _lib.ptr(out), _lib.opt(out_ds), B, S, CI, stride, int(act_domain))
    return out, out_ds, x_out


def conv1x1(x, wpacked, bias, residual=None, stride=1, relu=True, act_domain=0):
    """[relu](conv1x1/stride(x) + bias (+ residual)) through hdn_conv1x1_f32; x channels-last [B,CI,S,S] float32, residual / result channels-last
    [B,CO,So,So], So = (S - 1) // stride + 1; `wpacked` from pack_conv1x1, on x's device.  act_domain as conv3x3_bias_relu's."""
    dev = _lib.require_device(x, bias) if residual is None else _lib.require_device(x, bias, residual)
    if not _square_cl(x):
        raise ValueError("conv1x1: square channels-last float32 input [B,CI,S,S]")
    B, CI, S, _ = x.shape
    CO, So = bias.numel(), (S - 1) // stride + 1
    if not _stream_ok(wpacked, dev, SPLIT_PIECES * CO * CI):
        raise ValueError("conv1x1: weights must come from pack_conv1x1 for this (CO, CI), on the input's device")
    if residual is not None and (tuple(residual.shape) != (B, CO, So, So) or not residual.is_contiguous(memory_format=_CL)):
        raise ValueError(f"conv1x1: residual must be channels-last {(B, CO, So, So)}")
    out = _empty_cl((B, CO, So, So), dev)
    _lib.launch("conv1x1", dev, _lib.load().hdn_conv1x1_f32, _lib.ptr(x), _lib.ptr(wpacked), _lib.ptr(bias), _lib.opt(residual), _lib.ptr(out), B, S, CI, CO,
                int(stride), int(bool(relu)), int(act_domain))
    return out


def conv3x3s2(x, wpacked, bias, act_domain=0):
    """relu(conv3x3 / stride 2 / padding 1 (x) + bias) through hdn_conv3x3s2_f32; x channels-last [B,C,2S,2S] float32 with (S, C) = (16, 128),
    (8, 256) or (4, 512) -> channels-last [B,C,S,S]; `wpacked` from pack_conv3x3s2, on x's device.  act_domain as conv3x3_bias_relu's."""
    dev = _lib.require_device(x, bias)
    if not _square_cl(x) or x.shape[2] % 2:
        raise ValueError("conv3x3s2: square, even-sided channels-last float32 input [B,C,2S,2S]")
    B, C, H, _ = x.shape
    S = H // 2
    if not _stream_ok(wpacked, dev, 9 * SPLIT_PIECES * C * C) or bias.numel() != C:
        raise ValueError("conv3x3s2: weights must come from pack_conv3x3s2 for this channel count, on the input's device")
    lib = _lib.load()
    ws, nws = _lib.workspace("conv3x3s2", lib.hdn_conv3x3s2_workspace_bytes(B, S, C), dev)
    out = _empty_cl((B, C, S, S), dev)
    _lib.launch("conv3x3s2", dev, lib.hdn_conv3x3s2_f32, _lib.ptr(x), _lib.ptr(wpacked), _lib.ptr(bias), _lib.ptr(out), _lib.opt(ws), nws,
                B, S, C, int(act_domain))
    return out


def _conv3x3_dv(valid, x, wpacked, bias, step, relu, act_domain):
    """conv3x3d (step: the dilation, output side S) and, valid, conv3x3v (step: the stride, output side (S - 3) // step + 1), both on
    pack_conv3x3d's stream."""
    name = "conv3x3v" if valid else "conv3x3d"
    dev = _lib.require_device(x) if bias is None else _lib.require_device(x, bias)
    if not _square_cl(x):
        raise ValueError(f"{name}: square channels-last float32 input [B,CI,S,S]")
    B, CI, S, _ = x.shape
    CO = wpacked.numel() // (9 * SPLIT_PIECES * CI) if CI else 0
    if CO <= 0 or not _stream_ok(wpacked, dev, 9 * SPLIT_PIECES * CO * CI) or (bias is not None and bias.numel() != CO):
        raise ValueError(f"{name}: weights must come from pack_conv3x3d for this CI (and the bias's CO), on the input's device")
    lib = _lib.load()
    ws, nws = _lib.workspace(name, getattr(lib, f"hdn_{name}_workspace_bytes")(B, S, CI, CO, int(step)), dev)   # (also refuses a step or side without a kernel)
    So = (S - 3) // int(step) + 1 if valid else S
    out = _empty_cl((B, CO, So, So), dev)
    _lib.launch(name, dev, getattr(lib, f"hdn_{name}_f32"), _lib.ptr(x), _lib.ptr(wpacked), _lib.opt(bias), _lib.ptr(out), _lib.opt(ws), nws, B, S, CI, CO,
                int(step), int(bool(relu)), int(act_domain))
    return out


def conv3x3d(x, wpacked, bias, dilation=1, relu=True, act_domain=0):
    """[relu](conv3x3 / stride 1 / dilation / padding = dilation (x) [+ bias]) through hdn_conv3x3d_f32; x channels-last [B,CI,S,S] float32 -> channels-last
    [B,CO,S,S]; `wpacked` from pack_conv3x3d, on x's device (CO is read off its size); bias [CO] or None (zero).  act_domain as conv3x3_bias_relu's."""
    return _conv3x3_dv(False, x, wpacked, bias, dilation, relu, act_domain)


def conv3x3v(x, wpacked, bias, stride=2, relu=True, act_domain=0):
    """[relu](conv3x3 / stride 1 or 2 / padding 0 (x) [+ bias]) through hdn_conv3x3v_f32; x channels-last [B,CI,S,S] float32, S >= 3 -> channels-last
    [B,CO,So,So], So = (S - 3) // stride + 1; `wpacked` from pack_conv3x3d, on x's device (CO is read off its size); bias [CO] or None (zero).
    act_domain as conv3x3_bias_relu's."""
    return _conv3x3_dv(True, x, wpacked, bias, stride, relu, act_domain)


def simi_stem(x, wpacked, bias):
    """maxpool3x3/s2/p1(relu(conv7x7 / stride 2 / padding 0 (x) + bias)) through hdn_simi_stem_f32, one launch; x NCHW-contiguous [B,3,S,S] float32,
    7 <= S <= SIMI_STEM_MAX_SIDE -> channels-last [B,64,Sp,Sp], Sp = ((S - 7) // 2) // 2 + 1; `wpacked` from pack_simi_stem, bias [64], on x's device."""
    dev = _lib.require_device(x, bias)
    if x.dim() != 4 or x.dtype != torch.float32 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or not x.is_contiguous():
        raise ValueError("simi_stem: square NCHW-contiguous float32 input [B,3,S,S]")
    B, _, S, _ = x.shape
    lib = _lib.load()
    if not _stream_ok(wpacked, dev, lib.hdn_pack_simi_stem_bytes() // 2) or bias.numel() != 64:
        raise ValueError("simi_stem: weights must come from pack_simi_stem (and a bias of 64), on the input's device")
    if S < 7 or S > SIMI_STEM_MAX_SIDE:
        raise ValueError(f"simi_stem: side {S} outside 7 .. {SIMI_STEM_MAX_SIDE}")
    Sp = ((S - 7) // 2) // 2 + 1
    out = _empty_cl((B, 64, Sp, Sp), dev)
    _lib.launch("simi_stem", dev, lib.hdn_simi_stem_f32, _lib.ptr(x), _lib.ptr(wpacked), _lib.ptr(bias), _lib.ptr(out), B, S, 0)
    return out


# ------------------------------------------------------------------------------------------------------------------- the heads' entry points
def _head_levels(x_fs, nhwc):
    """The levels [B, C, Hi, Wi] of a head convolution as its kernel reads them -> (tensors, batch stride in elements).  An image that is dense NCHW
    (nhwc = 0) / dense channels-last (nhwc = 1) is read where it is, whatever the batch stride (a batch slice needs no copy); anything else is copied
    to that layout, and so is a level whose batch stride differs from the others' (one batch stride per launch)."""
    B, C, Hi, Wi = x_fs[0].shape
    image = C * Hi * Wi
    form = (1, Wi * C, C) if nhwc else (Hi * Wi, Wi, 1)                             # (channel, row, pixel) strides
    fmt = _CL if nhwc else torch.contiguous_format
    xs = [x.detach() for x in x_fs]
    xs = [x if tuple(x.stride()[1:]) == form and (B == 1 or x.stride(0) >= image) else x.contiguous(memory_format=fmt) for x in xs]
    if B > 1 and len({x.stride(0) for x in xs}) > 1:
        xs = [x if x.stride(0) == image else x.contiguous(memory_format=fmt) for x in xs]
    return xs, (image if B == 1 else xs[0].stride(0))


def head_conv_batch(x_fs, wsp, bsp, groups=2):
    """n levels [B, 256, Hi, Wi] through one launch of hdn_head_conv3x3_batch_f32 (3x3 / no padding + bias + ReLU with the stream `wsp` of
    _pack_conv_search and the bias `bsp` [n, CO]) -> [n, groups, B, CO / groups, Ho, Wo] contiguous: out[l, g] is a contiguous [B, CO / groups, Ho, Wo].
    Channels-last where level 0 is dense channels-last, NCHW otherwise (_head_levels)."""
    x0 = x_fs[0]
    dev = _lib.require_device(*x_fs)
    n, (B, C, Hi, Wi) = len(x_fs), x0.shape
    if C != 256 or any(x.shape != x0.shape for x in x_fs):
        raise ValueError("head_conv_batch: every level must be [B, 256, Hi, Wi] of one shape")
    nhwc = int(tuple(x0.stride()[1:]) == (1, Wi * C, C))
    xs, xbs = _head_levels(x_fs, nhwc)
    CO = bsp.shape[1]
    out = torch.empty((n, groups, B, CO // groups, Hi - 2, Wi - 2), dtype=torch.float32, device=dev)
    _lib.launch("head_conv_batch", dev, _lib.load().hdn_head_conv3x3_batch_f32, _lib.ptr_array(xs), _lib.ptr(wsp), _lib.ptr(bsp), _lib.ptr(out),
                n, B, groups, CO, Hi, Wi, nhwc, xbs)
    return out


def head_conv_search(x_fs, pk):
    """The n levels' conv_search (both branches) + bias + ReLU in one launch -> [n, 2 hidden, Ho, Wo] contiguous (hdn_head_conv3x3_f32; pk: wsp / bsp of
    a _PackedHead).  NCHW where level 0 is NCHW-contiguous, channels-last otherwise (_head_levels)."""
    x0 = x_fs[0]
    dev = _lib.require_device(*x_fs)
    n, (_, C, Hi, Wi) = len(x_fs), x0.shape
    nhwc = 0 if x0.is_contiguous() else 1
    xs, _ = _head_levels(x_fs, nhwc)
    CO = pk.bsp.shape[1]
    out = torch.empty((n, CO, Hi - 2, Wi - 2), dtype=torch.float32, device=dev)
    _lib.launch("head_conv_search", dev, _lib.load().hdn_head_conv3x3_f32, _lib.ptr_array(xs), _lib.ptr(pk.wsp), _lib.ptr(pk.bsp), _lib.ptr_array(list(out)),
                n, CO, Hi, Wi, nhwc)
    return out


def head_tail(feats, pk, n):
    """feats [2n, H, Ho, Wo] -> out [2, om, Ho * Wo] through hdn_head_tail_f32 (pk: a _PackedHead with w1p)."""
    dev = _lib.require_device(feats)
    H, P, om = feats.shape[1], feats.shape[2] * feats.shape[3], pk.wf.shape[1]
    out = torch.empty((2, om, P), dtype=torch.float32, device=dev)
    _lib.launch("head_tail", dev, _lib.load().hdn_head_tail_f32, _lib.ptr(feats), _lib.ptr(pk.w1p), _lib.ptr(pk.b1), _lib.ptr(pk.wf), _lib.ptr(pk.bf),
                _lib.ptr(out), n, H, P, om)
    return out


def head_tail_batch(feats, pk, n, B):
    """feats [2n, B, H, Ho, Wo] -> (cls [B, oc, Ho, Wo], loc [B, ol, Ho, Wo]), contiguous views of ONE output buffer, through hdn_head_tail_batch_f32
    (pk: a _PackedHead with w1p)."""
    dev = _lib.require_device(feats)
    if feats.dim() != 5 or feats.shape[0] != 2 * n or feats.shape[1] != B or feats.dtype != torch.float32 or not feats.is_contiguous():
        raise ValueError(f"head_tail_batch: feats must be a contiguous float32 [{2 * n}, {B}, H, Ho, Wo], got {tuple(feats.shape)}")
    H, Ho, Wo = feats.shape[2:]
    P = Ho * Wo
    out = torch.empty(B * (pk.oc + pk.ol) * P, dtype=torch.float32, device=dev)
    _lib.launch("head_tail_batch", dev, _lib.load().hdn_head_tail_batch_f32, _lib.ptr(feats), _lib.ptr(pk.w1p), _lib.ptr(pk.b1), _lib.ptr(pk.wf),
                _lib.ptr(pk.bf), _lib.ptr(out), n, B, H, P, pk.oc, pk.ol)
    split = B * pk.oc * P
    return out[:split].view(B, pk.oc, Ho, Wo), out[split:].view(B, pk.ol, Ho, Wo)
