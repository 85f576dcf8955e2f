"""The correlation heads around the HIP correlations.

    DepthwiseXCorr / DepthwiseBAN / MultiBAN             <- hdn/models/head/ban.py:51-127
    DepthwiseXCorrCirc / DepthwiseCircBAN / MultiCircBAN <- hdn/models/head/ban_lp.py:14-92

Same module / parameter names as the reference, so its snapshots load.  The 3x3 / 1x1 convolutions stay on
PyTorch-ROCm (MIOpen / hipBLASLt); what changes is the schedule of a frame:
  * all 3 levels x {cls, loc} correlations of a head are ONE launch (hdn_xcorr_depthwise_multi_f32);
  * at the tracker's B = 1 everything around the correlations is packed (_PackedHead: BatchNorm folded, the two branches of a
    level as one convolution, the 1x1 convolutions of all levels and the weighted sum as two batched matrix products): ~15 launches
    per head instead of ~70;
  * the template branch conv_kernel(z_f) is computed once per template (the reference recomputes it every
    frame although self.zf only changes in template(), model_builder_e2e_unconstrained_v2.py:87-96, ban.py:74);
  * opt-in (HDN_HIP_HEADS=1 or head._hdn_hip_heads = True, default off): the template branch of all levels and both branches as
    ONE launch of hdn_head_conv3x3_batch_f32 at any batch, and conv_search at B > 1 as one launch of the same kernel;
  * opt-in level 2 (HDN_HIP_HEADS=2 or head._hdn_hip_heads = 2): on top of that, everything behind the correlations at B > 1 as ONE launch
    of hdn_head_tail_batch_f32 - a head forward at any batch is then three launches of this project's kernels and no library call.
`fused_forward` works on any object with the reference's attribute layout, so install() can bind it onto the
reference's own MultiBAN / MultiCircBAN classes.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .ops import _c_pack, _host_f32, bias_relu_
from .xcorr import out_shape, xcorr_depthwise, xcorr_depthwise_circular, xcorr_depthwise_multi


def _conv_bn_relu(cin, cout, k):
    return nn.Sequential(nn.Conv2d(cin, cout, kernel_size=k, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))


class DepthwiseXCorr(nn.Module):
    _circular = False

    def __init__(self, in_channels, hidden, out_channels, kernel_size=3):
        super().__init__()
        self.conv_kernel = _conv_bn_relu(in_channels, hidden, kernel_size)
        self.conv_search = _conv_bn_relu(in_channels, hidden, kernel_size)
        self.head = nn.Sequential(
            nn.Conv2d(hidden, hidden, kernel_size=1, bias=False), nn.BatchNorm2d(hidden), nn.ReLU(inplace=True),
            nn.Conv2d(hidden, out_channels, kernel_size=1),
        )

    def forward(self, kernel, search):
        kernel = self.conv_kernel(kernel)
        search = self.conv_search(search)
        corr = xcorr_depthwise_circular if self._circular else xcorr_depthwise
        return self.head(corr(search, kernel))


class DepthwiseXCorrCirc(DepthwiseXCorr):
    _circular = True


class DepthwiseBAN(nn.Module):
    _xcorr = DepthwiseXCorr
    _loc_out = 2

    def __init__(self, in_channels=256, out_channels=256, cls_out_channels=2, weighted=False):
        super().__init__()
        self.cls = self._xcorr(in_channels, out_channels, cls_out_channels)
        self.loc = self._xcorr(in_channels, out_channels, self._loc_out)

    def forward(self, z_f, x_f):
        return self.cls(z_f, x_f), self.loc(z_f, x_f)


class DepthwiseCircBAN(DepthwiseBAN):
    _xcorr = DepthwiseXCorrCirc
    _loc_out = 4


class _TemplateCache:
    """conv_kernel(z_f) of every (level, branch) for ONE template.

    Holds strong references to the template tensors it was computed from: identity (`is`) and the in-place version
    counter then identify the template for as long as the entry lives (a freed tensor's id / address / version 0
    can all be reused by the next template: that is how a key of plain integers goes stale).  The version counters of
    the conv_kernel parameters and BN buffers are part of the key, so load_state_dict() / .to() / optimiser steps
    after a forward invalidate the entry as well."""

    __slots__ = ("z_fs", "z_versions", "param_versions", "training", "kern")

    def __init__(self, z_fs, branches, training, kern):
        self.z_fs = tuple(z_fs)
        self.z_versions = tuple(z._version for z in z_fs)
        self.param_versions = _param_versions(branches)
        self.training = training
        self.kern = kern

    def matches(self, z_fs, branches, training):
        return (len(z_fs) == len(self.z_fs) and all(a is b for a, b in zip(z_fs, self.z_fs))
                and tuple(z._version for z in z_fs) == self.z_versions and training == self.training
                and _param_versions(branches) == self.param_versions)


def _tensor_refs(modules):
    """(dict, name) of every parameter / buffer below `modules`: walking Module.parameters() costs ~1 us per tensor and frame in
    the eager loop; a held reference to the owning module's _parameters / _buffers dict is a plain lookup.  (Replacing a whole
    sub-module afterwards is not seen: invalidate_template_cache() drops the references.)"""
    refs = []
    for m in modules:
        for sub in m.modules():
            refs += [(sub._parameters, n) for n, t in sub._parameters.items() if t is not None]
            refs += [(sub._buffers, n) for n, t in sub._buffers.items() if t is not None]
    return refs


def _versions(refs):
    return tuple((id(t), t.data_ptr(), t._version) for t in (d[n] for d, n in refs))


def _param_versions(branches):
    head = getattr(branches[0], "_hdn_owner", None)
    refs = getattr(head, "_hdn_refs_template", None) if head is not None else None
    if refs is None:
        refs = _tensor_refs([br.conv_kernel for br in branches])
        if head is not None:
            object.__setattr__(head, "_hdn_refs_template", refs)
    return _versions(refs)


_CACHE_ATTRS = ("_hdn_template_cache", "_hdn_packed_head", "_hdn_refs_template", "_hdn_refs_head", "_hdn_packable", "_hdn_template_pack",
                "_hdn_search_pack")


def invalidate_template_cache(head):
    """Drop the cached template-branch features of a MultiBAN / MultiCircBAN.  install() wraps ModelBuilder.template() so that
    every new template calls this for both heads; call it yourself after mutating weights through .data (which bypasses the
    version counters the cache is keyed on) without re-running template()."""
    for name in _CACHE_ATTRS:
        object.__setattr__(head, name, None)


def template_cache_state(head):
    """Everything invalidate_template_cache drops, to be handed back with restore_template_cache_state: a captured hipGraph reads the buffers
    of these objects by address, so code that has to call template() between replays (a tracker slot handed a new video) keeps them alive."""
    return tuple(getattr(head, name, None) for name in _CACHE_ATTRS)


def restore_template_cache_state(head, state):
    for name, v in zip(_CACHE_ATTRS, state):
        object.__setattr__(head, name, v)


def refresh_template_cache(head, z_fs, rows=None):
    """After the template features `z_fs` (the tensors the last forward saw) were changed IN PLACE: recompute conv_kernel(z_f) for sample
    `rows` (an index or a slice; None: all) and write it INTO the cache's existing buffers, then bring the cache's key up to date.

    The cache is consulted by Python code, and a replayed hipGraph runs none: it keeps reading the `kern` buffers that existed at capture.
    An eager forward would notice the version counters and recompute into NEW buffers; a replay would silently correlate against the old
    template's features.  Same storage, same path as the forward took (the HDN_HIP_HEADS template pack where it is on, conv_kernel otherwise).
    Without a cache (no forward yet) there is nothing to refresh: the next forward computes it."""
    cache = getattr(head, "_hdn_template_cache", None)
    if cache is None:
        return False
    z_fs = list(z_fs)
    if len(z_fs) != len(cache.z_fs) or not all(a is b for a, b in zip(z_fs, cache.z_fs)):
        raise ValueError("refresh_template_cache takes the template tensors the cache was computed from, changed in place")
    n = len(z_fs)
    sel = slice(None) if rows is None else slice(rows, rows + 1) if isinstance(rows, int) else rows
    boxes = [getattr(head, "box" + str(i + 2)) for i in range(n)]
    branches = [br for box in boxes for br in (box.cls, box.loc)]
    with torch.no_grad():
        zs = [z[sel] for z in z_fs]
        tp = getattr(head, "_hdn_template_pack", None) if _hip_heads_on(head) else None
        if tp is not None and tp.ok and tp.key[0] == _param_versions(branches):
            y = head_conv_batch(zs, tp.wsp, tp.bsp)           # the pack holds weights only: it serves any batch
            new = [y[l, g] for l in range(n) for g in range(2)]
        else:
            new = [br.conv_kernel(z) for box, z in zip(boxes, zs) for br in (box.cls, box.loc)]
        for dst, src in zip(cache.kern, new):
            dst[sel].copy_(src)
    cache.z_versions = tuple(z._version for z in z_fs)
    return True


_HIP_HEADS = None


def hip_heads() -> bool:
    """HDN_HIP_HEADS (default off), read once: the template branch at any batch and conv_search at B > 1 on hdn_head_conv3x3_batch_f32."""
    global _HIP_HEADS
    if _HIP_HEADS is None:
        _HIP_HEADS = os.environ.get("HDN_HIP_HEADS", "0") not in ("", "0")
    return _HIP_HEADS


def _hip_heads_on(head) -> bool:
    v = getattr(head, "_hdn_hip_heads", None)                # the per-head attribute overrides the environment
    return hip_heads() if v is None else bool(v)


_HIP_HEADS_LEVEL = None


def hip_heads_level() -> int:
    """HDN_HIP_HEADS as a level, read once: 0 off (default), 1 what hip_heads() switches on, 2 also the 1x1 tail at B > 1 on hdn_head_tail_batch_f32.
    Any other non-empty value is level 1, as hip_heads() reads it."""
    global _HIP_HEADS_LEVEL
    if _HIP_HEADS_LEVEL is None:
        v = os.environ.get("HDN_HIP_HEADS", "0").strip()
        _HIP_HEADS_LEVEL = 0 if v in ("", "0") else 2 if v == "2" else 1
    return _HIP_HEADS_LEVEL


def _hip_heads_level_of(head) -> int:
    v = getattr(head, "_hdn_hip_heads", None)                # True and 1: level 1; 2: level 2
    if v is None:
        return hip_heads_level()
    return 2 if (v is not True and v == 2) else 1 if v else 0


class _ConvPack:
    """The 3x3 convolutions of one side (conv_search or conv_kernel) of all levels, BatchNorm folded, cls || loc along CO: ws / bs the fp32 weights
    and biases per level, wsp / bsp the stream and the [n, CO] bias hdn_head_conv3x3(_batch)_f32 take (None where the kernel does not fit).
    `key`: the version counters it was built from; `ok`: what the predicate of its path said for that key."""

    __slots__ = ("key", "ok", "ws", "bs", "wsp", "bsp")


class _PackedHead:
    """Everything of a head behind the correlations, packed for the tracker's B = 1 call (launch-bound: ~70 small kernels per
    forward in the module-by-module form, 313 us under a hipGraph at 256 channels; packed ~15):
      * conv_search of a level: BatchNorm folded into the weights, the cls and loc branches (same input) as ONE convolution with
        2 x hidden output channels, bias + ReLU in one pass (hdn_bias_relu_f32);
      * the first 1x1 convolution + BatchNorm of all 2n (level, branch) heads: one batched matrix product;
      * the second 1x1 convolution, loc_scale and the (softmax-)weighted sum over the levels are linear: one batched matrix
        product with the weights [cw_0 W_0 | cw_1 W_1 | ...] per branch.
    Keyed on the version counters of every tensor it was built from (as _TemplateCache is)."""

    __slots__ = ("key", "ws", "bs", "w1", "b1", "wf", "bf", "oc", "ol", "hidden", "w1p", "wsp", "bsp")


def _head_key(self, boxes):
    refs = getattr(self, "_hdn_refs_head", None)
    if refs is None:
        refs = _tensor_refs([m for box in boxes for br in (box.cls, box.loc) for m in (br.conv_search, br.head)])
        refs += [(self._parameters, n) for n in ("loc_scale", "cls_weight", "loc_weight") if self._parameters.get(n) is not None]
        object.__setattr__(self, "_hdn_refs_head", refs)
    return _versions(refs)


def _packable(self, boxes, x_fs):
    """The packed path covers the reference's configuration: B = 1 on a GPU, every level with the same channel counts and the
    module layout of DepthwiseXCorr (conv3x3 no bias + BN + ReLU; conv1x1 no bias + BN + ReLU + conv1x1)."""
    return x_fs[0].shape[0] == 1 and _packable_any_batch(self, boxes, x_fs)


def _packable_any_batch(self, boxes, x_fs):
    """_packable without its B = 1 condition: what the batched conv_search (hdn_head_conv3x3_batch_f32) asks of the modules."""
    x0 = x_fs[0]
    if not x0.is_cuda or x0.dtype != torch.float32 or any(x.shape != x0.shape for x in x_fs):
        return False
    ref = None
    for box in boxes:
        for br in (box.cls, box.loc):
            cs, hd = br.conv_search, br.head
            if not (isinstance(cs, nn.Sequential) and len(cs) == 3 and isinstance(cs[0], nn.Conv2d) and isinstance(cs[1], nn.BatchNorm2d)
                    and isinstance(hd, nn.Sequential) and len(hd) == 4 and isinstance(hd[0], nn.Conv2d) and isinstance(hd[1], nn.BatchNorm2d)
                    and isinstance(hd[3], nn.Conv2d)):
                return False
            if not (isinstance(cs[2], nn.ReLU) and isinstance(hd[2], nn.ReLU)):
                return False
            if any(bn.training or not bn.track_running_stats or not bn.affine or bn.running_mean is None for bn in (cs[1], hd[1])):
                return False          # _fold_bn folds the running statistics and the affine weights: eval-mode BatchNorm only
            c0, h0, h3 = cs[0], hd[0], hd[3]
            if (c0.bias is not None or c0.stride != (1, 1) or c0.padding != (0, 0) or c0.dilation != (1, 1) or c0.groups != 1
                    or h0.bias is not None or h0.kernel_size != (1, 1) or h3.kernel_size != (1, 1) or h3.bias is None):
                return False
            sig = (tuple(c0.weight.shape), tuple(h0.weight.shape))
            if ref is None:
                ref = sig
            elif sig != ref:
                return False
        if box.cls.head[3].weight.shape[1:] != box.loc.head[3].weight.shape[1:]:
            return False
    return all(tuple(box.cls.head[3].weight.shape) == tuple(boxes[0].cls.head[3].weight.shape)
               and tuple(box.loc.head[3].weight.shape) == tuple(boxes[0].loc.head[3].weight.shape) for box in boxes)


def _fold_bn(conv, bn):
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    return conv.weight * s.reshape(-1, 1, 1, 1), bn.bias - bn.running_mean * s


def _pack_w1(w1):
    """[G, H, H] fp32 (row = output channel) -> the stream hdn_head_tail_f32 takes (hdn_pack_head_tail_f32, csrc/pack.hip), on w1's device."""
    from . import _lib

    G, H, _ = w1.shape
    lib, w = _lib.load(), _host_f32(w1)
    return _c_pack("pack_head_tail", lib.hdn_pack_head_tail_bytes(G, H), lambda o, n: lib.hdn_pack_head_tail_f32(w.data_ptr(), G, H, o, n)).to(w1.device)


def _pack_conv_search(ws):
    """n folded conv_search weights [CO, 256, 3, 3] fp32 -> the stream hdn_head_conv3x3_f32 takes (hdn_pack_head_conv3x3_f32), on their device."""
    import ctypes

    from . import _lib

    host = [_host_f32(t) for t in ws]
    n, CO = len(host), host[0].shape[0]
    if any(tuple(t.shape) != (CO, 256, 3, 3) for t in host):
        raise ValueError("conv_search weights must be [CO, 256, 3, 3]")
    lib = _lib.load()
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in host])
    return _c_pack("pack_head_conv3x3", lib.hdn_pack_head_conv3x3_bytes(n, CO),
                   lambda o, nb: lib.hdn_pack_head_conv3x3_f32(ptrs, n, CO, o, nb)).to(ws[0].device)


def _patch_fits(Hi, Wi):
    """The patch of 64 consecutive output pixels (their rows + 2, full width) fits the 224 pixels head_conv.hip stages."""
    return Hi >= 3 and Wi >= 3 and min((63 + Wi - 3) // (Wi - 2) + 3, Hi) * Wi <= 224


def _pack_convs(boxes, name):
    """`name` (conv_search / conv_kernel) of every level -> a _ConvPack (key / ok left to the caller)."""
    pk = _ConvPack()
    pk.ws, pk.bs = [], []
    for box in boxes:
        wc, bc = _fold_bn(getattr(box.cls, name)[0], getattr(box.cls, name)[1])
        wl, bl = _fold_bn(getattr(box.loc, name)[0], getattr(box.loc, name)[1])
        pk.ws.append(torch.cat([wc, wl], 0).contiguous())
        pk.bs.append(torch.cat([bc, bl], 0).contiguous())
    # all levels as one launch on the matrix cores (hdn_head_conv3x3_f32 / _batch_f32): 3x3 / stride 1 / no padding, 256 input channels
    w0 = pk.ws[0]
    fits_conv = (w0.is_cuda and len(boxes) <= 4 and tuple(w0.shape[1:]) == (256, 3, 3) and w0.shape[0] % 32 == 0 and all(w.shape == w0.shape for w in pk.ws)
                 and max(float(w.abs().max()) for w in pk.ws) < 65504.0)
    pk.wsp = _pack_conv_search(pk.ws) if fits_conv else None
    pk.bsp = torch.stack(pk.bs).contiguous() if fits_conv else None
    return pk


def _template_packable(boxes, z_fs, need_gpu=True):
    """The template branch as one launch of hdn_head_conv3x3_batch_f32, at any B: fp32 on a GPU (need_gpu=False: anywhere, for host tests), every
    level the same shape with 256 channels inside the kernel's patch limit, n <= 4, and conv_kernel of every (level, branch) the reference's
    Sequential(Conv2d 3x3 no bias / stride 1 / no padding, eval-mode BatchNorm2d, ReLU) with one hidden width (a multiple of 32: the cls and loc
    halves are tile-aligned groups) and folded |w| < 65504 (two fp16 pieces)."""
    z0 = z_fs[0]
    n = len(boxes)
    if (need_gpu and not z0.is_cuda) or z0.dtype != torch.float32 or z0.dim() != 4 or any(z.shape != z0.shape for z in z_fs):
        return False
    B, C, Hi, Wi = z0.shape
    if n != len(z_fs) or not 1 <= n <= 4 or C != 256 or B < 1 or n * B > 65535 or not _patch_fits(Hi, Wi):
        return False
    ref = None
    for box in boxes:
        for br in (box.cls, box.loc):
            ck = br.conv_kernel
            if not (isinstance(ck, nn.Sequential) and len(ck) == 3 and isinstance(ck[0], nn.Conv2d) and isinstance(ck[1], nn.BatchNorm2d)
                    and isinstance(ck[2], nn.ReLU)):
                return False
            c0, bn = ck[0], ck[1]
            if bn.training or not bn.track_running_stats or not bn.affine or bn.running_mean is None:
                return False          # _fold_bn folds the running statistics and the affine weights: eval-mode BatchNorm only
            if c0.bias is not None or c0.stride != (1, 1) or c0.padding != (0, 0) or c0.dilation != (1, 1) or c0.groups != 1:
                return False
            shape = tuple(c0.weight.shape)
            if ref is None:
                ref = shape
            if shape != ref or shape[1:] != (256, 3, 3) or shape[0] % 32 != 0:
                return False
            if c0.weight.device.type != "meta" and not float(_fold_bn(c0, bn)[0].detach().abs().max()) < 65504.0:
                return False
    return True


def _template_pack(self, boxes, branches, z_fs):
    """The _ConvPack of conv_kernel for this head, or None where _template_packable refuses: rebuilt when a conv_kernel parameter / buffer or the
    template's shape changes (the version counters _TemplateCache is keyed on), dropped by invalidate_template_cache."""
    key = (_param_versions(branches), tuple(z_fs[0].shape), z_fs[0].device, z_fs[0].dtype)
    tp = getattr(self, "_hdn_template_pack", None)
    if tp is None or tp.key != key:
        if _template_packable(boxes, z_fs):
            tp = _pack_convs(boxes, "conv_kernel")
            tp.ok = tp.wsp is not None
        else:
            tp = _ConvPack()
            tp.ok = False
        tp.key = key
        object.__setattr__(self, "_hdn_template_pack", tp)
    return tp if tp.ok else None


def _search_pack(self, boxes, x_fs):
    """The _ConvPack of conv_search for the batched form (B > 1), or None where it does not apply; keyed as _PackedHead is."""
    key = (_head_key(self, boxes), tuple(x_fs[0].shape), x_fs[0].device, x_fs[0].dtype)
    sp = getattr(self, "_hdn_search_pack", None)
    if sp is None or sp.key != key:
        _, C, Hi, Wi = x_fs[0].shape
        if len(boxes) <= 4 and C == 256 and _patch_fits(Hi, Wi) and len(boxes) * x_fs[0].shape[0] <= 65535 and _packable_any_batch(self, boxes, x_fs):
            sp = _pack_convs(boxes, "conv_search")
            sp.ok = sp.wsp is not None
        else:
            sp = _ConvPack()
            sp.ok = False
        sp.key = key
        object.__setattr__(self, "_hdn_search_pack", sp)
    return sp if sp.ok else None


def head_conv_batch(x_fs, wsp, bsp, groups=2):
    """n levels [B, 256, Hi, Wi] through one launch of hdn_head_conv3x3_batch_f32 (3x3 / no padding + bias + ReLU with the stream `wsp` of
    _pack_conv_search and the bias `bsp` [n, CO]) -> [n, groups, B, CO / groups, Ho, Wo] contiguous: out[l, g] is a contiguous [B, CO / groups, Ho, Wo].
    An image that is dense NCHW or dense channels-last is read where it is, whatever the batch stride (a batch slice needs no copy)."""
    import ctypes

    from . import _lib

    x0 = x_fs[0]
    dev = _lib.require_device(*x_fs)
    n, (B, C, Hi, Wi) = len(x_fs), x0.shape
    if C != 256 or any(x.shape != x0.shape for x in x_fs):
        raise ValueError("head_conv_batch: every level must be [B, 256, Hi, Wi] of one shape")
    image = C * Hi * Wi
    forms = ((Hi * Wi, Wi, 1), (1, Wi * C, C))                                    # (channel, row, pixel) strides: NCHW, channels-last
    nhwc = 1 if tuple(x0.stride()[1:]) == forms[1] else 0

    def dense(x):
        return tuple(x.stride()[1:]) == forms[nhwc] and (B == 1 or x.stride(0) >= image)

    xs = [x.detach() for x in x_fs]
    xs = [x if dense(x) else x.contiguous(memory_format=torch.channels_last if nhwc else torch.contiguous_format) for x in xs]
    if B > 1 and len({x.stride(0) for x in xs}) > 1:                                # one batch stride per launch
        xs = [x if x.stride(0) == image else x.contiguous(memory_format=torch.channels_last if nhwc else torch.contiguous_format) for x in xs]
    xbs = image if B == 1 else xs[0].stride(0)
    CO = bsp.shape[1]
    out = torch.empty((n, groups, B, CO // groups, Hi - 2, Wi - 2), dtype=torch.float32, device=dev)
    with _lib.device_guard(dev):
        rc = _lib.load().hdn_head_conv3x3_batch_f32((ctypes.c_void_p * n)(*[t.data_ptr() for t in xs]), _lib.ptr(wsp), _lib.ptr(bsp), _lib.ptr(out),
                                                    n, B, groups, CO, Hi, Wi, nhwc, xbs, _lib.stream_ptr(dev))
    _lib.check(rc, "head_conv_batch")
    return out


def head_conv_search(x_fs, pk):
    """The n levels' conv_search (both branches) + bias + ReLU in one launch -> [n, 2 hidden, Ho, Wo] contiguous (hdn_head_conv3x3_f32)."""
    import ctypes

    from . import _lib

    x0 = x_fs[0]
    dev = _lib.require_device(*x_fs)
    n, (_, C, Hi, Wi) = len(x_fs), x0.shape
    nhwc = 0 if x0.is_contiguous() else 1
    xs = []
    for x in x_fs:
        x = x.detach()
        if not (x.is_contiguous() if nhwc == 0 else x.is_contiguous(memory_format=torch.channels_last)):
            x = x.contiguous() if nhwc == 0 else x.contiguous(memory_format=torch.channels_last)
        xs.append(x)
    CO = pk.bsp.shape[1]
    out = torch.empty((n, CO, Hi - 2, Wi - 2), dtype=torch.float32, device=dev)
    arr = ctypes.c_void_p * n
    with _lib.device_guard(dev):
        rc = _lib.load().hdn_head_conv3x3_f32(arr(*[t.data_ptr() for t in xs]), _lib.ptr(pk.wsp), _lib.ptr(pk.bsp),
                                              arr(*[out[i].data_ptr() for i in range(n)]), n, CO, Hi, Wi, nhwc, _lib.stream_ptr(dev))
    _lib.check(rc, "head_conv_search")
    return out


def head_tail(feats, pk, n):
    """feats [2n, H, Ho, Wo] -> out [2, om, Ho * Wo] through hdn_head_tail_f32 (pk: a _PackedHead with w1p)."""
    from . import _lib

    dev = _lib.require_device(feats)
    G, H = feats.shape[0], feats.shape[1]
    P = feats.shape[2] * feats.shape[3]
    om = pk.wf.shape[1]
    out = torch.empty((2, om, P), dtype=torch.float32, device=dev)
    with _lib.device_guard(dev):
        rc = _lib.load().hdn_head_tail_f32(_lib.ptr(feats), _lib.ptr(pk.w1p), _lib.ptr(pk.b1), _lib.ptr(pk.wf), _lib.ptr(pk.bf), _lib.ptr(out),
                                           n, H, P, om, _lib.stream_ptr(dev))
    _lib.check(rc, "head_tail")
    return out


def head_tail_batch(feats, pk, n, B):
    """feats [2n, B, H, Ho, Wo] -> (cls [B, oc, Ho, Wo], loc [B, ol, Ho, Wo]), contiguous views of ONE output buffer, through hdn_head_tail_batch_f32
    (pk: a _PackedHead with w1p)."""
    from . import _lib

    dev = _lib.require_device(feats)
    if feats.dim() != 5 or feats.shape[0] != 2 * n or feats.shape[1] != B or feats.dtype != torch.float32 or not feats.is_contiguous():
        raise ValueError(f"head_tail_batch: feats must be a contiguous float32 [{2 * n}, {B}, H, Ho, Wo], got {tuple(feats.shape)}")
    H, Ho, Wo = feats.shape[2:]
    P = Ho * Wo
    out = torch.empty(B * (pk.oc + pk.ol) * P, dtype=torch.float32, device=dev)
    with _lib.device_guard(dev):
        rc = _lib.load().hdn_head_tail_batch_f32(_lib.ptr(feats), _lib.ptr(pk.w1p), _lib.ptr(pk.b1), _lib.ptr(pk.wf), _lib.ptr(pk.bf), _lib.ptr(out),
                                                 n, B, H, P, pk.oc, pk.ol, _lib.stream_ptr(dev))
    _lib.check(rc, "head_tail_batch")
    split = B * pk.oc * P
    return out[:split].view(B, pk.oc, Ho, Wo), out[split:].view(B, pk.ol, Ho, Wo)


def _tail_lds_bytes(n, hidden, om):
    """What a workgroup of hdn_head_tail(_batch)_f32 stages (head_tail.hip; hdn_head_tail_lds_bytes): the split pixel tile of every level, b1, the branch's
    block of Wf and the waves' partial sums."""
    return n * (hidden * 128 + 4 * hidden + 4 * om * hidden) + (hidden // 32) * 8 * 32 * 4


def _tail_fits(n, hidden, om, w1):
    """The shapes and range hdn_head_tail_f32 / hdn_head_tail_batch_f32 take: hidden 128 or 256, at most 8 output rows and 4 levels, the staged operands
    inside the 160 KB of LDS, and the folded first 1x1 weights `w1` inside fp16 (two pieces).  Asks nothing of the device."""
    return (hidden in (128, 256) and 1 <= om <= 8 and 1 <= n <= 4 and _tail_lds_bytes(n, hidden, om) <= 160 * 1024
            and bool(float(w1.detach().abs().max()) < 65504.0))


def _pack_head(self, boxes, cs=None):
    n = len(boxes)
    pk = _PackedHead()
    pk.key = _head_key(self, boxes)
    if cs is None:
        cs = _pack_convs(boxes, "conv_search")               # (shared with the batched form: _search_pack hands its own over)
    pk.ws, pk.bs, pk.wsp, pk.bsp = cs.ws, cs.bs, cs.wsp, cs.bsp
    pk.hidden = hidden = boxes[0].cls.head[0].weight.shape[0]
    order = [box.cls for box in boxes] + [box.loc for box in boxes]          # stacked order: cls of every level, then loc
    w1, b1 = zip(*[_fold_bn(br.head[0], br.head[1]) for br in order])
    pk.w1 = torch.stack([w.reshape(hidden, -1) for w in w1]).contiguous()      # [2n, hidden, hidden]
    pk.b1 = torch.stack(b1).reshape(2 * n, hidden, 1).contiguous()
    dev, dt = pk.w1.device, pk.w1.dtype
    if self.weighted:
        cw, lw = F.softmax(self.cls_weight, 0), F.softmax(self.loc_weight, 0)
    else:
        cw = lw = torch.full((n,), 1.0 / n, device=dev, dtype=dt)
    lw = lw * self.loc_scale
    pk.oc, pk.ol = boxes[0].cls.head[3].weight.shape[0], boxes[0].loc.head[3].weight.shape[0]
    om = max(pk.oc, pk.ol)
    pk.wf = torch.zeros((2, om, n * hidden), device=dev, dtype=dt)
    pk.bf = torch.zeros((2, om, 1), device=dev, dtype=dt)
    for i, box in enumerate(boxes):
        pk.wf[0, :pk.oc, i * hidden:(i + 1) * hidden] = cw[i] * box.cls.head[3].weight.reshape(pk.oc, hidden)
        pk.wf[1, :pk.ol, i * hidden:(i + 1) * hidden] = lw[i] * box.loc.head[3].weight.reshape(pk.ol, hidden)
        pk.bf[0, :pk.oc, 0] += cw[i] * box.cls.head[3].bias
        pk.bf[1, :pk.ol, 0] += lw[i] * box.loc.head[3].bias
    # the whole tail as one launch (hdn_head_tail_f32) where its shapes allow; the two batched matrix products otherwise
    pk.w1p = _pack_w1(pk.w1) if pk.w1.is_cuda and _tail_fits(n, hidden, om, pk.w1) else None
    return pk


def _batched_forward(self, boxes, kern, x_fs, sp, circular):
    """Level 2 at B > 1: conv_search, the correlations and the tail as one launch each (head_conv_batch, xcorr_depthwise_multi into one feats buffer,
    head_tail_batch).  None where the tail does not fit (the caller goes on with the level-1 path)."""
    n, B = len(boxes), x_fs[0].shape[0]
    pk = getattr(self, "_hdn_packed_head", None)
    key = _head_key(self, boxes)
    if pk is None or pk.key != key:
        pk = _pack_head(self, boxes, sp)
        object.__setattr__(self, "_hdn_packed_head", pk)
    if pk.w1p is None or tuple(pk.w1.shape[1:]) != (sp.bsp.shape[1] // 2,) * 2:      # (the head's 1x1 is hidden x hidden on conv_search's channels)
        return None
    y = head_conv_batch(x_fs, sp.wsp, sp.bsp)                 # [n, 2, B, hidden, Ho, Wo]
    srch = [y[l, 0] for l in range(n)] + [y[l, 1] for l in range(n)]          # stacked order: cls of every level, then loc
    kern = list(kern[0::2]) + list(kern[1::2])
    shape = out_shape(srch[0].shape, kern[0].shape, circular)
    feats = torch.empty((2 * n, B, pk.hidden, shape[2], shape[3]), dtype=torch.float32, device=y.device)
    xcorr_depthwise_multi(srch, kern, circular=circular, outs=[feats[i] for i in range(2 * n)])
    return head_tail_batch(feats, pk, n, B)


def _packed_forward(self, boxes, kern, x_fs, circular):
    n = len(boxes)
    pk = getattr(self, "_hdn_packed_head", None)
    key = _head_key(self, boxes)
    if pk is None or pk.key != key:
        pk = _pack_head(self, boxes)
        object.__setattr__(self, "_hdn_packed_head", pk)
    h = pk.hidden
    s_cls, s_loc = [], []
    Hi, Wi = x_fs[0].shape[2], x_fs[0].shape[3]
    rows = min((63 + Wi - 3) // (Wi - 2) + 3, Hi) if Wi > 2 else 0          # patch rows of 64 consecutive output pixels (head_conv.hip)
    use_conv = (pk.wsp is not None and x_fs[0].shape[1] == 256 and Hi >= 3 and Wi >= 3 and rows * Wi <= 224
                and not getattr(self, "_hdn_no_head_conv", False))
    if use_conv:
        y = head_conv_search(x_fs, pk)
        s_cls = [y[l:l + 1, :h] for l in range(n)]
        s_loc = [y[l:l + 1, h:] for l in range(n)]
    for l in range(0 if not use_conv else n, n):
        # NCHW in, NCHW out: the correlation kernels read contiguous (b, c) planes.  A channels-last search feature (a channels-last
        # backbone / neck) is converted ONCE here; left as it is, the convolution's channels-last output cost 11 layout copies per
        # forward further down (54 of 201 us per head at 256 channels, tools/experiments/exp_head_profile.py).
        xl = x_fs[l] if x_fs[l].is_contiguous() else x_fs[l].contiguous()
        y = F.conv2d(xl, pk.ws[l])                       # [1, 2 hidden, Ho, Wo]: both branches of the level
        if not y.is_contiguous():
            y = y.contiguous()
        bias_relu_(y, pk.bs[l])
        s_cls.append(y[:, :h])
        s_loc.append(y[:, h:])
    k_cls, k_loc = kern[0::2], kern[1::2]                 # the template cache holds (cls, loc) per level
    shape = out_shape(s_cls[0].shape, k_cls[0].shape, circular)
    feats = torch.empty((2 * n, h, shape[2], shape[3]), dtype=torch.float32, device=y.device)
    xcorr_depthwise_multi(s_cls + s_loc, list(k_cls) + list(k_loc), circular=circular, outs=[feats[i:i + 1] for i in range(2 * n)])
    if pk.w1p is not None and not getattr(self, "_hdn_no_head_tail", False):
        out = head_tail(feats, pk, n)
    else:
        hid = torch.baddbmm(pk.b1, pk.w1, feats.view(2 * n, h, -1)).relu_()
        out = torch.baddbmm(pk.bf, pk.wf, hid.view(2, n * h, -1))
    return (out[0, :pk.oc].reshape(1, pk.oc, shape[2], shape[3]), out[1, :pk.ol].reshape(1, pk.ol, shape[2], shape[3]))


def fused_forward(self, z_fs, x_fs, circular=None):
    """MultiBAN.forward / MultiCircBAN.forward (ban.py:102-127, ban_lp.py:66-92) with one correlation launch and
    cached template-branch features.  `self` needs box2.., (cls|loc)_weight, loc_scale, weighted.

    Inference only (runs under no_grad, BN in eval mode): in training mode it defers to the class's original forward
    when install() saved one (`_hdn_orig_forward`), and raises otherwise, rather than silently dropping gradients.  The deferred
    forward trains: the xcorr_depthwise / xcorr_depthwise_circular it resolves are differentiable (hdn_amd/xcorr.py)."""
    if self.training:
        orig = getattr(type(self), "_hdn_orig_forward", None)
        if orig is not None:
            return orig(self, z_fs, x_fs)
        raise RuntimeError("hdn_amd heads are inference-only (fused forward under no_grad): call .eval(), or train with "
                           "the reference's own modules (hdn_amd.install.uninstall() restores them)")
    z_fs, x_fs = list(z_fs), list(x_fs)
    n = len(z_fs)
    boxes = [getattr(self, "box" + str(i + 2)) for i in range(n)]
    branches = [br for box in boxes for br in (box.cls, box.loc)]
    if getattr(branches[0], "_hdn_owner", None) is not self:
        object.__setattr__(branches[0], "_hdn_owner", self)       # (plain attribute, not a registered sub-module: where _param_versions keeps its references)
    if circular is None:
        circular = bool(getattr(boxes[0].cls, "_circular", False)) or type(boxes[0].cls).__name__.endswith("Circ")
    with torch.no_grad():
        cache = getattr(self, "_hdn_template_cache", None)
        hip_heads_on = _hip_heads_on(self)
        if cache is None or not cache.matches(z_fs, branches, False):
            tp = _template_pack(self, boxes, branches, z_fs) if hip_heads_on else None
            if tp is not None:
                y = head_conv_batch(z_fs, tp.wsp, tp.bsp)     # one launch; (cls, loc) per level, each a contiguous [B, hidden, h, w] view
                kern = [y[l, g] for l in range(n) for g in range(2)]
            else:
                kern = [br.conv_kernel(z).contiguous() for box, z in zip(boxes, z_fs) for br in (box.cls, box.loc)]   # (NCHW once, not per frame)
            cache = _TemplateCache(z_fs, branches, False, kern)
            object.__setattr__(self, "_hdn_template_cache", cache)
        kern = cache.kern
        pv = getattr(self, "_hdn_packable", None)
        sig = (tuple(x_fs[0].shape), x_fs[0].device, x_fs[0].dtype)
        if pv is None or pv[0] != sig:
            pv = (sig, 2 * n <= 8 and _packable(self, boxes, x_fs))
            object.__setattr__(self, "_hdn_packable", pv)
        if (pv[1] and all(x.shape == x_fs[0].shape for x in x_fs) and all(k.shape == kern[0].shape for k in kern)
                and not getattr(self, "_hdn_no_packed_head", False)):
            return _packed_forward(self, boxes, kern, x_fs, circular)
        sp = _search_pack(self, boxes, x_fs) if hip_heads_on and x_fs[0].shape[0] > 1 else None
        if (sp is not None and 2 * n <= 8 and _hip_heads_level_of(self) == 2 and all(k.shape == kern[0].shape for k in kern)
                and kern[0].shape[:2] == (x_fs[0].shape[0], sp.bsp.shape[1] // 2) and not getattr(self, "_hdn_no_head_tail", False)):
            out = _batched_forward(self, boxes, kern, x_fs, sp, circular)     # level 2: the 1x1 tail too, three launches in all
            if out is not None:
                return out
        if sp is not None:
            y = head_conv_batch(x_fs, sp.wsp, sp.bsp)         # conv_search of every level and both branches at B > 1: one launch
            srch = [y[l, g] for l in range(n) for g in range(2)]
        else:
            srch = [br.conv_search(x) for box, x in zip(boxes, x_fs) for br in (box.cls, box.loc)]
        same = all(k.shape == kern[0].shape for k in kern) and all(s.shape == srch[0].shape for s in srch)
        if same and len(kern) <= 8:
            feats = xcorr_depthwise_multi(srch, kern, circular=circular)
        else:
            one = xcorr_depthwise_circular if circular else xcorr_depthwise
            feats = [one(s, k) for s, k in zip(srch, kern)]
        cls = [boxes[i].cls.head(feats[2 * i]) for i in range(n)]
        loc = [boxes[i].loc.head(feats[2 * i + 1]) * self.loc_scale[i] for i in range(n)]
        if self.weighted:
            cw, lw = F.softmax(self.cls_weight, 0), F.softmax(self.loc_weight, 0)
            c = sum(cls[i] * cw[i] for i in range(n))
            l = sum(loc[i] * lw[i] for i in range(n))
            return c, l
        return sum(cls) / n, sum(loc) / n


class MultiBAN(nn.Module):
    _box = DepthwiseBAN

    def __init__(self, in_channels, cls_out_channels, weighted=False):
        super().__init__()
        self.weighted = weighted
        for i in range(len(in_channels)):
            self.add_module("box" + str(i + 2), self._box(in_channels[i], in_channels[i], cls_out_channels))
        if self.weighted:
            self.cls_weight = nn.Parameter(torch.ones(len(in_channels)))
            self.loc_weight = nn.Parameter(torch.ones(len(in_channels)))
        self.loc_scale = nn.Parameter(torch.ones(len(in_channels)))

    def forward(self, z_fs, x_fs):
        return fused_forward(self, z_fs, x_fs)


class MultiCircBAN(MultiBAN):
    _box = DepthwiseCircBAN
