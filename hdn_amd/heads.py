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

from .ops import _pack_conv_search, _pack_w1, bias_relu_, head_conv_batch, head_conv_search, head_tail, head_tail_batch
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
    tp = getattr(head, "_hdn_template_pack", None) if _hip_heads_on(head) else None
    if tp is not None and not (tp.ok and tp.key[0] == _param_versions(branches)):
        tp = None                                            # (never built here: only the pack the forward took, for these weights)
    with torch.no_grad():
        for dst, src in zip(cache.kern, _template_features(boxes, [z[sel] for z in z_fs], tp)):   # (the pack holds weights only: it serves any batch)
            dst[sel].copy_(src)
    cache.z_versions = tuple(z._version for z in z_fs)
    return True


_HIP_HEADS_LEVEL = None


def hip_heads_level() -> int:
    """HDN_HIP_HEADS as a level, read once: 0 off (unset, empty or "0" after strip(): the default), 1 the template branch at any batch and conv_search at
    B > 1 on hdn_head_conv3x3_batch_f32, 2 also the 1x1 tail at B > 1 on hdn_head_tail_batch_f32.  Any other value is level 1."""
    global _HIP_HEADS_LEVEL
    if _HIP_HEADS_LEVEL is None:
        v = os.environ.get("HDN_HIP_HEADS", "0").strip()
        _HIP_HEADS_LEVEL = 0 if v in ("", "0") else 2 if v == "2" else 1
    return _HIP_HEADS_LEVEL


def hip_heads() -> bool:
    """Is HDN_HIP_HEADS on at any level?"""
    return hip_heads_level() >= 1


def _hip_heads_level_of(head) -> int:
    v = getattr(head, "_hdn_hip_heads", None)                # the per-head attribute overrides the environment.  True and 1: level 1; 2: level 2
    if v is None:
        return hip_heads_level()
    return 2 if (v is not True and v == 2) else 1 if v else 0


def _hip_heads_on(head) -> bool:
    return _hip_heads_level_of(head) >= 1


class _ConvPack:
    """The 3x3 convolutions of one side (conv_search or conv_kernel) of all levels, BatchNorm folded, cls || loc along CO: ws / bs the fp32 weights
    and biases per level, wsp / bsp the stream and the [n, CO] bias hdn_head_conv3x3(_batch)_f32 take (None where the kernel does not fit).
    `key`: the version counters it was built from; `ok`: its path's predicate said yes for that key and the kernel fits."""

    __slots__ = ("key", "ok", "ws", "bs", "wsp", "bsp")

    def __init__(self):
        self.wsp = self.bsp = None


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


def _bn_folds(bn):
    """_fold_bn folds the running statistics and the affine weights: eval-mode BatchNorm only."""
    return not (bn.training or not bn.track_running_stats or not bn.affine or bn.running_mean is None)


def _conv_bn_relu_eval(seq):
    """Is `seq` the 3x3 stage of the reference's DepthwiseXCorr in eval mode: Sequential(Conv2d without bias / stride 1 / no padding / no dilation /
    groups 1, a BatchNorm2d _fold_bn can fold, ReLU)?  (The kernel size is the caller's business: it shows in the weight's shape.)"""
    if not (isinstance(seq, nn.Sequential) and len(seq) == 3 and isinstance(seq[0], nn.Conv2d) and isinstance(seq[1], nn.BatchNorm2d)
            and isinstance(seq[2], nn.ReLU)):
        return False
    c = seq[0]
    return _bn_folds(seq[1]) and c.bias is None and c.stride == (1, 1) and c.padding == (0, 0) and c.dilation == (1, 1) and c.groups == 1


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
            hd = br.head
            if not (_conv_bn_relu_eval(br.conv_search) and isinstance(hd, nn.Sequential) and len(hd) == 4 and isinstance(hd[0], nn.Conv2d)
                    and isinstance(hd[1], nn.BatchNorm2d) and isinstance(hd[2], nn.ReLU) and isinstance(hd[3], nn.Conv2d) and _bn_folds(hd[1])
                    and hd[0].bias is None and hd[0].kernel_size == (1, 1) and hd[3].kernel_size == (1, 1) and hd[3].bias is not None):
                return False
            sig = (tuple(br.conv_search[0].weight.shape), tuple(hd[0].weight.shape))
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


def _in_fp16(ws):
    """Folded |w| < 65504 everywhere (the kernels split a weight into two fp16 pieces; NaN is out).  `meta` weights have no values to look at: in."""
    return ws[0].device.type == "meta" or all(float(w.detach().abs().max()) < 65504.0 for w in ws)


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
    if (w0.is_cuda and len(boxes) <= 4 and tuple(w0.shape[1:]) == (256, 3, 3) and w0.shape[0] % 32 == 0 and all(w.shape == w0.shape for w in pk.ws)
            and _in_fp16(pk.ws)):
        pk.wsp, pk.bsp = _pack_conv_search(pk.ws), torch.stack(pk.bs).contiguous()
    return pk


def _template_packable(boxes, z_fs, need_gpu=True, in_range=True):
    """The template branch as one launch of hdn_head_conv3x3_batch_f32, at any B: fp32 on a GPU (need_gpu=False: anywhere, for host tests), every
    level the same shape with 256 channels inside the kernel's patch limit, n <= 4, and conv_kernel of every (level, branch) the reference's
    3x3 stage (_conv_bn_relu_eval) with one hidden width (a multiple of 32: the cls and loc halves are tile-aligned groups) and folded |w| < 65504
    (in_range=False: not looked at, for a caller that goes on to _pack_convs, which folds the weights anyway and looks then)."""
    z0 = z_fs[0]
    n = len(boxes)
    if (need_gpu and not z0.is_cuda) or z0.dtype != torch.float32 or z0.dim() != 4 or any(z.shape != z0.shape for z in z_fs):
        return False
    B, C, Hi, Wi = z0.shape
    if n != len(z_fs) or not 1 <= n <= 4 or C != 256 or B < 1 or n * B > 65535 or not _patch_fits(Hi, Wi):
        return False
    stages = [br.conv_kernel for box in boxes for br in (box.cls, box.loc)]
    if not all(_conv_bn_relu_eval(ck) for ck in stages):
        return False
    shape = tuple(stages[0][0].weight.shape)
    if shape[1:] != (256, 3, 3) or shape[0] % 32 != 0 or any(tuple(ck[0].weight.shape) != shape for ck in stages):
        return False
    return not in_range or _in_fp16([_fold_bn(ck[0], ck[1])[0] for ck in stages])


def _conv_pack(self, attr, key, applies, boxes, name):
    """The _ConvPack of side `name` kept in attribute `attr` of the head, or None where `applies()` refuses or the kernel does not fit: rebuilt when
    `key` changes (version counters and the input's shape), dropped by invalidate_template_cache."""
    pk = getattr(self, attr, None)
    if pk is None or pk.key != key:
        pk = _pack_convs(boxes, name) if applies() else _ConvPack()
        pk.key, pk.ok = key, pk.wsp is not None
        object.__setattr__(self, attr, pk)
    return pk if pk.ok else None


def _template_pack(self, boxes, branches, z_fs):
    """The _ConvPack of conv_kernel for this head, or None where _template_packable refuses; keyed on what _TemplateCache is and the template's shape."""
    key = (_param_versions(branches), tuple(z_fs[0].shape), z_fs[0].device, z_fs[0].dtype)
    return _conv_pack(self, "_hdn_template_pack", key, lambda: _template_packable(boxes, z_fs, in_range=False), boxes, "conv_kernel")


def _search_pack(self, boxes, x_fs):
    """The _ConvPack of conv_search for the batched form (B > 1), or None where it does not apply; keyed as _PackedHead is."""
    B, C, Hi, Wi = x_fs[0].shape
    key = (_head_key(self, boxes), tuple(x_fs[0].shape), x_fs[0].device, x_fs[0].dtype)
    return _conv_pack(self, "_hdn_search_pack", key, lambda: (len(boxes) <= 4 and C == 256 and _patch_fits(Hi, Wi) and len(boxes) * B <= 65535
                                                              and _packable_any_batch(self, boxes, x_fs)), boxes, "conv_search")


def _template_features(boxes, zs, tp):
    """conv_kernel(z) of every (level, branch), (cls, loc) per level: with the template pack `tp` one launch, each a contiguous [B, hidden, h, w] view
    of its output; without one (None) through the modules, in whatever layout they answer."""
    if tp is None:
        return [br.conv_kernel(z) for box, z in zip(boxes, zs) for br in (box.cls, box.loc)]
    y = head_conv_batch(zs, tp.wsp, tp.bsp)
    return [y[l, g] for l in range(len(zs)) for g in range(2)]


def _tail_lds_bytes(n, hidden, om):
    """What a workgroup of hdn_head_tail(_batch)_f32 stages (head_tail.hip; hdn_head_tail_lds_bytes): the split pixel tile of every level, b1, the branch's
    block of Wf and the waves' partial sums."""
    return n * (hidden * 128 + 4 * hidden + 4 * om * hidden) + (hidden // 32) * 8 * 32 * 4


def _tail_fits(n, hidden, om, w1):
    """The shapes and range hdn_head_tail_f32 / hdn_head_tail_batch_f32 take: hidden 128 or 256, at most 8 output rows and 4 levels, the staged operands
    inside the 160 KB of LDS, and the folded first 1x1 weights `w1` inside fp16 (two pieces).  Asks nothing of the device."""
    return (hidden in (128, 256) and 1 <= om <= 8 and 1 <= n <= 4 and _tail_lds_bytes(n, hidden, om) <= 160 * 1024
            and _in_fp16([w1]))


def _level_weights(self, n, like):
    """(cw, lw): what level i counts in the cls / loc sum (loc_scale apart) - the softmax of cls_weight / loc_weight of a weighted head, 1 / n otherwise."""
    if self.weighted:
        return F.softmax(self.cls_weight, 0), F.softmax(self.loc_weight, 0)
    even = torch.full((n,), 1.0 / n, device=like.device, dtype=like.dtype)
    return even, even


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
    cw, lw = _level_weights(self, n, pk.w1)
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


def _packed_head(self, boxes, cs=None):
    """The head's _PackedHead, rebuilt (around the _ConvPack `cs` of conv_search where the caller has one) when a tensor it was built from changed."""
    pk = getattr(self, "_hdn_packed_head", None)
    if pk is None or pk.key != _head_key(self, boxes):
        pk = _pack_head(self, boxes, cs)
        object.__setattr__(self, "_hdn_packed_head", pk)
    return pk


def _batched_forward(self, boxes, kern, x_fs, sp, circular):
    """Level 2 at B > 1: conv_search, the correlations and the tail as one launch each (head_conv_batch, xcorr_depthwise_multi into one feats buffer,
    head_tail_batch).  None where the tail does not fit (the caller goes on with the level-1 path)."""
    n, B = len(boxes), x_fs[0].shape[0]
    pk = _packed_head(self, boxes, sp)
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
    pk = _packed_head(self, boxes)
    h = pk.hidden
    s_cls, s_loc = [], []
    use_conv = (pk.wsp is not None and x_fs[0].shape[1] == 256 and _patch_fits(x_fs[0].shape[2], x_fs[0].shape[3])
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


def _module_forward(self, boxes, kern, x_fs, sp, circular, one_launch):
    """Module by module around the correlations; with the _ConvPack `sp` of conv_search (level 1 at B > 1) that side as one launch.  `one_launch`: the
    template features are of one shape and at most 8, what hdn_xcorr_depthwise_multi_f32 asks besides search features of one shape."""
    n = len(boxes)
    if sp is not None:
        y = head_conv_batch(x_fs, sp.wsp, sp.bsp)             # conv_search of every level and both branches at B > 1: one launch
        srch = [y[l, g] for l in range(n) for g in range(2)]
    else:
        srch = [br.conv_search(x) for box, x in zip(boxes, x_fs) for br in (box.cls, box.loc)]
    if one_launch and all(s.shape == srch[0].shape for s in srch):
        feats = xcorr_depthwise_multi(srch, kern, circular=circular)
    else:
        one = xcorr_depthwise_circular if circular else xcorr_depthwise
        feats = [one(s, k) for s, k in zip(srch, kern)]
    cls = [boxes[i].cls.head(feats[2 * i]) for i in range(n)]
    loc = [boxes[i].loc.head(feats[2 * i + 1]) * self.loc_scale[i] for i in range(n)]
    if not self.weighted:
        return sum(cls) / n, sum(loc) / n                     # (one division of the sum, as the reference has it: not _level_weights' 1 / n per level)
    cw, lw = _level_weights(self, n, cls[0])
    return sum(cls[i] * cw[i] for i in range(n)), sum(loc[i] * lw[i] for i in range(n))


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
        level = _hip_heads_level_of(self)
        cache = getattr(self, "_hdn_template_cache", None)
        if cache is None or not cache.matches(z_fs, branches, False):
            tp = _template_pack(self, boxes, branches, z_fs) if level >= 1 else None
            kern = [k.contiguous() for k in _template_features(boxes, z_fs, tp)]     # (NCHW once, not per frame; the pack's views are as they are)
            cache = _TemplateCache(z_fs, branches, False, kern)
            object.__setattr__(self, "_hdn_template_cache", cache)
        kern = cache.kern
        # the shape facts the four forms ask about
        B = x_fs[0].shape[0]
        one_x = all(x.shape == x_fs[0].shape for x in x_fs)
        one_k = all(k.shape == kern[0].shape for k in kern)
        few = 2 * n <= 8                                      # what one launch of hdn_xcorr_depthwise_multi_f32 takes
        pv = getattr(self, "_hdn_packable", None)
        sig = (tuple(x_fs[0].shape), x_fs[0].device, x_fs[0].dtype)
        if pv is None or pv[0] != sig:
            pv = (sig, few and _packable(self, boxes, x_fs))
            object.__setattr__(self, "_hdn_packable", pv)
        if pv[1] and one_x and one_k and not getattr(self, "_hdn_no_packed_head", False):
            return _packed_forward(self, boxes, kern, x_fs, circular)                # B = 1, packed
        sp = _search_pack(self, boxes, x_fs) if level >= 1 and B > 1 else None
        if (sp is not None and few and level == 2 and one_k and kern[0].shape[:2] == (B, sp.bsp.shape[1] // 2)
                and not getattr(self, "_hdn_no_head_tail", False)):
            out = _batched_forward(self, boxes, kern, x_fs, sp, circular)            # level 2: the 1x1 tail too, three launches in all
            if out is not None:
                return out
        return _module_forward(self, boxes, kern, x_fs, sp, circular, one_k and few)


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
