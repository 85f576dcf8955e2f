"""The similarity model's training geometry on HIP kernels: what lies between the head maps and the samplers in the reference's training forward.

    polar_pick(cls, loc)                                           <- hdn/models/model_builder_e2e_unconstrained_v2.py:377 (the `* STRIDE` folded in)
    similarity_warps(cls_lp, loc_lp, polar, temp_cx, temp_cy, search_poly)
                                                                   <- :390-415: lp_pick, the four combine_affine calls, pred_points, aug_sear_points
    lp_pick, combine_affine_c0_v2, combine_affine_lt0              <- hdn/utils/point.py:35, hdn/utils/transform.py:442, :486 (the names :27-28 import)
    get_polar_from_two_para_loc                                    <- hdn/models/logpolar.py:304 (Polar_Pick's method)

The reference spends more than a hundred small launches each way on these lines and uploads from pageable host memory in several of them
(torch.from_numpy(points).cuda(), torch.zeros(batch, 2).cuda(), torch.ones(...).cuda()), which no graph capture can hold.  Here each function is one
launch forward and one backward (csrc/simi_geometry.hip; formulas: include/hdn_hip.h): the point table is computed from (stride, S) in the kernel,
nothing is created on, uploaded from or read by the host, and polar_pick + similarity_warps + their backward can be captured in a graph.

The argmax follows csrc/argmax_order.h: NaN first, the larger value, the lower index - torch.argmax's first maximum on finite maps.  lp_pick's
scores are the fp32 softmax of the two logits, as in the reference, so cells that saturate to 1.0f tie and the lowest index wins.  Gradients are first
order only.  An input the reference treats as data (cls, cls_lp, temp_cx, temp_cy, search_poly, cx, cy) raises if it requires grad; it is never
silently detached.  Only cls_out_channels == 2 is restated.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

WARP_KEYS = ("scale", "rot", "affine_m", "affine_m_lt0", "affine_m_c_aug", "affine_m_lt0_aug", "pred_points", "aug_sear_points")


def lp_constants(map_size):
    """(mag, rot_unit) of lp_pick as the reference forms them (point.py:50-51): Python floats that meet fp32 tensors (the kernels round them to fp32)."""
    return float(np.log(map_size / 2) / map_size), float(2 * np.pi / map_size)


def _data(t, name):
    """An input the reference treats as data: it must not ask for a gradient."""
    if isinstance(t, torch.Tensor) and t.requires_grad:
        raise ValueError(f"{name} is data in the reference's training forward (no gradient reaches it); it requires grad here - detach it explicitly")
    return t


def _wants_grad(*ts):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


def _map(t, name, C):
    """[B,C,S,S] -> (B, S)"""
    if t.dim() != 4 or t.shape[1] != C or t.shape[2] != t.shape[3] or t.shape[2] < 1 or t.shape[0] < 1:
        raise ValueError(f"{name} must be [B,{C},S,S] with B, S >= 1, got {list(t.shape)}")
    return int(t.shape[0]), int(t.shape[2])


def _want(t, name, shape):
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")


def _c(t):
    return t.detach().contiguous()


def _new(shape, dev, dtype=torch.float32):
    """an output buffer: every element of it is written by the launch it is made for"""
    return torch.empty(shape, dtype=dtype, device=dev)


# ---------------------------------------------------------------------------------------------------------------------------------- the picks
def _pick_forward(mode, stride, mult, mag, rot_unit, cls, loc):
    """One launch of hdn_point_pick_f32 -> (out, best_idx): out [B,2] (mode 0) or [2,B] (mode 1: scale, rot), best_idx int32 [B]."""
    dev = _lib.require_device(cls, loc)
    B, S = _map(cls, "cls", 2)
    _want(loc, "loc", (B, 2 if mode == 0 else 4, S, S))
    out = _new((B, 2) if mode == 0 else (2, B), dev)
    best = _new(B, dev, torch.int32)
    cls, loc = _c(cls), _c(loc)
    _lib.launch("point_pick", dev, _lib.load().hdn_point_pick_f32, _lib.ptr(cls), _lib.ptr(loc), _lib.ptr(out), _lib.ptr(best), B, S, 2,
                int(mode), int(stride), float(mult), float(mag), float(rot_unit))
    return out, best


def _pick_backward(mode, mult, mag, rot_unit, best, grad_out, out, shape):
    """One launch of hdn_point_pick_bwd_f32 -> the gradient of loc, full size, every element written by the call."""
    dev = _lib.require_device(grad_out, out)
    g = _new(tuple(shape), dev)
    grad_out, out = _c(grad_out), _c(out)
    _lib.launch("point_pick_backward", dev, _lib.load().hdn_point_pick_bwd_f32, _lib.ptr(best), _lib.ptr(grad_out), _lib.ptr(out), _lib.ptr(g),
                int(shape[0]), int(shape[2]), int(mode), float(mult), float(mag), float(rot_unit))
    return g


class _PointPick(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mode, stride, mult, mag, rot_unit, cls, loc):
        out, best = _pick_forward(mode, stride, mult, mag, rot_unit, cls, loc)
        ctx.cfg = (mode, mult, mag, rot_unit, tuple(loc.shape))
        ctx.save_for_backward(best, out)
        ctx.mark_non_differentiable(best)
        return out, best

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, _grad_best):
        mode, mult, mag, rot_unit, shape = ctx.cfg
        best, out = ctx.saved_tensors
        return (None,) * 6 + (_pick_backward(mode, mult, mag, rot_unit, best, grad_out, out, shape),)


def _pick(mode, stride, mult, mag, rot_unit, cls, loc):
    _data(cls, "cls")
    if _wants_grad(loc):
        return _PointPick.apply(mode, stride, mult, mag, rot_unit, cls, loc)
    return _pick_forward(mode, stride, mult, mag, rot_unit, cls, loc)


def polar_pick(cls, loc, stride=8, return_index=False, mult=None):
    """:377 in one launch: cls [B,2,S,S], loc [B,2,S,S] (the raw head output) -> polar [B,2] = point(best) - stride * loc[:, :, best], best =
    argmax of the raw class-1 logit; carries the graph to loc.  mult: the multiplier of loc where it is not the stride (1 for a loc that was
    multiplied already).  return_index=True: (polar, best_idx int32 [B])."""
    out, best = _pick(0, stride, stride if mult is None else mult, 0.0, 0.0, cls, loc)
    return (out, best) if return_index else out


def lp_pick(cls, loc, CLS_OUT_CHANNELS, STRIDE, STRIDE_LP, OUTPUT_SIZE_LP, MAP_SIZE, return_index=False):
    """point.py:35 under its own signature: cls [B,2,S,S], loc [B,4,S,S] -> (scale [B], rot [B]); carries the graph to loc."""
    if CLS_OUT_CHANNELS != 2:
        raise ValueError(f"hdn_amd.lp_pick restates cls_out_channels == 2 only (every training configuration of the reference), got {CLS_OUT_CHANNELS}")
    if isinstance(cls, torch.Tensor) and cls.dim() == 4 and cls.shape[2] != OUTPUT_SIZE_LP:
        raise ValueError(f"OUTPUT_SIZE_LP = {OUTPUT_SIZE_LP} is not the side of cls {list(cls.shape)}: the point table would belong to another map")
    mag, rot_unit = lp_constants(MAP_SIZE)
    out, best = _pick(1, STRIDE, STRIDE_LP, mag, rot_unit, cls, loc)
    return (out[0], out[1], best) if return_index else (out[0], out[1])


def analytic_points(stride, size):
    """generate_points(stride, size) of the reference (point.py:13, logpolar.py:208): float32 [size^2, 2], x by column, y by row."""
    ori = -(size // 2) * stride
    ax = (ori + stride * np.arange(size)).astype(np.float32)
    x, y = np.meshgrid(ax, ax)
    return np.stack([x.ravel(), y.ravel()], 1)


def _table_geometry(points):
    """(stride, S) if the CPU tensor `points` is generate_points(stride, S) for an integer stride >= 1, else None."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 2 or points.shape[0] < 1:
        return None
    p = points.detach().cpu().numpy()
    S = int(round(p.shape[0] ** 0.5))
    if S * S != p.shape[0]:
        return None
    stride = float(p[1, 0] - p[0, 0]) if S > 1 else 1.0
    if stride < 1 or stride != int(stride):
        return None
    return (int(stride), S) if np.array_equal(p, analytic_points(int(stride), S)) else None


def make_get_polar(fallback=None):
    """Polar_Pick.get_polar_from_two_para_loc (logpolar.py:304) as a method: (stride, S) come from self.points, compared once with the analytic table
    on the CPU tensor; on a foreign table the call goes to `fallback` (the method this one replaced) or raises without one."""

    def get_polar_from_two_para_loc(self, cls, loc):
        key = getattr(self, "_hdn_points_geometry", None)
        if key is None or key[0] is not self.points:
            key = (self.points, _table_geometry(self.points))
            object.__setattr__(self, "_hdn_points_geometry", key)
        if key[1] is None:
            if fallback is None:
                raise ValueError("self.points is not generate_points(stride, size); hdn_amd computes the table from (stride, size) and has no other form")
            return fallback(self, cls, loc)
        stride, S = key[1]
        if isinstance(cls, torch.Tensor) and cls.dim() == 4 and cls.shape[2] != S:
            raise ValueError(f"self.points is the table of a {S} x {S} map, cls is {list(cls.shape)}")
        return polar_pick(cls, loc, stride=stride, mult=1.0)       # the caller passes loc * STRIDE (:377)

    get_polar_from_two_para_loc._hdn_wraps = fallback
    return get_polar_from_two_para_loc


get_polar_from_two_para_loc = make_get_polar(None)


# ------------------------------------------------------------------------------------------------------------------------ the two matrices
def _centre(cx, cy):
    """(cx tensor | None, cy tensor | None, cx scalar, cy scalar)"""
    vec = isinstance(cx, torch.Tensor), isinstance(cy, torch.Tensor)
    if vec[0] != vec[1]:
        raise TypeError("cx and cy must both be tensors [B] or both be numbers")
    return (cx, cy, 0.0, 0.0) if vec[0] else (None, None, float(cx), float(cy))


def _affine_prepare(nm_shift, scale, rot, cx, cy):
    cxt, cyt, cxs, cys = _centre(cx, cy)
    dev = _lib.require_device(nm_shift, scale, rot, *([cxt, cyt] if cxt is not None else []))
    if nm_shift.dim() != 2 or nm_shift.shape[1] != 2 or nm_shift.shape[0] < 1:
        raise ValueError(f"nm_shift must be [B,2] with B >= 1, got {list(nm_shift.shape)}")
    B = int(nm_shift.shape[0])
    for t, name in ((scale, "scale"), (rot, "rot"), (cxt, "cx"), (cyt, "cy")):
        if t is not None:
            _want(t, name, (B,))
    args = (_c(nm_shift), _c(scale), _c(rot), None if cxt is None else _c(cxt), None if cyt is None else _c(cyt))
    return dev, B, args, (cxs, cys)


def _affine_forward(kind, scale_h, in_sz, out_sz, cx, cy, nm_shift, scale, rot):
    dev, B, t, sc = _affine_prepare(nm_shift, scale, rot, cx, cy)
    out = _new((B, 2, 3), dev)
    _lib.launch("simi_affine", dev, _lib.load().hdn_simi_affine_f32, *(_lib.opt(v) for v in t), *sc, _lib.ptr(out), B, int(kind), int(bool(scale_h)),
                float(in_sz), float(out_sz))
    return out


def _affine_backward(kind, scale_h, in_sz, out_sz, cx, cy, nm_shift, scale, rot, grad, need=(True, True, True)):
    """(grad_nm_shift | None, grad_scale | None, grad_rot | None): one launch of hdn_simi_affine_bwd_f32."""
    dev, B, t, sc = _affine_prepare(nm_shift, scale, rot, cx, cy)
    _lib.require_device(grad)
    _want(grad, "grad", (B, 2, 3))
    gs = [_new(s, dev) if w else None for s, w in zip(((B, 2), (B,), (B,)), need)]
    grad = _c(grad)
    _lib.launch("simi_affine_backward", dev, _lib.load().hdn_simi_affine_bwd_f32, *(_lib.opt(v) for v in t), *sc, _lib.ptr(grad),
                *(_lib.opt(g) for g in gs), B, int(kind), int(bool(scale_h)), float(in_sz), float(out_sz))
    return tuple(gs)


class _SimiAffine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, scale_h, in_sz, out_sz, cx, cy, nm_shift, scale, rot):
        ctx.cfg = (kind, scale_h, in_sz, out_sz)
        vec = isinstance(cx, torch.Tensor)
        ctx.centre = None if vec else (cx, cy)
        ctx.save_for_backward(nm_shift, scale, rot, *((cx, cy) if vec else ()))
        return _affine_forward(kind, scale_h, in_sz, out_sz, cx, cy, nm_shift, scale, rot)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        need = tuple(ctx.needs_input_grad[6:9])
        if not any(need):
            return (None,) * 9
        nm_shift, scale, rot, *c = ctx.saved_tensors
        cx, cy = c if c else ctx.centre
        return (None,) * 6 + _affine_backward(*ctx.cfg, cx, cy, nm_shift, scale, rot, grad, need)


def _affine(kind, scale_h, in_sz, out_sz, cx, cy, nm_shift, scale, rot):
    _data(cx, "cx")
    _data(cy, "cy")
    if _wants_grad(nm_shift, scale, rot):
        return _SimiAffine.apply(kind, scale_h, in_sz, out_sz, cx, cy, nm_shift, scale, rot)
    return _affine_forward(kind, scale_h, in_sz, out_sz, cx, cy, nm_shift, scale, rot)


def combine_affine_c0_v2(cx, cy, nm_shift, scale, rot, scale_h, in_sz, out_sz):
    """transform.py:442 under its own signature: cx, cy numbers or [B], nm_shift [B,2], scale, rot [B] -> [B,2,3]; the graph goes to nm_shift, scale, rot."""
    return _affine(0, scale_h, in_sz, out_sz, cx, cy, nm_shift, scale, rot)


def combine_affine_lt0(cx, cy, nm_shift, scale, rot, in_sz, o_sz):
    """transform.py:486 under its own signature."""
    return _affine(1, False, in_sz, o_sz, cx, cy, nm_shift, scale, rot)


# --------------------------------------------------------------------------------------------------------------------------------- fused form
def _warps_forward(cfg, cls_lp, loc_lp, polar, temp_cx, temp_cy, search_poly):
    """One launch of hdn_simi_warps_f32 -> (best_idx, scale, rot, affine_m, affine_m_lt0, affine_m_c_aug, affine_m_lt0_aug, pred_points, aug_sear_points)."""
    stride, stride_lp, map_size, in_sz, out_sz = cfg
    dev = _lib.require_device(cls_lp, loc_lp, polar, temp_cx, temp_cy, search_poly)
    B, S = _map(cls_lp, "cls_lp", 2)
    _want(loc_lp, "loc_lp", (B, 4, S, S))
    _want(polar, "polar", (B, 2))
    _want(temp_cx, "temp_cx", (B,))
    _want(temp_cy, "temp_cy", (B,))
    _want(search_poly, "search_poly", (B, 4, 2))
    new = lambda *s: _new(s, dev)
    best = _new(B, dev, torch.int32)
    outs = (new(B), new(B), new(B, 2, 3), new(B, 2, 3), new(B, 2, 3), new(B, 2, 3), new(B, 3, 4), new(B, 3, 4))
    mag, rot_unit = lp_constants(map_size)
    ins = [_c(t) for t in (cls_lp, loc_lp, polar, temp_cx, temp_cy, search_poly)]
    _lib.launch("simi_warps", dev, _lib.load().hdn_simi_warps_f32, *(_lib.ptr(t) for t in ins),
                _lib.ptr(best), *(_lib.ptr(o) for o in outs), B, S, 2, int(stride), float(stride_lp), mag, rot_unit, float(in_sz), float(out_sz))
    return (best,) + outs


def _warps_backward(cfg, best, scale, rot, polar, search_poly, shape, grads, need=(True, True)):
    """(grad_loc_lp | None, grad_polar | None) for grads = the upstream gradients of (scale, rot, affine_m, affine_m_lt0, pred_points), None = zero."""
    stride, stride_lp, map_size, in_sz, out_sz = cfg
    dev = _lib.require_device(scale, rot, polar, search_poly, *(g for g in grads if g is not None))
    B, S = int(shape[0]), int(shape[2])
    for g, s, name in zip(grads, ((B,), (B,), (B, 2, 3), (B, 2, 3), (B, 3, 4)), ("scale", "rot", "affine_m", "affine_m_lt0", "pred_points")):
        if g is not None:
            _want(g, "the gradient of " + name, s)
    if not any(need):
        raise ValueError("similarity_warps backward: no gradient is asked for")
    g_loc = _new(tuple(shape), dev) if need[0] else None
    g_polar = _new((B, 2), dev) if need[1] else None
    mag, rot_unit = lp_constants(map_size)
    ins = [_c(t) for t in (scale, rot, polar, search_poly)]
    grads = [None if g is None else _c(g) for g in grads]
    _lib.launch("simi_warps_backward", dev, _lib.load().hdn_simi_warps_bwd_f32, _lib.ptr(best), *(_lib.ptr(t) for t in ins),
                *(_lib.opt(g) for g in grads), _lib.opt(g_loc), _lib.opt(g_polar), B, S, float(stride_lp), mag, rot_unit,
                float(in_sz), float(out_sz))
    return g_loc, g_polar


class _SimiWarps(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, cls_lp, loc_lp, polar, temp_cx, temp_cy, search_poly):
        out = _warps_forward(cfg, cls_lp, loc_lp, polar, temp_cx, temp_cy, search_poly)
        ctx.cfg, ctx.shape = cfg, tuple(loc_lp.shape)
        ctx.save_for_backward(out[0], out[1], out[2], polar, search_poly)
        ctx.mark_non_differentiable(out[0], out[5], out[6], out[8])      # best_idx and what depends on data only
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, _g_best, g_scale, g_rot, g_m, g_lt0, _g_c_aug, _g_lt0_aug, g_pts, _g_aug_pts):
        need = (ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        if not any(need):
            return (None,) * 7
        best, scale, rot, polar, search_poly = ctx.saved_tensors
        g_loc, g_polar = _warps_backward(ctx.cfg, best, scale, rot, polar, search_poly, ctx.shape, (g_scale, g_rot, g_m, g_lt0, g_pts), need)
        return None, None, g_loc, g_polar, None, None, None


def similarity_warps(cls_lp, loc_lp, polar, temp_cx, temp_cy, search_poly, *, stride=8, stride_lp=8, map_size=127, in_sz=255, out_sz=127,
                     return_index=False):
    """:390-415 in one launch: cls_lp [B,2,S,S], loc_lp [B,4,S,S], polar [B,2], temp_cx, temp_cy [B], search_poly [B,4,2] -> a dict under the
    reference's local names (WARP_KEYS: scale, rot [B]; affine_m, affine_m_lt0, affine_m_c_aug, affine_m_lt0_aug [B,2,3]; pred_points,
    aug_sear_points [B,3,4]) that carries the graph to loc_lp and polar.  stride, stride_lp, map_size, in_sz, out_sz are cfg.POINT.STRIDE,
    cfg.POINT.STRIDE_LP, cfg.TRAIN.EXEMPLAR_SIZE, cfg.TRACK.INSTANCE_SIZE, cfg.TRACK.EXEMPLAR_SIZE; the side S is cfg.TRAIN.OUTPUT_SIZE_LP.
    return_index=True adds best_idx_lp (int32 [B])."""
    for t, name in ((cls_lp, "cls_lp"), (temp_cx, "temp_cx"), (temp_cy, "temp_cy"), (search_poly, "search_poly")):
        _data(t, name)
    cfg = (stride, stride_lp, map_size, in_sz, out_sz)
    fn = _SimiWarps.apply if _wants_grad(loc_lp, polar) else _warps_forward
    out = fn(cfg, cls_lp, loc_lp, polar, temp_cx, temp_cy, search_poly)
    res = dict(zip(WARP_KEYS, out[1:]))
    if return_index:
        res["best_idx_lp"] = out[0]
    return res


DROP_INS = {f.__name__: f for f in (lp_pick, combine_affine_c0_v2, combine_affine_lt0)}
