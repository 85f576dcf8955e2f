"""The corner supervision of the similarity model's training forward on HIP kernels, and the dictionary the forward returns.

    corner_losses(H_mat, pred_points, template_poly, x, if_pos, if_unsup, aug_sear_points=None)
                                                  <- hdn/models/model_builder_e2e_unconstrained_v2.py:441-444 (corner_error_simi), :481-523
    training_outputs(head_losses, corner, sim_loss, loss_feature, cls_weight, loc_weight)
                                                  <- :526-562, the fourteen keys with total_loss

The reference writes this stretch as about sixty one-line launches forward and as many backward, uploads four constants and reads six nonzero() /
len() results on the host, which keeps the loss side of the step out of a graph.  Here one launch (hdn_corner_losses_f32, csrc/corner_losses.hip;
formulas: include/hdn_hip.h) computes the six values and the six set sizes, and one launch (hdn_corner_losses_bwd_f32) writes the gradients that
are asked for.  The sets (sup, sup_pos, sup_neg, unsup, unsup_pos, neg) are decided in the kernel from if_pos and if_unsup; training_outputs gates
on the returned counts with torch.where, so nothing is read by the host and a NaN in a term that is gated off cannot reach total_loss (a
multiplication by 0 would pass it on).

What differs from the reference, on purpose: its DLT_solve inverts the system of every sample of the batch, and torch.inverse raises for the whole
batch when one of them - selected or not - is singular; here only the sup_pos samples are solved, the others are not read.  The solve is the float64
elimination of hdn_dlt_solve_f32, not PyTorch's fp32 inverse.  These are statements of ModelBuilder.forward, not functions, so install() has nothing
to rebind: a training forward calls the three functions in place of those lines.  Every output is bit-reproducible between calls.
There is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib

KEYS = ("cor_err", "cor_err_aug", "cor_err_sim", "cor_pos_loss", "cor_neg_loss", "cor_loss")
COUNTS = ("n_sup", "n_sup_pos", "n_sup_neg", "n_unsup", "n_unsup_pos", "n_neg")
OUTPUT_KEYS = ("cls_loss_sup", "loc_loss_sup", "cls_loss_lp_sup", "loc_loss_lp_sup", "sim_cent_loss", "sim_loss", "cor_err_aug", "cor_err_sim",
               "cor_err", "cor_loss", "cor_pos_loss", "cor_neg_loss", "homo_unsup_loss", "total_loss")


def _new(*shape, dtype=torch.float32, device=None):
    return torch.empty(*shape, dtype=dtype, device=device)


def _prepare(H_mat, pred_points, aug_sear_points, template_poly, x, if_pos, if_unsup):
    """Check shapes and devices, make the tensors contiguous -> (tensors in the C order, device, B)."""
    t = dict(H_mat=H_mat, pred_points=pred_points, aug_sear_points=aug_sear_points, template_poly=template_poly, x=x, if_pos=if_pos,
             if_unsup=if_unsup)
    dev = _lib.require_device(*(v for v in t.values() if v is not None))
    if H_mat.dim() != 3 or tuple(H_mat.shape[1:]) != (3, 3) or H_mat.shape[0] < 1:
        raise ValueError(f"H_mat must be [B,3,3] with B >= 1, got {list(H_mat.shape)}")
    B = int(H_mat.shape[0])
    for k, shape in (("pred_points", (B, 3, 4)), ("aug_sear_points", (B, 3, 4)), ("template_poly", (B, 4, 2)), ("x", (B, 8)), ("if_pos", (B,)),
                     ("if_unsup", (B,))):
        if t[k] is not None and tuple(t[k].shape) != shape:
            raise ValueError(f"{k} must be {list(shape)}, got {list(t[k].shape)}")
    return [None if v is None else v.detach().contiguous() for v in t.values()], dev, B


def _forward(H_mat, pred_points, aug_sear_points, template_poly, x, if_pos, if_unsup):
    """One launch of hdn_corner_losses_f32 -> (out [6] fp32, counts [6] int32)."""
    c, dev, B = _prepare(H_mat, pred_points, aug_sear_points, template_poly, x, if_pos, if_unsup)
    out, counts = _new(6, device=dev), _new(6, dtype=torch.int32, device=dev)
    _lib.launch("corner_losses", dev, _lib.load().hdn_corner_losses_f32, *(_lib.opt(v) for v in c), _lib.ptr(out), _lib.ptr(counts), B)
    return out, counts


def _backward(H_mat, pred_points, aug_sear_points, template_poly, x, if_pos, if_unsup, grad_out, need):
    """One launch of hdn_corner_losses_bwd_f32 -> the gradients of H_mat, pred_points, aug_sear_points, x (None where not needed)."""
    c, dev, B = _prepare(H_mat, pred_points, aug_sear_points, template_poly, x, if_pos, if_unsup)
    _lib.require_device(grad_out)
    if grad_out.device != dev or tuple(grad_out.shape) != (6,):
        raise ValueError(f"grad_out must be [6] on {dev}, got {list(grad_out.shape)} on {grad_out.device}")
    if need[2] and aug_sear_points is None:
        raise ValueError("a gradient is asked for aug_sear_points, which is not given")
    src = (c[0], c[1], c[2], c[4])
    grads = [_new(s.shape, device=dev) if w else None for s, w in zip(src, need)]                  # every element is written by the call
    _lib.launch("corner_losses_backward", dev, _lib.load().hdn_corner_losses_bwd_f32, *(_lib.opt(v) for v in c),
                _lib.ptr(grad_out.detach().contiguous()), *(_lib.opt(g) for g in grads), B)
    return tuple(grads)


class _CornerLosses(torch.autograd.Function):
    """(out [6], counts [6]) of _forward with a backward: hdn_corner_losses_bwd_f32 for the inputs that need it (first order only)."""

    @staticmethod
    def forward(ctx, template_poly, if_pos, if_unsup, H_mat, pred_points, aug_sear_points, x):
        ctx.has_aug = aug_sear_points is not None
        ctx.save_for_backward(*(v for v in (H_mat, pred_points, aug_sear_points, template_poly, x, if_pos, if_unsup) if v is not None))
        out, counts = _forward(H_mat, pred_points, aug_sear_points, template_poly, x, if_pos, if_unsup)
        ctx.mark_non_differentiable(counts)
        return out, counts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, _grad_counts):
        need = list(ctx.needs_input_grad[3:7])
        if not any(need):
            return (None,) * 7
        s = list(ctx.saved_tensors)
        if not ctx.has_aug:
            s.insert(2, None)
        return (None, None, None) + _backward(*s, grad_out, need)


def _check(template_poly, if_pos, if_unsup):
    if isinstance(template_poly, torch.Tensor) and template_poly.requires_grad:
        raise ValueError("corner_losses has no gradient for template_poly (a label in the reference's forward): detach it")
    for k, v in (("if_pos", if_pos), ("if_unsup", if_unsup)):
        if isinstance(v, torch.Tensor) and v.requires_grad:
            raise ValueError(f"corner_losses has no gradient for {k}")


def corner_losses(H_mat, pred_points, template_poly, x, if_pos, if_unsup, aug_sear_points=None):
    """The corner errors and corner losses of model_builder_e2e_unconstrained_v2.py:441-444 and :481-523 with the gating of :552-556, one launch
    forward and one backward, no nonzero(): H_mat [B,3,3], pred_points [B,3,4], template_poly [B,4,2], x [B,8] (batch_out['x']), if_pos, if_unsup
    float [B], aug_sear_points [B,3,4] or None (cor_err_aug is 0 then) -> {cor_err, cor_err_aug, cor_err_sim, cor_pos_loss, cor_neg_loss, cor_loss}
    as 0-d tensors that carry the graph to H_mat, pred_points, aug_sear_points and x, and counts, int32 [6] = n_sup, n_sup_pos, n_sup_neg, n_unsup,
    n_unsup_pos, n_neg.  An empty set gives 0.  Capturable in a graph: the flags are read by the kernel only."""
    _check(template_poly, if_pos, if_unsup)
    out, counts = _CornerLosses.apply(template_poly, if_pos, if_unsup, H_mat, pred_points, aug_sear_points, x)
    res = {k: out[i] for i, k in enumerate(KEYS)}
    res["counts"] = counts
    return res


def corner_losses_backward(H_mat, pred_points, template_poly, x, if_pos, if_unsup, grad_out, aug_sear_points=None, need=(True, True, False, True)):
    """(grad_H_mat | None, grad_pred_points | None, grad_aug_sear_points | None, grad_x | None) of corner_losses for grad_out [6] = d L / d (the six
    values in KEYS order): one call of hdn_corner_losses_bwd_f32.  Full size, zero rows for samples outside the sets; bit-reproducible."""
    if not any(need):
        raise ValueError("corner_losses_backward: no gradient is asked for")
    _check(template_poly, if_pos, if_unsup)
    return _backward(H_mat, pred_points, aug_sear_points, template_poly, x, if_pos, if_unsup, grad_out, tuple(need))


def training_outputs(head_losses, corner, sim_loss, loss_feature, cls_weight, loc_weight):
    """The dictionary of model_builder_e2e_unconstrained_v2.py:526-562.  head_losses: what supervised_losses returns (0 with no supervised sample);
    corner: what corner_losses returns; sim_loss: the 0-d triplet term of :440 (used where n_unsup_pos > 0); loss_feature: the 0-d mean of
    batch_out['feature_loss'] (used where n_unsup > 0).  The reference's `if len(ids) > 0` become torch.where on corner['counts']: no host read, and
    a term that is gated off contributes neither its value nor a NaN."""
    n = corner["counts"]
    zero = torch.zeros_like(corner["cor_err"])
    some = lambda i: n[i] > 0
    out = {k: torch.where(some(0), head_losses[k], zero) for k in ("cls_loss_sup", "loc_loss_sup", "cls_loss_lp_sup", "loc_loss_lp_sup")}
    out["sim_cent_loss"] = cls_weight * (out["cls_loss_lp_sup"] + out["cls_loss_sup"]) + loc_weight * (out["loc_loss_sup"] + out["loc_loss_lp_sup"])
    out["sim_loss"] = torch.where(some(4), sim_loss, zero)
    for k in KEYS:                                               # gated in the kernel: an empty set gives 0
        out[k] = corner[k]
    out["homo_unsup_loss"] = torch.where(some(3), loss_feature, zero)
    out["total_loss"] = out["sim_cent_loss"] * 100 + out["homo_unsup_loss"] + out["cor_neg_loss"] + out["cor_err"] / 4
    return {k: out[k] for k in OUTPUT_KEYS}
