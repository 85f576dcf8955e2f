"""nn.TripletMarginLoss(margin, p=1, reduction='none') on HIP kernels: the feature loss of the reference's two training forwards.

    triplet_loss(sear, pred, tmp) -> loss_mat [n,1,127]      <- hdn/models/model_builder_e2e_unconstrained_v2.py:438 (sim_loss_mat)
                                                                 homo_estimator/.../models/homo_model_builder.py:197 (feature_loss_mat)

The reference's `triplet_loss` is nn.TripletMarginLoss(margin=1.0, p=1, reduce=False, size_average=False): two F.pairwise_distance calls over the last
dimension (eps added to the difference inside the absolute value), then clamp_min(margin + d_ap - d_an, 0) - a dozen elementwise and reduce launches
forward and as many backward, on three maps that were gathered by x[ids] just before.  Here one wave reads each row once (hdn_triplet_l1_f32) and one
call writes the gradients that are asked for (hdn_triplet_l1_bwd_f32, csrc/triplet_loss.hip; formulas: include/hdn_hip.h); with `ids` the gather is
part of the addressing, so no gathered copy is made and the gradients come back full size with zero rows for the samples that were not selected.

triplet_l1() is inference-only by default: with autograd recording, an input that requires grad raises instead of being detached.  With
differentiable=True (what TripletMarginLossL1 passes; hdn_amd.install.install(train=True) binds that module at the two `triplet_loss` sites while
TRIPLET_TRAIN_BOUND) such a call goes through a torch.autograd.Function whose forward is the same launch and whose backward is first order only.
Every output is bit-reproducible between calls (no atomics).  There is no CPU fallback.

    triplet_l1_mean(anchor, positive, negative, if_pos, if_unsup, rule) -> (value, counts)
                                                                 <- model_builder_e2e_unconstrained_v2.py:430-440 (rule 0: sim_loss)
                                                                    homo_model_builder.py:174-199 (rule 1: feature_loss)

is each site's whole term - the nonzero() selection, the rows, the sum and the division by a length that the reference reads on the host - with
the sample sets decided from the flags in the kernels (hdn_triplet_l1_mean_f32 / hdn_triplet_l1_mean_bwd_f32), so that a training forward built on
it can be captured in a graph.  `ids` needs the index list and therefore the host read; it remains for callers that hold one.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib


def _check(anchor, positive, negative, ids):
    """(N, R, D, n_sel) of three equal-shaped [..., D] tensors seen as [N, R, D]: N is the leading dimension (the one `ids` selects from), R the
    product of the dimensions between.  A one-dimensional input is one sample of one row."""
    for t in (anchor, positive, negative):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"expected a torch.Tensor, got {type(t).__name__}")
    if anchor.shape != positive.shape or anchor.shape != negative.shape:
        raise ValueError(f"anchor, positive and negative must have one shape (broadcasting is not supported), got {tuple(anchor.shape)}, "
                         f"{tuple(positive.shape)}, {tuple(negative.shape)}")
    if anchor.dim() < 1 or anchor.shape[-1] < 1:
        raise ValueError(f"the inputs must be [..., D] with D >= 1, got {tuple(anchor.shape)}")
    D = int(anchor.shape[-1])
    N = int(anchor.shape[0]) if anchor.dim() >= 2 else 1
    R = anchor.numel() // (N * D) if N else 0
    if ids is not None:
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.dim() != 1:
            raise ValueError("ids must be a one-dimensional int64 tensor (what nonzero().squeeze(1) gives)")
        if anchor.dim() < 2:
            raise ValueError("ids select along the leading dimension: the inputs must be at least [N, D]")
    return N, R, D, (int(ids.shape[0]) if ids is not None else N)


def _out_shape(anchor, ids):
    lead = tuple(anchor.shape[:-1])
    return lead if ids is None else (int(ids.shape[0]),) + lead[1:]


def _device_ids(ids, dev):
    if ids is None:
        return None
    if not ids.is_cuda or ids.device != dev:
        raise _lib.HdnHipError(f"ids live on {ids.device}, the inputs on {dev}; there is no CPU fallback")
    return ids.contiguous()


def _launch(anchor, positive, negative, margin, eps, ids):
    """The forward launch (inputs detached and made contiguous here); zero rows launch nothing."""
    N, R, D, n_sel = _check(anchor, positive, negative, ids)
    dev = _lib.require_device(anchor, positive, negative)
    ic = _device_ids(ids, dev)
    out = torch.empty(_out_shape(anchor, ids), dtype=torch.float32, device=dev)
    if out.numel() == 0:
        return out
    a, p, n = (t.detach().contiguous() for t in (anchor, positive, negative))
    _lib.launch("triplet_l1", dev, _lib.load().hdn_triplet_l1_f32, _lib.ptr(a), _lib.ptr(p), _lib.ptr(n), _lib.opt(ic), _lib.ptr(out), N, R, D,
                n_sel if ids is not None else 0, float(margin), float(eps))
    return out


def triplet_l1_backward(anchor, positive, negative, grad_loss, margin: float = 1.0, eps: float = 1e-6, ids=None, need_anchor: bool = True,
                        need_positive: bool = True, need_negative: bool = True):
    """(grad_anchor | None, grad_positive | None, grad_negative | None), each of the inputs' full shape, of triplet_l1 for grad_loss = d L / d loss:
    one call of hdn_triplet_l1_bwd_f32.  A gradient that is not needed is neither computed nor allocated.  grad_loss may be expanded or permuted;
    everything is made contiguous.  With ids, the rows of samples that ids does not name are zero.  Exact and bit-reproducible."""
    need = (need_anchor, need_positive, need_negative)
    if not any(need):
        raise ValueError("triplet_l1_backward: no gradient is asked for")
    N, R, D, n_sel = _check(anchor, positive, negative, ids)
    if tuple(grad_loss.shape) != _out_shape(anchor, ids):
        raise ValueError(f"grad_loss {tuple(grad_loss.shape)} does not have the loss's shape {_out_shape(anchor, ids)}")
    dev = _lib.require_device(anchor, positive, negative, grad_loss)
    ic = _device_ids(ids, dev)
    if anchor.numel() == 0:
        return tuple(torch.zeros_like(anchor) if w else None for w in need)
    if n_sel == 0:                                             # an empty selection: nothing to launch, every row is unselected
        return tuple(torch.zeros(anchor.shape, dtype=torch.float32, device=dev) if w else None for w in need)
    a, p, n, g = (t.detach().contiguous() for t in (anchor, positive, negative, grad_loss))
    grads = [torch.empty(anchor.shape, dtype=torch.float32, device=dev) if w else None for w in need]   # every element is written by the call
    _lib.launch("triplet_l1_backward", dev, _lib.load().hdn_triplet_l1_bwd_f32, _lib.ptr(a), _lib.ptr(p), _lib.ptr(n), _lib.opt(ic), _lib.ptr(g),
                _lib.opt(grads[0]), _lib.opt(grads[1]), _lib.opt(grads[2]), N, R, D, n_sel if ids is not None else 0, float(margin), float(eps))
    return tuple(grads)


class _TripletL1(torch.autograd.Function):
    """_launch with a backward: the forward is the same launch (same bits), the backward hdn_triplet_l1_bwd_f32 for the inputs that need it."""

    @staticmethod
    def forward(ctx, anchor, positive, negative, margin, eps, ids):
        ctx.save_for_backward(anchor, positive, negative)
        ctx.args = (margin, eps, ids)
        return _launch(anchor, positive, negative, margin, eps, ids)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        anchor, positive, negative = ctx.saved_tensors
        need = ctx.needs_input_grad[:3]
        if not any(need):
            return None, None, None, None, None, None
        margin, eps, ids = ctx.args
        ga, gp, gn = triplet_l1_backward(anchor, positive, negative, grad_loss, margin, eps, ids, *need)
        return ga, gp, gn, None, None, None


def triplet_l1(anchor, positive, negative, margin: float = 1.0, eps: float = 1e-6, ids=None, differentiable: bool = False):
    """anchor, positive, negative [..., D] of one shape -> loss [...] (the last dimension reduced), what
    nn.TripletMarginLoss(margin=margin, p=1, eps=eps, reduction='none')(anchor, positive, negative) computes.  ids (int64 [n_ids], unique, on the
    device): the loss of anchor[ids], positive[ids], negative[ids] - leading dimension n_ids - without the gathered copies.

    differentiable=False (the default): inference only; with autograd recording, an input that requires grad raises.
    differentiable=True: such a call carries the graph (backward: hdn_triplet_l1_bwd_f32, first order only).  Otherwise the same launch runs and
    the result carries no graph."""
    _check(anchor, positive, negative, ids)
    recording = torch.is_grad_enabled() and (anchor.requires_grad or positive.requires_grad or negative.requires_grad)
    if recording and not differentiable:
        # the reference's loss carries the gradient of the whole training step: detaching here would let that step run and learn nothing
        raise RuntimeError("hdn_amd.triplet_l1 is inference-only (differentiable=False) but an input requires grad: run inference under "
                           "torch.no_grad(), pass differentiable=True, or call hdn_amd.install.uninstall() before training so that the reference's "
                           "own nn.TripletMarginLoss is used")
    if recording:
        _lib.require_device(anchor, positive, negative)
        return _TripletL1.apply(anchor, positive, negative, float(margin), float(eps), ids)
    return _launch(anchor, positive, negative, margin, eps, ids)


# ------------------------------------------------------------------------------------------------------- the flag-selected mean: no host read
def _check_mean(anchor, positive, negative, if_pos, if_unsup, rule, denom):
    """(N, R, D) of the mean form: the inputs as _check sees them, flags [N], rule 0 or 1, denom > 0."""
    N, R, D, _ = _check(anchor, positive, negative, None)
    for k, v in (("if_pos", if_pos), ("if_unsup", if_unsup)):
        if not isinstance(v, torch.Tensor):
            raise TypeError(f"{k}: expected a torch.Tensor, got {type(v).__name__}")
        if v.requires_grad:
            raise ValueError(f"triplet_l1_mean has no gradient for {k}")
        if tuple(v.shape) != (N,):
            raise ValueError(f"{k} must be [{N}] (one flag per sample of the leading dimension), got {list(v.shape)}")
    if rule not in (0, 1):
        raise ValueError(f"rule must be 0 (similarity: model_builder_e2e_unconstrained_v2.py:430-440) or 1 (homography estimator: "
                         f"homo_model_builder.py:174-199), got {rule!r}")
    if not float(denom) > 0:
        raise ValueError(f"denom must be > 0, got {denom!r}")
    if anchor.numel() == 0:
        raise ValueError(f"the inputs must not be empty, got {tuple(anchor.shape)}")
    return N, R, D


def _launch_mean(anchor, positive, negative, if_pos, if_unsup, rule, denom, margin, eps):
    """One call of hdn_triplet_l1_mean_f32 -> (value 0-d fp32, counts int32 [2])."""
    N, R, D = _check_mean(anchor, positive, negative, if_pos, if_unsup, rule, denom)
    dev = _lib.require_device(anchor, positive, negative, if_pos, if_unsup)
    a, p, n, fp, fu = (t.detach().contiguous() for t in (anchor, positive, negative, if_pos, if_unsup))
    partial = torch.empty(N * R, dtype=torch.float32, device=dev)                     # (torch's caching allocator: no sync, graph-safe)
    out, counts = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
    _lib.launch("triplet_l1_mean", dev, _lib.load().hdn_triplet_l1_mean_f32, _lib.ptr(a), _lib.ptr(p), _lib.ptr(n), _lib.ptr(fp), _lib.ptr(fu),
                _lib.ptr(partial), _lib.ptr(out), _lib.ptr(counts), N, R, D, int(rule), float(denom), float(margin), float(eps))
    return out[0], counts


def triplet_l1_mean_backward(anchor, positive, negative, if_pos, if_unsup, grad_out, rule, denom=127 * 127, margin: float = 1.0,
                             eps: float = 1e-6, need_anchor: bool = True, need_positive: bool = True, need_negative: bool = True):
    """(grad_anchor | None, grad_positive | None, grad_negative | None), each of the inputs' full shape, of triplet_l1_mean for grad_out (one
    element) = d L / d value: one call of hdn_triplet_l1_mean_bwd_f32.  The sets are recounted from the flags on the device; rows of unused
    samples and inactive rows are zero, with an empty selection everything is.  Exact given each row's activity, bit-reproducible."""
    need = (need_anchor, need_positive, need_negative)
    if not any(need):
        raise ValueError("triplet_l1_mean_backward: no gradient is asked for")
    N, R, D = _check_mean(anchor, positive, negative, if_pos, if_unsup, rule, denom)
    if not isinstance(grad_out, torch.Tensor) or grad_out.numel() != 1:
        raise ValueError("grad_out must hold one element (the gradient of the 0-d value)")
    dev = _lib.require_device(anchor, positive, negative, if_pos, if_unsup, grad_out)
    a, p, n, fp, fu, g = (t.detach().contiguous() for t in (anchor, positive, negative, if_pos, if_unsup, grad_out))
    grads = [torch.empty(anchor.shape, dtype=torch.float32, device=dev) if w else None for w in need]   # every element is written by the call
    _lib.launch("triplet_l1_mean_backward", dev, _lib.load().hdn_triplet_l1_mean_bwd_f32, _lib.ptr(a), _lib.ptr(p), _lib.ptr(n), _lib.ptr(fp),
                _lib.ptr(fu), _lib.ptr(g), _lib.opt(grads[0]), _lib.opt(grads[1]), _lib.opt(grads[2]), N, R, D, int(rule), float(denom),
                float(margin), float(eps))
    return tuple(grads)


class _TripletL1Mean(torch.autograd.Function):
    """(value, counts) of _launch_mean with a backward: hdn_triplet_l1_mean_bwd_f32 for the inputs that need it (first order only)."""

    @staticmethod
    def forward(ctx, anchor, positive, negative, if_pos, if_unsup, rule, denom, margin, eps):
        ctx.save_for_backward(anchor, positive, negative, if_pos, if_unsup)
        ctx.args = (rule, denom, margin, eps)
        value, counts = _launch_mean(anchor, positive, negative, if_pos, if_unsup, rule, denom, margin, eps)
        ctx.mark_non_differentiable(counts)
        return value, counts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_value, _grad_counts):
        need = ctx.needs_input_grad[:3]
        if not any(need):
            return (None,) * 9
        rule, denom, margin, eps = ctx.args
        return triplet_l1_mean_backward(*ctx.saved_tensors, grad_value, rule, denom, margin, eps, *need) + (None,) * 6


def triplet_l1_mean(anchor, positive, negative, if_pos, if_unsup, rule, denom=127 * 127, margin: float = 1.0, eps: float = 1e-6):
    """The reference's two triplet terms without their nonzero() reads: anchor, positive, negative [N, ..., D] of one shape, if_pos, if_unsup
    float [N] on the device -> (value 0-d, counts int32 [2] = n_sel, n_neg).  sel: if_pos * if_unsup == 1, neg: if_pos == 0, decided in the kernel.

    rule 0 (sim_loss, model_builder_e2e_unconstrained_v2.py:430-440): the selected samples; value = sum / denom / n_sel.
    rule 1 (feature_loss, homo_model_builder.py:174-199): the selected samples where the batch has a negative, every sample otherwise;
    value = sum / n_sel / denom in both cases (the reference's own quirk).
    n_sel == 0 gives 0 and zero gradients, where the reference skips the term (rule 0) or divides by zero (rule 1).  A sample that is not used
    is not read: a NaN in it reaches neither the value nor a gradient.  The value carries the graph to the three inputs (first order only); the
    flags must not require grad.  Bit-reproducible; capturable in a graph (nothing is read by or uploaded from the host)."""
    _check_mean(anchor, positive, negative, if_pos, if_unsup, rule, denom)
    _lib.require_device(anchor, positive, negative, if_pos, if_unsup)
    return _TripletL1Mean.apply(anchor, positive, negative, if_pos, if_unsup, int(rule), float(denom), float(margin), float(eps))


class TripletMarginLossL1(nn.Module):
    """nn.TripletMarginLoss(margin, p=1, eps, swap=False, reduction='none') on the HIP kernels, differentiable in all three inputs: what
    install(train=True) binds at the two `triplet_loss` sites while hdn_amd.install.TRIPLET_TRAIN_BOUND."""

    def __init__(self, margin: float = 1.0, eps: float = 1e-6):
        super().__init__()
        self.margin, self.eps = float(margin), float(eps)

    def extra_repr(self):
        return f"margin={self.margin}, eps={self.eps}"

    def forward(self, anchor, positive, negative):
        return triplet_l1(anchor, positive, negative, self.margin, self.eps, differentiable=True)
