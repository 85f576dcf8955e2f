"""The similarity model's supervised head losses on HIP kernels: hdn/models/loss.py as the training forward uses it.

    supervised_losses(cls, loc, cls_lp, loc_lp, label_cls, label_loc_c, label_cls_lp, label_loc_lp, if_unsup)
                                                  <- hdn/models/model_builder_e2e_unconstrained_v2.py:457-478 (WEIGHTED_MAP_LP: False)
    select_xr_focal_fuse_smooth_l1_loss_top_k, select_l1_loss_c, select_cross_entropy_loss, select_l1_loss, kalyo_l1_loss
                                                  <- hdn/models/loss.py, the names model_builder_e2e_unconstrained_v2 imports (:468-478, :516, :523)

The reference computes the four head losses with about a hundred elementwise, nonzero, index_select, topk and reduce launches forward and as many
backward; ten of them are nonzero() calls, each a host synchronisation, so no step that contains them can be captured in a graph.  Here one launch
(hdn_sup_losses_f32, csrc/sup_losses.hip, one workgroup per loss; formulas: include/hdn_hip.h) computes them and one launch
(hdn_sup_losses_bwd_f32) writes the gradients that are asked for; the sample mask, the label predicates, the label maximum, the counts and the top-k
are all decided in the kernel.  supervised_losses() takes the raw head maps (form 0: softmax, log-softmax and the if_unsup.eq(0) gather folded in,
gradients full size with zero rows for unselected samples); the five drop-ins take what the reference's functions receive (form 1) and carry the
autograd graph through one torch.autograd.Function (first order only).

What differs from the reference, on purpose: where it raises because it finds fewer negatives than k = 100 n, the k_eff = min(k, n_neg) largest are
used (a kernel cannot raise without a host read); among negatives that tie at the top-k threshold the gradient goes to the lowest flat indices
(torch.topk's choice is unspecified).  The reference's one-hit rule is reproduced: exactly one selected cell makes that term 0 (not in
select_l1_loss).  select_xr_focal_fuse_smooth_l1_loss and select_l1_loss_lp (the WEIGHTED_MAP_LP: True branch) have no HIP form and stay the
reference's.  Every output is bit-reproducible between calls (no float atomics).  There is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib

TOPK_PER_SAMPLE = 100            # loss.py:70: torch.topk(reg_loss_neg, batch_size * 100)
KEYS = ("cls_loss_sup", "loc_loss_sup", "cls_loss_lp_sup", "loc_loss_lp_sup")
_SLOTS = ("cls", "loc", "cls_lp", "loc_lp", "rows")                 # the inputs that receive gradients, in the order of losses[5]
_NAMES = ("cls", "label_cls", "loc", "label_loc_c", "cls_lp", "label_cls_lp", "loc_lp", "label_loc_lp", "rows", "rows_target", "if_unsup")


def _side(t, what):
    """S of a [n,S,S] label map."""
    if t.dim() != 3 or t.shape[1] != t.shape[2]:
        raise ValueError(f"{what} must be [n,S,S], got {tuple(t.shape)}")
    return int(t.shape[1])


def _prepare(form, t):
    """Check the shapes and devices of the tensors in `t` (name -> tensor | None), make them contiguous -> (tensors, B, S, S_lp, n_rows, C)."""
    floats = [v for k, v in t.items() if v is not None and k != "label_cls_lp"]
    dev = _lib.require_device(*floats)
    lab = t["label_cls_lp"]
    if lab is not None:
        if not isinstance(lab, torch.Tensor):
            raise TypeError(f"expected a torch.Tensor, got {type(lab).__name__}")
        if lab.dtype != torch.int64:
            raise TypeError(f"label_cls_lp must be int64 (the target of F.nll_loss), got {lab.dtype}")
        if dev is None or lab.device != dev:
            if not lab.is_cuda:
                raise _lib.HdnHipError(f"hdn_amd runs on the GPU only (tensor is on {lab.device}); there is no CPU fallback")
            raise _lib.HdnHipError(f"tensors on different devices: {dev} vs {lab.device}")
    B = S = S_lp = n_rows = C = 0

    def batch(n):
        nonlocal B
        if B and n != B:
            raise ValueError(f"the inputs disagree about the batch size: {B} and {n}")
        B = n

    def want(name, shape):
        if tuple(t[name].shape) != shape:
            raise ValueError(f"{name} must be {list(shape)}, got {list(t[name].shape)}")

    if t["label_cls"] is not None:
        S = _side(t["label_cls"], "label_cls")
        batch(int(t["label_cls"].shape[0]))
    if t["label_cls_lp"] is not None:
        S_lp = _side(t["label_cls_lp"], "label_cls_lp")
        batch(int(t["label_cls_lp"].shape[0]))
    if t["cls"] is not None:
        want("cls", (B, 2, S, S) if form == 0 else (B, S, S, 2))
    if t["loc"] is not None:
        want("loc", (B, 2, S, S))
        want("label_loc_c", (B, 2, S, S))
    if t["cls_lp"] is not None:
        want("cls_lp", (B, 2, S_lp, S_lp) if form == 0 else (B, S_lp, S_lp, 2))
    if t["loc_lp"] is not None:
        want("loc_lp", (B, 4, S_lp, S_lp))
        want("label_loc_lp", (B, 4, S_lp, S_lp))
    if t["rows"] is not None:
        if t["rows"].dim() != 2 or t["rows"].shape != t["rows_target"].shape:
            raise ValueError(f"output and target must be [n,C] of one shape, got {tuple(t['rows'].shape)} and {tuple(t['rows_target'].shape)}")
        n_rows, C = (int(v) for v in t["rows"].shape)
    if t["if_unsup"] is not None:
        if form != 0:
            raise ValueError("if_unsup selects samples of the raw head maps (form 0) only")
        want("if_unsup", (B,))
    return {k: (None if v is None else v.detach().contiguous()) for k, v in t.items()}, dev, (B, S, S_lp, n_rows, C)


def _forward(form, topk, t):
    """One launch of hdn_sup_losses_f32 -> losses [5] (the entries of absent losses are not written)."""
    c, dev, dims = _prepare(form, t)
    out = torch.empty(5, dtype=torch.float32, device=dev)
    _lib.launch("sup_losses", dev, _lib.load().hdn_sup_losses_f32, *(_lib.opt(c[k]) for k in _NAMES), _lib.ptr(out), *dims, int(topk), int(form))
    return out


def _backward(form, topk, t, grad_losses, need):
    """One launch of hdn_sup_losses_bwd_f32 -> the gradients of cls, loc, cls_lp, loc_lp, rows (None where not needed)."""
    c, dev, dims = _prepare(form, t)
    _lib.require_device(grad_losses)
    if grad_losses.device != dev or tuple(grad_losses.shape) != (5,):
        raise ValueError(f"grad_losses must be [5] on {dev}, got {tuple(grad_losses.shape)} on {grad_losses.device}")
    for k, w in zip(_SLOTS, need):
        if w and c[k] is None:
            raise ValueError(f"a gradient is asked for {k}, which is not given")
    grads = [torch.empty_like(c[k]) if w else None for k, w in zip(_SLOTS, need)]            # every element is written by the call
    _lib.launch("sup_losses_backward", dev, _lib.load().hdn_sup_losses_bwd_f32, *(_lib.opt(c[k]) for k in _NAMES),
                _lib.ptr(grad_losses.detach().contiguous()), *(_lib.opt(g) for g in grads), *dims, int(topk), int(form))
    return tuple(grads)


class _SupLosses(torch.autograd.Function):
    """losses [5] of _forward with a backward: hdn_sup_losses_bwd_f32 for the inputs that need it.  The target of kalyo_l1_loss receives the
    negated gradient of its output (the loss is a function of their difference) when it carries a graph, as in the reference."""

    @staticmethod
    def forward(ctx, form, topk, label_cls, label_loc_c, label_cls_lp, label_loc_lp, if_unsup, rows_target, cls, loc, cls_lp, loc_lp, rows):
        t = dict(cls=cls, label_cls=label_cls, loc=loc, label_loc_c=label_loc_c, cls_lp=cls_lp, label_cls_lp=label_cls_lp, loc_lp=loc_lp,
                 label_loc_lp=label_loc_lp, rows=rows, rows_target=rows_target, if_unsup=if_unsup)
        ctx.keys = [k for k in _NAMES if t[k] is not None]
        ctx.save_for_backward(*(t[k] for k in ctx.keys))
        ctx.form, ctx.topk = form, topk
        return _forward(form, topk, t)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_losses):
        need = list(ctx.needs_input_grad[8:13])
        tgt = ctx.needs_input_grad[7]
        need[4] = need[4] or tgt
        if not any(need):
            return (None,) * 13
        t = dict.fromkeys(_NAMES)
        t.update(zip(ctx.keys, ctx.saved_tensors))
        g = _backward(ctx.form, ctx.topk, t, grad_losses, need)
        return (None,) * 7 + (-g[4] if tgt else None,) + tuple(g)


def _apply(form, topk=TOPK_PER_SAMPLE, **t):
    t = {k: t.get(k) for k in _NAMES}
    for k, v in t.items():
        if v is not None and not isinstance(v, torch.Tensor):
            raise TypeError(f"{k}: expected a torch.Tensor, got {type(v).__name__}")
    return _SupLosses.apply(form, topk, t["label_cls"], t["label_loc_c"], t["label_cls_lp"], t["label_loc_lp"], t["if_unsup"], t["rows_target"],
                            t["cls"], t["loc"], t["cls_lp"], t["loc_lp"], t["rows"])


def _float(label):
    return label if label.dtype == torch.float32 else label.float()


def _pos_int(label):
    """The label of select_l1_loss as the int64 map whose test is > 0 (what label_cls_lp is in the training forward)."""
    return label if label.dtype == torch.int64 else (label > 0).long()


# ------------------------------------------------------------------------------------------------------------------------------ the five drop-ins
def select_xr_focal_fuse_smooth_l1_loss_top_k(pred_cls, label_cls, delta_weight=0.1):
    """loss.py:37.  pred_cls [n,S,S,2] softmaxed, label_cls [n,S,S] -> 0-d loss (delta_weight is unused there too)."""
    return _apply(1, cls=pred_cls, label_cls=_float(label_cls))[0]


def select_l1_loss_c(pred_loc, label_loc, label_cls):
    """loss.py:159.  pred_loc, label_loc [n,2,S,S], label_cls [n,S,S] -> 0-d loss."""
    return _apply(1, loc=pred_loc, label_loc_c=label_loc, label_cls=_float(label_cls))[1]


def select_cross_entropy_loss(pred, label):
    """loss.py:27.  pred [n,S,S,2] log-softmaxed, label int64 [n,S,S] -> 0-d loss."""
    return _apply(1, cls_lp=pred, label_cls_lp=label)[2]


def select_l1_loss(pred_loc, label_loc, label_cls):
    """loss.py:148.  pred_loc, label_loc [n,4,S,S], label_cls [n,S,S] (rows: label > 0) -> 0-d loss."""
    return _apply(1, loc_lp=pred_loc, label_loc_lp=label_loc, label_cls_lp=_pos_int(label_cls))[3]


def kalyo_l1_loss(output, target, norm=False):
    """loss.py:201.  output, target [n,C] -> 0-d loss.  norm=True (no call site uses it) is not restated."""
    if norm:
        raise ValueError("hdn_amd.kalyo_l1_loss restates norm=False only (no call site of the reference passes norm=True)")
    if isinstance(output, torch.Tensor) and output.dim() == 2 and output.numel() == 0:        # no rows: 0 / 1
        _lib.require_device(output, target)
        return (output.sum() + target.sum()) * 0.0
    return _apply(1, rows=output, rows_target=target)[4]


# ------------------------------------------------------------------------------------------------------------------------------------ form 0
def supervised_losses(cls, loc, cls_lp, loc_lp, label_cls, label_loc_c, label_cls_lp, label_loc_lp, if_unsup=None):
    """The four supervised head losses of model_builder_e2e_unconstrained_v2.py:457-478 from the raw head maps, one launch forward and one
    backward, no nonzero(): cls, loc [B,2,S,S], cls_lp [B,2,S',S'], loc_lp [B,4,S',S'], label_cls float [B,S,S], label_loc_c [B,2,S,S],
    label_cls_lp int64 [B,S',S'], label_loc_lp [B,4,S',S'], if_unsup float [B] or None (every sample) -> {cls_loss_sup, loc_loss_sup,
    cls_loss_lp_sup, loc_loss_lp_sup}, 0-d tensors that carry the graph to the four maps.  A sample takes part iff if_unsup == 0; with none selected
    every loss is 0 (the reference leaves the names unbound there).  Capturable in a graph: labels and mask are read by the kernel only."""
    out = _apply(0, cls=cls, loc=loc, cls_lp=cls_lp, loc_lp=loc_lp, label_cls=_float(label_cls), label_loc_c=label_loc_c, label_cls_lp=label_cls_lp,
                 label_loc_lp=label_loc_lp, if_unsup=None if if_unsup is None else _float(if_unsup))
    return {k: out[i] for i, k in enumerate(KEYS)}


def supervised_losses_backward(cls, loc, cls_lp, loc_lp, label_cls, label_loc_c, label_cls_lp, label_loc_lp, grad_losses, if_unsup=None,
                               need=(True, True, True, True)):
    """(grad_cls | None, grad_loc | None, grad_cls_lp | None, grad_loc_lp | None) of supervised_losses for grad_losses [4] = d L / d (the four
    losses in KEYS order): one call of hdn_sup_losses_bwd_f32.  Full size, zero rows for unselected samples; bit-reproducible."""
    if not any(need):
        raise ValueError("supervised_losses_backward: no gradient is asked for")
    if tuple(grad_losses.shape) != (4,):
        raise ValueError(f"grad_losses must be [4], got {tuple(grad_losses.shape)}")
    _lib.require_device(grad_losses)
    g5 = torch.cat([grad_losses.detach(), grad_losses.new_zeros(1)])
    t = dict(cls=cls, loc=loc, cls_lp=cls_lp, loc_lp=loc_lp, label_cls=_float(label_cls), label_loc_c=label_loc_c, label_cls_lp=label_cls_lp,
             label_loc_lp=label_loc_lp, if_unsup=None if if_unsup is None else _float(if_unsup))
    return _backward(0, TOPK_PER_SAMPLE, {k: t.get(k) for k in _NAMES}, g5, tuple(need) + (False,))[:4]


DROP_INS = {f.__name__: f for f in (select_xr_focal_fuse_smooth_l1_loss_top_k, select_l1_loss_c, select_cross_entropy_loss, select_l1_loss,
                                    kalyo_l1_loss)}
