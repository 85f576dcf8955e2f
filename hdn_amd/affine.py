"""ModelBuilder.stn_with_theta on HIP kernels: the affine spatial transformer of the reference's training forward.

    stn_with_theta(self, x, theta, size) -> x_warped [B,C,size[2],size[3]]     <- hdn/models/model_builder_e2e_unconstrained_v2.py:233-237

The reference's method is `F.grid_sample(x, F.affine_grid(theta.view(-1, 2, 3), size))` with PyTorch's defaults (bilinear, padding_mode='zeros',
align_corners=False): a [B,Ho,Wo,2] grid is materialised on every call and the backward goes through a batched matmul and the generic grid_sample
backward.  Here one kernel forms the sample point from theta and samples all channels (hdn_affine_sample_f32), and one call gives the gradients
(hdn_affine_sample_bwd_f32, csrc/affine_stn.hip; formulas: include/hdn_hip.h).

affine_sample() is inference-only by default: with autograd recording, an x or theta that requires grad raises instead of being detached (the
reference's method is differentiable in both, and its training forward relies on the gradient of theta).  With differentiable=True (what the method
stn_with_theta below passes; hdn_amd.install.install(train=True) binds it while AFFINE_STN_TRAIN_BOUND) such a call goes through a
torch.autograd.Function whose forward is the same launch and whose backward is first order only.  The gradient with respect to theta is deterministic;
the one with respect to x is a scatter by fp32 atomics and not bit-reproducible between calls.  There is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib


def _geometry(x: torch.Tensor, theta: torch.Tensor, size):
    """(theta as [B,2,3], Ho, Wo) by the rules of the reference's call: theta.view(-1, 2, 3); of `size` only size[0] and size[2:] are read, as
    F.affine_grid does (the reference passes [B,1,127,127] for a three-channel image), and size[0] must be the batch of x and of theta."""
    if x.dim() != 4:
        raise ValueError(f"x must be [B,C,H,W], got {tuple(x.shape)}")
    if len(size) != 4:
        raise ValueError(f"size must be (N, C, H_out, W_out), got {tuple(size)}")
    th = theta.view(-1, 2, 3)
    B, Ho, Wo = int(size[0]), int(size[2]), int(size[3])
    if B != x.shape[0] or B != th.shape[0]:
        raise ValueError(f"size[0] = {B}, x has batch {x.shape[0]} and theta batch {th.shape[0]}: the three must agree")
    if Ho <= 0 or Wo <= 0:
        raise ValueError(f"size asks for an empty {Ho} x {Wo} output")
    return th, Ho, Wo


def _launch(x: torch.Tensor, th: torch.Tensor, Ho: int, Wo: int):
    """The forward launch on x [B,C,H,W] and th [B,2,3] (detached and made contiguous here)."""
    B, C, H, W = x.shape
    dev = _lib.require_device(x, th)
    xc, tc = x.detach().contiguous(), th.detach().contiguous()
    out = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=dev)
    _lib.launch("affine_sample", dev, _lib.load().hdn_affine_sample_f32, _lib.ptr(xc), _lib.ptr(tc), _lib.ptr(out), B, C, H, W, Ho, Wo)
    return out


def affine_sample_backward(x: torch.Tensor, theta: torch.Tensor, size, grad_out: torch.Tensor, need_x: bool = True, need_theta: bool = True):
    """(grad_x | None, grad_theta | None [B,2,3]) of affine_sample for grad_out = d loss / d out [B,C,Ho,Wo]: one call of hdn_affine_sample_bwd_f32.
    A gradient that is not needed is neither computed nor allocated.  grad_out may be expanded or permuted and theta anything .view(-1, 2, 3) accepts;
    all inputs are made contiguous.  grad_theta is deterministic, grad_x (fp32 atomics) is not bit-reproducible between calls."""
    if not (need_x or need_theta):
        raise ValueError("affine_sample_backward: neither gradient is asked for")
    th, Ho, Wo = _geometry(x, theta, size)
    B, C, H, W = x.shape
    if tuple(grad_out.shape) != (B, C, Ho, Wo):
        raise ValueError(f"grad_out {tuple(grad_out.shape)} does not have the sampler's shape {(B, C, Ho, Wo)}")
    dev = _lib.require_device(x, th, grad_out)
    xc, tc, gc = x.detach().contiguous(), th.detach().contiguous(), grad_out.detach().contiguous()
    lib = _lib.load()
    gx = torch.empty_like(xc) if need_x else None          # zero-filled by the call
    gt, ws, ws_bytes = None, None, 0
    if need_theta:
        gt = torch.empty((B, 2, 3), dtype=torch.float32, device=dev)
        ws, ws_bytes = _lib.workspace("affine_sample_backward", lib.hdn_affine_sample_bwd_workspace_bytes(B, Ho, Wo), dev)
    _lib.launch("affine_sample_backward", dev, lib.hdn_affine_sample_bwd_f32, _lib.ptr(xc), _lib.ptr(tc), _lib.ptr(gc), _lib.opt(gt), _lib.opt(gx),
                _lib.opt(ws), ws_bytes, B, C, H, W, Ho, Wo)
    return gx, gt


class _AffineSample(torch.autograd.Function):
    """_launch with a backward: the forward is the same launch (same bits), the backward hdn_affine_sample_bwd_f32 for the inputs that need it."""

    @staticmethod
    def forward(ctx, x, th, Ho, Wo):
        ctx.save_for_backward(x, th)
        ctx.out_hw = (Ho, Wo)
        return _launch(x, th, Ho, Wo)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, th = ctx.saved_tensors
        need_x, need_theta = ctx.needs_input_grad[:2]
        if not (need_x or need_theta):
            return None, None, None, None
        Ho, Wo = ctx.out_hw
        gx, gt = affine_sample_backward(x, th, (x.shape[0], x.shape[1], Ho, Wo), grad_out, need_x, need_theta)
        return gx, gt, None, None


def affine_sample(x: torch.Tensor, theta: torch.Tensor, size, differentiable: bool = False):
    """x [B,C,H,W], theta anything .view(-1, 2, 3) accepts with B rows, size = (B, *, Ho, Wo) -> [B,C,Ho,Wo], what
    F.grid_sample(x, F.affine_grid(theta.view(-1, 2, 3), size)) computes with PyTorch's defaults.

    differentiable=False (the default): inference only; with autograd recording, an x or theta that requires grad raises.
    differentiable=True: such a call carries the graph (backward: hdn_affine_sample_bwd_f32, first order only).  Otherwise the same launch runs and
    the result carries no graph."""
    th, Ho, Wo = _geometry(x, theta, size)
    recording = torch.is_grad_enabled() and (x.requires_grad or th.requires_grad)
    if recording and not differentiable:
        # the reference's stn_with_theta is differentiable in both, and its training forward (model_builder_e2e_unconstrained_v2.py:407,418) passes an
        # affine_m that carries the graph of both heads: detaching here would let that step run and silently lose sim_loss / homo_unsup_loss's gradient
        raise RuntimeError("hdn_amd.affine_sample is inference-only (differentiable=False) but x or theta requires grad: run inference under "
                           "torch.no_grad(), pass differentiable=True, or call hdn_amd.install.uninstall() before training so that the reference's "
                           "own stn_with_theta is used")
    if recording:
        _lib.require_device(x, th)
        return _AffineSample.apply(x, th, Ho, Wo)
    return _launch(x, th, Ho, Wo)


def stn_with_theta(self, x, theta, size):
    """ModelBuilder.stn_with_theta (model_builder_e2e_unconstrained_v2.py:233-237) on the HIP sampler, differentiable in x and theta: what
    install(train=True) binds at that site while hdn_amd.install.AFFINE_STN_TRAIN_BOUND."""
    return affine_sample(x, theta, size, differentiable=True)
