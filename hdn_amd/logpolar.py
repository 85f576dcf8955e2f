"""STN_Polar on a HIP kernel.

    STN_Polar(image_sz).forward(x, polar, delta=[0, 0]) -> (x_lp, grid)     <- hdn/models/logpolar.py:50-134

Same constructor / forward signature and return values as the reference module.  The reference rebuilds the
sampling grid on the CPU and uploads it on every call (logpolar.py:121,110-111); here the 1-D factors of the grid
are cached on the device per rotation offset and the grid point is formed inside the sampling kernel.

By default the module is inference-only: with autograd recording, an x or polar that requires grad raises instead of being detached (the
reference's module is differentiable in both, and its training forward relies on that).  With differentiable=True (STN_PolarTrain, or
`model.logpolar_instance.differentiable = True` on a built model; hdn_amd.install.install(train=True) binds STN_PolarTrain) such a call goes through a
torch.autograd.Function whose forward is the same launch and whose backward is hdn_logpolar_sample_bwd_f32 (csrc/geometry_bwd.hip; first order
only).  The gradient with respect to polar is deterministic; the one with respect to x is a scatter by fp32 atomics and not bit-reproducible between
calls.  The returned grid is marked non-differentiable: nothing in the reference differentiates it.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import _lib


def tables(size: int, rot: float = 0.0):
    """rho[r], cos(theta[a]), sin(theta[a]) exactly as STN_Polar._prepare_grid computes them (CPU, fp32)."""
    ls = torch.linspace(0, size - 1, size)
    mag = math.log(size / 2) / size
    rho = torch.exp(mag * ls) - 1.0
    theta = ls * 2.0 * math.pi / size + rot
    return rho, torch.cos(theta), torch.sin(theta)


def _launch(x: torch.Tensor, polar: torch.Tensor, tabs, want_grid: bool):
    """The forward launch on x [B,C,H,W] and polar [B,2] (detached and made contiguous here)."""
    B, C, H, W = x.shape
    rho, c, s = tabs
    S = rho.numel()
    dev = _lib.require_device(x, polar, rho, c, s)
    xc, pc = x.detach().contiguous(), polar.detach().contiguous()
    out = torch.empty((B, C, S, S), dtype=torch.float32, device=dev)
    grid = torch.empty((B, S, S, 2), dtype=torch.float32, device=dev) if want_grid else None
    _lib.launch("STN_Polar", dev, _lib.load().hdn_logpolar_sample_f32, _lib.ptr(xc), _lib.ptr(pc), _lib.ptr(rho), _lib.ptr(c), _lib.ptr(s), _lib.ptr(out),
                _lib.opt(grid), B, C, H, W, S)
    return out, grid


def logpolar_sample_backward(x: torch.Tensor, polar: torch.Tensor, tabs, grad_out: torch.Tensor, need_x: bool = True, need_polar: bool = True):
    """(grad_x | None, grad_polar | None) of logpolar_sample for grad_out = d loss / d x_lp [B,C,S,S]: one call of hdn_logpolar_sample_bwd_f32
    (formulas: include/hdn_hip.h).  polar is [B,2].  A gradient that is not needed is neither computed nor allocated.  grad_out may be expanded or
    permuted; all inputs are made contiguous.  grad_polar is deterministic, grad_x (fp32 atomics) is not bit-reproducible between calls."""
    if not (need_x or need_polar):
        raise ValueError("logpolar_sample_backward: neither gradient is asked for")
    if x.dim() != 4:
        raise ValueError(f"x must be [B,C,H,W], got {tuple(x.shape)}")
    B, C, H, W = x.shape
    rho, c, s = tabs
    S = rho.numel()
    if tuple(polar.shape) != (B, 2):
        raise ValueError(f"polar must be [{B},2], got {tuple(polar.shape)}")
    if tuple(grad_out.shape) != (B, C, S, S):
        raise ValueError(f"grad_out {tuple(grad_out.shape)} does not have the sampler's shape {(B, C, S, S)}")
    dev = _lib.require_device(x, polar, rho, c, s, grad_out)
    xc, pc, gc = x.detach().contiguous(), polar.detach().contiguous(), grad_out.detach().contiguous()
    lib = _lib.load()
    gx = torch.empty_like(xc) if need_x else None          # zero-filled by the call
    gp, ws, ws_bytes = None, None, 0
    if need_polar:
        gp = torch.empty((B, 2), dtype=torch.float32, device=dev)
        ws, ws_bytes = _lib.workspace("logpolar_sample_backward", lib.hdn_logpolar_sample_bwd_workspace_bytes(B, S), dev)
    _lib.launch("logpolar_sample_backward", dev, lib.hdn_logpolar_sample_bwd_f32, _lib.ptr(xc), _lib.ptr(pc), _lib.ptr(rho), _lib.ptr(c), _lib.ptr(s),
                _lib.ptr(gc), _lib.opt(gp), _lib.opt(gx), _lib.opt(ws), ws_bytes, B, C, H, W, S)
    return gx, gp


class _LogpolarSample(torch.autograd.Function):
    """_launch with a backward: the forward is the same launch (same bits), the backward hdn_logpolar_sample_bwd_f32 for the inputs that need it."""

    @staticmethod
    def forward(ctx, x, polar, rho, c, s, want_grid):
        ctx.save_for_backward(x, polar, rho, c, s)
        out, grid = _launch(x, polar, (rho, c, s), want_grid)
        if grid is not None:
            ctx.mark_non_differentiable(grid)
        return out, grid

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, _grad_grid):
        x, polar, rho, c, s = ctx.saved_tensors
        need_x, need_polar = ctx.needs_input_grad[:2]
        if not (need_x or need_polar):
            return (None,) * 6
        gx, gp = logpolar_sample_backward(x, polar, (rho, c, s), grad_out, need_x, need_polar)
        return gx, gp, None, None, None, None


def logpolar_sample(x: torch.Tensor, polar: torch.Tensor, tabs, want_grid: bool = True, differentiable: bool = False):
    """x [B,C,H,W], polar [B,2], tabs = device tensors (rho, cos, sin) of length S -> (x_lp [B,C,S,S], grid or None).

    differentiable=False (the default): inference only; with autograd recording, an x or polar that requires grad raises.
    differentiable=True: such a call carries the graph (backward: hdn_logpolar_sample_bwd_f32, first order only).  The returned grid is marked
    non-differentiable - nothing in the reference differentiates it.  Otherwise the same launch runs and the result carries no graph."""
    if x.dim() != 4:
        raise ValueError(f"x must be [B,C,H,W], got {tuple(x.shape)}")
    recording = torch.is_grad_enabled() and (x.requires_grad or polar.requires_grad)
    if recording and not differentiable:
        # the reference's STN_Polar is differentiable in both (grid = indices + polar, then F.grid_sample), and its training forward
        # (model_builder_e2e_unconstrained_v2.py:377-379) passes a polar that carries the graph of the first head: detaching here would let that
        # training step run and silently lose the log-polar losses' gradient
        raise RuntimeError("hdn_amd.STN_Polar is inference-only (its kernel has no backward) but x or polar requires grad: run inference under "
                           "torch.no_grad(), or call hdn_amd.install.uninstall() before training so that the reference's own STN_Polar is used")
    B = x.shape[0]
    if tuple(polar.shape) == (1, 2) and B > 1:
        # the reference broadcasts one origin over the batch (`x.repeat([batch, 1, 1]) + polar[:, 0]...`, hdn/models/logpolar.py:113-114;
        # ModelBuilder.track_new_lp always passes a [1, 2] zero origin, model_builder_e2e_unconstrained_v2.py:145); done before Function.apply, so
        # autograd sums the batch's gradient back
        polar = polar.expand(B, 2)
    if tuple(polar.shape) != (B, 2):
        raise ValueError(f"polar must be [{B},2] (or [1,2], broadcast), got {tuple(polar.shape)}")
    if recording:
        _lib.require_device(x, polar, *tabs)
        return _LogpolarSample.apply(x, polar, *tabs, want_grid)
    return _launch(x, polar, tabs, want_grid)


class STN_Polar(nn.Module):
    """Drop-in for hdn.models.logpolar.STN_Polar.  differentiable=False (default): inference; raises when autograd is recording and x or polar requires
    grad.  differentiable=True (a plain attribute: an already-built model is switched with `model.logpolar_instance.differentiable = True`): such a
    call carries the graph to x and polar; the returned grid is non-differentiable."""

    def __init__(self, image_sz, differentiable: bool = False):
        super().__init__()
        self.differentiable = bool(differentiable)
        self._orignal_sz = [image_sz // 2, image_sz // 2]  # (sic) the reference's attribute name
        self._tabs = {}

    def _tables(self, device, rot: float):
        key = (str(device), float(rot))
        if key not in self._tabs:
            if len(self._tabs) > 64:  # update_template() passes arbitrary rotations: keep the cache bounded
                self._tabs.clear()
            self._tabs[key] = tuple(t.to(device) for t in tables(self._orignal_sz[0], float(rot)))
        return self._tabs[key]

    def forward(self, x, polar, delta=[0, 0]):
        # like the reference, the S x S grid (S = image_sz // 2) is sampled from whatever H x W crop arrives
        # (ModelBuilder.update_template passes the 127 x 127 template through STN_Polar(255), model_builder…:98-107)
        if x.dim() != 4 or x.shape[-1] < 2 or x.shape[-2] < 2:
            raise ValueError(f"STN_Polar needs a [B,C,H,W] crop with H, W >= 2, got {tuple(x.shape)}")
        rot = float(delta[1])
        return logpolar_sample(x, polar, self._tables(x.device, rot), differentiable=self.differentiable)


class STN_PolarTrain(STN_Polar):
    """STN_Polar(image_sz, differentiable=True): what install(train=True) binds at the reference's two STN_Polar sites."""

    def __init__(self, image_sz):
        super().__init__(image_sz, differentiable=True)
