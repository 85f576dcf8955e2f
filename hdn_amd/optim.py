"""The optimizer stretch of a training iteration on HIP kernels, with no host read and no upload, so that it replays inside a graph.

    GatedAMSGrad(params, lr, betas, eps, weight_decay, max_norm, loss_limit, clip_grads_in_place).step(loss)
                                                  <- tools/train.py:271-281: is_valid_number(loss.item()), clip_grad_norm_(GRAD_CLIP),
                                                     Adam(amsgrad=True, weight_decay=1e-4).step() of build_opt_lr (:100-170)
    grad_norm(tensors)                            <- the total 2-norm clip_grad_norm_ returns, on its own

The reference reads the loss on the host in every step (.item()), which ends any capture, and its stock replacements are many small launches per
parameter list around a decision the host takes.  Here step() is hdn_grad_sqnorm_f32, hdn_opt_gate_f32 and hdn_amsgrad_apply_f32
(csrc/opt_step.hip; formulas: include/hdn_hip.h): the norm, the gate, the clip coefficient, the counters and the bias corrections are computed on
the device and left in a small control block that the update kernel reads.  Parameter and gradient pointers travel as kernel arguments
(TENSORS_PER_LAUNCH tensors per launch, work in chunks of CHUNK elements), so gradients allocated inside a capture are served.  The moments live in
three flat buffers the optimizer owns; state[p] holds views into them, in stock Adam's layout, so state_dict() loads into
torch.optim.Adam(amsgrad=True) and back.

param_groups[i]['lr'] is a 0-d float64 view of the device array the gate kernel reads when it runs: a scheduler that fills it in place
(ExponentialLR does) changes what a replayed graph uses.  betas, eps and weight_decay are one value for all groups (build_opt_lr's groups differ in
lr only).

What differs from the reference, on purpose: a finite loss with a non-finite gradient norm skips the step (report.status == 2), where
clip_grad_norm_ would multiply every gradient by NaN and Adam would write NaN into every parameter and moment.  install() rebinds nothing: a
training loop constructs GatedAMSGrad in place of torch.optim.Adam and calls step(outputs['total_loss']) in place of train.py:277-281
(INTEGRATION.md).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
from types import SimpleNamespace

import torch

from . import _lib
from ._lib import HdnHipError

TENSORS_PER_LAUNCH = 96   # hdn_opt_tensors_per_launch(): tensors whose pointers one launch carries
CHUNK = 4096              # hdn_opt_chunk(): elements per work item and per partial of the norm
_STATE_KEYS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def _lib_checked():
    lib = _lib.load()
    if lib.hdn_opt_tensors_per_launch() != TENSORS_PER_LAUNCH or lib.hdn_opt_chunk() != CHUNK:
        raise HdnHipError("libhdn_hip.so was built with another TENSORS_PER_LAUNCH / CHUNK than hdn_amd.optim states; rebuild")
    return lib


def _capturing(dev):
    return dev.type == "cuda" and torch.cuda.is_current_stream_capturing()


def _number(name, v, lo=None, lo_open=False, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f"GatedAMSGrad: {name} must be a finite number, got {v!r}")
    if lo is not None and (v <= lo if lo_open else v < lo):
        raise ValueError(f"GatedAMSGrad: {name} must be {'>' if lo_open else '>='} {lo}, got {v!r}")
    if hi is not None and v >= hi:
        raise ValueError(f"GatedAMSGrad: {name} must be < {hi}, got {v!r}")
    return float(v)


def _ptr_array(ptrs):
    return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)


def _numel_array(numels):
    return (ctypes.c_longlong * max(len(numels), 1))(*numels)


def _check_grad(g, dev, what):
    if g.is_sparse:
        raise ValueError(f"{what}: sparse gradients are not supported")
    if not g.is_cuda or g.device != dev:
        raise HdnHipError(f"{what}: the gradient is on {g.device}, the parameters on {dev}; there is no CPU fallback")
    if g.dtype != torch.float32:
        raise TypeError(f"{what}: gradients must be fp32, got {g.dtype}")
    if not g.is_contiguous():
        raise ValueError(f"{what}: the gradient is not contiguous")


def _sqnorm_and_gate(lib, dev, grads, numels, partials, ctrl, loss, loss_limit, max_norm, lr, group, n_opt, betas, steps, coef):
    """hdn_grad_sqnorm_f32 over `grads`, then hdn_opt_gate_f32 (n_opt = 0: the norm alone) on the current stream of `dev`."""
    gp, nn = _ptr_array([0 if g is None else g.data_ptr() for g in grads]), _numel_array(numels)
    _lib.launch("grad_sqnorm", dev, lib.hdn_grad_sqnorm_f32, gp, nn, len(grads), _lib.ptr(partials), partials.numel())
    _lib.launch("opt_gate", dev, lib.hdn_opt_gate_f32, _lib.ptr(partials), partials.numel(), _lib.opt(loss), loss_limit,
                0 if max_norm is None else 1, 0.0 if max_norm is None else max_norm, _lib.opt(lr), _lib.opt(group), gp, n_opt, betas[0], betas[1],
                _lib.ptr(ctrl), _lib.opt(steps), _lib.opt(coef))
    return gp, nn


def grad_norm(tensors):
    """The 2-norm of all the elements of `tensors` (gradients: fp32, contiguous, on one ROCm device; None entries contribute nothing) -> a 0-d
    fp32 device tensor, what clip_grad_norm_ returns for them.  Float64 sums in a fixed order: the same bits on every call.  No host read."""
    tensors = [None if t is None else t.detach() for t in tensors]
    present = [t for t in tensors if t is not None]
    if not present:
        raise ValueError("grad_norm: no tensor given")
    dev = _lib.require_device(*present)
    for t in present:
        _check_grad(t, dev, "grad_norm")
    lib = _lib_checked()
    numels = [0 if t is None else t.numel() for t in tensors]
    n_partials = lib.hdn_grad_sqnorm_partials(_numel_array(numels), len(numels))
    if n_partials < 0:
        _lib.check(int(n_partials), "grad_norm")
    partials = torch.empty(max(int(n_partials), 1), dtype=torch.float64, device=dev)[:int(n_partials)]
    ctrl = torch.empty(4, dtype=torch.float32, device=dev)
    _sqnorm_and_gate(lib, dev, tensors, numels, partials, ctrl, None, 0.0, None, None, None, 0, (0.0, 0.0), None, None)
    return ctrl[1]


class GatedAMSGrad(torch.optim.Optimizer):
    """Adam(amsgrad=True) with L2 weight decay behind clip_grad_norm_(max_norm) and the reference's loss gate, all on the device.

    step(loss=None): `loss` a 0-d fp32 device tensor or None (no loss gate).  The step is skipped - no byte of any parameter, moment or counter
    changes - when the loss is NaN, +-inf or > loss_limit (report.status 1) or the gradient norm is not finite (2).  A parameter whose .grad is
    None takes no part in norm or update and its counter does not advance.  report: status (int32 [1]), grad_norm (fp32 [1], before clipping),
    steps (fp32, one per parameter) - device tensors, read them when you want to know.  max_norm None: no clipping.  clip_grads_in_place: the
    clipped gradients are stored back into .grad, as clip_grad_norm_ leaves them (4 more bytes per element).  Construction uploads the constants:
    do it outside a capture."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None, loss_limit=1e4, clip_grads_in_place=False):
        lr = _number("lr", lr, 0.0)
        if not isinstance(betas, (tuple, list)) or len(betas) != 2:
            raise ValueError(f"GatedAMSGrad: betas must be a pair, got {betas!r}")
        betas = (_number("betas[0]", betas[0], 0.0, hi=1.0), _number("betas[1]", betas[1], 0.0, hi=1.0))
        eps = _number("eps", eps, 0.0)
        weight_decay = _number("weight_decay", weight_decay, 0.0)
        self.max_norm = None if max_norm is None else _number("max_norm", max_norm, 0.0, lo_open=True)
        if isinstance(loss_limit, bool) or not isinstance(loss_limit, (int, float)) or loss_limit != loss_limit:
            raise ValueError(f"GatedAMSGrad: loss_limit must be a number, got {loss_limit!r}")
        self.loss_limit = float(loss_limit)
        if not isinstance(clip_grads_in_place, bool):
            raise ValueError(f"GatedAMSGrad: clip_grads_in_place must be a bool, got {clip_grads_in_place!r}")
        self.clip_grads_in_place = clip_grads_in_place
        self._built = False
        # stock Adam's keys, so that a state_dict of either loads into the other
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=True, maximize=False, foreach=None, capturable=False,
                        differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        self._build()

    def add_param_group(self, param_group):
        if getattr(self, "_built", False):
            raise RuntimeError("GatedAMSGrad: the flat state is laid out at construction; a parameter group cannot be added afterwards")
        super().add_param_group(param_group)

    # ---- construction -------------------------------------------------------------------------------------------------------------------
    def _build(self):
        d = self.defaults
        flat, group_of = [], []
        for gi, group in enumerate(self.param_groups):
            group["lr"] = _number(f"param_groups[{gi}]['lr']", group["lr"], 0.0)
            for k in ("betas", "eps", "weight_decay"):
                if tuple(group[k]) != tuple(d[k]) if k == "betas" else group[k] != d[k]:
                    raise ValueError(f"GatedAMSGrad: param_groups[{gi}]['{k}'] = {group[k]!r} differs from {d[k]!r}; the groups share betas, eps "
                                     "and weight_decay (only lr is per group)")
            for p in group["params"]:
                flat.append(p)
                group_of.append(gi)
        dev = None
        for p in flat:
            if not p.is_cuda:
                raise HdnHipError(f"GatedAMSGrad runs on the GPU only (a parameter is on {p.device}); there is no CPU fallback")
            if p.dtype != torch.float32:
                raise TypeError(f"GatedAMSGrad: parameters must be fp32, got {p.dtype}")
            if p.is_sparse or not p.is_contiguous():
                raise ValueError("GatedAMSGrad: parameters must be dense and contiguous")
            if dev is None:
                dev = p.device
            elif p.device != dev:
                raise HdnHipError(f"GatedAMSGrad: parameters on different devices: {dev} vs {p.device}")
        if _capturing(dev):
            raise RuntimeError("GatedAMSGrad: construction uploads the learning rates and lays out the state; construct the optimizer outside "
                               "the capture")
        lib = _lib_checked()
        n = len(flat)
        self._flat, self._dev, self._numels = flat, dev, [p.numel() for p in flat]
        self._numel_arr = _numel_array(self._numels)
        total, n_partials = lib.hdn_opt_state_floats(self._numel_arr, n), lib.hdn_grad_sqnorm_partials(self._numel_arr, n)
        for v in (total, n_partials):
            if v < 0:
                _lib.check(int(v), "GatedAMSGrad")
        self._state_floats = int(total)
        zeros = lambda k, dtype=torch.float32: torch.zeros(max(int(k), 4), dtype=dtype, device=dev)
        self._bufs = {k: zeros(total) for k in _STATE_KEYS}
        self._steps, self._coef = zeros(n)[:n], zeros(2 * n)
        self._partials = zeros(n_partials, torch.float64)[:int(n_partials)]
        self._ctrl_i = torch.zeros(4, dtype=torch.int32, device=dev)
        self._ctrl = self._ctrl_i.view(torch.float32)
        self._lr = torch.tensor([g["lr"] for g in self.param_groups], dtype=torch.float64, device=dev)
        self._group = torch.tensor(group_of + [0], dtype=torch.int32, device=dev)[:n]
        self.report = SimpleNamespace(status=self._ctrl_i[0:1], grad_norm=self._ctrl[1:2], steps=self._steps)
        self._slots, slot = [], 0
        for k in self._numels:
            self._slots.append(slot)
            slot += (k + 3) // 4 * 4
        self._bind_state()
        self._bind_lr()
        self._built = True

    def _bind_state(self):
        for i, p in enumerate(self._flat):
            s, k = self._slots[i], self._numels[i]
            st = {"step": self._steps[i]}
            for key in _STATE_KEYS:
                st[key] = self._bufs[key][s:s + k].view(p.shape)
            self.state[p] = st

    def _bind_lr(self):
        self._lr_views = [self._lr[i] for i in range(len(self.param_groups))]
        for group, view in zip(self.param_groups, self._lr_views):
            group["lr"] = view

    def _sync_lr(self):
        """A group whose 'lr' was replaced by a number (not filled in place) is written to the device array and bound to its view again."""
        for i, group in enumerate(self.param_groups):
            if group["lr"] is not self._lr_views[i]:
                if _capturing(self._dev):
                    raise RuntimeError("GatedAMSGrad: param_groups[%d]['lr'] was replaced by a new object; writing it to the device uploads, "
                                       "which a capture cannot do.  Fill the tensor in place (lr.fill_(v)), as torch's schedulers do" % i)
                v = group["lr"]
                self._lr_views[i].fill_(float(v))
                group["lr"] = self._lr_views[i]

    # ---- the step -----------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, loss=None):
        dev, n = self._dev, len(self._flat)
        if loss is not None:
            if not isinstance(loss, torch.Tensor) or loss.dim() != 0:
                raise ValueError("GatedAMSGrad.step: loss must be a 0-d tensor (it is read on the device, never by the host)")
            if not loss.is_cuda or loss.device != dev:
                raise HdnHipError(f"GatedAMSGrad.step: loss is on {loss.device}, the parameters on {dev}; there is no CPU fallback")
            if loss.dtype != torch.float32:
                raise TypeError(f"GatedAMSGrad.step: loss must be fp32, got {loss.dtype}")
            loss = loss.detach()
        self._sync_lr()
        grads = []
        for p in self._flat:
            g = p.grad
            if g is not None:
                _check_grad(g, dev, "GatedAMSGrad.step")
                if g.shape != p.shape:
                    raise ValueError(f"GatedAMSGrad.step: a gradient of shape {list(g.shape)} for a parameter of shape {list(p.shape)}")
            grads.append(g)
        if n == 0:
            return
        lib, d = _lib.load(), self.defaults
        gp, nn = _sqnorm_and_gate(lib, dev, grads, self._numels, self._partials, self._ctrl, loss, self.loss_limit, self.max_norm, self._lr,
                                  self._group, n, d["betas"], self._steps, self._coef)
        pp = _ptr_array([p.data_ptr() for p in self._flat])
        _lib.launch("amsgrad_apply", dev, lib.hdn_amsgrad_apply_f32, pp, gp, nn, n, *(_lib.ptr(self._bufs[k]) for k in _STATE_KEYS),
                    self._state_floats, _lib.ptr(self._ctrl), _lib.ptr(self._coef), d["betas"][0], d["betas"][1], d["eps"], d["weight_decay"],
                    1 if (self.clip_grads_in_place and self.max_norm is not None) else 0)
        # the kernels wrote through raw pointers: tell autograd's version counters, which the package's parameter caches are keyed on
        # (PreShareFeature's folded and packed blocks, the heads' packed weights).  A step the device skipped costs those caches one rebuild.
        torch.autograd.graph.increment_version([p for p, g in zip(self._flat, grads) if g is not None])
        if self.clip_grads_in_place and self.max_norm is not None:
            torch.autograd.graph.increment_version([g for g in grads if g is not None])

    # ---- checkpoints: stock Adam's layout -------------------------------------------------------------------------------------------------
    def state_dict(self):
        """torch.optim.Adam(amsgrad=True)'s layout, as a snapshot (clones, not the views) with the learning rates as numbers (a host read)."""
        sd = super().state_dict()
        sd["state"] = {k: {name: (v.clone() if isinstance(v, torch.Tensor) else v) for name, v in st.items()} for k, st in sd["state"].items()}
        groups = []
        for g in sd["param_groups"]:
            g = dict(g)
            for k in ("lr", "initial_lr"):
                if isinstance(g.get(k), torch.Tensor):
                    g[k] = float(g[k])
            groups.append(g)
        sd["param_groups"] = groups
        return sd

    def load_state_dict(self, state_dict):
        """Loads a state_dict of this class or of torch.optim.Adam(amsgrad=True) on the same parameters: the moments and counters are copied into
        the flat buffers, the learning rates into the device array.  A parameter the checkpoint has no state for starts from zero."""
        if _capturing(self._dev):
            raise RuntimeError("GatedAMSGrad.load_state_dict uploads; call it outside the capture")
        for g in state_dict["param_groups"]:
            if not g.get("amsgrad", True):
                raise ValueError("GatedAMSGrad.load_state_dict: the checkpoint is of Adam(amsgrad=False); it has no max_exp_avg_sq")
        super().load_state_dict(state_dict)
        loaded = self.state
        self.state = type(loaded)()
        steps = []
        for i, p in enumerate(self._flat):
            st = loaded.get(p, {})
            if st and any(k not in st for k in _STATE_KEYS + ("step",)):
                raise ValueError("GatedAMSGrad.load_state_dict: a parameter's state lacks one of step, exp_avg, exp_avg_sq, max_exp_avg_sq")
            s, k = self._slots[i], self._numels[i]
            for key in _STATE_KEYS:
                dst = self._bufs[key][s:s + k]
                if st:
                    dst.copy_(st[key].reshape(-1))
                else:
                    dst.zero_()
            steps.append(float(st["step"]) if st else 0.0)
        if steps:
            self._steps.copy_(torch.tensor(steps, dtype=torch.float32))
        self._bind_state()
        lrs = [float(g["lr"]) for g in self.param_groups]
        self._lr.copy_(torch.tensor(lrs, dtype=torch.float64))
        self._bind_lr()
