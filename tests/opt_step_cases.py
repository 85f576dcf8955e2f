"""Shared cases and oracle of the gated, clipped AMSGrad step (hdn_amd.optim.GatedAMSGrad; the reference's tools/train.py:271-281).

reference_steps(...) restates those lines in float64 numpy over K steps: the loss gate, the total gradient norm, the clip coefficient, L2 weight
decay, Adam's moments with amsgrad, per-group learning rates, absent gradients, and the package's one deviation (a finite loss with a non-finite
gradient norm skips the step, status 2).  It also carries the simulated wrong kernels (MUTATIONS) the host test needs.

stock_steps(case, dtype) runs the reference's own formulation - is_valid_number, clip_grad_norm_(foreach=False), Adam(amsgrad=True, foreach=False) -
on the CPU: in float64 it must agree with the oracle to float64 rounding (where stock PyTorch would write NaN everywhere the deviation is applied
instead: the step is skipped); in float32 it gives d_ref, the distance of an honest fp32 implementation from the oracle.

The bound is the package's chain convention (docs/PARITY.md): |x - oracle| <= max(4 d_ref, 1 ulp_fp32(|oracle|)).  Distances are taken in units
of ulp_fp32(|oracle|) of the element and d_ref is the largest over all the elements of a quantity in a case (every parameter; every exp_avg; ...):
a case holds one-element tensors, whose own d_ref is a single draw of a rounding error and may be 0 where another honest implementation is one
rounding away.  Magnitudes are chosen so that nothing cancels (gradients carry their parameter's sign, parameters stay O(1), gradient scales
1e-3 .. 1e3 are per tensor), so one ulp scale per element is meaningful.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

CHUNK = 4096               # hdn_amd.optim.CHUNK / TENSORS_PER_LAUNCH, restated: the host test holds them to the module's
TENSORS_PER_LAUNCH = 96
K = 3
BETAS, EPS, WEIGHT_DECAY, LOSS_LIMIT = (0.9, 0.999), 1e-8, 1e-4, 1e4
LR_BASE, LR_HOMO, LR_THIRD = 2e-4, 2e-5, 1.6e-4          # the shipped YAML's two, and the first after one ExponentialLR(0.8) step
STEP_FACTOR = (1.0, 0.6, 1.3)                            # the gradients' common factor per step
QUANTITIES = ("param", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")
SIZES = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
MUTATIONS = ("decoupled_weight_decay", "v_for_vmax", "vmax_before_v", "eps_inside_sqrt", "no_clamp", "decay_before_norm", "norm_per_group",
             "first_group_lr", "gate_ge", "gate_neg_inf_passes", "count_skipped", "advance_gradless", "tail_not_updated",
             "chunk_first_not_updated")
_SCALES = (1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3)


@dataclass
class Case:
    name: str
    sizes: tuple
    group_of: tuple
    lrs: tuple                                       # one per group
    max_norm: object = 10.0                          # None: clipping off
    losses: tuple = (12.5, 9999.0, 0.25)             # per step: a number (fp32-exact) or None
    scales: tuple = ()                               # gradient scale per tensor (default: cycling 1e-3 .. 1e3)
    absent: frozenset = frozenset()                  # (step, tensor): .grad is None
    poison: dict = field(default_factory=dict)       # (step, tensor) -> a value written into the gradient's middle element
    warm: bool = False                               # start from moments and counters of earlier steps
    param_offset: tuple = ()                         # per tensor: the parameter is a view this many floats off a 16-byte boundary
    grad_offset: tuple = ()
    seed: int = 0

    def _rng(self, salt):
        return np.random.default_rng(1000 * self.seed + salt)

    def scale(self, i):
        return self.scales[i] if self.scales else _SCALES[i % len(_SCALES)]

    def params0(self):
        g = self._rng(1)
        return [(g.choice([-1.0, 1.0], n) * g.uniform(0.5, 2.0, n)).astype(np.float32) for n in self.sizes]

    def grads(self):
        """[step][tensor] -> fp32 array or None; a gradient has its parameter's sign, so c g + wd p never cancels"""
        g, p0 = self._rng(2), self.params0()
        out = []
        for k in range(K):
            row = []
            for i, n in enumerate(self.sizes):
                a = (np.sign(p0[i]) * self.scale(i) * STEP_FACTOR[k] * g.uniform(0.5, 1.5, n)).astype(np.float32)
                if (k, i) in self.poison:
                    a[n // 2] = self.poison[(k, i)]
                row.append(None if (k, i) in self.absent else a)
            out.append(row)
        return out

    def state0(self):
        """None, or the state of a run that has been going: counters 10 and 3, max_exp_avg_sq well above exp_avg_sq"""
        if not self.warm:
            return None
        g, p0 = self._rng(3), self.params0()
        st = dict(step=[], exp_avg=[], exp_avg_sq=[], max_exp_avg_sq=[])
        for i, n in enumerate(self.sizes):
            s = self.scale(i)
            v = ((s * g.uniform(0.5, 1.5, n)) ** 2).astype(np.float32)
            st["step"].append(10.0 if i % 2 == 0 else 3.0)
            st["exp_avg"].append((np.sign(p0[i]) * s * g.uniform(0.5, 1.5, n)).astype(np.float32))
            st["exp_avg_sq"].append(v)
            st["max_exp_avg_sq"].append((v * g.uniform(2.0, 6.0, n)).astype(np.float32))
        return st

    def loss32(self, k):
        return None if self.losses[k] is None else np.float32(self.losses[k])


def _alternate(n, groups):
    return tuple(i % groups for i in range(n))


NEXT_AFTER_LIMIT = float(np.nextafter(np.float32(LOSS_LIMIT), np.float32(np.inf)))
GATE_LOSSES = {"nan": float("nan"), "pos_inf": float("inf"), "neg_inf": float("-inf"), "at_limit": LOSS_LIMIT, "above_limit": NEXT_AFTER_LIMIT}
GATE_STATUS = {"nan": 1, "pos_inf": 1, "neg_inf": 1, "at_limit": 0, "above_limit": 1, "no_loss": 0, "nan_grad": 2, "inf_grad": 2}


def gate_case(kind):
    """Two tensors over two groups; the middle step meets the gate: `kind` one of GATE_STATUS"""
    kw = dict(name="gate_" + kind, sizes=(3, 65), group_of=(0, 1), lrs=(LR_BASE, LR_HOMO), scales=(1.0, 1e-2), seed=7)
    if kind in GATE_LOSSES:
        return Case(losses=(1.0, GATE_LOSSES[kind], 2.0), **kw)
    if kind == "no_loss":
        return Case(losses=(None, None, None), **kw)
    return Case(poison={(1, 1): float("nan") if kind == "nan_grad" else float("inf")}, **kw)


def all_cases():
    many = TENSORS_PER_LAUNCH + 1
    cases = [
        Case("sizes", SIZES, _alternate(len(SIZES), 2), (LR_BASE, LR_HOMO), seed=1),                               # norm far above max_norm
        Case("many", (1,) * many, _alternate(many, 3), (LR_BASE, LR_HOMO, LR_THIRD), absent=frozenset({(1, 5)}), seed=2),
        Case("below", (5, 64, 257), (0, 1, 0), (LR_BASE, LR_HOMO), scales=(1e-3, 1e-2, 1e-3), seed=3),             # norm < max_norm: c clamped to 1
        Case("small_clip", (5, 64, 257), (0, 1, 1), (LR_BASE, LR_HOMO), max_norm=1e-3, scales=(1e-3, 1e-3, 1e-3), seed=4),
        Case("no_clip", (7, 1025), (0, 1), (LR_BASE, LR_HOMO), max_norm=None, scales=(1e-1, 1e3), seed=5),
        Case("absent", (4, 63, 1023), (0, 1, 2), (LR_BASE, LR_HOMO, LR_THIRD), absent=frozenset({(1, 1)}), scales=(1.0, 1e-1, 1e1), seed=6),
        Case("warm", (8, 255), (0, 1), (LR_BASE, LR_HOMO), warm=True, scales=(1e-2, 1.0), seed=8),
        Case("misaligned", (CHUNK + 5, 9, 130), (0, 1, 0), (LR_BASE, LR_HOMO), param_offset=(1, 0, 1), grad_offset=(0, 1, 1),
             scales=(1e-1, 1.0, 1e1), seed=9),
    ]
    return cases + [gate_case(k) for k in GATE_STATUS]


def case(name):
    for c in all_cases():
        if c.name == name:
            return c
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------------------------------------------ the oracle
def _rejected(x, limit, mutation):
    """train.py:220-221: not is_valid_number(x)"""
    if mutation == "gate_ge":
        return math.isnan(x) or math.isinf(x) or x >= limit
    if mutation == "gate_neg_inf_passes":
        return math.isnan(x) or x == math.inf or x > limit
    return math.isnan(x) or math.isinf(x) or x > limit


def reference_steps(params, grads, group_of, lrs, losses, betas=BETAS, eps=EPS, weight_decay=WEIGHT_DECAY, max_norm=10.0, loss_limit=LOSS_LIMIT,
                    state=None, mutation=None, chunk=CHUNK):
    """float64.  params: list of arrays; grads: [step][tensor] arrays or None; lrs: one per group, or a list of such per step; losses: per step a
    number or None.  -> dict(param, exp_avg, exp_avg_sq, max_exp_avg_sq: lists; steps: array; status, grad_norm: per step; clipped: [step][tensor])"""
    assert mutation is None or mutation in MUTATIONS
    b1, b2 = betas
    n = len(params)
    p = [np.asarray(x, np.float64).copy() for x in params]
    get = (lambda key: [np.asarray(x, np.float64).copy() for x in state[key]]) if state else (lambda key: [np.zeros_like(x) for x in p])
    m, v, vmax = get("exp_avg"), get("exp_avg_sq"), get("max_exp_avg_sq")
    t = np.asarray(state["step"], np.float64).copy() if state else np.zeros(n)
    out = dict(status=[], grad_norm=[], clipped=[])
    with np.errstate(all="ignore"):
        for k, row in enumerate(grads):
            lr = lrs[k] if isinstance(lrs[0], (tuple, list)) else lrs
            g = [None if a is None else np.asarray(a, np.float64) for a in row]
            for_norm = [None if a is None else (a + weight_decay * p[i] if mutation == "decay_before_norm" else a) for i, a in enumerate(g)]
            sq = [0.0 if a is None else float(np.sum(a * a)) for a in for_norm]
            norm = math.sqrt(sum(sq)) if not math.isnan(sum(sq)) else math.nan
            loss = losses[k]
            status = 0
            if loss is not None and _rejected(float(loss), loss_limit, mutation):
                status = 1
            elif not math.isfinite(norm):
                status = 2

            def coef(nrm):
                if max_norm is None:
                    return 1.0
                c = max_norm / (nrm + 1e-6)
                return c if mutation == "no_clamp" else min(1.0, c)

            if mutation == "norm_per_group":
                gsq = {}
                for i in range(n):
                    gsq[group_of[i]] = gsq.get(group_of[i], 0.0) + sq[i]
                cs = [coef(math.sqrt(gsq[group_of[i]])) for i in range(n)]
            else:
                cs = [coef(norm)] * n
            out["status"].append(status)
            out["grad_norm"].append(norm)
            out["clipped"].append([None if a is None else (cs[i] * a if status == 0 else a) for i, a in enumerate(g)])  # skipped: untouched
            if status != 0:
                if mutation == "count_skipped":
                    t += np.array([0.0 if a is None else 1.0 for a in g])
                continue
            for i in range(n):
                if g[i] is None:
                    if mutation == "advance_gradless":
                        t[i] += 1
                    continue
                t[i] += 1
                old = (p[i].copy(), m[i].copy(), v[i].copy(), vmax[i].copy())
                gc = cs[i] * g[i]
                ge = gc if mutation == "decoupled_weight_decay" else gc + weight_decay * p[i]
                group_lr = lr[0] if mutation == "first_group_lr" else lr[group_of[i]]
                if mutation == "decoupled_weight_decay":
                    p[i] = p[i] * (1.0 - group_lr * weight_decay)
                m[i] = b1 * m[i] + (1 - b1) * ge
                v_old = v[i]
                v[i] = b2 * v[i] + (1 - b2) * ge * ge
                vmax[i] = np.maximum(vmax[i], v_old if mutation == "vmax_before_v" else v[i])
                step_size = group_lr / (1 - b1 ** t[i])
                inv_sqrt_bc2 = 1 / math.sqrt(1 - b2 ** t[i])
                second = v[i] if mutation == "v_for_vmax" else vmax[i]
                denom = np.sqrt(second + eps) * inv_sqrt_bc2 if mutation == "eps_inside_sqrt" else np.sqrt(second) * inv_sqrt_bc2 + eps
                p[i] = p[i] - step_size * m[i] / denom
                keep = np.zeros(p[i].size, bool)
                if mutation == "tail_not_updated":
                    keep[p[i].size - p[i].size % 4:] = True
                if mutation == "chunk_first_not_updated":
                    keep[chunk::chunk] = True
                if keep.any():
                    for new, was in zip((p[i], m[i], v[i], vmax[i]), old):
                        new[keep] = was[keep]
    out.update(param=p, exp_avg=m, exp_avg_sq=v, max_exp_avg_sq=vmax, steps=t)
    return out


def oracle(c, mutation=None):
    return reference_steps(c.params0(), c.grads(), c.group_of, c.lrs, [c.loss32(k) for k in range(K)], max_norm=c.max_norm, state=c.state0(),
                           mutation=mutation)


# ---------------------------------------------------------------------------------------------------- the reference's own lines, stock PyTorch, CPU
def is_valid_number(x):
    return not (math.isnan(x) or math.isinf(x) or x > 1e4)


def stock_steps(c, dtype, device="cpu", foreach=False, lrs_steps=None):
    """tools/train.py:271-281 with stock PyTorch in `dtype` on `device` -> the same dictionary as reference_steps.  Where the gradient norm is not
    finite the step is skipped (the package's deviation); stock PyTorch would turn every parameter and moment into NaN there."""
    p0, grads, st0 = c.params0(), c.grads(), c.state0()
    params = [torch.nn.Parameter(torch.tensor(a, dtype=dtype, device=device)) for a in p0]
    groups = [{"params": [p for i, p in enumerate(params) if c.group_of[i] == gi], "lr": lr} for gi, lr in enumerate(c.lrs)]
    opt = torch.optim.Adam(groups, lr=c.lrs[0], betas=BETAS, eps=EPS, weight_decay=WEIGHT_DECAY, amsgrad=True, foreach=foreach)
    if st0:
        for i, p in enumerate(params):
            opt.state[p] = {"step": torch.tensor(st0["step"][i], dtype=torch.float32)}
            for key in QUANTITIES[1:]:
                opt.state[p][key] = torch.tensor(st0[key][i], dtype=dtype, device=device)
    out = dict(status=[], grad_norm=[], clipped=[])
    for k in range(K):
        if lrs_steps is not None:
            for group, lr in zip(opt.param_groups, lrs_steps[k]):
                group["lr"] = lr
        for i, p in enumerate(params):
            p.grad = None if grads[k][i] is None else torch.tensor(grads[k][i], dtype=dtype, device=device)
        loss = c.loss32(k)
        status = 0 if loss is None or is_valid_number(float(loss)) else 1
        kept = [None if p.grad is None else p.grad.clone() for p in params]
        norm = torch.nn.utils.clip_grad_norm_(params, math.inf if c.max_norm is None else c.max_norm, foreach=foreach)
        if status == 0 and not math.isfinite(float(norm)):
            status = 2
        if status != 0:                                      # a skipped step leaves the gradients as they were
            for p, g in zip(params, kept):
                p.grad = g
        out["status"].append(status)
        out["grad_norm"].append(float(norm))
        out["clipped"].append([None if p.grad is None else p.grad.detach().double().cpu().numpy().copy() for p in params])
        if status == 0:
            opt.step()
    f64 = lambda t: t.detach().double().cpu().numpy()
    zero = lambda p: np.zeros(p.numel())
    out["param"] = [f64(p) for p in params]
    for key in QUANTITIES[1:]:
        out[key] = [f64(opt.state[p][key]) if key in opt.state[p] else zero(p) for p in params]
    out["steps"] = np.array([float(opt.state[p]["step"]) if "step" in opt.state[p] else 0.0 for p in params])
    return out


# ------------------------------------------------------------------------------------------------------------------------------------ the bound
def ulp32(x):
    """one unit in the last place of fp32 at |x| (x float64)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def distance(got, want):
    """the largest |got - want| / ulp_fp32(|want|) over the elements of two lists of arrays (None entries must coincide); a non-finite element of
    `want` must be met by the same value (distance 0), anything else is inf"""
    worst = 0.0
    for a, b in zip(got, want):
        if a is None or b is None:
            if not (a is None and b is None):
                return math.inf
            continue
        a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
        if a.size == 0:
            continue
        fin = np.isfinite(b)
        same = (np.isnan(a) & np.isnan(b)) | (a == b)
        if not same[~fin].all() or not np.isfinite(a[fin]).all():
            return math.inf
        if fin.any():
            worst = max(worst, float(np.max(np.abs(a[fin] - b[fin]) / ulp32(b[fin]))))
    return worst


def compared(res, clipped=False):
    """quantity -> list of arrays of one result dictionary: the four state quantities, grad_norm per step and, where asked for, the gradients
    every step leaves behind (clipped where the step was taken, untouched where it was skipped)"""
    q = {key: res[key] for key in QUANTITIES}
    q["grad_norm"] = [np.array(res["grad_norm"])]
    if clipped:
        q["clipped"] = [a for row in res["clipped"] for a in row]
    return q


def bound(d_ref):
    """in ulps: the chain convention max(4 d_ref, floor) with a floor of one unit in the last place"""
    return max(4.0 * d_ref, 1.0)


_REF = {}


def references(c):
    """(oracle, d_ref per quantity in ulps) of a case, computed once"""
    if c.name not in _REF:
        want = oracle(c)
        s32 = stock_steps(c, torch.float32)
        qw, qs = compared(want, clipped=True), compared(s32, clipped=True)
        _REF[c.name] = (want, {k: distance(qs[k], qw[k]) for k in qw}, s32)
    return _REF[c.name][:2]


def stock32(c):
    references(c)
    return _REF[c.name][2]


def check(res, c, clipped=False, label="", enforce=True):
    """Every compared quantity of `res` within the bound of case `c`, status and counters exact -> {quantity: (distance, bound)}; enforce=False
    prints the figures of the quantities and asserts status and counters only (a measurement of somebody else's code)"""
    want, d_ref = references(c)
    assert list(res["status"]) == want["status"], (c.name, label, res["status"], want["status"])
    assert np.array_equal(np.asarray(res["steps"], np.float64), want["steps"]), (c.name, label, "steps")
    got, exp, figures = compared(res, clipped), compared(want, clipped), {}
    for k in got:
        d, b = distance(got[k], exp[k]), bound(d_ref[k])
        figures[k] = (d, b)
        print(f"OPT_STEP {c.name} {label} {k}: d {d:.3f} ulp, d_ref {d_ref[k]:.3f} ulp, bound {b:.3f} ulp, d / bound {d / b:.3f}")
    for k, (d, b) in figures.items():
        assert d <= b or not enforce, (c.name, label, k, d, b)
    return figures
