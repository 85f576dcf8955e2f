"""The cases, the bounds and the expectations that tests/test_triplet_mean_host.py (CPU) and tests/test_gpu_triplet_mean.py (GPU) share for the
flag-selected triplet means of csrc/triplet_loss.hip (hdn_triplet_l1_mean_f32, hdn_triplet_l1_mean_bwd_f32).  Nothing here touches the device.

Truth: float64.  The sets from the flags (sel: fp32(if_pos if_unsup) == 1, neg: if_pos == 0), the row losses of the used samples from closed() of
tests/triplet_cases.py, summed and divided in float64.

The bound of the value, for any summation order, with M used rows, u = 2^-24 and n_sel the divisor (as it is `out`'s):

    bound = ( sum tol_row + (M + 2) u sum loss64 ) / (denom n_sel)

tol_row bounds each row (tests/triplet_cases.py), M - 1 additions and two divisions round once each.  n_sel == 0: the value is exactly 0.

Gradients: an element is c k with k {0, +-1, +-2} the sign pattern of the row kernels and ONE fp32 factor c per call.  check_grads() takes c_got
from the first element whose k is not 0 (a division by +-1 or +-2: exact), asserts got / c_got == k exactly (torch.equal) and |c_got - c64| <= 3 u |c64| (two divisions, and the
conversion of grad_out).  Rows with |v64| <= tol_row are left out of the gradient comparison only, at most 1 % of a case's rows (EXCLUDED_CAP;
the host test asserts that these seeds give none).  Rows of unused samples are always compared: they are zero.

Shapes: (N, R) in (1,1), (3,1), (2,2), (5,1), (3,3), (2,127), (9,3) - the row kernels hold four rows per workgroup, so 1, 3, 4, 5, 9 rows are a
lone row, one fewer, exactly one, one more and a tail after two workgroups; 2 x 127 and 9 x 3 = 27 put a sample boundary inside a workgroup - and
D in 1, 63, 64, 65, 127, 129, either side of one and two lane passes of the 64-lane wave.
"""
import functools

import numpy as np
import torch

from triplet_cases import EPS, SEED, U, closed, tol

EXCLUDED_CAP = 0.01
DENOM = 127 * 127
SHAPES = ((1, 1), (3, 1), (2, 2), (5, 1), (3, 3), (2, 127), (9, 3))
DS = (1, 63, 64, 65, 127, 129)
PATTERNS = ("all", "none_with_neg", "none_no_neg", "first", "last", "alternating", "half", "quirk", "nan_unused")


def flags(pattern, N):
    """(if_pos, if_unsup) float32 [N] of a named pattern.
    all: every sample selected.  none_with_neg / none_no_neg: nobody selected, everybody / nobody negative.  first: sample 0 selected, the others
    unsupervised negatives (if_unsup alone would select them).  last: the last selected, the others supervised positives (no negative: under rule 1
    every sample is used and the divisor stays n_sel).  alternating: even samples selected, odd ones negative.  half: sample 0 carries if_pos = 0.5,
    which fails both sets.  quirk: no negative and n_sel < N.  nan_unused: as alternating (the case fills the unused samples with NaN)."""
    pos, un = np.ones(N, np.float32), np.ones(N, np.float32)
    if pattern == "none_with_neg":
        pos[:] = 0
    elif pattern == "none_no_neg":
        un[:] = 0
    elif pattern == "first":
        pos[1:] = 0
    elif pattern == "last":
        un[:-1] = 0
    elif pattern in ("alternating", "nan_unused"):
        pos[1::2] = 0
        un[1::4] = 0
    elif pattern == "half":
        pos[0] = 0.5
        if N > 2:
            pos[2] = 0
    elif pattern == "quirk":
        un[1::2] = 0
    elif pattern != "all":
        raise KeyError(pattern)
    return pos, un


def sets(if_pos, if_unsup):
    """(sel [N] bool, neg [N] bool) as the kernel decides them: fp32 product compared with 1, if_pos compared with 0."""
    pos, un = np.asarray(if_pos, np.float32), np.asarray(if_unsup, np.float32)
    with np.errstate(invalid="ignore"):
        return (pos * un) == np.float32(1), pos == np.float32(0)


def used_samples(sel, neg, rule, variant=None):
    if sel.sum() == 0:
        return np.zeros_like(sel)
    if rule == 1 and neg.sum() == 0 and variant != "no_quirk":
        return np.ones_like(sel)
    return sel.copy()


class Case:
    """a, p, n [N,R,D] fp32, if_pos, if_unsup [N] fp32, rule, denom, margin, eps, g (grad_out, one fp32); exact: the value is the fp32
    restatement bit for bit (row losses and their sum are exact integers by construction)."""

    def __init__(self, name, a, p, n, if_pos, if_unsup, rule, denom=DENOM, margin=1.0, eps=EPS, g=1.0, exact=False):
        self.name, self.a, self.p, self.n, self.rule, self.denom, self.margin, self.eps, self.exact = name, a, p, n, rule, float(denom), margin, eps, exact
        self.if_pos, self.if_unsup = torch.from_numpy(np.asarray(if_pos, np.float32)), torch.from_numpy(np.asarray(if_unsup, np.float32))
        self.N, self.R, self.D = a.shape
        self.g = torch.tensor([g], dtype=torch.float32)

    @functools.lru_cache(maxsize=None)
    def truth(self):
        """Computed once: counts, the float64 value and its bound, c64, the integer patterns and which elements are compared."""
        sel, neg = sets(self.if_pos.numpy(), self.if_unsup.numpy())
        n_sel, n_neg = int(sel.sum()), int(neg.sum())
        used = used_samples(sel, neg, self.rule)
        idx = np.nonzero(used)[0]
        k = [torch.zeros(self.a.shape, dtype=torch.float32) for _ in range(3)]
        compared = torch.ones(self.a.shape, dtype=torch.bool)
        out = {"n_sel": n_sel, "n_neg": n_neg, "used": used, "value": 0.0, "bound": 0.0, "c64": 0.0, "excluded": 0, "rows": int(len(idx)) * self.R}
        if len(idx):
            a, p, n = (t[torch.from_numpy(idx)] for t in (self.a, self.p, self.n))
            c = closed(a.numpy(), p.numpy(), n.numpy(), self.margin, self.eps)
            t = tol(c["d_ap"], c["d_an"], self.D, self.margin, self.eps)
            M, S = c["loss"].size, float(c["loss"].sum())
            out["value"] = S / self.denom / n_sel
            out["bound"] = (float(t.sum()) + (M + 2) * U * S) / (self.denom * n_sel)
            out["c64"] = float(self.g[0]) / self.denom / n_sel
            e32 = torch.tensor(self.eps, dtype=torch.float32)
            s_ap, s_an = torch.sign((a - p) + e32), torch.sign((a - n) + e32)         # fp32 elementwise: no order to depend on
            act = torch.from_numpy(c["v"] >= 0).float().unsqueeze(-1)
            cmp_rows = torch.from_numpy(np.abs(c["v"]) > t)
            for dst, src in zip(k, (act * (s_ap - s_an), -act * s_ap, act * s_an)):
                dst[torch.from_numpy(idx)] = src
            compared[torch.from_numpy(idx)] = cmp_rows.unsqueeze(-1).expand(a.shape)
            out["excluded"] = int((~cmp_rows).sum())
        out.update(k=tuple(k), compared=compared)
        return out


def restate32(case, variant=None):
    """The value in fp32 as the kernel's formulas state it (the sum in numpy's order: any order is inside the bound) -> np.float32.  variant: one of
    MUTATIONS, a mistake the tests must be able to see."""
    pos, un = case.if_pos.numpy(), case.if_unsup.numpy()
    sel, neg = sets(pos, un)
    if variant == "unsup_only":
        sel = un == np.float32(1)
    n_sel = int(sel.sum())
    if n_sel == 0:
        return np.float32(0)
    used = used_samples(sel, neg, case.rule, variant)
    idx = torch.from_numpy(np.nonzero(used)[0])
    c = closed(case.a[idx].numpy(), case.p[idx].numpy(), case.n[idx].numpy(), case.margin, np.float32(case.eps), dtype=np.float32)
    S = c["loss"].sum(dtype=np.float32)
    div = np.float32(case.N if variant == "divisor_N" else n_sel)
    denom = np.float32(case.R * case.D if variant == "rd_denom" else case.denom)
    first_denom = (case.rule == 0) != (variant == "div_order")
    return (S / denom) / div if first_denom else (S / div) / denom


MUTATIONS = ("divisor_N", "no_quirk", "unsup_only", "rd_denom")            # each leaves the bound on at least one case; div_order: see ORDER_CASES


def check_value(case, value, counts, what=""):
    t = case.truth()
    assert [int(v) for v in counts] == [t["n_sel"], t["n_neg"]], (case.name, what, counts)
    got = float(value)
    if t["n_sel"] == 0:
        assert got == 0.0, (case.name, what, got)
        return 0.0
    err = abs(got - t["value"])
    assert err <= t["bound"], (case.name, what, got, t["value"], err, t["bound"])
    return err / t["bound"] if t["bound"] else 0.0


def check_grads(case, grads, what=""):
    """grads: (ga | None, gp | None, gn | None) fp32 on the CPU.  Returns c_got (None when no element is active)."""
    t = case.truth()
    c_got = None
    for got, k in zip(grads, t["k"]):
        if got is None:
            continue
        assert got.shape == k.shape and got.dtype == torch.float32
        cmp = t["compared"]
        live = (k != 0) & cmp
        if not bool(live.any()):
            assert not bool((got[cmp] != 0).any()), (case.name, what)          # nothing active: every compared element is zero
            continue
        pos = int(torch.nonzero(live.reshape(-1))[0])
        c = got.reshape(-1)[pos] / k.reshape(-1)[pos]                          # a division by +-1 or +-2: exact
        if c_got is None:
            c_got = c
        assert torch.equal(c, c_got), (case.name, what, "one factor per call")
        assert torch.equal((got / c_got)[cmp], k[cmp]), (case.name, what)
    if c_got is not None:
        assert abs(float(c_got) - t["c64"]) <= 3 * U * abs(t["c64"]), (case.name, what, float(c_got), t["c64"])
    return c_got


# ------------------------------------------------------------------------------------------------------------------------------------------ cases
def _data(N, R, D, seed, scale=1.0):
    gen = torch.Generator().manual_seed(SEED + 104729 + seed)
    return tuple(scale * torch.randn(N, R, D, generator=gen) for _ in range(3))


def _case(name, N, R, D, pattern, rule, seed):
    a, p, n = _data(N, R, D, seed)
    pos, un = flags(pattern, N)
    c = Case(name, a, p, n, pos, un, rule, g=1.3 + 0.01 * (seed % 17))
    if pattern == "nan_unused":
        for b in np.nonzero(~c.truth()["used"])[0]:
            a[b], p[b], n[b] = float("nan"), float("nan"), float("nan")
    return c


def _order_case(rule):
    """Exact rows: eps = 0, a = n = 0, p = (-x, 0, 0, 0) -> d_ap = x, d_an = 0, loss = 1 + x, integers.  Three selected samples of one row; x_0 is
    the first value for which (S / denom) / 3 and (S / 3) / denom differ in fp32, so the division order of each rule shows in the bits."""
    d, three = np.float32(DENOM), np.float32(3)
    S = next(s for s in range(3, 4000) if (np.float32(s) / d) / three != (np.float32(s) / three) / d)
    a, p, n = torch.zeros(3, 1, 4), torch.zeros(3, 1, 4), torch.zeros(3, 1, 4)
    p[0, 0, 0] = -float(S - 3)
    return Case(f"order_exact_rule{rule}", a, p, n, np.ones(3), np.ones(3), rule, eps=0.0, g=1.0, exact=True)


def _build():
    cases = []
    for D in DS:                                                             # every shape, the patterns and rules rotating over them
        for N, R in SHAPES:
            i = len(cases)
            cases.append(_case(f"s_{N}x{R}x{D}_{PATTERNS[i % len(PATTERNS)]}_r{i % 2}", N, R, D, PATTERNS[i % len(PATTERNS)], i % 2, i))
    for N, R, D in ((3, 3, 65), (9, 3, 127), (5, 1, 129)):                   # every pattern under both rules
        for pattern in PATTERNS:
            for rule in (0, 1):
                cases.append(_case(f"f_{N}x{R}x{D}_{pattern}_r{rule}", N, R, D, pattern, rule, len(cases)))
    cases += [_order_case(0), _order_case(1)]
    return {c.name: c for c in cases}


CASES = _build()
NAMES = list(CASES)
ORDER_CASES = ("order_exact_rule0", "order_exact_rule1")
