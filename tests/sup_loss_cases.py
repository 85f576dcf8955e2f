"""The cases, the float64 truth, the bounds and the mutations that tests/test_sup_loss_host.py (CPU) and tests/test_gpu_sup_loss.py (GPU) share for the
supervised head losses of csrc/sup_losses.hip (hdn_sup_losses_f32, hdn_sup_losses_bwd_f32).  Nothing here touches the device.

The truth is a float64 restatement in torch (ref_a .. ref_e below, quirks included, gradients by autograd) of the five functions of the reference's
hdn/models/loss.py; tests/golden/sup_losses.npz pins it to the reference itself (captured by tests/golden/make_sup_loss_golden.py, which executes
loss.py in float64 on the inputs that CASES regenerates by seed).  `variant` names a mistake the tests must be able to see (MUTATIONS).

Bounds, for any summation order.  u = 2^-24.  A sum of N terms t_i, each evaluated with absolute error <= e_i, then divided:

    B = (sum e_i + (N + 2) u sum |t_i|) / den                      at most N - 1 roundings in the sum, one in the division, one spare

and a loss that adds two such terms gets u |loss| per further operation.  The e_i, from two roundings per term and the condition numbers:

    form 0 probabilities    rel_p = (|x0 - x1| + A + 3) u           x - max is exact for the larger logit and rounded for the other: the rounding
                                                                    u |x0 - x1| and expf's A u go through exp (condition |x0 - x1|, 1), then the
                                                                    sum, the division and one spare rounding.  Form 1: the input is exact, rel_p = 0.
    (a) positives           e = p1 rel_p + u |label - p1|
    (a) negatives           e = dp / (1 - p) + u + A u l,   dp = p rel_p inside the clamp, 0 where the clamp holds the value
                                                                    -log(1 - p) has condition p / (1 - p) against p: 1 - p is rounded once, logf's A u l.
                                                                    The sum of the k largest is 1-Lipschitz in the max norm of the perturbation, so the
                                                                    k largest e of all negatives are charged, whichever cells either side selects.
    (b), (d), (e)           e = 4 u max(t, |d|)                     d rounded; 0.5 d^2 three more roundings, |d| - 0.5 one more
    (c) form 0              e = u (2 |x0 - x1| + 2 A + 1 + |logp|)   x - max, exp twice (A u each, relative to a sum in [1, 2]), the sum, logf, the last subtraction
    (c) form 1              e = 0
    gradients, kernel       (a) form 1: 4 u |G|;  (a) form 0: |G| (6 u + 2 rel_p + dp / (1 - p));  (b), (d), (e): 4 u |G|;
                            (c) form 1: 3 u |G|;  (c) form 0: (|a_j| + p_j |a_0 + a_1|) (rel_p + 5 u), a_j the gradient against logp_j
                            each times GRAD_SLACK = 2: the counts are the kernel's roundings, and PyTorch's own autograd chain, which the bound has
                            to hold for as well, is about twice as long (it multiplies by the indicator masks, by 0.5 and 2 and by the upstream,
                            and softmax's backward forms p (g - sum g p), where the kernel multiplies p1 p0).

A, the allowance for expf / logf in ulps, cannot be derived from the project: it is set so that PyTorch's own fp32 CPU evaluation (loss and autograd)
uses at most half of any bound on every case - the factor 2 because GPU and CPU libm differ by a few ulp.  With A_LIBM = 4 the largest ratio this
CPU measured is R_REF (tests/test_sup_loss_host.py prints and checks it).

Input conditions (the generator enforces them, the host test checks them): no selected cell within its bound of a branch point - the clamp edges
(saturated cells have logit gaps of +-40: both sides clamp exactly; form 1 may sit exactly on an edge, which is exact), |d| = 1, label == 0,
max_c - 0.2 - and, where k_eff < n_neg, the k-th and (k+1)-th largest l differ by more than twice their bounds unless they tie exactly.  Cells whose
|label - p1| or ||d| - 1| is inside its bound are left out of the gradient comparison: at most EXCLUDED_CAP of a case's cells; zero with these seeds.

Shapes: the workgroup has T = 1024 threads; cell counts 1, 5, T - 1, T, T + 1, 2 T + 3; S in {1, 3, 5, 13, 25}, n in {1, 2, 3, 5}; the full
32 x 625 / 32 x 169 with 24 samples selected once; topk_per_sample 1, 3, 100 with k below, equal to and above n_neg; 0, 1 and 2 hits in every term;
exact ties at the top-k threshold; masks that select none, all and only the last sample; one NaN case.
"""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sup_losses.npz")
SEED = 20261021
U = 2.0 ** -24
T = 1024
A_LIBM = 4.0
R_REF = 0.37           # the largest (error of PyTorch fp32 on this CPU) / bound over all views, losses and gradients; the host test asserts <= 0.5
EXCLUDED_CAP = 0.01
GRAD_SLACK = 2.0
LO, HI = float(np.float32(0.000001)), float(np.float32(0.9999999))
KEYS = ("a", "b", "c", "d", "e")
GRAD_OF = {"a": "cls", "b": "loc", "c": "cls_lp", "d": "loc_lp", "e": "rows"}
UPSTREAM = (0.75, 1.25, 0.5, 1.5, 0.625)          # d L / d loss_i: exact in fp32
MUTATIONS = ("clamp_omitted", "k_not_k_plus_1", "ge_threshold", "one_hit_dropped", "ties_from_top", "n_sel_no_plus_1")
# not a mistake but the reference executed in float64, as the fixture was captured: there the clamp literals and max_c - 0.2 are doubles, while its
# fp32 run - what the kernel restates, and what every other evaluation here uses - rounds them to fp32 (a saturated cell's l is 15.94, not 16.12)
AS_FLOAT64 = "as_float64_reference"
GOLDEN_GRAD_CELLS = 200                           # gradients are stored in the fixture for cases of at most this many cells


# ------------------------------------------------------------------------------------------------------------------------------- the restatement
def smooth(d):
    ad = d.abs()
    return torch.where(ad < 1, 0.5 * d * d, ad - 0.5)


def _one(variant):
    """A term with at most this many hits is 0: the reference's nonzero().squeeze() makes one hit a 0-d tensor, which its emptiness test accepts."""
    return 0 if variant == "one_hit_dropped" else 1


def _plus(variant):
    return 0 if variant == "n_sel_no_plus_1" else 1


def topk_take(l, k, from_top=False):
    """Positions of the k largest of l (1-d numpy), NaN largest; ties: the lowest positions first (from_top: the highest)."""
    key = np.where(np.isnan(l), np.inf, l)
    idx = np.arange(len(l))
    return np.lexsort((-idx if from_top else idx, -key))[:k]


def ref_a(p, label, topk, variant=None):
    """select_xr_focal_fuse_smooth_l1_loss_top_k on p [n,S,S,2] (probabilities), label [n,S,S] -> (loss, internals)."""
    n = label.shape[0]
    p1, L = p.reshape(-1, 2)[:, 1], label.reshape(-1).to(p.dtype)
    pos, neg = (L > 0).nonzero().flatten(), (L == 0).nonzero().flatten()
    zero = torch.zeros((), dtype=p.dtype)
    info = {"pos": pos, "neg": neg, "take": neg[:0], "k": 0}
    pos_loss = zero if len(pos) <= _one(variant) else (L[pos] - p1[pos]).abs().sum() / (len(pos) + 1)
    neg_loss = zero
    if len(neg) > _one(variant):
        pn = p1[neg]
        lo, hi = (0.000001, 0.9999999) if variant == AS_FLOAT64 else (LO, HI)
        l = -torch.log(1 - (pn if variant == "clamp_omitted" else pn.clamp(lo, hi)))
        k = min(topk * n, len(neg))
        take = torch.from_numpy(topk_take(l.detach().double().numpy(), k, variant == "ties_from_top").copy())
        neg_loss = l[take].sum() / (k + (0 if variant == "k_not_k_plus_1" else 1))
        info.update(take=neg[take], k=k, l=l.detach())
    return pos_loss + neg_loss, info


def threshold_b(label):
    """max_c - 0.2 as the reference's fp32 run evaluates it (both operands and the difference in fp32); NaN if a label is NaN."""
    return float(np.float32(label.max().item()) - np.float32(0.2))


def ref_b(pred, tgt, label, variant=None):
    """select_l1_loss_c on pred, tgt [n,2,S,S], label [n,S,S]."""
    L = label.reshape(-1)
    if L.numel() == 0:
        return torch.zeros((), dtype=pred.dtype), L.nonzero().flatten()
    thr = float(L.max()) - 0.2 if variant == AS_FLOAT64 else threshold_b(L)
    pos = ((L >= thr) if variant == "ge_threshold" else (L > thr)).nonzero().flatten()
    if len(pos) <= _one(variant):
        return torch.zeros((), dtype=pred.dtype), pos[:0]
    pr, tg = (x.permute(0, 2, 3, 1).reshape(-1, 2)[pos] for x in (pred, tgt))
    return smooth(pr - tg).sum() / (2 * len(pos) + _plus(variant)), pos


def ref_c(logp, label, variant=None):
    """select_cross_entropy_loss on logp [n,S,S,2] (log-probabilities), label int64 [n,S,S]."""
    lp, L = logp.reshape(-1, 2), label.reshape(-1)
    terms = []
    for v in (1, 0):
        idx = (L == v).nonzero().flatten()
        terms.append(torch.zeros((), dtype=lp.dtype) if len(idx) <= _one(variant) else (-lp[idx, v]).mean())
    return terms[0] * 0.5 + terms[1] * 0.5


def ref_e(out, tgt, variant=None):
    """kalyo_l1_loss on rows [n,C]."""
    return smooth(out - tgt).sum() / (out.numel() + _plus(variant))


def ref_d(pred, tgt, label, variant=None):
    """select_l1_loss on pred, tgt [n,4,S,S], label [n,S,S]: the rows with label > 0 (no one-hit rule here)."""
    pos = (label.reshape(-1) > 0).nonzero().flatten()
    pr, tg = (x.permute(0, 2, 3, 1).reshape(-1, 4)[pos] for x in (pred, tgt))
    return ref_e(pr, tg, variant)


# ----------------------------------------------------------------------------------------------------------------------------------------- cases
class View:
    """One input form of one case: t = the tensors the entry points take (fp32 / int64, CPU), form, topk."""

    def __init__(self, case, form, t):
        self.case, self.form, self.t, self.topk, self.name = case, form, t, case.topk, f"{case.name}/form{form}"

    def selected(self):
        m = self.t.get("if_unsup")
        B = self.t["label_cls"].shape[0]
        return torch.arange(B) if m is None else (m == 0).nonzero().flatten()

    def evaluate(self, dtype=torch.float64, variant=None):
        """-> (losses [5] at dtype, grads {name: full-size gradient} for UPSTREAM, internals).  float64: the truth; float32: PyTorch's own fp32."""
        t, sel = self.t, self.selected()
        leaves = {k: t[k].detach().clone().to(dtype).requires_grad_(True) for k in ("cls", "loc", "cls_lp", "loc_lp", "rows")}
        g = lambda k: leaves[k][sel] if self.form == 0 else leaves[k]
        lab = lambda k: t[k][sel] if self.form == 0 else t[k]
        if self.form == 0:
            p, logp = F.softmax(g("cls").permute(0, 2, 3, 1), dim=3), F.log_softmax(g("cls_lp").permute(0, 2, 3, 1), dim=3)
        else:
            p, logp = g("cls"), g("cls_lp")
        la, info = ref_a(p, lab("label_cls").to(dtype), self.topk, variant)
        lb, pos_b = ref_b(g("loc"), lab("label_loc_c").to(dtype), lab("label_cls"), variant)
        lc = ref_c(logp, lab("label_cls_lp"), variant)
        ld = ref_d(g("loc_lp"), lab("label_loc_lp").to(dtype), lab("label_cls_lp"), variant)
        le = ref_e(leaves["rows"], t["rows_target"].to(dtype), variant)
        losses = torch.stack([la, lb, lc, ld, le])
        (losses * torch.tensor(UPSTREAM, dtype=dtype)).sum().backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in leaves.items()}
        info.update(p=p.detach(), logp=logp.detach(), pos_b=pos_b, sel=sel)
        return losses.detach(), grads, info

    @functools.lru_cache(maxsize=None)
    def truth(self):
        losses, grads, info = self.evaluate()
        lb, gb, compared, cond = bounds(self, losses, grads, info)
        return {"losses": losses, "grads": grads, "loss_bounds": lb, "grad_bounds": gb, "compared": compared, "info": info, "conditions": cond}


def _scatter(sel, B, x):
    """x [n, ...] of the gathered samples as [B, ...] with zeros elsewhere."""
    full = torch.zeros((B,) + tuple(x.shape[1:]), dtype=x.dtype)
    full[sel] = x
    return full


def bounds(view, losses, grads, info):
    """-> (loss bounds [5], {name: gradient bound, the gradient's shape}, {name: bool mask of the elements compared}, the input conditions found)."""
    t, form, sel = view.t, view.form, info["sel"]
    B = t["label_cls"].shape[0]
    take = (lambda x: x[sel]) if form == 0 else (lambda x: x)
    d64 = lambda k: take(t[k]).double()
    lb = torch.zeros(5, dtype=torch.float64)
    cond = {"branch_ok": True, "gap_ok": True}

    def summed(e, terms, den, n=None):
        n = len(terms) if n is None else n
        return float((e.sum() + (n + 2) * U * terms.abs().sum()) / den) if n else 0.0

    def full(x):                                     # gathered [n, ...] -> the gradient's full-size layout
        return _scatter(sel, B, x) if form == 0 else x

    # ---- (a)
    p1 = info["p"].double().reshape(-1, 2)[:, 1]
    p0 = info["p"].double().reshape(-1, 2)[:, 0]
    L = d64("label_cls").reshape(-1)
    if form == 0:
        x = d64("cls").permute(0, 2, 3, 1).reshape(-1, 2)
        rel_p = ((x[:, 0] - x[:, 1]).abs() + A_LIBM + 3) * U
    else:
        rel_p = torch.zeros_like(p1)
    pos, neg = info["pos"], info["neg"]
    e_pos = p1 * rel_p + U * (L - p1).abs()
    b_pos = summed(e_pos[pos], (L - p1)[pos], len(pos) + 1) if len(pos) > 1 else 0.0
    near_a = torch.zeros_like(p1, dtype=torch.bool)
    near_a[pos] = (L - p1)[pos].abs() <= e_pos[pos]
    inside = (p1 > LO) & (p1 < HI)
    pc = p1.clamp(LO, HI)
    dp = torch.where(inside, p1 * rel_p, torch.zeros_like(p1))
    lall = -torch.log(1 - pc)
    e_l = dp / (1 - pc) + U + A_LIBM * U * lall
    b_neg = 0.0
    k = info["k"]
    if k:
        worst = torch.sort(e_l[neg], descending=True).values[:k]
        b_neg = float((worst.sum() + (k + 3) * U * lall[info["take"]].sum()) / (k + 1))
        # a selected value within its bound of a clamp edge without being held by it (form 1 exactly on an edge is exact)
        edge = ((p1 - LO).abs() <= dp) | ((p1 - HI).abs() <= dp)
        cond["branch_ok"] &= not bool((edge[neg] & (rel_p[neg] > 0)).any())
        if k < len(neg):                             # the k-th against the (k+1)-th largest
            order = topk_take(lall[neg].numpy(), k + 1)
            i, j = neg[order[k - 1]], neg[order[k]]
            gap = float(lall[i] - lall[j])
            cond["gap_ok"] &= gap == 0.0 or gap > 2 * float(e_l[i] + e_l[j])
    lb[0] = b_pos + b_neg + U * abs(float(losses[0]))
    ga = grads["cls"].double()
    ga_flat = (take(ga).permute(0, 2, 3, 1) if form == 0 else ga).reshape(-1, 2)
    fac = (6 * U + 2 * rel_p + dp / (1 - pc)) if form == 0 else torch.full_like(p1, 4 * U)
    gb_a = ga_flat.abs() * fac.unsqueeze(1)
    n_s, S = len(sel) if form == 0 else B, t["label_cls"].shape[1]
    shape_a = (lambda v: full(v.reshape(n_s, S, S, 2).permute(0, 3, 1, 2))) if form == 0 else (lambda v: v.reshape(n_s, S, S, 2))
    cmp_a = shape_a((~near_a).unsqueeze(1).expand(-1, 2).clone())
    if form == 0:
        cmp_a[[b for b in range(B) if b not in set(sel.tolist())]] = True
    gbounds = {"cls": shape_a(gb_a)}
    compared = {"cls": cmp_a.bool()}

    # ---- (b), (d), (e)
    def smooth_bound(pred, tgt, den_n, rows):       # pred, tgt [rows', C] of the selected rows
        d = pred - tgt
        tt = smooth(d)
        return summed(4 * U * torch.maximum(tt, d.abs()).reshape(-1), tt.reshape(-1), den_n) if rows else 0.0

    def near_one(pred, tgt):
        d = (pred - tgt).abs()
        return (d - 1).abs() <= 2 * U * d

    pos_b = info["pos_b"]
    if len(pos_b):
        pr, tg = (d64(k).permute(0, 2, 3, 1).reshape(-1, 2)[pos_b] for k in ("loc", "label_loc_c"))
        lb[1] = smooth_bound(pr, tg, 2 * len(pos_b) + 1, len(pos_b))
    Lf = take(t["label_cls"]).reshape(-1)
    if Lf.numel() and not bool(torch.isnan(Lf).any()):
        thr = threshold_b(Lf)
        cond["branch_ok"] &= not bool(((Lf.double() - thr).abs() <= 4 * U * max(abs(thr), 0.2)).any()) or view.case.on_threshold
    pos_d = (take(t["label_cls_lp"]).reshape(-1) > 0).nonzero().flatten()
    pr, tg = (d64(k).permute(0, 2, 3, 1).reshape(-1, 4)[pos_d] for k in ("loc_lp", "label_loc_lp"))
    lb[3] = smooth_bound(pr, tg, 4 * len(pos_d) + 1, len(pos_d))
    lb[4] = smooth_bound(t["rows"].double(), t["rows_target"].double(), t["rows"].numel() + 1, t["rows"].numel())
    for name, tgt in (("loc", "label_loc_c"), ("loc_lp", "label_loc_lp"), ("rows", "rows_target")):
        gbounds[name] = 4 * U * grads[name].double().abs()
        compared[name] = ~(near_one(t[name].double(), t[tgt].double()) & (grads[name] != 0))

    # ---- (c)
    Lc = take(t["label_cls_lp"]).reshape(-1)
    lp = info["logp"].double().reshape(-1, 2)
    gc = grads["cls_lp"].double()
    if form == 0:
        xc = d64("cls_lp").permute(0, 2, 3, 1).reshape(-1, 2)
        gap = (xc[:, 0] - xc[:, 1]).abs()
        rel_c = (gap + A_LIBM + 3) * U
        tb = []
        for v in (1, 0):
            idx = (Lc == v).nonzero().flatten()
            e = U * (2 * gap[idx] + 2 * A_LIBM + 1 + lp[idx, v].abs())
            tb.append(summed(e, lp[idx, v], len(idx)) if len(idx) > 1 else 0.0)
        lb[2] = 0.5 * (tb[0] + tb[1]) + 3 * U * abs(float(losses[2]))
        # a_j from the counts; the bound in the gathered cell order, then the layout of the gradient
        a = torch.zeros_like(lp)
        for v in (1, 0):
            idx = (Lc == v).nonzero().flatten()
            if len(idx) > 1:
                a[idx, v] = -0.5 * UPSTREAM[2] / len(idx)
        pj = lp.exp()
        gb_c = (a.abs() + pj * a.sum(1, keepdim=True).abs()) * (rel_c + 5 * U).unsqueeze(1)
        Sl = t["label_cls_lp"].shape[1]
        gbounds["cls_lp"] = full(gb_c.reshape(len(sel), Sl, Sl, 2).permute(0, 3, 1, 2))
    else:
        tb = []
        for v in (1, 0):
            idx = (Lc == v).nonzero().flatten()
            tb.append(summed(torch.zeros(len(idx), dtype=torch.float64), lp[idx, v], len(idx)) if len(idx) > 1 else 0.0)
        lb[2] = 0.5 * (tb[0] + tb[1]) + 3 * U * abs(float(losses[2]))
        gbounds["cls_lp"] = 3 * U * gc.abs()
    compared["cls_lp"] = torch.ones_like(gc, dtype=torch.bool)
    return lb, {k: GRAD_SLACK * v for k, v in gbounds.items()}, compared, cond


class Case:
    """Form-0 data (raw maps [B,...], labels, mask) of one case; views() derives form 1: the gathered samples, softmaxed in float64 and rounded to
    fp32 (then the fp32 probabilities are the input, and the truth of form 1 is computed from them)."""

    def __init__(self, name, t, topk, on_threshold=False, golden=True, ties=False, nan=False):
        self.name, self.t, self.topk, self.on_threshold, self.golden, self.ties, self.nan = name, t, topk, on_threshold, golden, ties, nan
        self.B, self.S, self.S_lp = t["label_cls"].shape[0], t["label_cls"].shape[1], t["label_cls_lp"].shape[1]
        self.cells = self.B * self.S * self.S

    @functools.lru_cache(maxsize=None)
    def views(self):
        t = self.t
        v0 = View(self, 0, t)
        sel = v0.selected()
        if len(sel) == 0:
            return (v0,)
        f1 = {k: t[k][sel].clone() for k in ("loc", "label_loc_c", "loc_lp", "label_loc_lp", "label_cls", "label_cls_lp")}
        f1["cls"] = F.softmax(t["cls"][sel].double().permute(0, 2, 3, 1), dim=3).float().contiguous()
        f1["cls_lp"] = F.log_softmax(t["cls_lp"][sel].double().permute(0, 2, 3, 1), dim=3).float().contiguous()
        f1["rows"], f1["rows_target"] = t["rows"], t["rows_target"]
        return (v0, View(self, 1, f1))


def _away_from_one(pred, tgt):
    """|pred - tgt| within 1e-4 of 1: make the difference 0 (far from the branch)."""
    near = ((pred - tgt).abs() - 1).abs() < 1e-4
    pred[near] = tgt[near]


def make(name, B, S, S_lp=None, mask=None, topk=100, seed=0, hits=None, ties=0, nan=False, on_threshold=False, p_zero=0.6, golden=True):
    """N(0, 2) logits with saturated cells (gaps of +-40) among the negatives, N(0, 1.5) locations, labels: float {0, U(0.3, 1), -1} and int64
    {-1, 0, 1}.  hits = h: exactly h cells in every term ((a) positives, (a) negatives, (b), both terms of (c), (d))."""
    S_lp = S if S_lp is None else S_lp
    gen = torch.Generator().manual_seed(SEED + seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    ru = lambda *s: torch.rand(*s, generator=gen)
    t = {"cls": 2 * rn(B, 2, S, S), "loc": 1.5 * rn(B, 2, S, S), "label_loc_c": 1.5 * rn(B, 2, S, S), "cls_lp": 2 * rn(B, 2, S_lp, S_lp),
         "loc_lp": 1.5 * rn(B, 4, S_lp, S_lp), "label_loc_lp": 1.5 * rn(B, 4, S_lp, S_lp), "rows": 1.5 * rn(B, 8), "rows_target": 1.5 * rn(B, 8)}
    r, val = ru(B, S, S), 0.3 + 0.7 * ru(B, S, S)
    label = torch.where(r < p_zero, torch.zeros(()), torch.where(r < 0.9, val, -torch.ones(())))
    r2 = ru(B, S_lp, S_lp)
    label_lp = torch.where(r2 < 0.5, 0, torch.where(r2 < 0.8, 1, -1)).long()
    if hits is not None:                             # exactly `hits` cells per term, in the last sample (the one a mask may select alone)
        label = -torch.ones(B, S, S)
        label_lp = -torch.ones(B, S_lp, S_lp, dtype=torch.long)
        fl, fl_lp = label[B - 1].view(-1), label_lp[B - 1].view(-1)
        assert 2 * hits <= fl.numel() and 2 * hits <= fl_lp.numel()
        fl[:hits], fl[hits:2 * hits] = 1.0, 0.0
        fl_lp[:hits], fl_lp[hits:2 * hits] = 1, 0
    # saturated negatives: the first two zeros get gaps of +40 and -40
    zeros = (label.view(-1) == 0).nonzero().flatten()
    cl = t["cls"].permute(0, 2, 3, 1).reshape(-1, 2).clone()
    for q, gapv in zip(zeros[:2].tolist(), (40.0, -40.0)):
        cl[q, 0], cl[q, 1] = 0.0, gapv
    for j in range(ties):                            # exact ties: cells that share one logit pair (the 3rd .. (2 + ties)th zero)
        if 2 + j < len(zeros):
            cl[zeros[2 + j], 0], cl[zeros[2 + j], 1] = -3.0, 4.0
    t["cls"] = cl.reshape(B, S, S, 2).permute(0, 3, 1, 2).contiguous()
    if on_threshold:                                 # a cell exactly on fl32(max_c - 0.2f): 1.0 and 0.8f
        fl = label.view(-1)
        fl[-1], fl[-2], fl[-3] = 1.0, float(np.float32(0.8)), 0.9
    else:                                            # labels within 1e-3 of max_c - 0.2 become 0.5 below it
        thr = float(label.max()) - 0.2
        label[(label - thr).abs() < 1e-3] = max(thr - 0.05, 0.05) if thr > 0.1 else -1.0
    _away_from_one(t["loc"], t["label_loc_c"])
    _away_from_one(t["loc_lp"], t["label_loc_lp"])
    _away_from_one(t["rows"], t["rows_target"])
    if nan:
        t["cls"][B - 1, 1, 0, 0] = float("nan")
        t["loc"][B - 1, 0, 0, 0] = float("nan")
        t["cls_lp"][B - 1, 0, 0, 0] = float("nan")
        t["loc_lp"][B - 1, 2, 0, 0] = float("nan")
        t["rows"][0, 0] = float("nan")
        label[B - 1, 0, 0], label_lp[B - 1, 0, 0] = 1.0, 1
        label[B - 1].view(-1)[1:3] = 1.0
    t["label_cls"], t["label_cls_lp"] = label, label_lp
    if mask is not None:
        t["if_unsup"] = torch.tensor(mask, dtype=torch.float32)
    return Case(name, t, topk, on_threshold=on_threshold, golden=golden and not on_threshold, ties=bool(ties), nan=nan)


def _build():
    cases, s = [], [0]

    def add(*a, **k):
        s[0] += 1
        cases.append(make(*a, seed=s[0], **k))

    add("cells_1", 1, 1, topk=1)
    add("cells_5", 5, 1, topk=1)
    add("cells_T-1", T - 1, 1, topk=1)
    add("cells_T", 1, 32, topk=100)
    add("cells_T_n4", 4, 16, topk=3)
    add("cells_T+1", 41, 5, topk=3)
    add("cells_2T+3", 2 * T + 3, 1, topk=1)
    add("n1_S3", 1, 3, topk=3)
    add("n2_S5", 2, 5, topk=3)
    add("n3_S13", 3, 13, topk=100)
    add("n5_S25", 5, 25, S_lp=13, topk=100)
    add("n2_S25_k1", 2, 25, S_lp=13, topk=1)
    add("full_32_mask24", 32, 25, S_lp=13, topk=100, mask=[1.0 if i % 4 == 1 else 0.0 for i in range(32)])
    for h in (0, 1, 2):
        add(f"hits_{h}", 2, 3, topk=3, hits=h)
    add("k_equal_n_neg", 2, 3, topk=1, hits=2)                      # k = 2 = n_neg
    add("k_above_n_neg", 2, 3, topk=3, hits=2)                      # k = 6 > n_neg = 2
    add("ties_k_inside", 2, 5, topk=2, ties=5)                      # k = 4: two saturated-or-larger cells, then a tie group of 5 cut by k
    add("ties_k_inside_T", 41, 5, topk=1, ties=60)
    add("mask_none", 3, 5, topk=3, mask=[1.0, 2.0, 1.0])
    add("mask_all", 3, 5, topk=3, mask=[0.0, 0.0, 0.0])
    add("mask_last", 3, 5, topk=3, mask=[1.0, 1.0, 0.0])
    add("mask_last_hits_1", 3, 3, topk=3, mask=[1.0, 1.0, 0.0], hits=1)
    add("negative_labels", 2, 5, topk=3, p_zero=0.0)
    add("on_threshold", 2, 5, topk=3, on_threshold=True)
    add("nan", 2, 5, topk=3, nan=True)
    return {c.name: c for c in cases}


CASES = _build()
NAMES = list(CASES)
VIEWS = {v.name: v for c in CASES.values() for v in c.views()}
VIEW_NAMES = list(VIEWS)

# the case that shows each mutation (a view name); the host test asserts that the mutated restatement leaves the bound there
MUTATION_CASES = {"clamp_omitted": "n2_S5/form0", "k_not_k_plus_1": "n2_S5/form1", "ge_threshold": "on_threshold/form1",
                  "one_hit_dropped": "hits_1/form1", "ties_from_top": "ties_k_inside/form1", "n_sel_no_plus_1": "n2_S5/form1"}


def check(got_losses, got_grads, view, what=""):
    """Assert losses [5] and gradients {name: tensor} (any subset) against the truth of `view`; -> the largest error / bound seen."""
    tr = view.truth()
    worst = 0.0
    want, bound = tr["losses"], tr["loss_bounds"]
    got = got_losses.detach().cpu().double()
    for i, key in enumerate(KEYS):
        if torch.isnan(want[i]):
            assert torch.isnan(got[i]), (what, view.name, key, float(got[i]))
            continue
        err = abs(float(got[i] - want[i]))
        print(f"SUP {what} {view.name} loss {key}: got {float(got[i]):.9g} want {float(want[i]):.9g} err {err:.3e} bound {float(bound[i]):.3e}")
        assert err <= float(bound[i]), (what, view.name, key, float(got[i]), float(want[i]), err, float(bound[i]))
        if bound[i] > 0:
            worst = max(worst, err / float(bound[i]))
    for name, g in (got_grads or {}).items():
        if g is None:
            continue
        key = [k for k, v in GRAD_OF.items() if v == name][0]
        if torch.isnan(want[KEYS.index(key)]):
            continue
        g = g.detach().cpu().double()
        w, b, m = tr["grads"][name].double(), tr["grad_bounds"][name], tr["compared"][name]
        assert g.shape == w.shape, (what, view.name, name, g.shape, w.shape)
        err = (g - w).abs()
        ok = (err <= b) | ~m
        ratio = float((err[m & (b > 0)] / b[m & (b > 0)]).max()) if bool((m & (b > 0)).any()) else 0.0
        print(f"SUP {what} {view.name} grad {name}: worst err / bound {ratio:.3f}; left out {int((~m).sum())} of {m.numel()}")
        assert bool(ok.all()), (what, view.name, name, float(err[~ok].max()), int((~ok).sum()))
        worst = max(worst, ratio)
    return worst
