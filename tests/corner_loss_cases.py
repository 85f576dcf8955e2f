"""Fixtures, restatements and bounds for csrc/corner_losses.hip (tests/test_corner_loss_host.py, tests/test_gpu_corner_loss.py).  No device.

The lines under test are hdn/models/model_builder_e2e_unconstrained_v2.py:441-444 (corner_error_simi), :481-523 (the corner errors and the two
kalyo_l1_loss terms) and the gating of :552-556.  They are restated ONCE (Case.evaluate), as functions of an arithmetic `A`, and read as

    NPA(np.float32)     every operation individually rounded (the simulated wrong kernels are variants of this reading)
    NPA(np.float64)     the truth of the forward
    TA(dtype, device)   PyTorch's own run (fp32 on the CPU: r_ref; fp32 on the device: PyTorch-ROCm; float64 with autograd: the truth of the gradients)
    QA()                float64 values that carry a first-order running error bound (Qv of tests/simi_geometry_cases.py): each fp32 operation adds
                        u |result| (u = 2^-24), each division DIV_ROUNDINGS u |result|, a sum of N terms (N - 1) u sum |terms| (any order), and the
                        errors of the operands are carried through by the operation's derivative.

H_gt enters QA as the float64 solution with ONE fp32 rounding: the kernel solves in float64, so nothing is charged for the elimination.  What is
charged is what reaches the system: off = pred_points_xy / pred_points_w - template_poly and dst = src + off are fp32 operations, and their errors
pass through the solve by its derivative d h / d u = A^-1 (e_row (1 + x h6 + y h7)); in the backward the same perturbation moves the adjoint
solution (d lambda = A^-T (x, y of the perturbed row at columns 6, 7) lambda_row du).

DIV_ROUNDINGS is not guessed: it is the smallest integer for which PyTorch's fp32 run on the CPU stays within half the bound on every case, over the
terms that do not pass the solve (slots 0, 1, 2, 4 and their gradients); test_corner_loss_host.py measures that ratio (R_REF) and asserts it.
PyTorch's fp32 inverse is up to 1.4e-4 off on general quads (docs/PARITY.md), so for slot 3 and the gradients through H_gt its ratio is recorded
(R_REF_SOLVE), not asserted; the kernel is held to the full bound against float64 everywhere.
"""
import os

import numpy as np
import torch

from simi_geometry_cases import U, Qv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "corner_losses.npz")

DIV_ROUNDINGS = 1             # roundings charged per division: the smallest count with r_ref <= 0.5
R_REF = 0.459                 # the worst ratio of PyTorch's CPU fp32 run to the bound over the terms that do not pass the solve, as measured
R_REF_SOLVE = 162.0           # the same over slot 3, slot 5 and the gradients through H_gt (torch.inverse in fp32): recorded, not asserted
MARGIN = 16                   # every |d| stays this many forward bounds away from 1, every corner difference from 0
GOLDEN_MAX_B = 65             # cases up to this batch size are in the fixture

KEYS = ("cor_err", "cor_err_aug", "cor_err_sim", "cor_pos_loss", "cor_neg_loss", "cor_loss")
SETS = ("sup", "sup_pos", "sup_neg", "unsup", "unsup_pos", "neg")
GRADS = ("grad_H_mat", "grad_pred_points", "grad_aug_sear_points", "grad_x")
SQUARE = np.array([[0, 0], [0, 127], [127, 127], [127, 0]], dtype=np.float64)
NO_SOLVE = np.array([1, 1, 1, 0, 1, 0], dtype=np.float32)        # the weights of the slots that do not pass the solve

MUTATIONS = ("neg_loss_over_sup_neg_only", "tsz_without_plus_1", "slot2_divided_by_w", "two_search_corners_swapped",
             "slot4_reported_without_sup_neg", "slot0_divided_by_n_neg", "dlt_point_swap_omitted", "h_gt_applied_as_inverse",
             "w_row_gradient_dropped", "off_from_unnormalised_points")


def set_ids(if_pos, if_unsup):
    """the six index sets from fp32 flags, by the reference's predicates (float comparisons with 0 and 1; NaN, 0.5 and 2 fail them)"""
    pos, un = np.asarray(if_pos, dtype=np.float32), np.asarray(if_unsup, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        m = {"sup": un == 0, "sup_pos": (un == 0) & (pos == 1), "sup_neg": (un == 0) & (pos == 0), "unsup": un == 1,
             "unsup_pos": (pos * un) == 1, "neg": pos == 0}
    return {k: np.nonzero(v)[0] for k, v in m.items()}


# ------------------------------------------------------------------------------------------------------------------ the DLT, float64 core
def dlt_system(src, u):
    """src, u = src + off: [n,4,2] float64 -> A [n,8,8], b [n,8]; row 2 p + c of point p (the kernel orders the points 0, 1, 3, 2: the same system)"""
    n = src.shape[0]
    A, b = np.zeros((n, 8, 8)), np.zeros((n, 8))
    for p in range(4):
        x, y = src[:, p, 0], src[:, p, 1]
        for c in range(2):
            r, d = 2 * p + c, u[:, p, c]
            A[:, r, 3 * c], A[:, r, 3 * c + 1], A[:, r, 3 * c + 2] = x, y, 1.0
            A[:, r, 6], A[:, r, 7], b[:, r] = -d * x, -d * y, d
    return A, b


class Solve:
    """h = A^-1 b of a batch with what the bounds and the adjoint need: M = A^-1, s[e] = 1 + x_p h6 + y_p h7 of row e = 2 p + c"""

    def __init__(self, src, u):
        self.src = src
        A, b = dlt_system(src, u)
        self.M = np.linalg.inv(A)
        self.h = np.linalg.solve(A, b[:, :, None])[:, :, 0]
        self.xr, self.yr = np.repeat(src[:, :, 0], 2, 1), np.repeat(src[:, :, 1], 2, 1)                 # x_p, y_p of row e
        self.s = 1.0 + self.xr * self.h[:, 6:7] + self.yr * self.h[:, 7:8]
        self.J = self.M * self.s[:, None, :]                                                             # d h / d u

    def adjoint(self, g):
        """grad_h [n,8] -> (lambda, grad_off [n,8])"""
        lam = np.einsum("nrk,nr->nk", self.M, g)
        return lam, lam * self.s


def solve8_np(rows):
    """csrc/geometry.h solve8 restated in numpy float64 for ONE 8 x 9 system: Gauss-Jordan, partial pivoting with ties to the lowest row, the update
    a[j] - f prow[j] (the kernel's fma differs from it only where a product is inexact)."""
    a = np.array(rows, dtype=np.float64)
    for k in range(8):
        piv = k + int(np.argmax(np.abs(a[k:, k])))
        a[[k, piv]] = a[[piv, k]]
        for r in range(8):
            if r != k:
                f = a[r, k] / a[k, k]
                a[r, k:] = a[r, k:] - f * a[k, k:]
    return a[:, 8] / np.diag(a[:, :8])


def kernel_rows(src, off):
    """the 8 x 9 system of dlt_row in the kernel's row order (points 0, 1, 3, 2), from fp32 src, off [4,2]"""
    rows = []
    for q in range(4):
        p = (0, 1, 3, 2)[q]
        x, y = float(src[p, 0]), float(src[p, 1])
        uv = (np.float32(src[p, 0]) + np.float32(off[p, 0]), np.float32(src[p, 1]) + np.float32(off[p, 1]))
        rows.append([x, y, 1, 0, 0, 0, -float(uv[0]) * x, -float(uv[0]) * y, float(uv[0])])
        rows.append([0, 0, 0, x, y, 1, -float(uv[1]) * x, -float(uv[1]) * y, float(uv[1])])
    return rows


# ------------------------------------------------------------------------------------------------------------------------------- arithmetics
class NPA:
    """numpy arrays of one dtype: every operator rounds once; the solve is float64 on the dtype's operands, rounded to the dtype once"""
    closed_form = True

    def __init__(self, dtype):
        self.dtype = dtype

    def inp(self, x):
        return np.asarray(x, dtype=self.dtype)

    def const(self, v):
        return self.dtype(v)

    def div(self, a, b):
        return a / b

    abs, sign = staticmethod(np.abs), staticmethod(np.sign)

    def total(self, terms):
        return np.stack(terms).sum(dtype=self.dtype)

    def kalyo(self, d):
        a = np.abs(d)
        quad = a < 1
        return np.where(quad, self.dtype(0.5) * (d * d), a - self.dtype(0.5)), np.where(quad, d, np.sign(d))

    def dlt(self, src, off):
        """src: [n,4,2] input array; off: list [p][c] of vectors -> (h: list of 8 vectors, solve)"""
        o = np.stack([np.stack(r, -1) for r in off], 1)
        u = (self.inp(src) + o).astype(np.float64)                    # dst = src + off in the dtype
        sv = Solve(np.asarray(src, dtype=np.float64), u)
        return [sv.h[:, k].astype(self.dtype) for k in range(8)], sv

    def dlt_adjoint(self, sv, g):
        _, goff = sv.adjoint(np.stack(g, -1).astype(np.float64))
        return [[goff[:, 2 * p + c].astype(self.dtype) for c in range(2)] for p in range(4)]

    def scatter(self, B, ids, comps, shape):
        out = np.zeros((B, int(np.prod(shape))), dtype=self.dtype)
        if len(ids):
            out[ids] = np.stack([np.broadcast_to(np.asarray(v, dtype=self.dtype), (len(ids),)) for v in comps], -1)
        return out.reshape(B, *shape)

    def add_full(self, a, b):
        return a + b

    def zero(self):
        return self.dtype(0)


class TA:
    """torch tensors; constants stay Python numbers.  The solve is torch.inverse(A) @ b in the dtype, as the reference's DLT_solve forms it."""
    closed_form = False

    def __init__(self, dtype, device="cpu"):
        self.dtype, self.device = dtype, device

    def inp(self, x):
        return x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), dtype=self.dtype, device=self.device)

    def const(self, v):
        return float(v)

    def div(self, a, b):
        return a / b

    abs, sign = staticmethod(torch.abs), staticmethod(torch.sign)

    def total(self, terms):
        return torch.stack(terms).sum()

    def kalyo(self, d):                                                   # loss.py:201 written out; the slope comes from autograd
        a = torch.abs(d)
        inds = a.lt(1).to(d.dtype)
        return inds * (0.5 * d ** 2) + (1 - inds) * (a - 0.5), None

    def dlt(self, src, off):
        o = torch.stack([torch.stack(r, -1) for r in off], 1)
        s = self.inp(src)
        u = s + o
        n = s.shape[0]
        one, zero = torch.ones(n, dtype=self.dtype, device=self.device), torch.zeros(n, dtype=self.dtype, device=self.device)
        rows, b = [], []
        for p in range(4):
            x, y = s[:, p, 0], s[:, p, 1]
            for c in range(2):
                d = u[:, p, c]
                xy1 = [x, y, one]
                rows.append(torch.stack((xy1 + [zero] * 3 if c == 0 else [zero] * 3 + xy1) + [-d * x, -d * y], -1))
                b.append(d)
        h = torch.matmul(torch.inverse(torch.stack(rows, 1)), torch.stack(b, -1).unsqueeze(-1))[:, :, 0]
        return [h[:, k] for k in range(8)], None

    def zero(self):
        return torch.zeros((), dtype=self.dtype, device=self.device)


class QA:
    closed_form = True

    def inp(self, x):
        return Qv(x)

    def const(self, v):
        return Qv(v, 0.0 if float(np.float32(v)) == float(v) else U * abs(v))

    def div(self, a, b):
        a, b = Qv.of(a), Qv.of(b)
        v = a.v / b.v
        return Qv(v, a.e / np.abs(b.v) + np.abs(v) * b.e / np.abs(b.v) + DIV_ROUNDINGS * U * np.abs(v))

    def abs(self, a):
        return Qv(np.abs(a.v), a.e)

    def sign(self, a):                                                     # a constant of the fp32 run too: the cases keep |a| >= MARGIN a.e
        return Qv(np.sign(a.v))

    def total(self, terms):
        v = np.stack([t.v for t in terms])
        return Qv(v.sum(), np.stack([t.e for t in terms]).sum() + (v.size - 1) * U * np.abs(v).sum())

    def kalyo(self, d):
        quad = np.abs(d.v) < 1                                             # the fp32 run takes the same branch: |d| is MARGIN bounds away from 1
        a = self.abs(d)
        q, l = Qv(0.5) * (d * d), a - Qv(0.5)
        return Qv(np.where(quad, q.v, l.v), np.where(quad, q.e, l.e)), Qv(np.where(quad, d.v, np.sign(d.v)), np.where(quad, d.e, 0.0))

    def dlt(self, src, off):
        ov = np.stack([np.stack([c.v for c in r], -1) for r in off], 1)
        oe = np.stack([np.stack([c.e for c in r], -1) for r in off], 1)
        s = np.asarray(src, dtype=np.float64)
        u = s + ov
        sv = Solve(s, u)
        sv.e_u = (oe + U * np.abs(u)).reshape(-1, 8)                          # off's own error and the fp32 add src + off
        sv.e_h = np.einsum("nke,ne->nk", np.abs(sv.J), sv.e_u)               # before the rounding: the backward uses the float64 h
        return [Qv(sv.h[:, k], sv.e_h[:, k] + U * np.abs(sv.h[:, k])) for k in range(8)], sv

    def dlt_adjoint(self, sv, g):
        gv, ge = np.stack([c.v for c in g], -1), np.stack([c.e for c in g], -1)
        lam, goff = sv.adjoint(gv)
        e_lam = np.einsum("nrk,nr->nk", np.abs(sv.M), ge)
        # the perturbed system: d lambda_r = sum_e (M[6,r] x_e + M[7,r] y_e) lambda_e du_e
        w = np.abs(sv.M[:, 6, :, None] * sv.xr[:, None, :] + sv.M[:, 7, :, None] * sv.yr[:, None, :])    # [n, r, e]
        e_lam = e_lam + np.einsum("nre,ne->nr", w, np.abs(lam) * sv.e_u)
        e = np.abs(sv.s) * e_lam + np.abs(lam) * (np.abs(sv.xr) * sv.e_h[:, 6:7] + np.abs(sv.yr) * sv.e_h[:, 7:8]) + U * np.abs(goff)
        return [[Qv(goff[:, 2 * p + c], e[:, 2 * p + c]) for c in range(2)] for p in range(4)]

    def scatter(self, B, ids, comps, shape):
        v, e = np.zeros((B, int(np.prod(shape)))), np.zeros((B, int(np.prod(shape))))
        if len(ids):
            comps = [Qv.of(c) for c in comps]
            v[ids] = np.stack([np.broadcast_to(c.v, (len(ids),)) for c in comps], -1)
            e[ids] = np.stack([np.broadcast_to(c.e, (len(ids),)) for c in comps], -1)
        return Qv(v.reshape(B, *shape), e.reshape(B, *shape))

    def add_full(self, a, b):                                              # rows of disjoint sample sets: no rounding
        return Qv(a.v + b.v, a.e + b.e)

    def zero(self):
        return Qv(0.0)


def _sum(terms):
    s = terms[0]
    for t in terms[1:]:
        s = s + t
    return s


# ----------------------------------------------------------------------------------------------------------------------------------- cases
def _quads(g, B):
    """[B,4,2] quads inside 127 x 127 in the corner order of SQUARE, each corner in its own quadrant: sides >= 47 px"""
    lo = g.uniform(5, 40, (B, 4, 2))
    far = SQUARE[None] > 0
    return np.where(far, 127.0 - lo, lo)


class Case:
    """One batch, float32, made from a seed.  flags: "mix" or an explicit (if_pos, if_unsup) pair; family "w1": pred_points w = 1, "w": w in [0.5, 2]"""

    def __init__(self, name, B, seed, flags="mix", family="w1", bounded=True):
        self.name, self.B, self.family, self.bounded = name, B, family, bounded
        for attempt in range(64):
            self._draw(B, seed + 1000 * attempt, flags)
            if not bounded or self.margin_ok():
                break
        else:
            raise AssertionError(f"{name}: no seed keeps the kinks {MARGIN} bounds away")
        self.seed = seed + 1000 * attempt

    def _draw(self, B, seed, flags):
        self._truth = None
        g = np.random.default_rng(seed)
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        if isinstance(flags, str):
            self.if_pos = f(g.uniform(0, 1, B) < 0.8)
            self.if_unsup = f(g.uniform(0, 1, B) < 0.3)
        else:
            self.if_pos, self.if_unsup = f(flags[0]), f(flags[1])
        self.ids = set_ids(self.if_pos, self.if_unsup)
        tp = _quads(g, B)
        self.template_poly = f(tp)
        w = g.uniform(0.5, 2.0, (B, 4)) if self.family == "w" else np.ones((B, 4))
        xy = (tp + g.uniform(-16, 16, (B, 4, 2))) * w[:, :, None]
        self.pred_points = f(np.concatenate([xy.transpose(0, 2, 1), w[:, None, :]], 1))
        self.aug_sear_points = f(np.concatenate([(tp + g.uniform(-16, 16, (B, 4, 2))).transpose(0, 2, 1), np.ones((B, 1, 4))], 1))
        H = np.tile(np.eye(3), (B, 1, 1))
        H[:, :2, :2] += g.uniform(-0.05, 0.05, (B, 2, 2))
        H[:, :2, 2] += g.uniform(-4, 4, (B, 2))
        H[:, 2, :2] += g.uniform(-1e-3, 1e-3, (B, 2))
        H[:, 2, 2] += g.uniform(-0.01, 0.01, B)
        self.H_mat = f(H)
        self.w = f(g.uniform(0.5, 1.5, 6) * g.choice([-1.0, 1.0], 6))                      # grad_out
        # d = target - x from both branches of the loss, |d| in [0, 0.9] or [1.1, 2.5]: x = delta (float64) - d for the sup_pos samples, -d elsewhere
        d = np.where(g.uniform(0, 1, (B, 8)) < 0.4, g.uniform(0, 0.9, (B, 8)), g.uniform(1.1, 2.5, (B, 8))) * g.choice([-1.0, 1.0], (B, 8))
        x = -d
        sp = self.ids["sup_pos"]
        if len(sp):
            x[sp] += self._delta64(sp)
        self.x = f(x)

    def _delta64(self, sp):
        pp, tp = self.pred_points[sp].astype(np.float64), self.template_poly[sp].astype(np.float64)
        off = (pp[:, :2] / pp[:, 2:3]).transpose(0, 2, 1) - tp
        h = np.concatenate([Solve(tp, tp + off).h, np.ones((len(sp), 1))], 1).reshape(-1, 3, 3)
        Q = np.einsum("nrk,kj->nrj", h, np.concatenate([SQUARE.T, np.ones((1, 4))]))
        return ((Q[:, :2] / Q[:, 2:3]).transpose(0, 2, 1) - SQUARE[None]).reshape(-1, 8)

    def arrays(self):
        return {k: getattr(self, k) for k in ("H_mat", "pred_points", "aug_sear_points", "template_poly", "x", "if_pos", "if_unsup")}

    # -- the forward and the closed-form backward in one arithmetic; `variant` simulates a wrong kernel (NPA only)
    def evaluate(self, A, variant=None, weights=None, leaves=None):
        """-> {the six KEYS, "counts", and for an arithmetic with a closed form the four GRADS for grad_out = weights (default: self.w); "margins":
        the values whose sign decides a branch (corner differences, |d| - 1), for the condition of the bounded cases}.  leaves: TA only, the input tensors to use."""
        B, ids = self.B, self.ids
        src = leaves or self.arrays()
        H, pp, aug, tp, x = (A.inp(src[k]) for k in ("H_mat", "pred_points", "aug_sear_points", "template_poly", "x"))
        sp, up = ids["sup_pos"], ids["unsup_pos"]
        ng = ids["sup_neg"] if variant == "neg_loss_over_sup_neg_only" else ids["neg"]
        n_sp, n_sn, n_up, n_ng = len(sp), len(ids["sup_neg"]), len(up), len(ng)
        sq = SQUARE.copy()
        if variant == "two_search_corners_swapped":
            sq[[1, 3]] = sq[[3, 1]]
        out = {"counts": np.array([len(ids[k]) for k in SETS], dtype=np.int32), "margins": []}
        g = A.inp(self.w if weights is None else weights)
        zero = A.zero()
        plus1 = 0 if variant == "tsz_without_plus_1" else 1
        cf = A.closed_form
        gH = gpp = gaug = gx = None
        R4, R2 = range(4), range(2)

        def signed(v):
            out["margins"].append(v)
            return A.sign(v)

        # ---- the supervised positives: slots 0, 1, 3
        out.update(cor_err=zero, cor_err_aug=zero, cor_pos_loss=zero)
        if n_sp:
            Hs, P, T, X, G = H[sp], pp[sp], tp[sp], x[sp], aug[sp]
            pk = [[P[:, k, j] for j in R4] for k in range(3)]                                     # pk[k][j]: row k (x, y, w) of corner j
            Pw = [(Hs[:, 2, 0] * pk[0][j] + Hs[:, 2, 1] * pk[1][j]) + Hs[:, 2, 2] * pk[2][j] for j in R4]
            cor = [[A.div((Hs[:, c, 0] * pk[0][j] + Hs[:, c, 1] * pk[1][j]) + Hs[:, c, 2] * pk[2][j], Pw[j]) for c in R2] for j in R4]
            e0 = [[cor[j][c] - T[:, j, c] for c in R2] for j in R4]
            e1 = [[G[:, c, j] - T[:, j, c] for c in R2] for j in R4]
            den0 = A.const(n_ng if variant == "slot0_divided_by_n_neg" else n_sp)
            out["cor_err"] = A.div(A.div(A.total([A.abs(e0[j][c]) for j in R4 for c in R2]), den0), A.const(4))
            out["cor_err_aug"] = A.div(A.div(A.total([A.abs(e1[j][c]) for j in R4 for c in R2]), A.const(n_sp)), A.const(4))
            if variant == "off_from_unnormalised_points":
                homo = [[pk[c][j] for c in R2] for j in R4]
            else:
                homo = [[A.div(pk[c][j], pk[2][j]) for c in R2] for j in R4]
            off = [[homo[j][c] - T[:, j, c] for c in R2] for j in R4]
            h, sv = A.dlt(self.template_poly[sp], off)
            if variant == "h_gt_applied_as_inverse":
                full = np.concatenate([np.stack(h, -1).astype(np.float64), np.ones((n_sp, 1))], 1).reshape(-1, 3, 3)
                inv = np.linalg.inv(full)
                h = [A.inp((inv / inv[:, 2:3, 2:3]).reshape(-1, 9)[:, k]) for k in range(8)]
            Qw = [(h[6] * A.const(sq[j, 0]) + h[7] * A.const(sq[j, 1])) + A.const(1) for j in R4]
            q = [[A.div((h[3 * c] * A.const(sq[j, 0]) + h[3 * c + 1] * A.const(sq[j, 1])) + h[3 * c + 2], Qw[j]) for c in R2] for j in R4]
            delta = [[q[j][c] - A.const(sq[j, c]) for c in R2] for j in R4]
            d = [[delta[j][c] - X[:, 2 * j + c] for c in R2] for j in R4]
            ks = [[A.kalyo(d[j][c]) for c in R2] for j in R4]
            for j in R4:
                for c in R2:
                    out["margins"].append(A.abs(d[j][c]) - A.const(1))
            tsz = A.const(8 * n_sp + plus1)
            out["cor_pos_loss"] = A.div(A.total([ks[j][c][0] for j in R4 for c in R2]), tsz)
            if cf:
                k0 = A.div(A.div(g[0], A.const(4)), A.const(n_sp))
                k1 = A.div(A.div(g[1], A.const(4)), A.const(n_sp))
                k3 = A.div(g[3] + g[5], tsz)
                # slot 0
                ge = [[k0 * signed(e0[j][c]) for c in R2] for j in R4]
                dPc = [[A.div(ge[j][c], Pw[j]) for c in R2] for j in R4]
                dPw = [-(A.div(ge[j][0] * cor[j][0], Pw[j]) + A.div(ge[j][1] * cor[j][1], Pw[j])) for j in R4]
                gH_c = [_sum([dPc[j][c] * pk[k][j] for j in R4]) for c in R2 for k in range(3)] + [_sum([dPw[j] * pk[k][j] for j in R4]) for k in range(3)]
                g0pp = [[(Hs[:, 0, k] * dPc[j][0] + Hs[:, 1, k] * dPc[j][1]) + Hs[:, 2, k] * dPw[j] for j in R4] for k in range(3)]
                # slot 3 (and 5)
                gdel = [[k3 * ks[j][c][1] for c in R2] for j in R4]
                dQc = [[A.div(gdel[j][c], Qw[j]) for c in R2] for j in R4]
                dQw = [-(A.div(gdel[j][0] * q[j][0], Qw[j]) + A.div(gdel[j][1] * q[j][1], Qw[j])) for j in R4]
                gh = [_sum([dQc[j][c] * A.const(sq[j, k]) if k < 2 else dQc[j][c] for j in R4]) for c in R2 for k in range(3)]
                gh += [_sum([dQw[j] * A.const(sq[j, k]) for j in R4]) for k in R2]
                goff = A.dlt_adjoint(sv, gh)
                if variant == "dlt_point_swap_omitted":                                             # the adjoint's rows left in the solve's point order
                    goff = [goff[0], goff[1], goff[3], goff[2]]
                s3c = [[A.div(goff[j][c], pk[2][j]) for c in R2] for j in R4]
                s3w = [-(A.div(goff[j][0] * homo[j][0], pk[2][j]) + A.div(goff[j][1] * homo[j][1], pk[2][j])) for j in R4]
                if variant == "off_from_unnormalised_points":
                    s3c, s3w = goff, [zero * pk[2][j] for j in R4]
                rows = [[g0pp[c][j] + s3c[j][c] for j in R4] for c in R2] + [[g0pp[2][j] + s3w[j] for j in R4]]
                if variant == "w_row_gradient_dropped":
                    rows[2] = [zero * r for r in rows[2]]
                gH = A.scatter(B, sp, gH_c, (3, 3))
                gpp = A.scatter(B, sp, [rows[k][j] for k in range(3) for j in R4], (3, 4))
                gaug = A.scatter(B, sp, [k1 * signed(e1[j][c]) for c in R2 for j in R4] + [0.0] * 4, (3, 4))
                gx = A.scatter(B, sp, [-gdel[j][c] for j in R4 for c in R2], (8,))

        # ---- the unsupervised positives: slot 2
        out["cor_err_sim"] = zero
        if n_up:
            P, T = pp[up], tp[up]
            if variant == "slot2_divided_by_w":
                e2 = [[A.div(P[:, c, j], P[:, 2, j]) - T[:, j, c] for c in R2] for j in R4]
            else:
                e2 = [[P[:, c, j] - T[:, j, c] for c in R2] for j in R4]
            out["cor_err_sim"] = A.div(A.div(A.total([A.abs(e2[j][c]) for j in R4 for c in R2]), A.const(n_up)), A.const(4))
            if cf:
                k2 = A.div(A.div(g[2], A.const(4)), A.const(n_up))
                part = A.scatter(B, up, [k2 * signed(e2[j][c]) for c in R2 for j in R4] + [0.0] * 4, (3, 4))
                gpp = part if gpp is None else A.add_full(gpp, part)

        # ---- the negatives: slot 4, computed over every negative, reported with a supervised one
        out["cor_neg_loss"] = zero
        report = n_ng > 0 and (n_sn > 0 or variant == "slot4_reported_without_sup_neg")
        if report:
            X = x[ng]
            ks = [A.kalyo(-X[:, r]) for r in range(8)]
            for r in range(8):
                out["margins"].append(A.abs(X[:, r]) - A.const(1))
            tsz = A.const(8 * n_ng + plus1)
            out["cor_neg_loss"] = A.div(A.total([k[0] for k in ks]), tsz)
            if cf:
                k4 = A.div(g[4] + g[5], tsz)
                part = A.scatter(B, ng, [-(k4 * k[1]) for k in ks], (8,))
                gx = part if gx is None else A.add_full(gx, part)
        out["cor_loss"] = out["cor_pos_loss"] + out["cor_neg_loss"]
        if cf:
            empty = lambda shape: A.scatter(B, np.zeros(0, dtype=np.int64), [], shape)
            out["grad_H_mat"] = gH if gH is not None else empty((3, 3))
            out["grad_pred_points"] = gpp if gpp is not None else empty((3, 4))
            out["grad_aug_sear_points"] = gaug if gaug is not None else empty((3, 4))
            out["grad_x"] = gx if gx is not None else empty((8,))
        return out

    def margin_ok(self):
        """every sign and branch decision of the float64 run lies MARGIN bounds away from its kink"""
        for v in self.truth()["q"]["margins"]:
            if (np.abs(v.v) < MARGIN * v.e).any():
                return False
        return True

    def truth(self):
        """{"q": QA outputs for grad_out = w (value = the float64 truth, e = the bound), "q_ns": the same for grad_out = w * NO_SOLVE}"""
        if self._truth is None:
            with np.errstate(invalid="ignore"):
                self._truth = {"q": self.evaluate(QA()), "q_ns": self.evaluate(QA(), weights=self.w * NO_SOLVE)}
        return self._truth

    def torch_run(self, dtype, device="cpu", weights=None, fn=None):
        """PyTorch's own run of the restated lines with autograd to the leaves -> KEYS, counts, GRADS.  fn: a replacement for the forward (the GPU
        test passes hdn_amd.corner_losses)."""
        T = lambda a: torch.as_tensor(a, dtype=dtype, device=device)
        arr = self.arrays()
        leaves = {k: T(arr[k]).requires_grad_(k in ("H_mat", "pred_points", "aug_sear_points", "x")) for k in arr}
        if fn is None:
            out = self.evaluate(TA(dtype, device), leaves=leaves)
        else:
            out = fn(leaves)
        w = T(self.w if weights is None else weights)
        scalar = sum(w[i] * out[k] for i, k in enumerate(KEYS))
        res = {k: out[k].detach() for k in KEYS}
        res["counts"] = out["counts"]
        names = ("H_mat", "pred_points", "aug_sear_points", "x")
        if scalar.requires_grad:
            gr = torch.autograd.grad(scalar, [leaves[k] for k in names], allow_unused=True)
        else:
            gr = [None] * 4
        for k, n, v in zip(GRADS, names, gr):
            res[k] = torch.zeros_like(leaves[n]) if v is None else v
        return res


def ratio(v, q, ctx):
    """max error / bound of v against the Qv q; where no rounding is on the path (bound 0) the values must be equal"""
    v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    assert v.shape == q.v.shape, ctx + (v.shape, q.v.shape)
    err = np.abs(v.astype(np.float64) - q.v)
    assert not np.isnan(err).any(), ctx
    zero = q.e == 0
    if zero.any():
        assert (err[zero] == 0).all(), ctx + ("an element with no rounding on its path differs",)
    if not (~zero).any():
        return 0.0
    return float((err[~zero] / q.e[~zero]).max())


def check(got, case, truth="q", keys=None, what="", limit=1.0):
    """Hold `got` (name -> array or tensor) to the float64 truth of `case` within the QA bounds; counts exactly.  -> the worst error / bound."""
    tr = case.truth()[truth]
    worst = 0.0
    for k, v in got.items():
        if k not in tr or k == "margins" or (keys is not None and k not in keys):
            continue
        if k == "counts":
            v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            assert v.dtype == np.int32 and np.array_equal(v, tr[k]), (what, case.name, k, v, tr[k])
            continue
        r = ratio(v, tr[k], (what, case.name, k))
        assert r <= limit, (what, case.name, k, r)
        worst = max(worst, r)
    return worst


def _flags(B, pos, un):
    return (np.full(B, pos, dtype=np.float32), np.full(B, un, dtype=np.float32))


def _one(B, idx):
    """only sample idx is a supervised positive; the others are unsupervised, positive and negative in turn"""
    pos, un = (np.arange(B) % 2).astype(np.float32), np.ones(B, dtype=np.float32)
    pos[idx], un[idx] = 1, 0
    return pos, un


def _production(B=32, sup=24):
    """24 supervised samples of 32, one in five negative"""
    un = (np.arange(B) >= sup).astype(np.float32)
    pos = (np.arange(B) % 5 != 4).astype(np.float32)
    return pos, un


def _odd(B):
    """flags of 0.5, 2 and NaN among regular ones: those samples are in no set whose predicate they fail"""
    g = np.random.default_rng(77)
    pos = g.choice(np.array([0, 1, 1, 1, 0.5, 2, np.nan], dtype=np.float32), B)
    un = g.choice(np.array([0, 0, 0, 1, 0.5, 2, np.nan], dtype=np.float32), B)
    pos[:4], un[:4] = (1, 0, 1, 0), (0, 0, 1, 1)
    return pos, un


def _cases():
    cs = [Case("B1_sup_pos", 1, 11, _flags(1, 1, 0)), Case("B1_sup_neg", 1, 12, _flags(1, 0, 0)), Case("B1_unsup_pos", 1, 13, _flags(1, 1, 1)),
          Case("B1_unsup_neg", 1, 14, _flags(1, 0, 1))]
    for B in (7, 8, 9, 31, 32, 33, 64, 65, 257, 1000):
        cs.append(Case(f"mix_B{B}", B, 100 + B))
    cs.append(Case("all_sup_pos_B33", 33, 201, _flags(33, 1, 0)))
    cs.append(Case("no_sup_pos_B33", 33, 202, ((np.arange(33) % 3 == 0).astype(np.float32), (np.arange(33) % 3 != 1).astype(np.float32))))
    cs.append(Case("first_only_B65", 65, 203, _one(65, 0)))
    cs.append(Case("last_only_B65", 65, 204, _one(65, 64)))
    cs.append(Case("neg_all_unsup_B33", 33, 205, ((np.arange(33) % 4 != 0).astype(np.float32), (np.arange(33) % 4 == 0).astype(np.float32))))
    cs.append(Case("production_B32", 32, 206, _production()))
    cs.append(Case("odd_flags_B33", 33, 207, _odd(33)))
    cs.append(Case("w_B33", 33, 301, family="w"))
    cs.append(Case("w_B65", 65, 302, family="w"))
    return {c.name: c for c in cs}


CASES = _cases()
CASE_NAMES = tuple(CASES)

# which case catches which wrong kernel
MUTATION_CASES = {
    "neg_loss_over_sup_neg_only": "mix_B33",
    "tsz_without_plus_1": "mix_B9",
    "slot2_divided_by_w": "w_B33",
    "two_search_corners_swapped": "mix_B9",
    "slot4_reported_without_sup_neg": "neg_all_unsup_B33",
    "slot0_divided_by_n_neg": "mix_B33",
    "dlt_point_swap_omitted": "mix_B9",
    "h_gt_applied_as_inverse": "mix_B9",
    "w_row_gradient_dropped": "mix_B9",
    "off_from_unnormalised_points": "w_B33",
}


# ---------------------------------------------------------------------------------------------------------------------------- exact fixtures
EXACT_TRANSLATIONS = ((0.0, 0.0), (4.0, -8.0), (0.5, 1.0), (3.0, 5.0), (-16.0, 32.0))
EXACT_D = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 3.5, -3.5)


class ExactCase:
    """template_poly = SQUARE, pred_points = its corners + a dyadic translation t_b (w = 1), H_mat a dyadic translation: the float64 elimination
    returns the translation exactly (test_corner_loss_host.py repeats the proof), so delta = t_b, every sum is a sum of dyadic numbers far below 2^24
    and each output is the fp32 sequence of its one or two divisions.  x = delta - d with d cycling through EXACT_D."""

    def __init__(self, name, if_pos, if_unsup, th=(2.0, -4.0)):
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        self.name, self.B = name, len(if_pos)
        B = self.B
        self.if_pos, self.if_unsup = f(if_pos), f(if_unsup)
        self.ids = set_ids(self.if_pos, self.if_unsup)
        t = np.array([EXACT_TRANSLATIONS[b % len(EXACT_TRANSLATIONS)] for b in range(B)])
        self.t, self.th = t, np.array(th)
        self.template_poly = f(np.tile(SQUARE, (B, 1, 1)))
        xy = SQUARE[None] + t[:, None, :]
        self.pred_points = f(np.concatenate([xy.transpose(0, 2, 1), np.ones((B, 1, 4))], 1))
        ta = t[:, ::-1] * 2                                                # another dyadic translation for the augmented points
        self.ta = ta
        self.aug_sear_points = f(np.concatenate([(SQUARE[None] + ta[:, None, :]).transpose(0, 2, 1), np.ones((B, 1, 4))], 1))
        H = np.tile(np.eye(3), (B, 1, 1))
        H[:, :2, 2] = th
        self.H_mat = f(H)
        self.d = np.array([[EXACT_D[(3 * b + r) % len(EXACT_D)] for r in range(8)] for b in range(B)])
        delta = np.repeat(t[:, None, :], 4, 1).reshape(B, 8)
        sp = np.zeros(B, dtype=bool)
        sp[self.ids["sup_pos"]] = True
        self.x = f(np.where(sp[:, None], delta - self.d, -self.d))         # elsewhere d = 0 - x
        self.w = f([1.0, -0.5, 2.0, 0.75, -1.5, 0.25])

    arrays = Case.arrays

    def expected(self):
        """KEYS, counts and grad_x in fp32, from exact sums and the kernel's sequence of divisions"""
        F = np.float32
        ids = self.ids
        n_sp, n_sn, n_up, n_ng = (len(ids[k]) for k in ("sup_pos", "sup_neg", "unsup_pos", "neg"))
        k = lambda d: np.where(np.abs(d) < 1, 0.5 * d * d, np.abs(d) - 0.5)
        slope = lambda d: np.where(np.abs(d) < 1, d, np.sign(d))
        out = dict.fromkeys(KEYS, F(0))
        gx = np.zeros((self.B, 8), dtype=np.float32)
        g = self.w
        if n_sp:
            sp = ids["sup_pos"]
            out["cor_err"] = F(4 * np.abs(self.t[sp] + self.th).sum()) / F(n_sp) / F(4)
            out["cor_err_aug"] = F(4 * np.abs(self.ta[sp]).sum()) / F(n_sp) / F(4)
            out["cor_pos_loss"] = F(k(self.d[sp]).sum()) / F(8 * n_sp + 1)
            gx[sp] = -(((g[3] + g[5]) / F(8 * n_sp + 1)) * slope(self.d[sp]).astype(np.float32))
        if n_up:
            out["cor_err_sim"] = F(4 * np.abs(self.t[ids["unsup_pos"]]).sum()) / F(n_up) / F(4)
        if n_sn:
            ng = ids["neg"]
            out["cor_neg_loss"] = F(k(self.d[ng]).sum()) / F(8 * n_ng + 1)
            gx[ng] = -(((g[4] + g[5]) / F(8 * n_ng + 1)) * slope(self.d[ng]).astype(np.float32))
        out["cor_loss"] = F(out["cor_pos_loss"]) + F(out["cor_neg_loss"])
        out = {k_: np.float32(v) for k_, v in out.items()}
        out["counts"] = np.array([len(ids[k_]) for k_ in SETS], dtype=np.int32)
        out["grad_x"] = gx
        return out


EXACT_CASES = {c.name: c for c in (
    ExactCase("exact_B1", [1], [0]),
    ExactCase("exact_B8_mixed", [1, 0, 1, 1, 0, 1, 0, 1], [0, 0, 1, 0, 1, 0, 0, 1]),
    ExactCase("exact_B33_all_sup_pos", [1] * 33, [0] * 33),
    ExactCase("exact_B130_mixed", [(b % 4 != 1) for b in range(130)], [(b % 3 == 2) for b in range(130)], th=(-0.5, 8.0)),
)}
EXACT_NAMES = tuple(EXACT_CASES)
