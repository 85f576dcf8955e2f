"""The cases, the bound and the expectations that tests/test_triplet_host.py (CPU) and tests/test_gpu_triplet.py (GPU) share for the L1 triplet rows of
csrc/triplet_loss.hip (hdn_triplet_l1_f32, hdn_triplet_l1_bwd_f32).  Nothing here touches the device.

The reference of every check is float64: torch.triplet_margin_loss (the operator behind nn.TripletMarginLoss; p=1, reduction 'none') with autograd on
the fp32 inputs cast up (the operator itself, because the cases use margins <= 0, which the Python wrappers refuse), restated in numpy by closed() so that the mutations can be written down beside it.

The bound of a loss row, for any summation order:

    tol = (D + 3) 2^-24 (margin + d_ap + d_an) + 2 D 2^-24 eps          d_ap, d_an from float64

two roundings per term, at most D - 1 in a sum, two in v, and the clamp is 1-Lipschitz.  Gradients are exact: the signs come from elementwise fp32
operations, g {0, +-1, +-2} is exact, so for every row with |v64| > tol the gradients are torch.equal to expected_grads(); rows with |v64| <= tol are
left out of the gradient comparison only, at most 1 % of a case's rows (EXCLUDED_CAP; the host test counts them: zero with these seeds).

The kernel's workgroup holds ROWS_PER_WG = 4 rows (one wave each), so the row counts 3, 4, 5 are one fewer, exactly one and one more workgroup; 1, 9
and 2 x 127 add a lone row, a tail after two workgroups and the reference's row length over many workgroups.  The wave is 64 lanes: D = 63, 64, 65,
127, 128, 129 are either side of one and two lane passes, 1 and 2 the shortest rows, 257 a tail after four passes.
"""
import functools
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261020
U = 2.0 ** -24
ROWS_PER_WG = 4
EXCLUDED_CAP = 0.01
EPS = 1e-6
EPS32 = float(np.float32(1e-6))

DS = (1, 2, 63, 64, 65, 127, 128, 129, 257)
ROW_SHAPES = {1: (1, 1), 3: (3, 1), 4: (2, 2), 5: (5, 1), 9: (3, 3), 254: (2, 127)}      # N R -> (N, R)


# ------------------------------------------------------------------------------------------------------------------------------------ the reference
def closed(a, p, n, margin, eps, g=None, variant=None, dtype=np.float64):
    """The row arithmetic in numpy at `dtype` (sums in numpy's order) -> dict(loss, v, d_ap, d_an[, ga, gp, gn]).  variant: None = the kernel's
    formulas; otherwise one of MUTATIONS, a mistake the tests must be able to see."""
    a, p, n = (np.asarray(t, dtype=dtype) for t in (a, p, n))
    e, m = dtype(eps), dtype(margin)
    x, y = a - p, a - n
    if variant is None or variant == "order":
        t_ap, t_an = np.abs(x + e), np.abs(y + e)
    elif variant == "eps_outside":
        t_ap, t_an = np.abs(x) + e, np.abs(y) + e
    elif variant == "eps_subtracted":
        t_ap, t_an = np.abs(x - e), np.abs(y - e)
    elif variant == "eps_omitted":
        t_ap, t_an = np.abs(x), np.abs(y)
    elif variant == "l2":
        t_ap, t_an = (x + e) ** 2, (y + e) ** 2
    else:
        raise KeyError(variant)
    d_ap, d_an = t_ap.sum(-1, dtype=dtype), t_an.sum(-1, dtype=dtype)
    if variant == "l2":
        d_ap, d_an = np.sqrt(d_ap), np.sqrt(d_an)
    v = (d_ap - d_an) + m if variant == "order" else (m + d_ap) - d_an
    out = {"loss": np.where(v < 0, dtype(0), v), "v": v, "d_ap": d_ap, "d_an": d_an}
    if g is not None:
        gg = np.where(v >= 0, np.asarray(g, dtype=dtype), dtype(0))[..., None]
        s_ap, s_an = np.sign(x + e), np.sign(y + e)
        out.update(ga=gg * (s_ap - s_an), gp=-gg * s_ap, gn=gg * s_an)
    return out


MUTATIONS = {"eps_outside": "eps_rows", "eps_subtracted": "eps_rows", "eps_omitted": "eps_rows", "l2": "eps_rows", "order": "order_rows"}


def tol(d_ap64, d_an64, D, margin, eps):
    return (D + 3) * U * (margin + d_ap64 + d_an64) + 2 * D * U * eps


def torch_loss(a, p, n, margin, eps):
    """PyTorch's own operator behind nn.TripletMarginLoss(p=1, reduction='none'), called directly: the Python wrappers refuse margin <= 0."""
    return torch.triplet_margin_loss(a, p, n, float(margin), 1.0, float(eps), False, 0)


def autograd64(a, p, n, g, margin, eps, dtype=torch.float64):
    """(loss, ga, gp, gn) of PyTorch's own triplet loss at `dtype` on the CPU."""
    a, p, n = (t.detach().to(dtype).requires_grad_(True) for t in (a, p, n))
    loss = torch_loss(a, p, n, margin, eps)
    loss.backward(g.to(dtype))
    return loss.detach(), a.grad, p.grad, n.grad


# ------------------------------------------------------------------------------------------------------------------------------------------ cases
class Case:
    """a, p, n [N,R,D] fp32, g [n_sel,R] fp32, margin, eps, ids (list | None); exact: the expectation is the fp32 restatement bit for bit on
    every row (rows whose sums are order-independent by construction), otherwise the float64 truth within tol."""

    def __init__(self, name, a, p, n, margin=1.0, eps=EPS, ids=None, exact=False, seed=0):
        self.name, self.a, self.p, self.n, self.margin, self.eps, self.ids, self.exact = name, a, p, n, float(margin), float(eps), ids, exact
        self.N, self.R, self.D = a.shape
        self.n_sel = self.N if ids is None else len(ids)
        gen = torch.Generator().manual_seed(SEED + 7919 + seed)
        self.g = torch.randn(self.n_sel, self.R, generator=gen)

    def gathered(self):
        """(a, p, n) as the reference's x[ids] copies."""
        if self.ids is None:
            return self.a, self.p, self.n
        idx = torch.tensor(self.ids, dtype=torch.long)
        return self.a[idx], self.p[idx], self.n[idx]

    def scatter(self, grad_sel):
        """A gradient of the gathered copies as the full-size one: zero rows for the samples left out."""
        if self.ids is None:
            return grad_sel
        full = torch.zeros_like(self.a, dtype=grad_sel.dtype)
        full[torch.tensor(self.ids, dtype=torch.long)] = grad_sel
        return full

    @functools.lru_cache(maxsize=None)
    def truth(self):
        """Computed once: float64 loss, tol and v per selected row, which rows are compared for gradients, the expected full-size fp32 gradients."""
        a, p, n = self.gathered()
        c64 = closed(a.numpy(), p.numpy(), n.numpy(), self.margin, self.eps)
        t = tol(c64["d_ap"], c64["d_an"], self.D, self.margin, self.eps)
        if self.exact:
            c32 = closed(a.numpy(), p.numpy(), n.numpy(), self.margin, np.float32(self.eps), dtype=np.float32)
            active, compared = c32["v"] >= 0, np.ones_like(t, dtype=bool)
            loss = torch.from_numpy(c32["loss"])
        else:
            active, compared = c64["v"] >= 0, np.abs(c64["v"]) > t
            loss = torch.from_numpy(c64["loss"])
        e32 = torch.tensor(self.eps, dtype=torch.float32)
        s_ap, s_an = torch.sign((a - p) + e32), torch.sign((a - n) + e32)            # fp32 elementwise: no order to depend on
        gg = (self.g * torch.from_numpy(active).float()).unsqueeze(-1)
        grads = tuple(self.scatter(x) for x in (gg * (s_ap - s_an), -gg * s_ap, gg * s_an))
        compared_full = torch.ones(self.a.shape, dtype=torch.bool)                   # the rows of samples left out are compared too: they are zero
        compared_full[list(range(self.N)) if self.ids is None else self.ids] = torch.from_numpy(compared).unsqueeze(-1).expand(a.shape)
        return {"loss": loss, "tol": torch.from_numpy(t), "v64": torch.from_numpy(c64["v"]), "compared": torch.from_numpy(compared),
                "compared_full": compared_full, "grads": grads, "excluded": int((~compared).sum())}


def _normal(name, N, R, D, scale=1.0, ids=None, seed=0, margin=1.0):
    gen = torch.Generator().manual_seed(SEED + seed)
    a, p, n = (scale * torch.randn(N, R, D, generator=gen) for _ in range(3))
    return Case(name, a, p, n, margin=margin, ids=ids, seed=seed)


def _eps_rows():
    """margin = 0, a = p = 0, a - n = k 1e-6 with k of both signs, chosen so that v > 0 on every row (the loss feels every term) and every eps
    mistake and L2 changes it: |k + 1| sums to less than D."""
    ks = [[-1, -1, -2, 1, -1, -2, -1, -3], [-1, -2, -1, -1, 2, -1, -1, -1], [-2, -1, -1, 1, -1, -1, -3, -1], [-1, -1, -1, -1, -2, 3, -1, -1]]
    n = -(torch.tensor(ks, dtype=torch.float64) * 1e-6).float().reshape(2, 2, 8)
    z = torch.zeros_like(n)
    return Case("eps_rows", z, z.clone(), n, margin=0.0)


def _order_rows():
    """eps = 0 and terms whose sums are exact in any order; margin = -1000 against d_ap = 1001 and d_an = 3 2^-20: (margin + d_ap) - d_an is exact up
    to the last rounding, (d_ap - d_an) + margin rounds the difference at the size of 1000 first."""
    D = 4
    a = torch.zeros(1, 3, D)
    p = torch.full((1, 3, D), -250.25)
    n = torch.zeros(1, 3, D)
    for r, k in enumerate((3.0, 5.0, -7.0)):
        n[0, r, r] = k * 2.0 ** -20
    return Case("order_rows", a, p, n, margin=-1000.0, eps=0.0)


BOUNDARY_DS = (1, 65, 127)


def _boundary(D):
    """margin = 1.  One live element (a, p, n) = (0, 0, -1): fl(1 + fl(1e-6)) - fl(1 + fl(1e-6)) = 0 exactly; every other element is (0, 1e-6f, 1e-6f),
    whose two terms are exactly 0, so the row is order-independent.  Sample i puts the live element at POSITIONS[i]; its three rows have
    n = -1 (v = 0: loss 0, the gradient passes), n = -1 + 2^-20 (strictly active) and n = -1 - 2^-20 (strictly inactive)."""
    pos = [q for q in (0, 63, 64, D - 1) if q < D]
    pos = sorted(set(pos))
    e = torch.tensor(EPS, dtype=torch.float32)
    a = torch.zeros(len(pos), 3, D)
    p, n = e.expand(len(pos), 3, D).clone(), e.expand(len(pos), 3, D).clone()
    for i, q in enumerate(pos):
        p[i, :, q] = 0.0
        n[i, 0, q], n[i, 1, q], n[i, 2, q] = -1.0, -1.0 + 2.0 ** -20, -1.0 - 2.0 ** -20
    return Case(f"boundary_D{D}", a, p, n, margin=1.0, exact=True), pos


@functools.lru_cache(maxsize=None)
def boundary_positions(D):
    return _boundary(D)[1]


def _build():
    cases = []
    for D in DS:
        for rows, (N, R) in ROW_SHAPES.items():
            cases.append(_normal(f"n01_{N}x{R}x{D}", N, R, D, seed=len(cases)))
    for D in DS:
        cases.append(_normal(f"n100_3x3x{D}", 3, 3, D, scale=100.0, seed=len(cases)))
    cases.append(_normal("n100_2x127x127", 2, 127, 127, scale=100.0, seed=len(cases)))
    for N, R, D in ((3, 3, 127), (2, 127, 127)):
        cases.append(_normal(f"small_{N}x{R}x{D}", N, R, D, scale=1e-4, seed=len(cases)))
    cases += [_eps_rows(), _order_rows()] + [_boundary(D)[0] for D in BOUNDARY_DS]
    cases.append(_normal("ids_all_3x5x65", 3, 5, 65, ids=[0, 1, 2], seed=len(cases)))
    cases.append(_normal("ids_0_2_of_3", 3, 5, 127, ids=[0, 2], seed=len(cases)))
    cases.append(_normal("ids_24_of_32", 32, 3, 65, ids=[i for i in range(32) if i % 4 != 1], seed=len(cases)))
    cases.append(_normal("ids_single", 5, 3, 129, ids=[3], seed=len(cases)))
    cases.append(_normal("ids_unordered", 4, 2, 64, ids=[3, 0, 2], seed=len(cases)))
    return {c.name: c for c in cases}


CASES = _build()
NAMES = list(CASES)


def expected_boundary(case, D):
    """The issue's statement of the boundary rows, written out (not derived from closed()): loss (0, > 0, 0); at the live element of rows 0 and 1
    grad_p = -g, grad_n = g, grad_a = 0; everything else exactly 0."""
    pos = boundary_positions(D)
    ga, gp, gn = (torch.zeros_like(case.a) for _ in range(3))
    for i, q in enumerate(pos):
        for r in (0, 1):
            gp[i, r, q], gn[i, r, q] = -case.g[i, r], case.g[i, r]
    return ga, gp, gn
