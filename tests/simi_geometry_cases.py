"""Fixtures, restatements and bounds for csrc/simi_geometry.hip (tests/test_simi_geometry_host.py, tests/test_gpu_simi_geometry.py).  No device.

The lines under test are hdn/models/model_builder_e2e_unconstrained_v2.py:377 and :390-415: Polar_Pick.get_polar_from_two_para_loc, lp_pick, the two
combine_affine functions and the homogeneous products.  They are restated ONCE, as functions of an arithmetic `A` (r_* below), and read four ways:

    NP(np.float32)      every operation individually rounded: what the kernel must equal bit for bit where no libm call or division is on the path
                        (best_idx, polar, rot, the gradient of loc, the gradient of loc_lp[:, 2] of the pick)
    NP(np.float64)      the truth of the forward
    TorchA(dtype, dev)  PyTorch's own run (fp32 on the CPU: r_ref; fp32 on the device: PyTorch-ROCm; float64 with autograd: the truth of the gradients)
    Q                   float64 values that carry a first-order running error bound: each operation adds u |result| (u = 2^-24, one rounding), each
                        libm call (exp, sin, cos) and each division adds LIBM_ROUNDINGS u |result| (sin, cos: of 1), and the errors of the operands
                        are carried through by the operation's derivative.  For a sum of terms that is (roundings on the term's path) u |term|, summed:
                        the bound "(number of fp32 roundings on the path) 2^-24 sum |terms|".  A constant that fp32 cannot hold costs one rounding.

LIBM_ROUNDINGS is not guessed: it is the smallest integer for which PyTorch's fp32 run on the CPU stays within half the bound on every case
(test_simi_geometry_host.py measures r_ref and asserts it); the kernel and PyTorch-ROCm are then held to the full bound.

The gradients are restated in closed form (r_lp_bwd, r_affine_grads) for the bounds; the host test holds their float64 values to float64 autograd.
"""
import functools
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "simi_geometry.npz")

U = 2.0 ** -24
LIBM_ROUNDINGS = 5            # roundings charged per libm call and per division: the smallest count with r_ref <= 0.5
R_REF = 0.476                 # the worst ratio of PyTorch's CPU fp32 run to the bound, as measured (test_r_ref_is_what_the_module_records)

STRIDE, STRIDE_LP, MAP_SIZE, IN_SZ, OUT_SZ = 8, 8, 127, 255, 127
MAG, ROT_UNIT = float(np.log(MAP_SIZE / 2) / MAP_SIZE), float(2 * np.pi / MAP_SIZE)
GOLDEN_GRAD_CELLS = 700       # cases with at most this many cells (B S S) carry the reference's autograd gradients in the fixture

EXACT = ("best_idx", "polar", "best_idx_lp", "rot", "pick_grad_loc")        # bit-equal to NP(np.float32); pick_grad_loc_lp: channel 2 only
MATS = ("affine_m", "affine_m_lt0", "affine_m_c_aug", "affine_m_lt0_aug")
BOUNDED = ("scale",) + MATS + ("pred_points", "aug_sear_points", "grad_loc_lp", "grad_polar", "pick_grad_loc_lp", "chain_grad_loc")


# ------------------------------------------------------------------------------------------------------------------------------- arithmetics
class NP:
    """numpy arrays of one dtype: every operator rounds once."""

    def __init__(self, dtype):
        self.dtype = dtype

    def inp(self, x):
        return np.asarray(x, dtype=self.dtype)

    def const(self, v):
        return self.dtype(v)

    exp, sin, cos = staticmethod(np.exp), staticmethod(np.sin), staticmethod(np.cos)

    def div(self, a, b):
        return a / b

    def stack(self, comps, shape):
        comps = [np.broadcast_to(np.asarray(c, dtype=self.dtype), np.shape(comps[0])) for c in comps]
        return np.stack(comps, -1).reshape(-1, *shape)


class TorchA:
    """torch tensors: constants stay Python floats, as in the reference, and meet the tensors there."""

    def __init__(self, dtype, device="cpu"):
        self.dtype, self.device = dtype, device

    def inp(self, x):
        return x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), dtype=self.dtype, device=self.device)

    def const(self, v):
        return float(v)

    exp, sin, cos = staticmethod(torch.exp), staticmethod(torch.sin), staticmethod(torch.cos)

    def div(self, a, b):
        return a / b

    def stack(self, comps, shape):
        return torch.stack([c if isinstance(c, torch.Tensor) else torch.full_like(comps[0], c) for c in comps], -1).reshape(-1, *shape)


class Qv:
    """a float64 value with a bound on the error of its fp32 evaluation"""
    __array_priority__ = 1000

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape).copy()

    @staticmethod
    def of(x):
        return x if isinstance(x, Qv) else Qv(x)

    def __neg__(self):
        return Qv(-self.v, self.e)

    def __getitem__(self, i):
        return Qv(self.v[i], self.e[i])

    def reshape(self, *shape):
        return Qv(self.v.reshape(*shape), self.e.reshape(*shape))

    def _lin(self, o, sign):
        o = Qv.of(o)
        v = self.v + sign * o.v
        return Qv(v, self.e + o.e + U * np.abs(v))

    def __add__(self, o):
        return self._lin(o, 1.0)

    __radd__ = __add__

    def __sub__(self, o):
        return self._lin(o, -1.0)

    def __rsub__(self, o):
        return Qv.of(o)._lin(self, -1.0)

    def __mul__(self, o):
        o = Qv.of(o)
        v = self.v * o.v
        return Qv(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + U * np.abs(v))

    __rmul__ = __mul__


class Q:
    def inp(self, x):
        return Qv(x)

    def const(self, v):
        return Qv(v, 0.0 if float(np.float32(v)) == float(v) else U * abs(v))

    def exp(self, a):
        v = np.exp(a.v)
        return Qv(v, v * a.e + LIBM_ROUNDINGS * U * v)

    def sin(self, a):
        return Qv(np.sin(a.v), a.e + LIBM_ROUNDINGS * U)

    def cos(self, a):
        return Qv(np.cos(a.v), a.e + LIBM_ROUNDINGS * U)

    def div(self, a, b):
        a, b = Qv.of(a), Qv.of(b)
        v = a.v / b.v
        return Qv(v, a.e / np.abs(b.v) + np.abs(v) * b.e / np.abs(b.v) + LIBM_ROUNDINGS * U * np.abs(v))

    def stack(self, comps, shape):
        comps = [Qv.of(c) for c in comps]
        full = np.shape(comps[0].v)
        return Qv(np.stack([np.broadcast_to(c.v, full) for c in comps], -1).reshape(-1, *shape),
                  np.stack([np.broadcast_to(c.e, full) for c in comps], -1).reshape(-1, *shape))


# ------------------------------------------------------------------------------------------------------------------------------ restatements
def analytic_points(stride, S):
    """generate_points(stride, S): float32 [S S, 2], x by column, y by row"""
    ori = -(S // 2) * stride
    ax = (ori + stride * np.arange(S)).astype(np.float32)
    x, y = np.meshgrid(ax, ax)
    return np.stack([x.ravel(), y.ravel()], 1)


def softmax_class1(c0, c1):
    """score.softmax(2)[:, :, 1] in the dtype of the inputs: exp(x - max) for both, times 1 / sum"""
    with np.errstate(invalid="ignore"):
        m = np.maximum(c0, c1)
        e0, e1 = np.exp(c0 - m), np.exp(c1 - m)
        return e1 * (c0.dtype.type(1) / (e0 + e1))


def r_polar(A, px, py, l0, l1, mult):
    return px - l0 * mult, py - l1 * mult


def r_lp(A, px, py, l0, l2, stride_lp):
    scale = A.exp((px - l0 * stride_lp) * A.const(MAG))
    rot = (py - l2 * stride_lp) * A.const(ROT_UNIT)
    return scale, rot


def r_lp_bwd(A, g_scale, g_rot, scale, stride_lp):
    return -((g_scale * scale) * A.const(MAG)) * stride_lp, -(g_rot * A.const(ROT_UNIT)) * stride_lp


def r_operands(A, kind, cx, cy, nm0, nm1, scale, scale_h, in_sz, out_sz):
    """(sc, U, V, W0, W1, div | None) of the two combine_affine functions; cx, cy numbers or arrays"""
    vec = not isinstance(cx, (int, float))
    if kind == 0:
        sc = A.const(out_sz / in_sz) * scale
        if vec:
            U_, V_ = (A.div((c - A.const(out_sz / 2)) * A.const(in_sz), A.const(out_sz)) for c in (cx, cy))
        else:
            U_, V_ = (A.const((c - out_sz / 2) * in_sz / out_sz) for c in (cx, cy))
        return sc, U_, V_, nm0, nm1, (A.const(out_sz) if scale_h else None)
    W0, W1 = (cx, cy) if vec else (A.const(cx), A.const(cy))
    return scale, nm0 + A.const(in_sz / 2), nm1 + A.const(in_sz / 2), W0, W1, None


def r_rows(A, ops, rot, variant=None):
    sc, U_, V_, W0, W1, div = ops
    cc, ss = A.cos(rot), A.sin(rot)
    a, c = sc * cc, sc * ss
    b = -c
    t0 = ((-a) * U_ - b * V_) + W0
    t1 = ((-c) * U_ - a * V_) + W1
    if div is not None and variant != "scale_h_division_dropped":
        t0, t1 = A.div(t0, div), A.div(t1, div)
    return [a, b, t0, c, a, t1]


def r_affine_grads(A, ops, rot, G):
    """d / d (sc, rot, U, V, W0, W1) of sum(G * r_rows): t0 = -a U + c V + W0, t1 = -c U - a V + W1"""
    sc, U_, V_, _, _, div = ops
    cc, ss = A.cos(rot), A.sin(rot)
    a, c = sc * cc, sc * ss
    h0, h1 = (G[2], G[5]) if div is None else (A.div(G[2], div), A.div(G[5], div))
    Ga = (G[0] + G[4]) - (U_ * h0 + V_ * h1)
    Gc = (G[3] - G[1]) + (V_ * h0 - U_ * h1)
    return (Ga * cc + Gc * ss, sc * (Gc * cc - Ga * ss), -(a * h0 + c * h1), c * h0 - a * h1, h0, h1)


def r_poly(A, m, xs, ys):
    """[m; 0 0 1] [x; y; 1] -> 12 components, row-major [3,4]"""
    rows = [[(m[3 * r] * xs[j] + m[3 * r + 1] * ys[j]) + m[3 * r + 2] for j in range(4)] for r in range(2)]
    return rows[0] + rows[1] + [1.0] * 4


# ----------------------------------------------------------------------------------------------------------------------------------- cases
class Case:
    """One batch: head maps, template centres, the search polygon and the upstream weights, all float32, made from a seed."""

    def __init__(self, name, family, B, S, seed, golden=True):
        self.name, self.family, self.B, self.S, self.n, self.golden = name, family, B, S, S * S, golden
        g = np.random.default_rng(seed)
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        n = self.n
        c0 = g.uniform(-1, 1, (B, n))
        d = g.uniform(-2, 2, (B, n))
        c0_lp = g.uniform(-1, 1, (B, n))
        d_lp = g.uniform(-2, 2, (B, n))
        self.want = self.want_lp = None
        if family in ("every_cell", "separated"):
            ws = np.arange(B) % n if family == "every_cell" else g.integers(0, n, B)          # the softmax winner; the raw winner sits elsewhere
            wr = (n - 1 - ws) if family == "every_cell" else g.integers(0, n, B)
            for maps in ((c0, d), (c0_lp, d_lp)):
                for b in range(B):
                    maps[0][b, wr[b]], maps[1][b, wr[b]] = 4.0, 1.0
                    maps[0][b, ws[b]], maps[1][b, ws[b]] = (1.0, 5.0) if ws[b] == wr[b] else (-3.0, 5.0)
            self.want, self.want_lp = wr, ws
        c1, c1_lp = c0 + d, c0_lp + d_lp
        if family == "saturated":                 # p == 1.0f at three cells at least; a later one has the larger difference
            first = g.integers(0, max(1, n - 70), B)
            for b in range(B):
                for k, extra in ((first[b], 21.0), (min(first[b] + 64, n - 2), 20.0), (n - 1, 30.0)):
                    c0_lp[b, k], c1_lp[b, k] = -extra / 2, extra / 2
                    c0[b, k], c1[b, k] = -extra / 2, 10.0                                  # mode 0: an exact tie of the raw logit at the same cells
            self.want, self.want_lp = first, first
        if family == "exact_tie":                 # the same bits at three cells of different lanes and strides; the lowest index wins
            first = g.integers(0, max(1, n - 70), B)
            for b in range(B):
                for k in (first[b], min(first[b] + 64, n - 2), n - 1):
                    c0[b, k], c1[b, k], c0_lp[b, k], c1_lp[b, k] = -1.25, 6.5, -1.25, 6.5
            self.want, self.want_lp = first, first
        if family == "nan_first":                 # a NaN is the maximum, the first NaN wins; a NaN in class 0 counts for the softmax only
            lo, hi = g.integers(1, max(2, n // 2), B), g.integers(n // 2, n, B)
            for b in range(B):
                c1[b, hi[b]] = c1_lp[b, hi[b]] = np.nan
                c0[b, lo[b]] = c0_lp[b, lo[b]] = np.nan
                if b % 2:
                    c1[b, n - 1] = c1_lp[b, n - 1] = np.nan
            self.want, self.want_lp = hi, np.minimum(lo, hi)
        self.cls = f(np.stack([c0, c1], 1).reshape(B, 2, S, S))
        self.cls_lp = f(np.stack([c0_lp, c1_lp], 1).reshape(B, 2, S, S))
        self.loc = f(g.uniform(-1.5, 1.5, (B, 2, S, S)))
        self.loc_lp = f(g.uniform(-1, 1, (B, 4, S, S)))
        self.temp_cx, self.temp_cy = f(63.5 + g.uniform(-10, 10, B)), f(63.5 + g.uniform(-10, 10, B))
        self.search_poly = f(g.uniform(60, 190, (B, 4, 2)))
        self.w = {k: f(g.uniform(-1, 1, s)) for k, s in (("polar", (B, 2)), ("scale", (B,)), ("rot", (B,)), ("affine_m", (B, 2, 3)),
                                                        ("affine_m_lt0", (B, 2, 3)), ("pred_points", (B, 3, 4)))}

    def sub(self, b):
        """sample b alone, as a case of B = 1"""
        c = object.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.name, c.B = f"{self.name}[{b}]", 1
        for k in ("cls", "cls_lp", "loc", "loc_lp", "temp_cx", "temp_cy", "search_poly"):
            setattr(c, k, np.ascontiguousarray(getattr(self, k)[b:b + 1]))
        c.w = {k: np.ascontiguousarray(v[b:b + 1]) for k, v in self.w.items()}
        c.want = c.want_lp = None
        return c

    # -- the forward and the closed-form backward in one arithmetic; `variant` simulates a wrong kernel (fp32 numpy only)
    def evaluate(self, A, variant=None, polar_override=None, points_weight=True):
        """polar_override: the polar the matrices are built from (the fixture feeds the reference its own fp32 polar); points_weight=False: no
        upstream gradient on pred_points (the fixture's scalar has none: :409-415 are lines of the model's forward, not a function)."""
        B, S, n = self.B, self.S, self.n
        ar = np.arange(B)
        out = {}

        def index(mode, cls):
            B_ = cls.shape[0]
            c0, c1 = cls[:, 0].reshape(B_, -1), cls[:, 1].reshape(B_, -1)
            if variant == "scan_stops_at_full_strides" and n >= 64:
                c0, c1 = c0[:, :n - n % 64], c1[:, :n - n % 64]
            soft = mode == 1
            if (variant, mode) in (("polar_pick_over_softmax", 0), ("lp_pick_over_raw_logit", 1)):
                soft = not soft
            v = softmax_class1(c0, c1) if soft else c1
            if variant == "tie_break_ge":                       # the last of the equal maxima (NaN: the last NaN)
                key = np.where(np.isnan(v), np.inf, v)
                return v.shape[1] - 1 - np.argmax(key[:, ::-1], 1)
            return np.argmax(v, 1)

        def point(best):
            ori = -(S // 2) * STRIDE
            x, y = ori + STRIDE * (best % S), ori + STRIDE * (best // S)
            if variant == "points_xy_swapped":
                x, y = y, x
            return A.inp(x.astype(np.float64)), A.inp(y.astype(np.float64))

        best = index(0, self.cls)
        loc = A.inp(self.loc)
        flat = loc.reshape(B, 2, n)
        px, py = point(best)
        p0, p1 = r_polar(A, px, py, flat[ar, 0, best], flat[ar, 1, best], float(STRIDE))
        out["best_idx"], out["polar"] = best, A.stack([p0, p1], (2,))
        if polar_override is not None:
            p0, p1 = A.inp(polar_override[:, 0]), A.inp(polar_override[:, 1])

        best_lp = index(1, self.cls_lp)
        loc_lp = A.inp(self.loc_lp)
        flat_lp = loc_lp.reshape(B, 4, n)
        px, py = point(best_lp)
        scale, rot = r_lp(A, px, py, flat_lp[ar, 0, best_lp], flat_lp[ar, 1 if variant == "rot_from_channel_1" else 2, best_lp], float(STRIDE_LP))
        out["best_idx_lp"], out["scale"], out["rot"] = best_lp, scale, rot

        half = OUT_SZ / 2
        one, zero = A.inp(np.ones(B)), A.inp(np.zeros(B))
        tcx, tcy = A.inp(self.temp_cx), A.inp(self.temp_cy)
        ops0 = r_operands(A, 0, half, half, p0, p1, scale, True, IN_SZ, OUT_SZ)
        inv = scale if variant == "lt0_scale_not_inverted" else A.div(1.0, scale)
        nrot = rot if variant == "lt0_rot_sign_kept" else -rot
        ops1 = r_operands(A, 1, half, half, p0, p1, inv, False, 0.0 if variant == "in_sz_half_shift_dropped" else IN_SZ, OUT_SZ)
        m0, m1 = r_rows(A, ops0, rot, variant), r_rows(A, ops1, nrot, variant)
        m2 = r_rows(A, r_operands(A, 0, tcx, tcy, zero, zero, one, True, IN_SZ, OUT_SZ), zero, variant)
        m3 = r_rows(A, r_operands(A, 1, tcx, tcy, zero, zero, one, False, 0.0 if variant == "in_sz_half_shift_dropped" else IN_SZ, OUT_SZ), zero, variant)
        poly = A.inp(self.search_poly)
        xs, ys = [poly[:, j, 0] for j in range(4)], [poly[:, j, 1] for j in range(4)]
        for k, m in zip(MATS, (m0, m1, m2, m3)):
            out[k] = A.stack(m, (2, 3))
        out["pred_points"], out["aug_sear_points"] = A.stack(r_poly(A, m1, xs, ys), (3, 4)), A.stack(r_poly(A, m3, xs, ys), (3, 4))

        # ---- backward, closed form.  The upstream gradients are the weights self.w (exact fp32 inputs).
        w = {k: A.inp(v) for k, v in self.w.items()}
        G0 = [w["affine_m"].reshape(B, 6)[:, q] for q in range(6)]
        G1 = [w["affine_m_lt0"].reshape(B, 6)[:, q] for q in range(6)]
        gp = w["pred_points"]
        for r in range(2 if points_weight else 0):
            for j in range(4):
                G1[3 * r] = G1[3 * r] + gp[:, r, j] * xs[j]
                G1[3 * r + 1] = G1[3 * r + 1] + gp[:, r, j] * ys[j]
                G1[3 * r + 2] = G1[3 * r + 2] + gp[:, r, j]
        a0, a1 = r_affine_grads(A, ops0, rot, G0), r_affine_grads(A, ops1, nrot, G1)
        gs = (w["scale"] + a0[0] * A.const(OUT_SZ / IN_SZ)) - (a1[0] * inv) * inv
        gr = (w["rot"] + a0[1]) - a1[1]
        g0, g2 = r_lp_bwd(A, gs, gr, scale, float(STRIDE_LP))
        gpol = [a0[4] + a1[2], a0[5] + a1[3]]
        out["grad_polar"] = A.stack(gpol, (2,))
        out["grad_loc_lp"] = self._scatter(A, [(0, g0), (2, g2)], best_lp, 4, variant)
        q0, q2 = r_lp_bwd(A, w["scale"], w["rot"], scale, float(STRIDE_LP))                       # the pick alone: upstream on scale and rot only
        out["pick_grad_loc_lp"] = self._scatter(A, [(0, q0), (2, q2)], best_lp, 4, variant)
        wp = w["polar"]
        out["pick_grad_loc"] = self._scatter(A, [(0, -wp[:, 0] * float(STRIDE)), (1, -wp[:, 1] * float(STRIDE))], best, 2, variant)
        out["chain_grad_loc"] = self._scatter(A, [(0, -(wp[:, 0] + gpol[0]) * float(STRIDE)), (1, -(wp[:, 1] + gpol[1]) * float(STRIDE))], best, 2,
                                              variant)
        return out

    def _scatter(self, A, items, best, C, variant):
        """a [B,C,S,S] map that is zero except at cell `best` of the channels named in items"""
        B, n = self.B, self.n
        if variant == "gradient_one_cell_off":
            best = np.where(best + 1 < n, best + 1, best - 1)
        is_q = isinstance(A, Q)
        v, e = np.zeros((B, C, n)), np.zeros((B, C, n))
        for ch, val in items:
            if is_q:
                v[np.arange(B), ch, best], e[np.arange(B), ch, best] = val.v, val.e
            else:
                v[np.arange(B), ch, best] = val
        v = v.reshape(B, C, self.S, self.S)
        return Qv(v, e.reshape(v.shape)) if is_q else v.astype(A.dtype)

    @functools.lru_cache(maxsize=None)
    def truth(self):
        """{"exact": NP(float32) outputs, "q": Q outputs (value = the float64 truth, e = the bound)}"""
        with np.errstate(invalid="ignore"):
            return {"exact": self.evaluate(NP(np.float32)), "q": self.evaluate(Q()), "f64": self.evaluate(NP(np.float64))}

    def torch_run(self, dtype, device="cpu", pick=None, warps=None):
        """PyTorch's own run of the restated lines with autograd: every key of evaluate() (the gradients through torch.autograd.grad of the weighted
        scalars).  pick / warps: replacements for the forward of :377 / :390-415 (the GPU test passes the package's functions)."""
        A = TorchA(dtype, device)
        B, n, ar = self.B, self.n, torch.arange(self.B, device=device)
        T = lambda a: torch.as_tensor(a, dtype=dtype, device=device)
        loc, loc_lp = T(self.loc).requires_grad_(True), T(self.loc_lp).requires_grad_(True)
        cls, cls_lp = (torch.as_tensor(a, device=device) for a in (self.cls, self.cls_lp))      # the scores are fp32 in every run: they choose, no more
        w = {k: T(v) for k, v in self.w.items()}
        out = {}
        table = T(analytic_points(STRIDE, self.S))
        pt = lambda best: (table[best, 0], table[best, 1])
        if pick is None:
            best = torch.argmax(cls.reshape(B, 2, n)[:, 1], 1)
            px, py = pt(best)
            flat = (loc * STRIDE).reshape(B, 2, n)
            polar = torch.stack(r_polar(A, px, py, flat[ar, 0, best], flat[ar, 1, best], 1.0), 1)
        else:
            polar, best = pick(cls, loc)
        out["best_idx"], out["polar"] = best, polar
        half = OUT_SZ / 2
        if warps is None:
            best_lp = torch.argmax(cls_lp.reshape(B, 2, n).permute(0, 2, 1).softmax(2)[:, :, 1], 1)
            px, py = pt(best_lp)
            flat_lp = loc_lp.reshape(B, 4, n)
            scale, rot = r_lp(A, px, py, flat_lp[ar, 0, best_lp], flat_lp[ar, 2, best_lp], STRIDE_LP)
            one, zero, tcx, tcy = torch.ones_like(scale), torch.zeros_like(scale), T(self.temp_cx), T(self.temp_cy)
            p0, p1 = polar[:, 0], polar[:, 1]
            m = [r_rows(A, r_operands(A, 0, half, half, p0, p1, scale, True, IN_SZ, OUT_SZ), rot),
                 r_rows(A, r_operands(A, 1, half, half, p0, p1, 1 / scale, False, IN_SZ, OUT_SZ), -rot),
                 r_rows(A, r_operands(A, 0, tcx, tcy, zero, zero, one, True, IN_SZ, OUT_SZ), zero),
                 r_rows(A, r_operands(A, 1, tcx, tcy, zero, zero, one, False, IN_SZ, OUT_SZ), zero)]
            res = {"scale": scale, "rot": rot, "best_idx_lp": best_lp}
            res.update({k: A.stack(v, (2, 3)) for k, v in zip(MATS, m)})
            hmg = torch.cat([T(self.search_poly).permute(0, 2, 1), torch.ones(B, 1, 4, dtype=dtype, device=device)], 1)
            last = torch.tensor([0, 0, 1], dtype=dtype, device=device).repeat(B, 1, 1)
            res["pred_points"] = torch.bmm(torch.cat([res["affine_m_lt0"], last], 1), hmg)
            res["aug_sear_points"] = torch.bmm(torch.cat([res["affine_m_lt0_aug"], last], 1), hmg)
        else:
            res = warps(cls_lp, loc_lp, polar)
        out.update(res)
        pick_scalar = (w["scale"] * out["scale"]).sum() + (w["rot"] * out["rot"]).sum()
        full = pick_scalar + sum((w[k] * out[k]).sum() for k in ("affine_m", "affine_m_lt0", "pred_points"))
        out["pick_grad_loc"], = torch.autograd.grad((w["polar"] * polar).sum(), loc, retain_graph=True)
        out["pick_grad_loc_lp"], = torch.autograd.grad(pick_scalar, loc_lp, retain_graph=True)
        out["grad_loc_lp"], out["grad_polar"] = torch.autograd.grad(full, (loc_lp, polar), retain_graph=True)
        out["chain_grad_loc"], = torch.autograd.grad(full + (w["polar"] * polar).sum(), loc)
        return {k: v.detach() for k, v in out.items()}


def _ratio(v, q, ctx):
    """max error / bound of v against the Q value q; where no rounding is on the path (bound 0) the values must be equal"""
    err = np.abs(v.astype(np.float64) - q.v)
    assert not np.isnan(err).any(), ctx
    zero = q.e == 0
    assert (err[zero] == 0).all(), ctx + ("an element with no rounding on its path differs",)
    if not (~zero).any():
        return 0.0
    r = float((err[~zero] / q.e[~zero]).max())
    assert r <= 1.0, ctx + (r,)
    return r


def check(got, case, keys=None, what=""):
    """Hold `got` (name -> array or tensor) to the truth of `case`: the EXACT names bit for bit against NP(float32) (pick_grad_loc_lp: channel 2, and
    zero wherever the truth is zero), the BOUNDED names within the Q bound of the float64 truth.  Returns the worst ratio error / bound."""
    tr = case.truth()
    worst = 0.0
    for k, v in got.items():
        if keys is not None and k not in keys:
            continue
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        if k in ("best_idx", "best_idx_lp"):
            assert np.array_equal(v.astype(np.int64), tr["exact"][k]), (what, case.name, k)
            assert ((v >= 0) & (v < case.n)).all()
            continue
        ex = np.asarray(tr["exact"][k], dtype=np.float32)
        assert v.shape == ex.shape, (what, case.name, k, v.shape, ex.shape)
        if k in EXACT:
            assert np.array_equal(v.astype(np.float32).view(np.int32), ex.view(np.int32)), (what, case.name, k)
            continue
        worst = max(worst, _ratio(v, tr["q"][k], (what, case.name, k)))
        if k == "pick_grad_loc_lp":
            assert np.array_equal(v[:, 2].astype(np.float32).view(np.int32), ex[:, 2].view(np.int32)), (what, case.name, k, "channel 2")
    return worst


def _cases():
    cs = []
    for S in (1, 2, 8, 9, 13, 25):
        cs.append(Case(f"every_cell_S{S}", "every_cell", S * S, S, 100 + S, golden=S <= 13))
    for fam, seed in (("exact_tie", 200), ("saturated", 300), ("nan_first", 400)):
        for S in (13, 25):
            cs.append(Case(f"{fam}_S{S}", fam, 4, S, seed + S))
    for B in (1, 2, 3, 65):
        cs.append(Case(f"separated_B{B}", "separated", B, 13, 500 + B))
    cs.append(Case("step_B32", "separated", 32, 13, 600))
    return {c.name: c for c in cs}


CASES = _cases()
CASE_NAMES = tuple(CASES)

# which family catches which wrong kernel
MUTATION_CASES = {
    "polar_pick_over_softmax": "separated_B3",
    "lp_pick_over_raw_logit": "separated_B3",
    "tie_break_ge": "exact_tie_S13",
    "scan_stops_at_full_strides": "every_cell_S13",
    "rot_from_channel_1": "separated_B3",
    "lt0_scale_not_inverted": "separated_B3",
    "lt0_rot_sign_kept": "separated_B3",
    "in_sz_half_shift_dropped": "separated_B3",
    "scale_h_division_dropped": "separated_B3",
    "gradient_one_cell_off": "separated_B3",
    "points_xy_swapped": "every_cell_S13",
}
MUTATIONS = tuple(MUTATION_CASES)

# the stand-alone matrices: both kinds, scale_h both ways, the centre as numbers and as vectors, over the range lp_pick can produce at S = 13
AFFINE_ROTS = (0.0, np.pi / 2, -np.pi / 2, 2.4, -2.4)
AFFINE_SCALES = (0.2, 1.0, 4.8)
AFFINE_FORMS = tuple((kind, scale_h, vec) for kind in (0, 1) for scale_h in ((True, False) if kind == 0 else (False,)) for vec in (False, True))


class AffineCase:
    """every (rot, scale) pair of the lists above as one batch of 15, for one (kind, scale_h, centre form)"""

    def __init__(self, kind, scale_h, vec):
        self.kind, self.scale_h, self.vec = kind, scale_h, vec
        self.name = f"kind{kind}_scale_h{int(scale_h)}_{'vector' if vec else 'scalar'}"
        g = np.random.default_rng(700 + 4 * kind + 2 * int(scale_h) + int(vec))
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        self.rot = f([r for r in AFFINE_ROTS for _ in AFFINE_SCALES])
        self.scale = f([s for _ in AFFINE_ROTS for s in AFFINE_SCALES])
        self.B = B = len(self.rot)
        self.nm = f(g.uniform(-40, 40, (B, 2)))
        self.cx, self.cy = (f(63.5 + g.uniform(-10, 10, B)), f(63.5 + g.uniform(-10, 10, B))) if vec else (70.25, 58.5)
        self.grad = f(g.uniform(-1, 1, (B, 2, 3)))

    def evaluate(self, A):
        vec = self.vec
        cx, cy = (A.inp(self.cx), A.inp(self.cy)) if vec else (self.cx, self.cy)
        nm, scale, rot, G = A.inp(self.nm), A.inp(self.scale), A.inp(self.rot), A.inp(self.grad).reshape(self.B, 6)
        ops = r_operands(A, self.kind, cx, cy, nm[:, 0], nm[:, 1], scale, self.scale_h, IN_SZ, OUT_SZ)
        g = r_affine_grads(A, ops, rot, [G[:, q] for q in range(6)])
        return {"out": A.stack(r_rows(A, ops, rot), (2, 3)), "grad_nm": A.stack([g[4], g[5]] if self.kind == 0 else [g[2], g[3]], (2,)),
                "grad_scale": g[0] * A.const(OUT_SZ / IN_SZ) if self.kind == 0 else g[0], "grad_rot": g[1]}

    def torch_run(self, dtype, device="cpu", fn=None):
        A = TorchA(dtype, device)
        T = lambda a: torch.as_tensor(a, dtype=dtype, device=device)
        nm, scale, rot = (T(v).requires_grad_(True) for v in (self.nm, self.scale, self.rot))
        cx, cy = (T(self.cx), T(self.cy)) if self.vec else (self.cx, self.cy)
        if fn is None:
            out = A.stack(r_rows(A, r_operands(A, self.kind, cx, cy, nm[:, 0], nm[:, 1], scale, self.scale_h, IN_SZ, OUT_SZ), rot), (2, 3))
        else:
            out = fn(self, cx, cy, nm, scale, rot)
        g = torch.autograd.grad((out * T(self.grad)).sum(), (nm, scale, rot))
        return {"out": out.detach(), "grad_nm": g[0], "grad_scale": g[1], "grad_rot": g[2]}

    @functools.lru_cache(maxsize=None)
    def truth(self):
        return self.evaluate(Q())

    def check(self, got, what=""):
        tr, worst = self.truth(), 0.0
        for k, v in got.items():
            v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            q = tr[k]
            assert v.shape == q.v.shape, (what, self.name, k)
            worst = max(worst, _ratio(v, q, (what, self.name, k)))
        return worst


AFFINE_CASES = {c.name: c for c in (AffineCase(*f) for f in AFFINE_FORMS)}
AFFINE_NAMES = tuple(AFFINE_CASES)
