"""Shared by tests/test_gpu_xcorr_bwd.py and tests/test_xcorr_bwd_host.py: the shapes, the float64 reference, the magnitudes of the bound, the form rule
of csrc/xcorr_bwd.hip restated, the fixtures and the case tables of the depthwise correlations' backward (hdn_xcorr_depthwise_bwd_f32).  Nothing here
launches a kernel except run().

The reference: torch autograd in float64 through xcorr_cases.direct_sum (tap by tap, the pad by index arithmetic) - no formula of the kernel's.
The exact fixture: integer x, k and g in [-3, 3]; every partial sum of either gradient is an integer, and exactness_headroom() computes that the largest
possible one stays below 2^24, so fp32 is exact in any order and the kernel must be torch.equal to float64.
The position fixture: plane p has g = a single 1 at output position p, over xcorr_cases.pattern taps and image (multiples of a power of two, at most 32,
every element of a plane different): gk[u][v] is then xp[i + u][j + v] and gx the taps scattered through the preimage rule of include/hdn_hip.h, both
built here by index arithmetic without a convolution."""
import functools
from collections import namedtuple

import numpy as np
import torch

import xcorr_cases as XC

SEED = 20261019
ABS_TOL, REL_TOL = XC.ABS_TOL, XC.REL_TOL                # |hip - f64| <= 1e-4 + 2e-6 M, M = the same backward on |x|, |k|, |g|, largest of the plane
LDS_LIMIT_BYTES = 60 * 1024                              # csrc/xcorr_bwd.hip: (HP WP + Hk Wk + Ho Wo) 4 bytes <= 60 KiB -> the LDS form
FORM_LDS, FORM_GLOBAL = 0, 1

Shape = namedtuple("Shape", "name circular Hx Wx Hk Wk")


def _from_kind(name):
    K = XC.KINDS[name]
    return Shape(name, K.circular, K.Hx, K.Wx, K.Hk, K.Wk)


def _circ(Hx, Wx, Hk, Wk):
    return Shape(f"circ_{Hx}x{Wx}_{Hk}x{Wk}", True, Hx, Wx, Hk, Wk)


# the degenerate circular planes (no pad at all; one column: both column rules at once; a pad as large as the plane) and the 15 x 15 log-polar shape
DEGENERATE = (_circ(1, 1, 1, 1), _circ(3, 1, 2, 1), _circ(2, 2, 3, 3), _circ(15, 15, 15, 15))
# both sides of the form switch, plain and circular (the circular planes pad to the plain ones, 96 x 97): 9312 + 372 + 5676 = 15360 floats = 60 KiB
# stays in LDS, 9312 + 35 + 6014 = 15361 does not
SWITCH = (Shape("gen_96x97_31x12", False, 96, 97, 31, 12), Shape("gen_96x97_35x1", False, 96, 97, 35, 1),
          Shape("genc_48x49_31x12", True, 48, 49, 31, 12), Shape("genc_48x49_35x1", True, 48, 49, 35, 1))
SHAPES = {s.name: s for s in tuple(_from_kind(n) for n in ("prod29", "cfg5", "circ13") + XC.GENERIC_SMALL) + DEGENERATE + SWITCH}

EXACT_KINDS = ("prod29", "cfg5", "circ13") + XC.GENERIC_SMALL + tuple(s.name for s in DEGENERATE)
SWITCH_KINDS = tuple(s.name for s in SWITCH)
SWITCH_PLANES = 2
POSITION_KINDS = ("prod29", "circ13", "genc_6x7_4x6", "genc_5x4_9x8", "gen_9x8_4x1")
OFFSETS = [(0, 0, 0, 0, 0), (1, 2, 3, 1, 2)]            # float offsets of the x, k, g, gx and gk base pointers inside a 16-byte line


def plane_counts(kind):
    return tuple(range(1, 10)) + ((19,) if kind in ("prod29", "circ13") else ())


def geometry(S):
    """(ph, pw, HP, WP, Ho, Wo)."""
    ph, pw = (S.Hx // 2, S.Wx // 2) if S.circular else (0, 0)
    HP, WP = S.Hx + 2 * ph, S.Wx + 2 * pw
    return ph, pw, HP, WP, HP - S.Hk + 1, WP - S.Wk + 1


def form(S):
    """The rule of hdn_xcorr_bwd_form, restated."""
    _, _, HP, WP, Ho, Wo = geometry(S)
    return FORM_LDS if 4 * (HP * WP + S.Hk * S.Wk + Ho * Wo) <= LDS_LIMIT_BYTES else FORM_GLOBAL


# ----------------------------------------------------------------------------------------------------------------- references
def backward_ref(x, k, g, circular, dtype=torch.float64):
    """(gx, gk) of sum(direct_sum(x, k) * g) by torch autograd in `dtype`, on [P, H, W] tensors."""
    xr, kr = x.detach().to(dtype).requires_grad_(True), k.detach().to(dtype).requires_grad_(True)
    XC.direct_sum(xr, kr, circular, dtype=dtype).backward(g.to(dtype))
    return xr.grad, kr.grad


def magnitudes(x, k, g, circular):
    """(Mx [P], Mk [P]): the same backward on |x|, |k|, |g|, the largest element of each plane - the sum of the absolute terms of the worst gradient."""
    mx, mk = backward_ref(x.abs(), k.abs(), g.abs(), circular)
    return mx.amax(dim=(1, 2)), mk.amax(dim=(1, 2))


def bound(M):
    return ABS_TOL + REL_TOL * M.double()


def exactness_headroom(x, k, g, circular):
    """The largest possible |partial sum| of either gradient over 2^24: below 1, fp32 is exact in any summation order, fused or not."""
    mx, mk = magnitudes(x, k, g, circular)
    return float(torch.maximum(mx.max(), mk.max())) / 2.0 ** 24


# ----------------------------------------------------------------------------------------------------------------- the exact fixture
@functools.lru_cache(maxsize=None)
def exact_problem(kind, planes):
    """(x [P, Hx, Wx], k [P, Hk, Wk], g [P, Ho, Wo], fp32 integers in [-3, 3]; gx, gk: float64 autograd), seeded per shape and plane count."""
    S = SHAPES[kind]
    _, _, _, _, Ho, Wo = geometry(S)
    rng = np.random.default_rng(SEED + 1000003 * planes + 10007 * S.Hx + 1009 * S.Wx + 101 * S.Hk + 11 * S.Wk + 5 * S.circular)
    x, k, g = (torch.from_numpy(rng.integers(-3, 4, (planes, h, w)).astype(np.float32)) for h, w in ((S.Hx, S.Wx), (S.Hk, S.Wk), (Ho, Wo)))
    gx, gk = backward_ref(x, k, g, S.circular)
    return x, k, g, gx, gk


def exact_table():
    """Every (kind, planes) the exact GPU test runs."""
    return [(kind, P) for kind in EXACT_KINDS for P in plane_counts(kind)] + [(kind, SWITCH_PLANES) for kind in SWITCH_KINDS]


# ----------------------------------------------------------------------------------------------------------------- the position fixture
@functools.lru_cache(maxsize=None)
def position_problem(kind):
    """(x, k, g, want_gx, want_gk): plane p = output position (i, j) = divmod(p, Wo), g[p] a single 1 there.
    want_gk[p][u][v] = xp[i + u][j + v] = x[(i + u - ph) mod Hx][clamp(j + v - pw)].
    want_gx[p][r][s] = the sum of k[P - i][Q - j] over the padded positions (P, Q) that are copies of (r, s) and whose tap exists:
    rows P in {r + ph - Hx, r + ph, r + ph + Hx} within [0, HP); columns [0, pw] at s == 0, joined with [pw + Wx - 1, WP) at s == Wx - 1, else s + pw."""
    S = SHAPES[kind]
    ph, pw, HP, WP, Ho, Wo = geometry(S)
    P = Ho * Wo
    x, k = XC.pattern(P, S.Hx, S.Wx), XC.pattern(P, S.Hk, S.Wk)
    g = XC.impulses(list(range(P)), Ho, Wo)
    want_gx, want_gk = torch.zeros(P, S.Hx, S.Wx, dtype=torch.float64), torch.zeros(P, S.Hk, S.Wk, dtype=torch.float64)
    for p in range(P):
        i, j = divmod(p, Wo)
        rows = [(i + u - ph) % S.Hx for u in range(S.Hk)]
        cols = [min(max(j + v - pw, 0), S.Wx - 1) for v in range(S.Wk)]
        want_gk[p] = x[p][rows][:, cols].double()
        for r in range(S.Hx):
            prow = [r + ph + t * S.Hx for t in (-1, 0, 1)]
            for s in range(S.Wx):
                pcol = set([s + pw] if 0 < s < S.Wx - 1 else [])
                if s == 0:
                    pcol |= set(range(0, pw + 1))
                if s == S.Wx - 1:
                    pcol |= set(range(pw + S.Wx - 1, WP))
                want_gx[p, r, s] = sum(float(k[p, Pr - i, Q - j]) for Pr in prow if 0 <= Pr < HP and 0 <= Pr - i < S.Hk
                                       for Q in sorted(pcol) if 0 <= Q - j < S.Wk)
    return x, k, g, want_gx, want_gk


# ----------------------------------------------------------------------------------------------------------------- random data
RANDOM_SHAPES = (Shape("prod29", False, 29, 29, 5, 5), Shape("circ13", True, 13, 13, 13, 13), Shape("cfg5", False, 35, 35, 5, 5),
                 Shape("circ_15x15_15x15", True, 15, 15, 15, 15))
RANDOM_PLANES = 128


@functools.lru_cache(maxsize=None)
def random_problem(kind):
    """relu(N(0, 1)) features and taps, N(0, 1) g, 128 planes; (x, k, g, gx, gk float64, Mx, Mk)."""
    S = SHAPES[kind]
    _, _, _, _, Ho, Wo = geometry(S)
    rng = np.random.default_rng(SEED + 77 * S.Hx + S.Hk)
    x = torch.from_numpy(np.maximum(rng.standard_normal((RANDOM_PLANES, S.Hx, S.Wx), dtype=np.float32), 0))
    k = torch.from_numpy(np.maximum(rng.standard_normal((RANDOM_PLANES, S.Hk, S.Wk), dtype=np.float32), 0))
    g = torch.from_numpy(rng.standard_normal((RANDOM_PLANES, Ho, Wo), dtype=np.float32))
    gx, gk = backward_ref(x, k, g, S.circular)
    mx, mk = magnitudes(x, k, g, S.circular)
    return x, k, g, gx, gk, mx, mk


def worst_ratio(got, truth, M):
    """max |got - truth| / (1e-4 + 2e-6 M) over all elements, M per plane."""
    return float(((got.double() - truth.double()).abs() / bound(M).view(-1, 1, 1)).max())


# ----------------------------------------------------------------------------------------------------------------- on the device
BYTE = 0xA5
FILL = float(np.frombuffer(bytes([BYTE] * 4), dtype=np.float32)[0])     # the fp32 whose four bytes are 0xA5


def run(kind, x, k, g, dev, offsets=(0, 0, 0, 0, 0), need_x=True, need_k=True, margin=8):
    """One raw call of hdn_xcorr_depthwise_bwd_f32 on [P, H, W] host tensors as B = 1, C = P, the five base pointers `offsets` floats into a 16-byte
    line.  The output buffers hold NaN where a result belongs and 0xA5 bytes in `margin` floats around it; an output that is not asked for is passed
    as NULL and its buffer holds 0xA5 everywhere.  Returns (gx | None, gk | None on the CPU, [P, H, W]; the two whole buffers on the CPU)."""
    from hdn_amd import _lib
    S = SHAPES[kind]
    P = x.shape[0]
    xd, _ = XC.at_offset(x, offsets[0], dev)
    kd, _ = XC.at_offset(k, offsets[1], dev)
    gd, _ = XC.at_offset(g, offsets[2], dev)
    gxv, gxb = XC.at_offset(P * S.Hx * S.Wx, offsets[3], dev, margin=margin, fill=FILL)
    gkv, gkb = XC.at_offset(P * S.Hk * S.Wk, offsets[4], dev, margin=margin, fill=FILL)
    if not need_x:
        gxb.fill_(FILL)
    if not need_k:
        gkb.fill_(FILL)
    for t, o in zip((xd, kd, gd, gxv, gkv), (offsets[0], offsets[1], offsets[2], margin + offsets[3], margin + offsets[4])):
        assert t.data_ptr() % 16 == 4 * (o % 4)
    rc = _lib.load().hdn_xcorr_depthwise_bwd_f32(_lib.ptr(xd), _lib.ptr(kd), _lib.ptr(gd), _lib.ptr(gxv) if need_x else None,
                                                 _lib.ptr(gkv) if need_k else None, int(S.circular), 1, P, S.Hx, S.Wx, S.Hk, S.Wk, _lib.stream_ptr(dev))
    _lib.check(rc, "hdn_xcorr_depthwise_bwd_f32")
    torch.cuda.synchronize(dev)
    gx = gxv.cpu().view(P, S.Hx, S.Wx) if need_x else None
    gk = gkv.cpu().view(P, S.Hk, S.Wk) if need_k else None
    return gx, gk, (gxb.cpu(), gkb.cpu())


def untouched(buf, lo, hi):
    """Is every byte of the whole buffer outside the floats [lo, hi) still 0xA5?"""
    raw = buf.numpy().view(np.uint8).reshape(-1, 4)
    return bool((raw[:lo] == BYTE).all()) and bool((raw[hi:] == BYTE).all())


def first_difference(got, truth):
    """None, or where got [P, H, W] (fp32) first differs from truth (float64 holding fp32-exact values)."""
    bad = ~(got.double() == truth.double())
    if not bool(bad.any()):
        return None
    p, r, c = bad.nonzero()[0].tolist()
    return f"{int(bad.sum())} of {bad.numel()} differ; first (plane, row, column) = ({p}, {r}, {c}): got {float(got[p, r, c])!r}, want {float(truth[p, r, c])!r}"
