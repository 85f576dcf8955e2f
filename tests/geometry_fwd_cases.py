"""Shared by tests/test_gpu_geometry_fwd.py and tests/test_geometry_fwd_host.py: the fixtures, the float64 truths and the raw-ABI runners of the
geometry forwards - warp_kernel / dlt_warp_kernel / dlt_solve_kernel / l1_score_kernel (csrc/dlt_warp.hip), logpolar_kernel (csrc/logpolar.hip) and
refine_warp_kernel (csrc/refine_warp.hip).  The restatements, at_offset / untouched / first_difference / worst_ratio / k_bound and the exact fixtures
of the backward suite come from tests/geometry_bwd_cases.py.  Nothing here launches a kernel except the run_* functions.

Truths.  Exact fixtures (integer images, dyadic parameters): float64 through the restatements, compared by torch.equal; the host test proves float64 ==
fp32 == the oracle on each of them.  Everything else: |got - truth| <= K M per element with M = sum |w_i| |I_i| over the four taps and K =
max(4 r_ref, 2e-6) (k_bound), r_ref = the worst ratio of the reference formulation's own fp32 CPU evaluation of the same fixture; the four taps are
the cells that the fp32 coordinates pick by the kernel's own statements (warp_xy32 / logpolar_coords in fp32), the weights and the sum are float64.
An element whose truth is not finite or whose M is 0 must match bit for bit (NaN equal to NaN).

The float -> int rule of the warp (f2i_x86: out of range and NaN -> INT_MIN, then `+ 1` as an unsigned add, then the clamp) is restated here on
integers and never left to the host's conversion.

fma in fp32 is restated as fp32(float64(a) float64(b) + float64(c)): the product is exact in float64 and the sum is rounded twice, which differs from
one rounding only when the float64 sum lands on an fp32 tie; the host test counts such sums on every fixture (none) and compares warp_xy32 with
torch's fp32 path.  Where a proof needs
the single rounding (normalise_rs, dlt_eliminate) the fma is evaluated on fractions."""
import functools
import os
from fractions import Fraction

import numpy as np
import torch

import geometry_bwd_cases as GC
from geometry_bwd_cases import (BYTE, DLT_CORNERS, DLT_POINT_ORDER, FILL, LOGPOLAR_EXACT, OFFSETS, PAD, ROOT, SEED, WARP_THETAS, at_offset,  # noqa: F401 (dlt_excess, k_bound: for the tests)
                                dlt_excess, dlt_rs, first_difference, k_bound, logpolar_coords, logpolar_rs, transformer_rs, untouched, warp_coords,
                                worst_ratio)

f32, f64 = np.float32, np.float64
INT_MIN = -2 ** 31

# ================================================================================================================= launch constants, restated
HDN_BLOCK, HDN_WAVE = 256, 64
WARP_PX_PER_THREAD = 4
WARP_PX_PER_BLOCK = HDN_BLOCK * WARP_PX_PER_THREAD        # 1,024 pixels per workgroup of warp_kernel / dlt_warp_kernel
L1_THREADS, L1_PER_THREAD = 1024, 16                       # one pass of l1_score_kernel: 16,384 elements
L1_PASS = L1_THREADS * L1_PER_THREAD
RW_BW, RW_BH = 64, 16                                      # OpenCV's block walk at 127 x 127
RW_CAP = 64                                                # refine_warp_kernel: at most 64 workgroups per sample, then a grid-stride loop
DLT_LANES = 8                                              # lanes per solve
DLT_PER_WAVE, DLT_PER_BLOCK = HDN_WAVE // DLT_LANES, HDN_BLOCK // DLT_LANES

CSRC = os.path.join(ROOT, "hdn_amd", "csrc")
# (file, text that must stand in it): the constants above as the sources spell them
SOURCE_FACTS = (
    ("hdn_common.h", f"#define HDN_WAVE {HDN_WAVE}"), ("hdn_common.h", f"#define HDN_BLOCK {HDN_BLOCK}"),
    ("geometry.h", f"constexpr int WARP_PX_PER_THREAD = {WARP_PX_PER_THREAD};"),
    ("geometry.h", "constexpr int WARP_PX_PER_BLOCK = HDN_BLOCK * WARP_PX_PER_THREAD;"),
    ("dlt_warp.hip", f"constexpr int L1_THREADS = {L1_THREADS}, L1_PER_THREAD = {L1_PER_THREAD};"),
    ("dlt_warp.hip", "base += L1_THREADS * L1_PER_THREAD"), ("dlt_warp.hip", "min(base + q * L1_THREADS + (int)threadIdx.x, n - 1)"),
    ("dlt_warp.hip", f"const int groups_per_block = HDN_BLOCK / {DLT_LANES};"), ("geometry.h", f"__shfl_xor(best, m, {DLT_LANES})"),
    ("dlt_warp.hip", "const int r = lane & %d;" % (DLT_LANES - 1)), ("dlt_warp.hip", "dim3 grid(hdn::cdiv(H * W, hdn::WARP_PX_PER_BLOCK), B);"),
    ("geometry.h", "if (ob > best || (ob == best && oi < bidx))"), ("dlt_warp.hip", "if (v > best) { best = v; p = r; }"),
    ("geometry.h", "(fabsf(t) >= 1e-7f) ? 0.0f : 1.0f"), ("dlt_warp.hip", "return fabsf(p.t) > 1e-7f;"),
    ("geometry.h", "return p == 2 ? 3 : (p == 3 ? 2 : p);"), ("geometry.h", "(f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : (int)0x80000000"),
    ("logpolar.hip", "dim3 grid(hdn::cdiv(S * S, HDN_BLOCK), B);"), ("logpolar.hip", "(e_ok && s_ok) ? pl[y1 * W + x1] : 0.f"),
    ("cv_warp.h", f"constexpr int RW_BW = {RW_BW}, RW_BH = {RW_BH};"),
    ("cv_warp.h", f"int bh = H < {RW_BH} ? H : {RW_BH};"),
    ("cv_warp.h", f"int bw = {RW_BW * RW_BH} / bh < W ? {RW_BW * RW_BH} / bh : W;"),
    ("cv_warp.h", f"bh = {RW_BW * RW_BH} / bw < H ? {RW_BW * RW_BH} / bw : H;"),
    ("refine_warp.hip", f"dim3(blocks < {RW_CAP} ? blocks : {RW_CAP}, B)"), ("refine_warp.hip", "pix += gridDim.x * HDN_BLOCK"),
)


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def cdiv(a, b):
    return (a + b - 1) // b


def rw_blocks(H, W):
    """(bw, bh) of hdn_refine_warp_f32: OpenCV's block geometry."""
    bh = min(RW_BH, H)
    bw = min(RW_BW * RW_BH // bh, W)
    return bw, min(RW_BW * RW_BH // bw, H)


def rw_grid(H, W):
    return min(cdiv(H * W, HDN_BLOCK), RW_CAP)


def where_warp(pix):
    return f"workgroup {pix // WARP_PX_PER_BLOCK}, thread {pix % HDN_BLOCK}, pass {(pix % WARP_PX_PER_BLOCK) // HDN_BLOCK} of {WARP_PX_PER_THREAD}"


def where_sampler(pix):
    return f"workgroup {pix // HDN_BLOCK}, thread {pix % HDN_BLOCK}"


def where_refine(pix, H, W):
    g, bw = rw_grid(H, W), rw_blocks(H, W)[0]
    return (f"workgroup {(pix // HDN_BLOCK) % g} of {g}, thread {pix % HDN_BLOCK}, grid-stride pass {pix // (g * HDN_BLOCK)}, "
            f"block column {(pix % W) // bw} (bw = {bw})")


def where_solve(b):
    return f"workgroup {b // DLT_PER_BLOCK}, wave {(b % DLT_PER_BLOCK) // DLT_PER_WAVE}, lane group {b % DLT_PER_WAVE}"


def difference(got, truth, where=None, nan_equal=False):
    """first_difference extended with the block arithmetic of the first differing element: where(index tuple) -> text.  nan_equal: a NaN in both
    places is no difference (truths that hold NaN or inf on purpose)."""
    g, t = got.double(), truth.double()
    if nan_equal:                                                                                 # a NaN on both sides becomes the same number
        both = g.isnan() & t.isnan()
        g, t = torch.where(both, torch.zeros_like(g), g), torch.where(both, torch.zeros_like(t), t)
    text = first_difference(g, t)
    if text is None or where is None:
        return text
    return text + f" [{where(tuple((~(g == t)).nonzero()[0].tolist()))}]"


def km_check(got, truth, M, K):
    """(worst |got - truth| / M over the regular elements, number of irregular elements that differ, index of the worst or first bad element).
    Regular: truth and M finite and M > 0.  Irregular elements must match bit for bit, NaN equal to NaN."""
    g, t, M = got.double(), truth.double(), M.double()
    reg = t.isfinite() & M.isfinite() & (M > 0)
    ratio = torch.where(reg, (g - t).abs() / torch.where(reg, M, torch.ones_like(M)), torch.zeros_like(M))
    ratio = torch.where(ratio.isnan(), torch.full_like(ratio, float("inf")), ratio)              # a NaN where the truth is finite
    same = (g == t) | (g.isnan() & t.isnan())
    n_bad = int((~reg & ~same).sum())
    flat = (~reg & ~same).reshape(-1).nonzero()
    at = int(flat[0]) if n_bad else int(ratio.reshape(-1).argmax())
    return float(ratio.max()), n_bad, tuple(np.unravel_index(at, tuple(g.shape)))


def _ints(rng, shape, lo=-3, hi=3):
    return torch.from_numpy(rng.integers(lo, hi + 1, shape).astype(np.float32))


def pattern(H, W, a=1, b=7, m=31):
    """1 + (a x + b y) mod m: every pixel differs from its eight neighbours (for a, b, a +- b not multiples of m)."""
    y, x = np.mgrid[0:H, 0:W]
    return torch.from_numpy((1 + (a * x + b * y) % m).astype(np.float32))


def pattern_planes(C, H, W):
    return torch.stack([pattern(H, W, *p) for p in ((1, 7, 31), (5, 3, 29), (2, 11, 23))[:C]])


# ================================================================================================================= projective warp
FMA_TIES = [0]                                             # float64 sums of _fma32 that landed on an fp32 tie (the host test asserts there are none)


def _fma32(a, b, c):
    """fma in fp32 through float64: the product is exact, the sum is rounded to float64 and then to fp32.  The two roundings can differ from one
    only if the float64 sum was itself rounded (TwoSum error != 0) and lies exactly half way between two fp32 values (low 29 mantissa bits
    1000...0); such sums are counted in FMA_TIES."""
    with np.errstate(all="ignore"):
        p, c = np.broadcast_arrays(np.asarray(a, f64) * np.asarray(b, f64), np.asarray(c, f64))
        s = p + c
        bp = s - p
        err = (p - (s - bp)) + (c - bp)                                                           # TwoSum: what the rounding to float64 dropped
    tie = (np.ascontiguousarray(s).view(np.int64) & (2 ** 29 - 1)) == 2 ** 28
    FMA_TIES[0] += int((np.isfinite(s) & tie & (err != 0)).sum())
    return s.astype(f32)


def grid_coord32(n):
    """grid_coord(i, n) of csrc/geometry.h for i = 0 .. n - 1 (= torch.linspace(-1, 1, n) on the CPU)."""
    step = f32(2.0) / f32(n - 1)
    i = np.arange(n)
    return np.where(i < n // 2, _fma32(step, i.astype(f32), f32(-1.0)), _fma32(-step, (n - 1 - i).astype(f32), f32(1.0))).astype(f32)


def warp_xy32(theta, H, W):
    """(t after the nudge, x, y) [B, H W] in fp32 by the statements of warp_point (csrc/geometry.h), every operation rounded once."""
    th = np.asarray(theta, f32).reshape(-1, 9)[:, :, None]
    gx = np.broadcast_to(grid_coord32(W)[None, :], (H, W)).reshape(1, -1)
    gy = np.broadcast_to(grid_coord32(H)[:, None], (H, W)).reshape(1, -1)
    with np.errstate(all="ignore"):
        row = lambda q: (_fma32(th[:, q + 1], gy, th[:, q] * gx) + th[:, q + 2]).astype(f32)
        T0, T1, t = row(0), row(3), row(6)
        t = (t + f32(1e-6) * np.where(np.abs(t) >= f32(1e-7), f32(0.0), f32(1.0)).astype(f32)).astype(f32)
        xs, ys = (T0 / t).astype(f32), (T1 / t).astype(f32)
        x = (((xs + f32(1.0)) * f32(W)) * f32(0.5)).astype(f32)
        y = (((ys + f32(1.0)) * f32(H)) * f32(0.5)).astype(f32)
    return t, x, y


def f2i_x86(v):
    """f2i_x86 of csrc/geometry.h on integers: a float inside [-2^31, 2^31) truncates, everything else (NaN, inf, out of range) is INT_MIN."""
    v = np.asarray(v, f64)
    ok = np.isfinite(v) & (v >= -2147483648.0) & (v < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, v, 0.0)).astype(np.int64), INT_MIN)


def _inc32(v):
    """(int)((unsigned)v + 1u): the kernel's wrap-around increment."""
    return (v + 1 - INT_MIN) % 2 ** 32 + INT_MIN


def warp_taps(x, y, H, W):
    """The clamped tap indices (x0, x1, y0, y1) that warp_point forms from fp32 coordinates: floor, f2i_x86, + 1, clamp."""
    with np.errstate(all="ignore"):
        xf, yf = f2i_x86(np.floor(x)), f2i_x86(np.floor(y))
    return np.clip(xf, 0, W - 1), np.clip(_inc32(xf), 0, W - 1), np.clip(yf, 0, H - 1), np.clip(_inc32(yf), 0, H - 1)


def warp_expect(U, theta):
    """The float64 truth of one warp call on the cells the fp32 coordinates pick: U [B,C,H,W], theta [B,9] ->
    dict(out [B,H,W,C], M, count, per_sample_count, taps, t).  Weights: the clamped taps against the unclamped float64 coordinate, as the reference."""
    B, C, H, W = U.shape
    t32, x32, y32 = warp_xy32(theta.numpy(), H, W)
    x0, x1, y0, y1 = warp_taps(x32, y32, H, W)
    with np.errstate(all="ignore"):
        per = (np.abs(t32) > f32(1e-7)).sum(axis=1)
        c64 = warp_coords(theta, B, H, W, torch.float64)
        x, y = c64[5].numpy(), c64[6].numpy()
        ax, bx, ay, by = x1 - x, x - x0, y1 - y, y - y0
        flat = U.double().numpy().reshape(B, C, H * W)
        take = lambda yy, xx: np.take_along_axis(flat, np.broadcast_to((yy * W + xx)[:, None, :], (B, C, H * W)), axis=2)
        Ia, Ib, Ic, Id = take(y0, x0), take(y1, x0), take(y0, x1), take(y1, x1)
        u = lambda v: v[:, None, :]
        out = u(ax * ay) * Ia + u(ax * by) * Ib + u(bx * ay) * Ic + u(bx * by) * Id
        M = np.abs(u(ax * ay) * Ia) + np.abs(u(ax * by) * Ib) + np.abs(u(bx * ay) * Ic) + np.abs(u(bx * by) * Id)
    nhwc = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 1))).reshape(B, H, W, C)
    return dict(out=nhwc(out), M=nhwc(M), count=int(per.sum()), per_sample_count=per, taps=(x0, x1, y0, y1), t=t32, xy=(x32, y32))


def warp_expect32(U, theta):
    """The fp32 output of warp_pixel restated in numpy, every operation rounded once in the kernel's order (coordinates: warp_xy32; taps: warp_taps;
    weights from the clamped taps; wa Ia + wb Ib + wc Ic + wd Id left to right, no fusion): [B,H,W,C] fp32.  The kernel compiles this part with
    contraction off, so it must return these bits on any data, NaN for NaN."""
    B, C, H, W = U.shape
    _, x, y = warp_xy32(theta.numpy(), H, W)
    x0, x1, y0, y1 = warp_taps(x, y, H, W)
    with np.errstate(all="ignore"):
        x0f, x1f, y0f, y1f = (v.astype(f32) for v in (x0, x1, y0, y1))
        wa, wb, wc, wd = (x1f - x) * (y1f - y), (x1f - x) * (y - y0f), (x - x0f) * (y1f - y), (x - x0f) * (y - y0f)
        flat = U.numpy().astype(f32).reshape(B, C, H * W)
        take = lambda yy, xx: np.take_along_axis(flat, np.broadcast_to((yy * W + xx)[:, None, :], (B, C, H * W)), axis=2)
        u = lambda v: v[:, None, :]
        out = ((u(wa) * take(y0, x0) + u(wb) * take(y1, x0)) + u(wc) * take(y0, x1)) + u(wd) * take(y1, x1)
    assert out.dtype == f32
    return torch.from_numpy(np.ascontiguousarray(out.transpose(0, 2, 1))).reshape(B, H, W, C)


def warp_r_ref(U, theta, exp):
    """The worst ratio of the oracle's fp32 CPU transformer on the regular elements of the fixture."""
    from oracle import hdn_oracle as O
    ref, _ = O.transformer(U, theta.reshape(-1, 3, 3), U.shape[2:])
    return km_check(ref, exp["out"], exp["M"], 0.0)[0]


# ---- exact fixtures
FWD_THETAS = tuple(WARP_THETAS) + ([1, 0, 1.5, 0, 1, -1.25, 0, 0, 1], [1, 0, -2.5, 0, 1, 2, 0, 0, 1], [2, 0, 0, 0, 2, 0, 0, 0, 1],
                                   [1, 0, 0, 0, 1, 0, 0, 0, .5], [.5, .25, 0, -.25, .5, .125, 0, 0, 2])
# (H, W): H, W in {5, 9, 17, 33, 65, 129} (a dyadic linspace step); 165 and 289 pixels either side of one pass of a workgroup's four (256), 561 inside
# one workgroup, 1,089 .. 2,145 in two or three workgroups
WARP_FWD_SHAPES = ((5, 33), (17, 17), (17, 33), (33, 33), (17, 65), (65, 33), (129, 9), (9, 129))
WARP_FWD_GROUPS = ((0, 1, 2), (3, 4, 5), (6, 7, None))    # thetas of one call; None: an all-NaN sample under the identity


@functools.lru_cache(maxsize=None)
def warp_exact_fwd(shape_i, group_i):
    """(U [3,C,H,W], theta [3,9], out float64 [3,H,W,C], count): integer image in [-3, 3]; C = 1, 2, 3 in turn."""
    H, W = WARP_FWD_SHAPES[shape_i]
    C = 1 + (shape_i + group_i) % 3
    rng = np.random.default_rng(SEED + 7919 * shape_i + 131 * group_i)
    U = _ints(rng, (3, C, H, W))
    rows = []
    for b, k in enumerate(WARP_FWD_GROUPS[group_i]):
        if k is None:
            U[b] = float("nan")
        rows.append(FWD_THETAS[k] if k is not None else WARP_THETAS[2])
    theta = torch.tensor(rows, dtype=torch.float32)
    out = transformer_rs(U.double(), theta.double())
    t = warp_coords(theta, 3, H, W, torch.float64)[2]
    return U, theta, out, int((t.abs() > 1e-7).sum())


# ---- position fixture: shifts by half grid steps; expectation by integer arithmetic
POSITION_SHAPES = ((9, 17), (17, 9), (5, 33), (33, 33))
POSITION_CANDIDATES = ((0, 0), (2, 0), (0, -2), (2, -4), (-6, 2), (1, 0), (0, 1), (-1, 3), (5, -1), (8, -8))   # (s2x, s2y): shift in half grid steps


def position_theta(H, W, s2x, s2y):
    """The identity moved by s2x / 2 grid steps in x and s2y / 2 in y: x = (2 j + s2x) W / (2 (W - 1)) pixels."""
    return [1, 0, s2x / (W - 1), 0, 1, s2y / (H - 1), 0, 0, 1]


def position_expect(P, s2x, s2y):
    """warp of the planes P [C,H,W] (integers) under position_theta by integer arithmetic on numerators over 2 (W - 1) and 2 (H - 1): [H,W,C]."""
    C, H, W = P.shape
    Dx, Dy = 2 * (W - 1), 2 * (H - 1)
    Xn = ((2 * np.arange(W) + s2x) * W)[None, :].astype(np.int64)
    Yn = ((2 * np.arange(H) + s2y) * H)[:, None].astype(np.int64)
    x0, y0 = Xn // Dx, Yn // Dy
    x0c, x1c, y0c, y1c = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1), np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
    ax, bx, ay, by = x1c * Dx - Xn, Xn - x0c * Dx, y1c * Dy - Yn, Yn - y0c * Dy
    Pi = P.numpy().astype(np.int64)
    num = (ax * ay) * Pi[:, y0c, x0c] + (ax * by) * Pi[:, y1c, x0c] + (bx * ay) * Pi[:, y0c, x1c] + (bx * by) * Pi[:, y1c, x1c]
    assert int(np.abs(num).max()) < 2 ** 53
    return torch.from_numpy(num.astype(f64) / float(Dx * Dy)).permute(1, 2, 0).contiguous()


@functools.lru_cache(maxsize=None)
def position_shifts(H, W):
    """The candidates under which the CPU's fp32 evaluation (the restatement and the oracle) of the pattern equals the integer arithmetic bit for
    bit: derived, not assumed.  The host test asserts that the identity, whole and half steps are among them."""
    from oracle import hdn_oracle as O
    P = pattern_planes(2, H, W)
    keep = []
    for s2x, s2y in POSITION_CANDIDATES:
        theta = torch.tensor([position_theta(H, W, s2x, s2y)], dtype=torch.float32)
        want = position_expect(P, s2x, s2y)
        r32 = transformer_rs(P[None], theta, torch.float32)[0]
        o32 = O.transformer(P[None], theta.reshape(1, 3, 3), (H, W))[0][0]
        if torch.equal(r32.double(), want) and torch.equal(o32.double(), want) and torch.equal(theta.double()[0], torch.tensor(position_theta(H, W, s2x, s2y), dtype=torch.float64)):
            keep.append((s2x, s2y))
    return tuple(keep)


@functools.lru_cache(maxsize=None)
def position_problem(H, W):
    """(U [B,2,H,W], theta [B,9], out float64 [B,H,W,2]): one sample per kept shift."""
    shifts = position_shifts(H, W)
    P = pattern_planes(2, H, W)
    theta = torch.tensor([position_theta(H, W, *s) for s in shifts], dtype=torch.float32)
    return P[None].repeat(len(shifts), 1, 1, 1).contiguous(), theta, torch.stack([position_expect(P, *s) for s in shifts])


# ---- degenerate branches
TINY = 2.0 ** -21                                          # 4.8e-7: between the kernel's 1e-7 and a wrong threshold of 1e-6
T_EDGE = float(f32(1e-7))                                  # |t| == 1e-7f: not nudged (>=) and not counted (>)
WARP_DEGENERATE = (
    ("nudge", [1, 0, 0, 0, 1, 0, 1, 0, 0]),                # t = gx: exactly 0 on the centre column -> t = 1e-6, counted; elsewhere xs = 1
    ("zero_row", [1, 0, .25, 0, 1, -.5, 0, 0, 0]),         # t = 0 everywhere -> 1e-6: coordinates of 1e6 pixels, inside int32
    ("huge", [1e12, 0, 0, 0, 1e12, 0, 0, 0, 1]),           # coordinates beyond int32 except on the centre row / column
    ("nan_y", [1, 0, 0, 0, float("nan"), 0, 0, 0, 1]),     # y NaN -> INT_MIN -> row 0 twice; t = 1: counted
    ("nan_t", [1, 0, 0, 0, 1, 0, 0, float("nan"), 1]),     # t NaN: nudged (NaN >= is false), stays NaN, NOT counted
    ("tiny", [TINY, 0, .25 * TINY, 0, TINY, -.5 * TINY, 0, 0, TINY]),      # |t| = 2^-21 >= 1e-7: no nudge; a dyadic affine map, exact
    ("edge", [T_EDGE, 0, 0, 0, T_EDGE, 0, 0, 0, T_EDGE]),  # the identity scaled by 1e-7f: not nudged, not counted
)
WARP_DEGENERATE_SHAPES = ((9, 17), (17, 9))


@functools.lru_cache(maxsize=None)
def warp_degenerate_problem(H, W):
    """(U [7,2,H,W] the pattern planes, theta [7,9], warp_expect)."""
    theta = torch.tensor([t for _, t in WARP_DEGENERATE], dtype=torch.float32)
    U = pattern_planes(2, H, W)[None].repeat(len(WARP_DEGENERATE), 1, 1, 1).contiguous()
    return U, theta, warp_expect(U, theta)


# ---- block and tail edges on N(0,1) data
WARP_EDGE_SHAPES = ((31, 33), (32, 32), (25, 41), (127, 127))                 # 1,023, 1,024, 1,025 and 16,129 pixels; B = 2, C = 3


@functools.lru_cache(maxsize=None)
def warp_random_fwd(H, W, B=2, C=3):
    """(U, theta = I + 0.08 N(0,1), warp_expect, r_ref): the backward suite's random fixture at this shape."""
    U, theta, _ = GC._warp_random(GC.WARP_BOUND_SEED, B, C, H, W)
    exp = warp_expect(U, theta)
    return U, theta, exp, warp_r_ref(U, theta, exp)


# ---- the fused kernel's theta
def round32(fr):
    """The fp32 nearest to a fraction, ties to even."""
    c = f32(float(fr))
    cands = sorted({float(c), float(np.nextafter(c, f32(np.inf))), float(np.nextafter(c, f32(-np.inf)))}, key=lambda v: abs(Fraction(v) - fr))
    if len(cands) > 1 and abs(Fraction(cands[0]) - fr) == abs(Fraction(cands[1]) - fr):
        cands = [v for v in cands[:2] if int(f32(v).view(np.uint32)) & 1 == 0]
    return f32(cands[0])


def _mat3_mul(A, B):
    """mat3_mul of csrc/dlt_warp.hip: C[i][j] = fma(A[i][2], B[2][j], fma(A[i][1], B[1][j], A[i][0] B[0][j])), each step rounded once."""
    Fr = lambda v: Fraction(float(v))
    C = np.zeros(9, f32)
    for i in range(3):
        for j in range(3):
            s = round32(Fr(A[3 * i]) * Fr(B[j]))
            s = round32(Fr(A[3 * i + 1]) * Fr(B[3 + j]) + Fr(s))
            C[3 * i + j] = round32(Fr(A[3 * i + 2]) * Fr(B[6 + j]) + Fr(s))
    return C


def normalise_rs(Hm, H, W):
    """normalise_H of csrc/dlt_warp.hip for finite fp32 matrices Hm [B,9]: theta = Minv Hm M with M = [[W/2, 0, W/2], [0, H/2, H/2], [0, 0, 1]]."""
    ax, ay = f32(W) * f32(0.5), f32(H) * f32(0.5)
    Minv = np.array([f32(1.0) / ax, 0, -1, 0, f32(1.0) / ay, -1, 0, 0, 1], f32)
    M = np.array([ax, 0, ax, 0, ay, ay, 0, 0, 1], f32)
    return torch.from_numpy(np.stack([_mat3_mul(_mat3_mul(Minv, h), M) for h in np.asarray(Hm, f32).reshape(-1, 9)]))


FUSED_SHAPES = ((33, 33), (31, 33), (25, 41), (127, 127))  # 1,089, 1,023, 1,025 and 16,129 pixels


@functools.lru_cache(maxsize=None)
def fused_problem(H, W, B=3):
    """(h4p [B,8] the crop's corners, off [B,8] uniform in +- W / 8 (sample 0: none), img [B,H,W] N(0,1)) for hdn_dlt_warp_strided_f32."""
    rng = np.random.default_rng(SEED + 4099 * H + W)
    h4p = torch.tensor([0.0, 0.0, W, 0.0, 0.0, H, W, H]).repeat(B, 1)
    off = torch.from_numpy(rng.uniform(-W / 8, W / 8, (B, 8)).astype(f32))
    off[0] = 0.0
    return h4p, off, torch.from_numpy(rng.standard_normal((B, H, W), dtype=f32))


# ================================================================================================================= DLT solve
QUAD = DLT_CORNERS["production"]                           # (0,0) (127,0) (0,127) (127,127)
SKEWED = DLT_CORNERS["skewed"]
TIE_QUAD = [-64.0, -60.0, 64.0, -60.0, -64.0, 68.0, 64.0, 68.0]               # |x| of all four points is 64, with both signs: the first pivot search ties
# found by search: under the point order (0, 1, 2, 3) instead of dlt_point's the elimination leaves other float64 residues where H is exactly 0
ORDER_QUAD = [16.0, -55.0, 48.0, 92.0, -83.0, -87.0, 83.0, -38.0]
DLT_KNOWN = (                                              # (name, source corners, H): dst = H src is exact in fp32
    ("shift_whole", QUAD, [1, 0, 3, 0, 1, -5, 0, 0, 1]), ("shift_half", QUAD, [1, 0, .5, 0, 1, 2.5, 0, 0, 1]),
    ("scale_2", QUAD, [2, 0, 0, 0, 2, 0, 0, 0, 1]), ("scale_half", QUAD, [.5, 0, 0, 0, .5, 0, 0, 0, 1]),
    ("rot90", QUAD, [0, -1, 127, 1, 0, 0, 0, 0, 1]), ("affine", QUAD, [1.25, .5, 3, -.25, .75, -2, 0, 0, 1]),
    ("affine_skewed", SKEWED, [1.25, .5, 3, -.25, .75, -2, 0, 0, 1]), ("shift_tie", TIE_QUAD, [1, 0, -4, 0, 1, 6.5, 0, 0, 1]),
    ("scale_order", ORDER_QUAD, [1.5, 0, 0, 0, 1.5, 0, 0, 0, 1]),
)
DLT_FWD_BATCHES = (1, 7, 8, 9, 31, 32, 33, 65, 257)       # either side of the 8-lane group, of a wave (8 samples) and of a workgroup (32)


def dlt_truth(src, off):
    """float64 dlt_rs.  The arguments go in as float64: handed fp32 tensors, dlt_rs would add src + off in fp32 and then add the rounding of that
    sum a second time."""
    return dlt_rs(src.double(), off.double())


def _apply(Hm, src):
    p = np.asarray(src, f64).reshape(4, 2)
    Hm = np.asarray(Hm, f64).reshape(3, 3)
    q = np.concatenate([p, np.ones((4, 1))], 1) @ Hm.T
    return (q[:, :2] / q[:, 2:]).reshape(8)


@functools.lru_cache(maxsize=None)
def dlt_fixture_rows():
    """(names, src [n,8], off [n,8]): the known maps, each corner displaced alone, and production / skewed / tie quads under random offsets."""
    names, src, off = [], [], []
    for name, quad, Hm in DLT_KNOWN:
        names.append(name), src.append(quad), off.append(_apply(Hm, quad) - np.asarray(quad, f64))
    for p in range(4):
        o = np.zeros(8)
        o[2 * p:2 * p + 2] = (4.0, -6.0)
        names.append(f"corner{p}"), src.append(QUAD), off.append(o)
    rng = np.random.default_rng(SEED + 977)
    for name, quad in (("production", QUAD), ("skewed", SKEWED), ("tie", TIE_QUAD)):
        names.append(name + "_random"), src.append(quad), off.append(rng.uniform(-32, 32, 8).astype(f32))
    return tuple(names), torch.tensor(np.asarray(src), dtype=torch.float32), torch.tensor(np.asarray(off), dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def dlt_fwd_problem(B):
    """(names, src [B,8], off [B,8], H float64 [B,9]): the fixture rows in turn; after one round every row takes fresh random offsets."""
    names, s, o = dlt_fixture_rows()
    n = len(names)
    rng = np.random.default_rng(SEED + 19 * B)
    idx = [(b + B) % n for b in range(B)]                  # a batch starts at another row than its neighbours
    src, off = s[idx].clone(), o[idx].clone()
    for b in range(n, B):
        off[b] = torch.from_numpy(rng.uniform(-32, 32, 8).astype(f32))
    return tuple(names[i] if b < n else names[i] + "+random" for b, i in enumerate(idx)), src, off, dlt_truth(src, off)


def dlt_restated(src, off, tie="low", point=None):
    """fp32(dlt_eliminate) with H[8] = 1 for every sample: [B,9] fp32.  The kernel is deterministic float64 (fma, division) rounded once to fp32,
    so both solvers must give these values; where H is exactly 0 the elimination leaves residues of 1e-17 that depend on its path, which is what
    pins the tie rule (shift_tie) and the point order (scale_order) at the level of values."""
    rows = [np.concatenate([dlt_eliminate(src[b], off[b], tie, point)[0], [1.0]]).astype(f32) for b in range(src.shape[0])]
    return torch.from_numpy(np.stack(rows))


@functools.lru_cache(maxsize=None)
def dlt_fwd_restated(B):
    _, src, off, _ = dlt_fwd_problem(B)
    return dlt_restated(src, off)


def dlt_eliminate(src, off, tie="low", point=None):
    """dlt_solve_rows of csrc/dlt_warp.hip for one sample, operation for operation in float64 (the fma on fractions: one rounding):
    -> (h [8] float64, list of (k, pivot row) where rows were swapped, list of k at which the pivot search met a tie).
    tie: 'low' as the kernel, 'high' the other way; point: the point order (default DLT_POINT_ORDER)."""
    point = DLT_POINT_ORDER if point is None else point
    s, o = np.asarray(src, f32).reshape(8), np.asarray(off, f32).reshape(8)
    A = []
    for r in range(8):
        p = point[r >> 1]
        x, y = float(s[2 * p]), float(s[2 * p + 1])
        u, v = float(f32(s[2 * p] + o[2 * p])), float(f32(s[2 * p + 1] + o[2 * p + 1]))
        A.append([x, y, 1.0, 0.0, 0.0, 0.0, -u * x, -u * y, u] if r % 2 == 0 else [0.0, 0.0, 0.0, x, y, 1.0, -v * x, -v * y, v])
    fma = lambda a, b, c: float(Fraction(a) * Fraction(b) + Fraction(c)) if all(map(np.isfinite, (a, b, c))) else a * b + c
    swaps, ties = [], []
    for k in range(8):
        mags = [abs(A[r][k]) for r in range(k, 8)]
        best = max(mags)
        rows = [k + i for i, m in enumerate(mags) if m == best]
        if len(rows) > 1:
            ties.append(k)
        piv = k if not rows else (rows[0] if tie == "low" else rows[-1])      # no row compares equal to a NaN maximum (a singular system)
        if piv != k:
            swaps.append((k, piv))
            A[k], A[piv] = A[piv], A[k]
        for r in range(8):
            if r != k:
                with np.errstate(all="ignore"):
                    f = float(f64(A[r][k]) / f64(A[k][k]))
                for j in range(k, 9):
                    A[r][j] = fma(-f, A[k][j], A[r][j])
    with np.errstate(all="ignore"):
        return np.array([float(f64(A[r][8]) / f64(A[r][r])) for r in range(8)]), swaps, ties


DEGENERATE_AT = 4


@functools.lru_cache(maxsize=None)
def dlt_degenerate_problem(B=9):
    """dlt_fwd_problem(B) with sample 4's four source corners equal: a singular system in the middle of a batch."""
    names, src, off, _ = dlt_fwd_problem(B)
    src = src.clone()
    src[DEGENERATE_AT] = torch.tensor([5.0, 7.0] * 4)
    return src, off


# ================================================================================================================= log-polar sampler
def dyadic_tabs(S):
    """rho: multiples of 0.25; cos, sin from {0, +-0.5, +-1} (a table, not trigonometry: the kernel only multiplies)."""
    cyc = (1.0, 0.5, 0.0, -0.5, -1.0, -0.5, 0.0, 0.5)
    i = np.arange(S)
    return (torch.from_numpy((0.25 * ((3 * i) % 19)).astype(f32)), torch.tensor([cyc[k % 8] for k in i], dtype=torch.float32),
            torch.tensor([cyc[(k + 6) % 8] for k in i], dtype=torch.float32))


# (S, H, W, C, polar): H // 2 and W // 2 are powers of two (16 / 8), the crops oblong, the origins dyadic and past every border between them
LOGPOLAR_DYADIC = ((16, 16, 33, 2, [[-7.25, 14.5], [7.5, -15.75], [0.25, 0.5]]), (17, 33, 16, 3, [[15.5, -7.25], [-16.0, 7.75]]))
N_LOGPOLAR_EXACT = len(LOGPOLAR_EXACT) + len(LOGPOLAR_DYADIC)


def logpolar_grid32(polar, tabs, H, W):
    """The two statements of logpolar_point (csrc/geometry.h) that form the grid, in numpy fp32: [B,S,S,2]."""
    rho, c, s = (t.numpy().astype(f32) for t in tabs)
    p = polar.numpy().astype(f32)
    gx = ((rho[None, None, :] * c[None, :, None]).astype(f32) + p[:, 0, None, None]).astype(f32) / f32(H // 2)
    gy = ((rho[None, None, :] * s[None, :, None]).astype(f32) + p[:, 1, None, None]).astype(f32) / f32(W // 2)
    return torch.from_numpy(np.stack([gx.astype(f32), gy.astype(f32)], axis=3))


def logpolar_cells(polar, tabs, H, W, dtype=torch.float32):
    """(x0, y0, e_ok, s_ok) [B,S,S] by the kernel's rule from the coordinates in `dtype`: clamp, floor, east / south taps masked past the last index."""
    pxu, pyu = logpolar_coords(polar, tabs, H, W, dtype)
    x0, y0 = pxu.clamp(0, W - 1).floor().long(), pyu.clamp(0, H - 1).floor().long()
    return x0, y0, x0 + 1 < W, y0 + 1 < H


def logpolar_expect(x, polar, tabs, cells=torch.float32):
    """The float64 truth of the sampler on the cells that `cells` coordinates pick, by the kernel's tap rule (a masked tap is not read, so a NaN
    there does not reach the output; an unmasked tap of weight 0 is read): (out [B,C,S,S], M)."""
    B, C, H, W = x.shape
    S = tabs[0].numel()
    pxu, pyu = logpolar_coords(polar, tabs, H, W, torch.float64)
    x0, y0, e_ok, s_ok = logpolar_cells(polar, tabs, H, W, cells)
    px, py = pxu.clamp(0, W - 1), pyu.clamp(0, H - 1)
    w, n = px - x0.double(), py - y0.double()
    e, s = 1.0 - w, 1.0 - n
    x1, y1 = torch.where(e_ok, x0 + 1, x0), torch.where(s_ok, y0 + 1, y0)
    flat = x.double().reshape(B, C, H * W)
    out, M = torch.zeros(B, C, S, S, dtype=torch.float64), torch.zeros(B, C, S, S, dtype=torch.float64)
    for yy, xx, ok, wt in ((y0, x0, torch.ones_like(e_ok), s * e), (y0, x1, e_ok, s * w), (y1, x0, s_ok, n * e), (y1, x1, e_ok & s_ok, n * w)):
        v = flat.gather(2, (yy * W + xx).reshape(B, 1, S * S).expand(B, C, S * S)).reshape(B, C, S, S)
        v = torch.where(ok.unsqueeze(1), v, torch.zeros_like(v))
        out, M = out + v * wt.unsqueeze(1), M + (v * wt.unsqueeze(1)).abs()
    return out, M


def logpolar_expect32(x, polar, tabs):
    """The fp32 output of logpolar_kernel restated in numpy, every operation rounded once in the kernel's order (no fma anywhere in it): [B,C,S,S]."""
    B, C, H, W = x.shape
    S = tabs[0].numel()
    g = logpolar_grid32(polar, tabs, H, W).numpy()
    one, half = f32(1.0), f32(0.5)
    px = ((g[..., 0] + one) * (f32(W) * half) - half).astype(f32)
    py = ((g[..., 1] + one) * (f32(H) * half) - half).astype(f32)
    px, py = np.minimum(f32(W - 1), np.maximum(f32(0.0), px)), np.minimum(f32(H - 1), np.maximum(f32(0.0), py))
    xw, yn = np.floor(px), np.floor(py)
    w, n = px - xw, py - yn
    e, s = one - w, one - n
    x0, y0 = xw.astype(np.int64), yn.astype(np.int64)
    e_ok, s_ok = x0 + 1 < W, y0 + 1 < H
    x1, y1 = np.where(e_ok, x0 + 1, x0), np.where(s_ok, y0 + 1, y0)
    flat = x.numpy().astype(f32).reshape(B, C, H * W)
    take = lambda yy, xx, ok: np.where(ok.reshape(B, 1, S * S), np.take_along_axis(flat, np.broadcast_to((yy * W + xx).reshape(B, 1, S * S), (B, C, S * S)), axis=2), f32(0.0))
    u = lambda v: v.reshape(B, 1, S * S)
    with np.errstate(all="ignore"):
        out = ((take(y0, x0, np.ones_like(e_ok)) * u(s * e) + take(y0, x1, e_ok) * u(s * w)) + take(y1, x0, s_ok) * u(n * e)) + take(y1, x1, e_ok & s_ok) * u(n * w)
    assert out.dtype == f32
    return torch.from_numpy(out.reshape(B, C, S, S))


def logpolar_reach(polar, tabs, H, W, col=None, row=None):
    """[B,S,S] bool: the outputs one of whose unmasked taps lies in image column `col` or row `row`."""
    x0, y0, e_ok, s_ok = logpolar_cells(polar, tabs, H, W)
    hit = torch.zeros_like(e_ok)
    if col is not None:
        hit |= (x0 == col) | (e_ok & (x0 + 1 == col))
    if row is not None:
        hit |= (y0 == row) | (s_ok & (y0 + 1 == row))
    return hit


@functools.lru_cache(maxsize=None)
def logpolar_exact_fwd(i):
    """(x, polar, tabs, out float64, grid float64): the five fixtures of the backward suite, then the two dyadic-table ones."""
    if i < len(LOGPOLAR_EXACT):
        x, polar, tabs = GC.logpolar_exact_problem(i)[:3]
    else:
        S, H, W, C, polar = LOGPOLAR_DYADIC[i - len(LOGPOLAR_EXACT)]
        polar, tabs = torch.tensor(polar), dyadic_tabs(S)
        x = _ints(np.random.default_rng(SEED + 613 * i), (polar.shape[0], C, H, W))
    B, _, H, W = x.shape
    rho, c, s = (t.double() for t in tabs)
    gx = ((rho.unsqueeze(0) * c.unsqueeze(1)).unsqueeze(0) + polar.double()[:, 0].reshape(B, 1, 1)) / (H // 2)
    gy = ((rho.unsqueeze(0) * s.unsqueeze(1)).unsqueeze(0) + polar.double()[:, 1].reshape(B, 1, 1)) / (W // 2)
    return x, polar, tabs, logpolar_rs(x.double(), polar.double(), tabs), torch.stack([gx, gy], dim=3)


def logpolar_poisoned(i, value, col=None, row=None):
    """Exact fixture i with `value` in image column `col` and / or row `row` (an index, -1 the last) of every plane."""
    x, polar, tabs = logpolar_exact_fwd(i)[:3]
    x = x.clone()
    if col is not None:
        x[:, :, :, col] = value
    if row is not None:
        x[:, :, row, :] = value
    return x, polar, tabs


@functools.lru_cache(maxsize=None)
def logpolar_inf_row(i):
    """The image row that most outputs with a masked east and an unmasked south tap (x0 = W - 1, so the south-east tap is the south-west one) read as
    their south row: +inf there stays +-inf through the south-west tap and turns into NaN if the masked south-east tap is read with its weight 0."""
    x, polar, tabs = logpolar_exact_fwd(i)[:3]
    x0, y0, e_ok, s_ok = logpolar_cells(polar, tabs, x.shape[2], x.shape[3])
    rows = (y0 + 1)[~e_ok & s_ok & (logpolar_coords(polar, tabs, x.shape[2], x.shape[3], torch.float32)[1] > y0)]
    return int(rows.mode().values)


LOGPOLAR_FWD_RANDOM = ((2, 3, 31, 29, 15), (1, 2, 24, 37, 16), (1, 1, 255, 255, 127), (1, 3, 127, 127, 127))


@functools.lru_cache(maxsize=None)
def logpolar_random_fwd(B, C, H, W, S):
    """(x, polar, tabs, out float64 on the fp32 cells, M, r_ref of F.grid_sample in fp32 on the CPU)."""
    x, polar, tabs = GC.logpolar_random_problem(B, C, H, W, S, cells32=True)[:3]
    out, M = logpolar_expect(x, polar, tabs)
    return x, polar, tabs, out, M, worst_ratio(logpolar_rs(x, polar, tabs, torch.float32), out, M)


# ================================================================================================================= refinement warp
REFINE_SHAPES = ((127, 127), (8, 200), (129, 128), (1, 1), (3, 300))
REFINE_SHIFTS = ((3.0, -2.0), (-4.0, 5.0), (0.5, -1.5), (5 / 32, 37 / 32), (-40.0, 2.5))      # (tx, ty) px, multiples of 1/32; both signs on both axes
REFINE_PROJECTIVE_SHAPES = ((127, 127), (129, 128), (8, 200))
REFINE_SEED = 1                                            # the host test asserts the cap for it


def shift_H(shifts):
    Hm = torch.eye(3).reshape(1, 9).repeat(len(shifts), 1)
    for b, (tx, ty) in enumerate(shifts):
        Hm[b, 2], Hm[b, 5] = tx, ty
    return Hm


def bilinear_replicate64(img, tx, ty):
    """dst(x, y) = src(x - tx, y - ty), bilinear in float64, every tap clamped to the image."""
    H, W = img.shape
    X, Y = np.arange(W)[None, :] - tx + 0.0 * np.arange(H)[:, None], np.arange(H)[:, None] - ty + 0.0 * np.arange(W)[None, :]
    x0, y0 = np.floor(X).astype(np.int64), np.floor(Y).astype(np.int64)
    fx, fy = X - x0, Y - y0
    cx, cy = lambda v: np.clip(v, 0, W - 1), lambda v: np.clip(v, 0, H - 1)
    a = np.asarray(img, f64)
    return ((1 - fy) * (1 - fx) * a[cy(y0), cx(x0)] + (1 - fy) * fx * a[cy(y0), cx(x0 + 1)] + fy * (1 - fx) * a[cy(y0 + 1), cx(x0)]
            + fy * fx * a[cy(y0 + 1), cx(x0 + 1)])


def shifted_index(img, tx, ty):
    """A whole-pixel shift as index arithmetic: out[y, x] = img[clamp(y - ty), clamp(x - tx)]."""
    H, W = img.shape
    return np.asarray(img)[np.clip(np.arange(H) - int(ty), 0, H - 1)[:, None], np.clip(np.arange(W) - int(tx), 0, W - 1)[None, :]]


@functools.lru_cache(maxsize=None)
def refine_exact_problem(H, W, B):
    """(Hm [B,9], img [B,H,W] integers in [-3, 3] (sample 0: the position pattern), out float64 [B,H,W]): translations by multiples of 1/32 px."""
    shifts = REFINE_SHIFTS[:B]
    img = _ints(np.random.default_rng(SEED + 389 * H + W + B), (B, H, W))
    img[0] = pattern(H, W)
    want = np.stack([bilinear_replicate64(img[b].numpy(), *shifts[b]) for b in range(B)])
    return shift_H(shifts), img, torch.from_numpy(want)


def refine_chain(Hm):
    """(H_hm, M) in fp32 as refine_warp_kernel and hdn_oracle.refine_step form them from H [3,3] fp32."""
    from oracle import hdn_oracle as O
    t = O._inv3(np.asarray(Hm, f32).reshape(3, 3).astype(f64)).astype(f32)
    Hhm = ((1.0 / f64(t[2, 2])) * t.astype(f64)).astype(f32)
    return Hhm, O._inv3(Hhm.astype(f64)).astype(f32)


def hcomp_product(Hc, Hhm):
    """H_comp @ H_hm as the kernel adds it: c0 h0j + c1 h1j + c2 h2j, left to right, no fma."""
    c, h = np.asarray(Hc, f64).reshape(3, 3), np.asarray(Hhm, f64).reshape(3, 3)
    return (c[:, 0:1] * h[0:1, :] + c[:, 1:2] * h[1:2, :]) + c[:, 2:3] * h[2:3, :]


@functools.lru_cache(maxsize=None)
def refine_projective_problem(H, W, seed=REFINE_SEED, B=4):
    """(Hm [B,9] fp32, img [B,H,W] N(0,1), H_comp0 [B,3,3] float64): H = I + a perturbation that grows with the sample, projective terms of 1e-4."""
    rng = np.random.default_rng(SEED + 100003 * seed + 1009 * H + W)
    img = torch.from_numpy(rng.standard_normal((B, H, W), dtype=f32))
    Hm = np.tile(np.eye(3), (B, 1, 1))
    for b in range(B):
        s = (0.0, 0.3, 1.0, 2.5)[b % 4]
        Hm[b] += s * np.array([[0.04, 0.04, 6.0], [0.04, 0.04, 6.0], [2e-4, 2e-4, 0.0]]) * rng.standard_normal((3, 3))
    Hc = np.tile(np.eye(3), (B, 1, 1))
    Hc[1 % B] *= 2.0
    Hc[B - 1] = np.array([[1.5, 0.25, 3.0], [0.125, 0.75, 2.0], [0.001, 0.002, 1.0]])
    return torch.from_numpy(Hm.astype(f32)).reshape(B, 9), img, Hc


# ---- the block walk: a fixture on which bw decides rounding ties
REFINE_TIE_SHAPE = (8, 200)                                # bw = 128 by the rule
REFINE_TIE_H = ([5, 0, 3 / 64, 0, 1, .5, 0, 0, 1], [3, 1, 3 / 64, 0, 1, .5, 0, 0, 1])


def warp_perspective_bw(img, M, bw=None):
    """hdn_oracle.warp_perspective_replicate with the block walk's width as a parameter (None: the rule's).  The source coordinate of a pixel is
    (X0 + M0 x1) W with X0 = M0 bx + M1 y + M2 taken at the block's first column bx = (x // bw) bw and x1 = x - bx: with M0 = 1/5 or 1/3 in
    float64 and a translation that puts every fifth (third) column on a cvRound tie in exact arithmetic, where bx falls decides which way the
    tie goes."""
    from oracle import hdn_oracle as O
    img = np.asarray(img, f32)
    Hh, Ww = img.shape
    m = O._inv3(np.asarray(M, f64))
    bw = rw_blocks(Hh, Ww)[0] if bw is None else bw
    y = np.arange(Hh, dtype=f64)[:, None]
    x = np.arange(Ww)[None, :]
    bx, x1 = ((x // bw) * bw).astype(f64), (x - (x // bw) * bw).astype(f64)
    X0, Y0, W0 = m[0, 0] * bx + m[0, 1] * y + m[0, 2], m[1, 0] * bx + m[1, 1] * y + m[1, 2], m[2, 0] * bx + m[2, 1] * y + m[2, 2]
    Wd = W0 + m[2, 0] * x1
    Wd = np.where(Wd != 0.0, 32.0 / np.where(Wd != 0.0, Wd, 1.0), 0.0)
    X = np.rint(np.clip((X0 + m[0, 0] * x1) * Wd, -2147483648.0, 2147483647.0)).astype(np.int64)
    Y = np.rint(np.clip((Y0 + m[1, 0] * x1) * Wd, -2147483648.0, 2147483647.0)).astype(np.int64)
    sx, sy = X >> 5, Y >> 5
    fx, fy = (X & 31).astype(f32) * f32(1 / 32), (Y & 31).astype(f32) * f32(1 / 32)
    one = f32(1.0)
    x0, x1c, y0, y1c = np.clip(sx, 0, Ww - 1), np.clip(sx + 1, 0, Ww - 1), np.clip(sy, 0, Hh - 1), np.clip(sy + 1, 0, Hh - 1)
    return ((img[y0, x0] * ((one - fy) * (one - fx)) + img[y0, x1c] * ((one - fy) * fx)) + img[y1c, x0] * (fy * (one - fx))) + img[y1c, x1c] * (fy * fx)


@functools.lru_cache(maxsize=None)
def refine_tie_problem():
    """(Hm [2,9], img [2,8,200] N(0,1)): scale 5 (3, with a shear) in x and a shift of 3/64 px."""
    rng = np.random.default_rng(SEED + 811)
    return torch.tensor(REFINE_TIE_H, dtype=torch.float32), torch.from_numpy(rng.standard_normal((2,) + REFINE_TIE_SHAPE, dtype=f32))


# ================================================================================================================= L1 score
L1_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 16129, 16383, 16384, 16385, 32769, 40000)
L1_SCALE = 2.0 ** -7
L1_BATCH = tuple((B, pad) for B in (1, 3, 5) for pad in (0, 1, 37))
L1_BATCH_SIZES = (65, 1025, 16129, 16385)


@functools.lru_cache(maxsize=None)
def l1_problem(n, B=1):
    """(a, b0, b1 [B,n] integers in [-8, 8], truth float64 [B,2]): sum |a - b| <= 16 x 40,000 = 640,000 < 2^24: exact in any order."""
    rng = np.random.default_rng(SEED + 3 * n + B)
    a, b0, b1 = (_ints(rng, (B, n), -8, 8) for _ in range(3))
    truth = torch.stack([(a.double() - b0.double()).abs().sum(1), (a.double() - b1.double()).abs().sum(1)], dim=1) * L1_SCALE
    return a, b0, b1, truth


# ================================================================================================================= on the device
class _Out:
    """An output of `n` floats that starts as NaN at float offset `off` inside margins of PAD floats of 0xA5."""

    def __init__(self, n, off, dev):
        self.n, self.off = n, off
        self.view, self.buf = at_offset(n, off, dev, margin=PAD, fill=FILL)

    def clean(self):
        return untouched(self.buf.cpu(), PAD + self.off, PAD + self.off + self.n)


def _put(t, off, dev):
    return at_offset(t.contiguous(), off, dev)[0]


def _same_bits(views_and_hosts):
    return all(torch.equal(v.cpu().view(torch.int32), h.contiguous().reshape(-1).view(torch.int32)) for v, h in views_and_hosts)


def _call(name, *args):
    from hdn_amd import _lib
    _lib.check(getattr(_lib.load(), name)(*args), name)


def _p(t):
    from hdn_amd import _lib
    return _lib.ptr(t) if t is not None else None


def _stream(dev):
    from hdn_amd import _lib
    return _lib.stream_ptr(dev)


def run_warp(U, theta, dev, offsets=OFFSETS[0], count=True):
    """One raw call of hdn_warp_count_f32 (count=True) or hdn_warp_f32: -> (out [B,H,W,C] on the CPU, count | None, nothing outside the results
    written?, inputs bit-unchanged?)."""
    B, C, H, W = U.shape
    Ud, td = _put(U, offsets[0], dev), _put(theta, offsets[1], dev)
    out, cnt = _Out(U.numel(), offsets[3], dev), _Out(1, offsets[4], dev)
    if count:
        _call("hdn_warp_count_f32", _p(Ud), _p(td), _p(out.view), _p(cnt.view), B, C, H, W, _stream(dev))
    else:
        _call("hdn_warp_f32", _p(Ud), _p(td), _p(out.view), B, C, H, W, _stream(dev))
    torch.cuda.synchronize(dev)
    clean = out.clean() and cnt.clean() and (count or bool(cnt.view.cpu().isnan().all()))
    n = int(cnt.view.cpu().view(torch.int32)[0]) if count else None
    return out.view.cpu().view(B, H, W, C), n, clean, _same_bits(((Ud, U), (td, theta)))


def run_dlt(src, off, dev, offsets=OFFSETS[0]):
    """One raw call of hdn_dlt_solve_f32: -> (H [B,9], clean, inputs unchanged)."""
    B = src.shape[0]
    sd, od = _put(src, offsets[0], dev), _put(off, offsets[1], dev)
    out = _Out(B * 9, offsets[3], dev)
    _call("hdn_dlt_solve_f32", _p(sd), _p(od), _p(out.view), B, _stream(dev))
    torch.cuda.synchronize(dev)
    return out.view.cpu().view(B, 9), out.clean(), _same_bits(((sd, src), (od, off)))


def run_dlt_warp(h4p, off, img, dev, offsets=OFFSETS[0], gap=0):
    """One raw call of hdn_dlt_warp_strided_f32 on img [B,H,W] with `gap` floats of NaN between the planes:
    -> (H [B,9], warped [B,H,W], clean, inputs unchanged)."""
    B, H, W = img.shape
    planes = torch.full((B, H * W + gap), float("nan"))
    planes[:, :H * W] = img.reshape(B, -1)
    hd, od, pd = _put(h4p, offsets[0], dev), _put(off, offsets[1], dev), _put(planes, offsets[2], dev)
    Ho, wo = _Out(B * 9, offsets[3], dev), _Out(B * H * W, offsets[4], dev)
    _call("hdn_dlt_warp_strided_f32", _p(hd), _p(od), _p(pd), H * W + gap, _p(Ho.view), _p(wo.view), B, H, W, _stream(dev))
    torch.cuda.synchronize(dev)
    return Ho.view.cpu().view(B, 9), wo.view.cpu().view(B, H, W), Ho.clean() and wo.clean(), _same_bits(((hd, h4p), (od, off), (pd, planes)))


def run_logpolar(x, polar, tabs, dev, offsets=OFFSETS[0], want_grid=True):
    """One raw call of hdn_logpolar_sample_f32: -> (out [B,C,S,S], grid [B,S,S,2] | None, clean, inputs unchanged).  Without the grid its buffer is
    handed over as NULL and must keep its NaN."""
    B, C, H, W = x.shape
    S = tabs[0].numel()
    xd, pd = _put(x, offsets[0], dev), _put(polar, offsets[1], dev)
    td = [_put(t, o, dev) for t, o in zip(tabs, (offsets[2], offsets[1], offsets[0]))]
    out, grid = _Out(B * C * S * S, offsets[3], dev), _Out(B * S * S * 2, offsets[4], dev)
    _call("hdn_logpolar_sample_f32", _p(xd), _p(pd), _p(td[0]), _p(td[1]), _p(td[2]), _p(out.view), _p(grid.view) if want_grid else None,
          B, C, H, W, S, _stream(dev))
    torch.cuda.synchronize(dev)
    clean = out.clean() and grid.clean() and (want_grid or bool(grid.view.cpu().isnan().all()))
    same = _same_bits(((xd, x), (pd, polar)) + tuple(zip(td, tabs)))
    return out.view.cpu().view(B, C, S, S), (grid.view.cpu().view(B, S, S, 2) if want_grid else None), clean, same


FILL64 = float(np.frombuffer(bytes([BYTE] * 8), dtype=np.float64)[0])


def run_refine(Hm, img, Hc, dev, offsets=OFFSETS[0]):
    """One raw call of hdn_refine_warp_f32 on img [B,H,W]; Hc: [B,3,3] float64 or None (NULL).  The record of H_comp lies at double offset
    offsets[4] % 2 inside margins of 0xA5: -> (warped [B,H,W], H_comp after | None, clean, inputs unchanged)."""
    B, H, W = img.shape
    hd, pd = _put(Hm, offsets[0], dev), _put(img, offsets[2], dev)
    out = _Out(B * H * W, offsets[3], dev)
    lo = PAD + offsets[4] % 2
    host = torch.full((lo + B * 9 + PAD,), FILL64, dtype=torch.float64)
    if Hc is not None:
        host[lo:lo + B * 9] = torch.as_tensor(Hc, dtype=torch.float64).reshape(-1)
    cbuf = host.to(dev)
    _call("hdn_refine_warp_f32", _p(hd), _p(pd), _p(out.view), _p(cbuf[lo:lo + B * 9]) if Hc is not None else None, B, H, W, _stream(dev))
    torch.cuda.synchronize(dev)
    back = cbuf.cpu()
    raw = back.numpy().view(np.uint8).reshape(-1, 8)
    clean = out.clean() and bool((raw[:lo] == BYTE).all()) and bool((raw[lo + (B * 9 if Hc is not None else 0):] == BYTE).all())
    return (out.view.cpu().view(B, H, W), (back[lo:lo + B * 9].view(B, 3, 3).numpy() if Hc is not None else None), clean,
            _same_bits(((hd, Hm), (pd, img))))


def run_l1(a, b0, b1, dev, offsets=OFFSETS[0], form="pair", pad=0):
    """One raw call of hdn_l1_score_f32 (form 'one': a against b0), hdn_l1_score2_f32 ('pair') or hdn_l1_score2_batch_f32 ('batch': a, b0, b1
    [B,n] laid out with plane_stride n + pad, the gaps NaN): -> (scores [1] / [2] / [B,2], clean, inputs unchanged)."""
    B, n = a.shape
    assert form == "batch" or (B == 1 and pad == 0)

    def lay(t):
        host = torch.full((B, n + pad), float("nan"))
        host[:, :n] = t
        return host
    hosts = [lay(t) for t in (a, b0, b1)]
    ad, b0d, b1d = (_put(h, o, dev) for h, o in zip(hosts, offsets[:3]))
    n_out = {"one": 1, "pair": 2, "batch": 2 * B}[form]
    out = _Out(n_out, offsets[3], dev)
    if form == "one":
        _call("hdn_l1_score_f32", _p(ad), _p(b0d), _p(out.view), n, L1_SCALE, _stream(dev))
    elif form == "pair":
        _call("hdn_l1_score2_f32", _p(ad), _p(b0d), _p(b1d), _p(out.view), n, L1_SCALE, _stream(dev))
    else:
        _call("hdn_l1_score2_batch_f32", _p(ad), _p(b0d), _p(b1d), _p(out.view), n, n + pad, B, L1_SCALE, _stream(dev))
    torch.cuda.synchronize(dev)
    got = out.view.cpu()
    return (got.view(B, 2) if form == "batch" else got), out.clean(), _same_bits(zip((ad, b0d, b1d), hosts))
