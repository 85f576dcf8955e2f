"""Shared by tests/test_gpu_xcorr_forms.py and tests/test_xcorr_cases_host.py: fixtures, float64 references, the grouping rules of the depthwise
correlation kernels (csrc/xcorr.hip, csrc/xcorr_fft.hip) restated, and the case tables that reach every tail, alignment branch and launch form.
Nothing here launches a kernel except run(), run_multi() and the __main__ block, which is the child process of
test_capped_persistent_grids_in_a_child_process (HDN_NORTH_BLOCKS is read once per process).

The exact fixture: integer images and taps in [-3, 3] (a seventh of the taps is exactly zero; the 31 x 31 taps also carry whole zero rows, one all-zero
plane and one -0.0 tap).  The largest window has 31 x 31 taps, so sum|x k| <= 961 x 9 = 8649: every partial sum is an integer far below 2^24 and fp32 is
exact in any summation order, fused or not, and 2e-6 x 8649 = 0.017 < 0.25, so rounding a result that is inside the project's bound gives the exact
integer.  exactness_headroom() works both figures out for an input instead of trusting this paragraph.

The position fixtures: plane p of the x-impulse has a single 1 at input position p (row-major) over taps that differ from tap to tap, plane p of the
k-impulse has its single 1 at tap position p over an image that differs from pixel to pixel.  The pattern is (1 + (t + 7 p) mod T) 2^-s for element t
of T in plane p: multiples of a power of two (exact in fp32 in any order), every element of a plane different, at most 32 (so the two transform kernels'
bound 1e-4 + 2e-6 M stays far below the step 2^-s between two elements: separation())."""
import functools
import json
import os
import sys
from collections import namedtuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 20261020
ABS_TOL, REL_TOL = 1e-4, 2e-6                        # tests/test_gpu_parity.py: |hip - ref| <= 1e-4 + 2e-6 sum|x k|

Kind = namedtuple("Kind", "name circular Hx Wx Hk Wk variant north exact")
#   variant: what hdn_amd.xcorr.last_variant() must answer; north: the hdn_amd.xcorr.north_variant to select; exact: must be torch.equal to float64
KINDS = {k.name: k for k in (
    Kind("prod29", False, 29, 29, 5, 5, "prod_29x29_5x5", None, True),
    Kind("cfg5", False, 35, 35, 5, 5, "cfg5_35x35_5x5", None, True),
    Kind("north_direct", False, 61, 61, 31, 31, "north_61x61_31x31", "direct", True),
    Kind("north_fft", False, 61, 61, 31, 31, "north_fftc_61x61_31x31", "fft", False),
    Kind("circ13", True, 13, 13, 13, 13, "circ13", None, False),
    # generic kernel, LDS form: even x odd and odd x even planes, Hk == HP and Wk == WP (a 1 x 1 result), Wk == 1
    Kind("gen_7x6_3x2", False, 7, 6, 3, 2, "generic_lds", None, True),
    Kind("gen_6x7_2x3", False, 6, 7, 2, 3, "generic_lds", None, True),
    Kind("gen_5x5_5x5", False, 5, 5, 5, 5, "generic_lds", None, True),
    Kind("gen_9x8_4x1", False, 9, 8, 4, 1, "generic_lds", None, True),
    Kind("genc_6x7_4x6", True, 6, 7, 4, 6, "generic_lds", None, True),
    Kind("genc_7x6_5x3", True, 7, 6, 5, 3, "generic_lds", None, True),
    Kind("genc_5x4_9x8", True, 5, 4, 9, 8, "generic_lds", None, True),     # padded plane 9 x 8 = the taps: a 1 x 1 result
    Kind("genc_7x5_3x1", True, 7, 5, 3, 1, "generic_lds", None, True),
    # both sides of the 60 KB switch, (HP WP + Hk Wk) 4 bytes <= 61440: 123 x 124 + 108 = 15360 floats stays in LDS, + 109 does not; circular:
    # 61 x 62 pads to 121 x 124 = 15004, + 356 = 15360 stays, + 357 does not; 62 x 62 pads to 124 x 124 = 15376: beyond it whatever the taps
    Kind("gen_123x124_12x9", False, 123, 124, 12, 9, "generic_lds", None, True),
    Kind("gen_123x124_109x1", False, 123, 124, 109, 1, "generic_l2", None, True),
    Kind("genc_61x62_89x4", True, 61, 62, 89, 4, "generic_lds", None, True),
    Kind("genc_61x62_119x3", True, 61, 62, 119, 3, "generic_l2", None, True),
    Kind("genc_62x62_5x1", True, 62, 62, 5, 1, "generic_l2", None, True),
)}
SPECIALISED = ("prod29", "cfg5", "north_direct", "north_fft", "circ13")
GENERIC = tuple(n for n in KINDS if n.startswith("gen"))
GENERIC_SMALL = tuple(n for n in GENERIC if KINDS[n].Hx < 20)


def out_size(K):
    HP = K.Hx + 2 * (K.Hx // 2) if K.circular else K.Hx
    WP = K.Wx + 2 * (K.Wx // 2) if K.circular else K.Wx
    return HP - K.Hk + 1, WP - K.Wk + 1


# ----------------------------------------------------------------------------------------------------------------- references
def pad_circular(x):
    """[P, H, W] -> [P, H + 2 (H // 2), W + 2 (W // 2)]: rows wrap, columns replicate (hdn/core/xcorr.py:48-61), by index arithmetic."""
    H, W = x.shape[-2:]
    rows = (torch.arange(H + 2 * (H // 2)) - H // 2) % H
    cols = (torch.arange(W + 2 * (W // 2)) - W // 2).clamp(0, W - 1)
    return x[:, rows][:, :, cols]


def direct_sum(x, k, circular, dtype=torch.float64):
    """out[p, i, j] = sum_uv xp[p, i + u, j + v] k[p, u, v] on [P, H, W] tensors, tap by tap in `dtype`; independent of oracle.hdn_oracle."""
    x, k = x.to(dtype), k.to(dtype)
    if circular:
        x = pad_circular(x)
    P, Hk, Wk = k.shape
    HO, WO = x.shape[1] - Hk + 1, x.shape[2] - Wk + 1
    out = torch.zeros(P, HO, WO, dtype=dtype)
    for u in range(Hk):
        for v in range(Wk):
            out.addcmul_(x[:, u:u + HO, v:v + WO], k[:, u:u + 1, v:v + 1])
    return out


def magnitude(x, k, circular):
    """M[p]: the largest sum|x k| of a window of plane p (float64)."""
    return direct_sum(x.abs(), k.abs(), circular).amax(dim=(1, 2))


def pair_max(M):
    """M of the pair of planes (2q, 2q + 1) that shares a transform in the FFT kernel, for every plane; an odd last plane is alone."""
    M = M.clone()
    n = M.numel() // 2 * 2
    both = torch.maximum(M[0:n:2], M[1:n:2])
    M[0:n:2], M[1:n:2] = both, both
    return M


def bound(K, M):
    """The project's bound per plane, [P]: 1e-4 + 2e-6 M, with M over the pair of planes for the FFT kernel."""
    return ABS_TOL + REL_TOL * (pair_max(M) if K.name == "north_fft" else M)


def exactness_headroom(x, k, circular):
    """(largest possible |partial sum| / 2^24, 2e-6 x the largest sum|x k|) of an input: below (1, 0.25) fp32 is exact in any order and rounding a result
    inside the project's bound gives the exact integer."""
    M = float(magnitude(x, k, circular).max())
    return M / 2.0 ** 24, REL_TOL * M


def fft32_plain(x, k):
    """The yardstick for the 61 x 61 FFT kernel: the same correlation with torch.fft in float32 on the CPU, zero-padded to 64 x 64."""
    assert x.dtype == k.dtype == torch.float32
    HO, WO = x.shape[1] - k.shape[1] + 1, x.shape[2] - k.shape[2] + 1
    y = torch.fft.irfft2(torch.fft.rfft2(x, s=(64, 64)) * torch.fft.rfft2(k, s=(64, 64)).conj(), s=(64, 64))
    assert y.dtype == torch.float32
    return y[:, :HO, :WO]


def fft32_circ13(x, k):
    """The yardstick for the circular kernel: 13-point float32 transforms along the wrapping axis, the clamped correlation along the columns in complex64."""
    assert x.dtype == k.dtype == torch.float32 and x.shape[1:] == k.shape[1:] == (13, 13)
    X, Kf = torch.fft.fft(x, dim=1), torch.fft.fft(k, dim=1)
    Xp = X[:, :, (torch.arange(25) - 6).clamp(0, 12)]
    Z = torch.zeros_like(X)
    for j in range(13):
        Z += Kf[:, :, j:j + 1].conj() * Xp[:, :, j:j + 13]
    corr = torch.fft.ifft(Z, dim=1).real                 # corr[m] = sum_u k[u] x[(m + u) mod 13]; output row i is m = i - 6
    assert corr.dtype == torch.float32
    return corr[:, (torch.arange(13) + 7) % 13]


# ----------------------------------------------------------------------------------------------------------------- the exact fixture
@functools.lru_cache(maxsize=None)
def exact_problem(kind, planes, tag=0):
    """(x [P, Hx, Wx], k [P, Hk, Wk], both fp32 integers in [-3, 3]; truth: float64 direct sum; M [P]) seeded per shape, plane count and tag."""
    K = KINDS[kind]
    g = np.random.default_rng(SEED + 1000003 * planes + 10007 * K.Hx + 1009 * K.Wx + 101 * K.Hk + 11 * K.Wk + 5 * K.circular + 7919 * tag)
    x = torch.from_numpy(g.integers(-3, 4, (planes, K.Hx, K.Wx)).astype(np.float32))
    k = torch.from_numpy(g.integers(-3, 4, (planes, K.Hk, K.Wk)).astype(np.float32))
    if (K.Hk, K.Wk) == (31, 31):
        for p in range(planes):
            k[p, (p % 5)::5] = 0                         # whole zero rows, other ones from plane to plane
        if planes >= 3:
            k[planes - 2] = 0                            # one all-zero plane (the partner of a live one in the FFT kernel's pairs)
        k[0, 2, 3] = -0.0                                # the direct kernel's zero-tap test must ignore the sign bit
    return x, k, direct_sum(x, k, K.circular), magnitude(x, k, K.circular)


# ----------------------------------------------------------------------------------------------------------------- the position fixtures
def pattern(P, H, W):
    """[P, H, W] fp32, (1 + (t + 7 p) mod T) 2^-s: every element of a plane different, the largest 32 or less."""
    T = H * W
    s = max(0, int(np.ceil(np.log2(T / 32.0))))
    t = (torch.arange(T).view(1, T) + 7 * torch.arange(P).view(P, 1)) % T
    return ((1 + t).double() * 2.0 ** -s).float().view(P, H, W)


def separation(pat):
    """The smallest of |value| and |value - neighbour| over the 8 neighbours, over all planes: what a shift by one position changes a result by."""
    d = [pat.abs().min()]
    for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
        a = pat[:, dr:, max(dc, 0):pat.shape[2] + min(dc, 0)]
        b = pat[:, :pat.shape[1] - dr, max(-dc, 0):pat.shape[2] - max(dc, 0)]
        if a.numel():
            d.append((a - b).abs().min())
    return float(min(d))


def impulses(positions, H, W):
    P = len(positions)
    z = torch.zeros(P, H * W)
    z[torch.arange(P), torch.as_tensor(positions)] = 1.0
    return z.view(P, H, W)


def x_impulse(kind, positions=None):
    """(x, k, want): plane p holds a single 1 at input position positions[p] (default: every position, one plane each) over pattern taps.
    want[p][i, j] = k[p][r - i, c - j] where that tap exists, else 0; circular: the sum of the taps (u, v) whose padded position (i + u, j + v) is a copy
    of (r, c): the one u with (i + u - H // 2) mod H == r, every v with clamp(j + v - W // 2) == c.  Index arithmetic, no convolution."""
    K = KINDS[kind]
    positions = list(range(K.Hx * K.Wx)) if positions is None else list(positions)
    P = len(positions)
    x, k = impulses(positions, K.Hx, K.Wx), pattern(P, K.Hk, K.Wk)
    HO, WO = out_size(K)
    pos = torch.as_tensor(positions)
    r, c = (pos // K.Wx).view(P, 1, 1), (pos % K.Wx).view(P, 1, 1)
    if not K.circular:
        U, V = r - torch.arange(HO).view(1, HO, 1), c - torch.arange(WO).view(1, 1, WO)
        ok = (U >= 0) & (U < K.Hk) & (V >= 0) & (V < K.Wk)
        want = torch.where(ok, k[torch.arange(P).view(P, 1, 1), U.clamp(0, K.Hk - 1), V.clamp(0, K.Wk - 1)], torch.zeros(()))
    else:
        rows = (torch.arange(HO).view(1, HO, 1) + torch.arange(K.Hk).view(1, 1, K.Hk) - K.Hx // 2) % K.Hx == r              # [P, HO, Hk]
        cols = (torch.arange(WO).view(1, WO, 1) + torch.arange(K.Wk).view(1, 1, K.Wk) - K.Wx // 2).clamp(0, K.Wx - 1) == c  # [P, WO, Wk]
        want = torch.einsum("piu,puv,pjv->pij", rows.double(), k.double(), cols.double()).float()
    return x, k, want


def k_impulse(kind, positions=None):
    """(x, k, want): plane p holds a single 1 at tap position positions[p] over a pattern image.  want[p][i, j] = x[p][i + u, j + v]; circular:
    x[p][(i + u - H // 2) mod H, clamp(j + v - W // 2)]."""
    K = KINDS[kind]
    positions = list(range(K.Hk * K.Wk)) if positions is None else list(positions)
    P = len(positions)
    x, k = pattern(P, K.Hx, K.Wx), impulses(positions, K.Hk, K.Wk)
    HO, WO = out_size(K)
    pos = torch.as_tensor(positions)
    R = torch.arange(HO).view(1, HO, 1) + (pos // K.Wk).view(P, 1, 1)
    C = torch.arange(WO).view(1, 1, WO) + (pos % K.Wk).view(P, 1, 1)
    if K.circular:
        R, C = (R - K.Hx // 2) % K.Hx, (C - K.Wx // 2).clamp(0, K.Wx - 1)
    return x, k, x[torch.arange(P).view(P, 1, 1), R, C]


def sampled_positions(H, W, step=241):
    """For planes too large to give every position a plane of its own: the corners, the edge midpoints, the centre and every step-th position."""
    pts = {0, W - 1, (H - 1) * W, H * W - 1, W // 2, (H - 1) * W + W // 2, (H // 2) * W, (H // 2) * W + W - 1, (H // 2) * W + W // 2}
    return sorted(pts | set(range(0, H * W, step)))


def position_fixtures(kind):
    """[(name, x, k, want)] of a kind; the 123 x 124 and 61 x 62 planes get sampled input positions."""
    K = KINDS[kind]
    xpos = None if K.Hx * K.Wx <= 4096 else sampled_positions(K.Hx, K.Wx)
    return [("x-impulse",) + x_impulse(kind, xpos), ("k-impulse",) + k_impulse(kind)]


# ----------------------------------------------------------------------------------------------------------------- checks
def first_difference(K, got, truth, M, exact_data):
    """None, or a description of the first wrong output of got [P, HO, WO] (fp32) against truth (float64 or fp32).  Direct kernels: bit-for-value equal.
    Transform kernels: |got - truth| <= 1e-4 + 2e-6 M per plane (pair of planes), and on the exact fixture got.round() == truth as well."""
    assert got.shape == truth.shape, (tuple(got.shape), tuple(truth.shape))
    if K.exact:
        bad = got != truth.float()
        how = "not equal"
    else:
        b = bound(K, M.double()).view(-1, 1, 1)
        err = (got.double() - truth.double()).abs()
        bad = ~(err <= b)                                # (a NaN is bad)
        how = "outside 1e-4 + 2e-6 M"
        if exact_data:
            bad |= got.round() != truth.float()
            how += " or rounds to another integer"
    if not bool(bad.any()):
        return None
    p, r, c = bad.nonzero()[0].tolist()
    d = {"count": int(bad.sum()), "of": bad.numel(), "plane": p, "row": r, "column": c, "got": float(got[p, r, c]), "want": float(truth[p, r, c]), "how": how}
    if not K.exact:
        d["bound"] = float(b[p, 0, 0])
        d["worst_error_over_bound"] = float((err / b).nan_to_num(nan=float("inf")).max())
    return d


def worst_ratio(K, got, truth, M):
    """max |got - truth| / bound over all outputs (what the tests print for the two transform kernels)."""
    return float(((got.double() - truth.double()).abs() / bound(K, M.double()).view(-1, 1, 1)).max())


# ----------------------------------------------------------------------------------------------------------------- the grouping rules, restated
PPB = 4                        # planes per workgroup of xcorr_prod29_kernel and xcorr_cfg5_kernel (one wave per plane)
NORTH_WAVES = 4                # xcorr_north_kernel: 4 autonomous waves per workgroup, each a whole plane at a time
FFT_WPG = 4                    # xcorr_north_fft4_kernel<4>: workers (waves) per workgroup; a worker owns PAIRS of planes
FFT_STAGGER_PASSES = 4         # the staggered start: npairs >= 4 * nmain
CIRC_PPW, CIRC_WAVES = 9, 4    # xcorr_circ13f_kernel: planes per wave, waves per workgroup; the groups of all problems are one flat grid
CAP_DIRECT, CAP_FFT = 512, 1024
CAP_ENV = "HDN_NORTH_BLOCKS"
GENERIC_LDS_BYTES = 60 * 1024
MAX_PROBLEMS = 8


def cdiv(a, b):
    return -(-a // b)


def groups4(planes):
    """[(first plane, np)] of the workgroups of the two 4-plane kernels."""
    return [(p0, min(PPB, planes - p0)) for p0 in range(0, planes, PPB)]


def wide_copy(np_, float_offset):
    """The 16-byte all-in-flight path of a workgroup (np == PPB && aligned16): a group of 4 planes is a multiple of 16 bytes for x and out of both shapes,
    so the alignment of a group is that of the base pointer."""
    return np_ == PPB and float_offset % 4 == 0


def north_direct_plan(planes, n=1, cap=CAP_DIRECT):
    """launch_north: per-problem workgroups, waves, passes of the busiest wave."""
    wgs = max(1, min(cdiv(planes, NORTH_WAVES), cap // n))
    waves = NORTH_WAVES * wgs
    return {"workgroups": wgs, "waves": waves, "live_waves": min(waves, planes), "passes": cdiv(planes, waves)}


def fft4_plan(planes, cap=CAP_FFT):
    """launch_north_fft4: interior pairs go to nmain persistent workers (p, p + nmain, ...), an odd last plane to one extra tail worker on the guarded v1
    path, one plane alone to the v1 kernel."""
    nfast, npairs = planes // 2, (planes + 1) // 2
    if nfast == 0:
        return {"v1_alone": True, "nmain": 0, "tail": False, "workers": 1, "workgroups": 1, "surplus": 0, "passes": 1, "stagger": False}
    nmain = min(nfast, cap)
    tail = nfast < npairs
    workers = nmain + tail
    wgs = cdiv(workers, FFT_WPG)
    return {"v1_alone": False, "nmain": nmain, "tail": tail, "workers": workers, "workgroups": wgs, "surplus": FFT_WPG * wgs - workers,
            "passes": cdiv(nfast, nmain), "stagger": nfast >= FFT_STAGGER_PASSES * nmain,
            "prefetch_clamped": any(p + nmain > nfast - 1 for p in range(nfast)), "prefetch_next": any(p + nmain <= nfast - 1 for p in range(nfast))}


def circ_groups(planes, n=1):
    """launch_circ13: [[(problem, first plane, np) of each wave] of each workgroup] of the flat grid."""
    gpp = cdiv(planes, CIRC_PPW)
    flat = [(g // gpp, (g % gpp) * CIRC_PPW, min(CIRC_PPW, planes - (g % gpp) * CIRC_PPW)) for g in range(gpp * n)]
    return [flat[i:i + CIRC_WAVES] for i in range(0, len(flat), CIRC_WAVES)]


def generic_variant(K):
    HO, WO = out_size(K)
    floats = (HO + K.Hk - 1) * (WO + K.Wk - 1) + K.Hk * K.Wk
    return "generic_lds" if 4 * floats <= GENERIC_LDS_BYTES else "generic_l2"


# ----------------------------------------------------------------------------------------------------------------- the cases
OFFSETS_4 = [(0, 0, 0), (1, 0, 0), (0, 0, 1), (0, 3, 0), (2, 1, 3)]       # float offsets of the x, k and out base pointers
OFFSETS_FFT = [(0, 0, 0), (1, 0, 0), (0, 0, 1), (2, 1, 3)]
OFFSETS_CIRC = [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3)]               # the four residues of a 4-byte aligned pointer in a 16-byte line
SINGLE = {                                                                  # kind -> (plane counts, offsets)
    "prod29": (tuple(range(1, 10)), OFFSETS_4),
    "cfg5": (tuple(range(1, 10)), OFFSETS_4),
    "north_direct": (tuple(range(1, 10)) + (33,), [(0, 0, 0)]),
    "north_fft": ((1, 2, 3, 4, 5, 7, 8, 9, 33), OFFSETS_FFT),
    "circ13": (tuple(range(1, 20)) + (37,), OFFSETS_CIRC),
}
GENERIC_PLANES = 3
MULTI_N = (1, 2, 3, 6, 8)
MULTI = {                                                                   # kind -> [(n, planes)]
    "prod29": [(n, P) for P in (5, 6) for n in MULTI_N],
    "cfg5": [(n, P) for P in (5, 6) for n in MULTI_N],
    "north_direct": [(n, P) for P in (3, 4) for n in MULTI_N],
    "north_fft": [(n, P) for P in (3, 4) for n in MULTI_N],
    "circ13": [(n, 10) for n in MULTI_N] + [(8, 1)],
}
CHILD_BLOCKS = 3                                                            # HDN_NORTH_BLOCKS of the child
CHILD_CASES = ("37", "38", "3x9")                                          # planes through the single call; n x planes through the multi call
GUARD = {                                                                   # kind -> plane counts of the stray-write and NaN-plane tests (tail counts)
    "prod29": (5, 7), "cfg5": (5, 7), "north_direct": (5,), "north_fft": (3, 4, 5), "circ13": (10, 19),
    "gen_7x6_3x2": (3,), "genc_6x7_4x6": (3,), "gen_123x124_109x1": (2,),
}
GUARD_OFFSETS = [(0, 0, 0), (3, 2, 1)]


def parse_child_case(s):
    """'37' -> (1, 37); '3x9' -> (3, 9)."""
    return (int(s.split("x")[0]), int(s.split("x")[1])) if "x" in s else (1, int(s))


# ----------------------------------------------------------------------------------------------------------------- on the device
def at_offset(t, off, dev, margin=0, fill=0.0):
    """(view, whole buffer): the values of t (None: uninitialised result space of that many floats, here NaN) on the device at float offset margin + off
    of a fresh allocation that ends `margin` floats behind them; the rest of the buffer holds `fill`."""
    n = t if isinstance(t, int) else t.numel()
    host = torch.full((margin + off + n + margin,), float(fill))
    host[margin + off:margin + off + n] = float("nan") if isinstance(t, int) else t.reshape(-1)
    buf = host.to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf[margin + off:margin + off + n], buf


last = {"variant": None}          # hdn_amd.xcorr.last_variant() after the latest launch()


def run(kind, x, k, dev, offsets=(0, 0, 0)):
    """One problem through hdn_xcorr_depthwise_multi_f32 with n = 1 (the single-call entry points are this call), the base pointers of x, k and out
    `offsets` floats into a 16-byte line, out holding NaN beforehand.  Returns (result on the CPU [P, HO, WO], last_variant())."""
    return run_multi(kind, [x], [k], dev, offsets)[0][0], last["variant"]


def run_multi(kind, xs, ks, dev, offsets=(0, 0, 0), stacked=True):
    """n problems in one launch.  stacked: the results are the n slices of ONE buffer [n, P, HO, WO] (which starts offsets[2] floats into a 16-byte line)
    and held NaN beforehand.  Returns ([result on the CPU], the device tensors used)."""
    K = KINDS[kind]
    n, P = len(xs), xs[0].shape[0]
    HO, WO = out_size(K)
    xd = [at_offset(x, offsets[0], dev)[0].view(1, P, K.Hx, K.Wx) for x in xs]
    kd = [at_offset(k, offsets[1], dev)[0].view(1, P, K.Hk, K.Wk) for k in ks]
    if stacked:
        stack = at_offset(n * P * HO * WO, offsets[2], dev)[0].view(n, 1, P, HO, WO)
        outs = [stack[i] for i in range(n)]
    else:
        outs = [at_offset(P * HO * WO, offsets[2], dev)[0].view(1, P, HO, WO) for _ in range(n)]
    for t, o in zip(xd + kd + outs[:1], [offsets[0]] * n + [offsets[1]] * n + [offsets[2]]):
        assert t.data_ptr() % 16 == 4 * (o % 4)
    launch(K, xd, kd, outs)
    return [o.cpu().view(P, HO, WO) for o in outs], (xd, kd, outs)


def launch(K, xd, kd, outs):
    from hdn_amd import xcorr as X
    if K.north:
        with X.north_variant(K.north):
            X.xcorr_depthwise_multi(xd, kd, circular=K.circular, outs=outs)
    else:
        X.xcorr_depthwise_multi(xd, kd, circular=K.circular, outs=outs)
    last["variant"] = X.last_variant()


def check_exact_case(kind, planes, dev, offsets=(0, 0, 0), n=1):
    """The exact fixture at `planes` planes (n problems with other data each, in one launch, into one stacked buffer): (None, or what is wrong; the
    largest error as a share of the bound, 0 for the direct kernels)."""
    K = KINDS[kind]
    probs = [exact_problem(kind, planes, tag) for tag in range(n)]
    got, _ = run_multi(kind, [p[0] for p in probs], [p[1] for p in probs], dev, offsets)
    if last["variant"] != K.variant:
        return {"how": f"dispatched to {last['variant']}, not {K.variant}"}, 0.0
    worst = 0.0
    for i, (y, (x, k, truth, M)) in enumerate(zip(got, probs)):
        d = first_difference(K, y, truth, M, True)
        if d is not None:
            d["problem"] = i
            return d, worst
        if not K.exact:
            worst = max(worst, worst_ratio(K, y, truth, M))
    return None, worst


if __name__ == "__main__":
    # the child of test_capped_persistent_grids_in_a_child_process: HDN_NORTH_BLOCKS is set by the parent; argv = kind, then the cases; one JSON line
    if not torch.cuda.is_available():
        sys.exit("no GPU")
    kind, cases = sys.argv[1], sys.argv[2:]
    device = torch.device("cuda:0")
    answer = {"kind": kind, "blocks": os.environ.get(CAP_ENV), "cases": []}
    for case in cases:
        n_, planes_ = parse_child_case(case)
        first, worst = check_exact_case(kind, planes_, device, n=n_)
        answer["cases"].append({"case": case, "first": first, "error_over_bound": worst, "variant": last["variant"]})
    print(json.dumps(answer))
