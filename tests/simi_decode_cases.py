"""The fixtures, the expectations and the numpy restatement that tests/test_simi_decode_host.py (CPU) and tests/test_gpu_simi_decode.py (GPU) share
for the two decode kernels of csrc/similarity.hip (hdn_similarity_translation_f32, hdn_similarity_logpolar_f32).  Nothing here touches the device.

Every expectation is what oracle.tracker_oracle.decode_translation / decode_logpolar answer for the record (numpy + PyTorch-CPU, pinned to the
executed reference by tests/golden/similarity*.npz), called at batch 1 with the fixture's own window / points tables.

A fixture ("family") is one launch of each kernel over B records: the translation half (S, window, window_influence) and the log-polar half (S_lp).
The half a family is not about is a small filler that is still checked against the oracle.

    sweep      record b has its class-1 logit +6 at cell b, -6 elsewhere: the maximum in every cell, B = n = S * S, production window influence
    ties       window_influence = 0 (the blended score is the float32 score, equal logits are equal bits on any expf): pairs and triples of a cell set
               built on the kernel's lane structure (lane = i mod 64, round = i // 64), all logits equal, all logits saturated
    gates      winners 1e-4 ... 1e-2 either side of 0.05 (translation) and 0.25 (log-polar); a log-polar record gated by `stop` alone; d0 = 0 / d2 = 0
    nonfinite  NaN / +inf logits, an all-NaN map, a NaN in the window table, mixed with clean records: np.argmax's rule (the first NaN, else the maximum)

kernel_argmax() restates the device argmax (the per-lane strided scan, then the six-step xor butterfly; lane 0's answer) in numpy with the mistakes
of WRONG, so that the host test can show which family sees which mistake."""
import functools
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import tracker_oracle as TO  # noqa: E402

WAVE = 64
WI = TO.WINDOW_INFLUENCE
STRIDE = 8.0                                         # _convert_c hard-codes 8; cfg.POINT.STRIDE_LP = 8
EXEMPLAR = 127.0
MAG = float(np.log(127 / 2) / 127)                   # hdn_tracker.py:63
ROT_UNIT = float(np.float32(2 * np.pi / 127))        # :62
HI, LO, SAT = 6.0, -6.0, 30.0
NO_CELL = 0x7FFFFFFF

TR_SWEEP_SIZES = (1, 2, 3, 7, 8, 9, 13, 25, 31)
LP_SWEEP_SIZES = (1, 2, 7, 8, 9, 13)
TIE_BASE = (0, 1, 2, 4, 8, 16, 32, 63, 64, 65, 96, 127, 128, 576, 577, 608, 624)
TIE_SIZES = {"tr": (25, 7), "lp": (13, 7)}
GATE_WI = 0.03                                       # with the Hanning window the floor of the blended map is 0.03 at the centre: below the 0.05 gate
GATE_OFFSETS = (2e-4, 5e-3)                          # distances from a gate; the host test holds every one inside [1e-4, 1e-2]

# what a mistake in the argmax / the decode looks like (kernel_argmax, restate)
WRONG = ("no_tiebreak", "tiebreak_reversed", "scan_ge", "scan_short", "plane", "nan_skipped")


# ------------------------------------------------------------------------------------------------------------------------------------ building blocks
def seq_records(B):
    """[B, 8] per-sequence records (include/hdn_hip.h): a different position and template size per record, s_x = floor(s_z * 2)."""
    b = np.arange(B, dtype=np.float64)
    s_z = 377.0 + (b % 5)
    return np.stack([311.5 + 0.5 * b, 207.25 - 0.25 * b, s_z, np.floor(s_z * 2.0), 244.0 + (b % 3), 10.0 + 0 * b, 20.0 + 0 * b, 30.0 + 0 * b], 1)


def logit_maps(hot, S, ch, hi=HI, lo=LO):
    """[B, ch, S, S] float32: record b has `hi` at the cells hot[b] and `lo` elsewhere - in the class-1 plane (class 0 = 0), or in the single plane."""
    B, n = len(hot), S * S
    plane = np.full((B, n), lo, np.float32)
    for b, cells in enumerate(hot):
        plane[b, list(cells)] = hi
    planes = [plane] if ch == 1 else [np.zeros_like(plane), plane]
    return np.ascontiguousarray(np.stack(planes, 1).reshape(B, ch, S, S))


def loc_planes(n, shift=0):
    """Two planes of n cells, a dyadic value per cell: points - 8 * loc is exact in float32, another cell or the other plane is another number."""
    i = np.arange(n) + shift
    return ((i % 17) - 8) / 8.0, ((i % 13) - 6) / 4.0


def loc_c_maps(B, S, per_record=False):
    n = S * S
    out = np.empty((B, 2, n), np.float32)
    for b in range(B):
        out[b, 0], out[b, 1] = loc_planes(n, 3 * b if per_record else 0)
    return out.reshape(B, 2, S, S)


def loc_lp_maps(B, S, per_record=False):
    """Planes 0 and 2 as loc_c_maps; planes 1 and 3 (never read by the decode) hold values outside the range of 0 and 2 at every cell."""
    n = S * S
    out = np.empty((B, 4, n), np.float32)
    tell = 1.625 + (np.arange(n) % 5) / 8.0
    for b in range(B):
        out[b, 0], out[b, 2] = loc_planes(n, 3 * b if per_record else 0)
        out[b, 1], out[b, 3] = tell, -tell - 1.0
    return out.reshape(B, 4, S, S)


def logit_of(score):
    return float(np.log(score / (1.0 - score)))


class Family:
    """One launch of each kernel.  cls [B,ch,S,S], loc_c [B,2,S,S], window [S*S] float64, cls_lp [B,ch,S_lp,S_lp], loc_lp [B,4,S_lp,S_lp], seq [B,8]."""

    def __init__(self, name, kind, focus, ch, wi, S, window, cls, loc_c, S_lp, cls_lp, loc_lp, tags=None, clean=None):
        self.name, self.kind, self.focus, self.ch, self.wi, self.S, self.S_lp = name, kind, focus, ch, float(wi), S, S_lp
        self.window = np.ascontiguousarray(window, np.float64)
        self.cls, self.loc_c, self.cls_lp, self.loc_lp = (np.ascontiguousarray(a, np.float32) for a in (cls, loc_c, cls_lp, loc_lp))
        self.B = self.cls.shape[0]
        self.seq = seq_records(self.B)
        self.points, self.points_lp = TO.generate_points(8, S), TO.generate_points(8, S_lp)
        self.tags = list(tags) if tags is not None else [""] * self.B
        self.clean = clean                 # nonfinite families: the records without a non-finite value
        self.nonfinite = kind == "nonfinite"
        assert self.cls.shape == (self.B, ch, S, S) and self.loc_c.shape == (self.B, 2, S, S) and self.window.shape == (S * S,)
        assert self.cls_lp.shape == (self.B, ch, S_lp, S_lp) and self.loc_lp.shape == (self.B, 4, S_lp, S_lp) and len(self.tags) == self.B
        self._expected = None

    def __repr__(self):
        return self.name

    def subset(self, rows):
        """The same launch with the records `rows` alone (their seq records kept)."""
        rows = list(rows)
        f = Family(self.name + "/subset", self.kind, self.focus, self.ch, self.wi, self.S, self.window, self.cls[rows], self.loc_c[rows], self.S_lp,
                   self.cls_lp[rows], self.loc_lp[rows], [self.tags[r] for r in rows])
        f.seq = np.ascontiguousarray(self.seq[rows])
        return f

    def expected(self):
        if self._expected is None:
            self._expected = _expected(self)
        return self._expected


def _expected(f):
    """Per record, from the oracle alone: the fields of the state record that the two kernels write."""
    out = {k: [] for k in ("best_idx", "stop", "delta", "center", "best_score", "pscore", "best_idx_lp", "score_lp", "scale_delta", "rot_delta", "sim0",
                           "gated", "pscore_map", "score_lp_map")}
    T = torch.from_numpy
    for b in range(f.B):
        s_z = f.seq[b, 2]
        tr = TO.decode_translation(T(f.cls[b:b + 1]), T(f.loc_c[b:b + 1]), f.window, f.points, s_z, f.wi)
        lp = TO.decode_logpolar(T(f.cls_lp[b:b + 1]), T(f.loc_lp[b:b + 1]), f.points_lp, tr["stop"], s_z, s_z)
        i, j = tr["best_idx"], lp["best_idx_lp"]
        gated = bool(tr["stop"]) or bool(lp["score_lp"][j] < 0.25)          # the reference's own condition (hdn_tracker_proj_e2e.py:207)
        out["best_idx"].append(i), out["stop"].append(int(tr["stop"])), out["delta"].append(tr["center"])
        out["center"].append(tr["center"] + f.seq[b, 0:2])
        out["best_score"].append(float(tr["best_score"])), out["pscore"].append(float(tr["pscore"][i]))
        out["best_idx_lp"].append(j), out["score_lp"].append(float(lp["score_lp"][j]))
        out["scale_delta"].append(lp["scale_delta"]), out["rot_delta"].append(lp["rot_delta"])
        out["sim0"].append(float(lp["sim_lp"][0])), out["gated"].append(int(gated))
        out["pscore_map"].append(np.asarray(tr["pscore"], np.float64)), out["score_lp_map"].append(np.asarray(lp["score_lp"], np.float64))
    return {k: np.asarray(v) for k, v in out.items()}


def _filler_tr(B, ch):
    """Translation half of a log-polar family: S = 3, a clear winner at cell b mod 9 (never gated)."""
    return 3, logit_maps([[b % 9] for b in range(B)], 3, ch), loc_c_maps(B, 3)


def _filler_lp(B, ch, S_lp=2):
    n = S_lp * S_lp
    return S_lp, logit_maps([[(7 * b) % n] for b in range(B)], S_lp, ch), loc_lp_maps(B, S_lp)


# ------------------------------------------------------------------------------------------------------------------------------------ the families
@functools.lru_cache(maxsize=None)
def sweep(S, ch):
    """Both kernels at S where the log-polar sweep has that size, else the translation kernel with a 13 x 13 log-polar filler."""
    n = S * S
    hot = [[b] for b in range(n)]
    if S in LP_SWEEP_SIZES:
        S_lp, cls_lp, loc_lp, focus = S, logit_maps(hot, S, ch), loc_lp_maps(n, S), "both"
    else:
        (S_lp, cls_lp, loc_lp), focus = _filler_lp(n, ch, 13), "tr"
    return Family(f"sweep-S{S}-ch{ch}", "sweep", focus, ch, WI, S, TO.hanning_window(S), logit_maps(hot, S, ch), loc_c_maps(n, S), S_lp, cls_lp, loc_lp)


def tie_set(n):
    return sorted({c for c in TIE_BASE if c < n} | {n - 1})


def tie_groups(n):
    """(pairs, a dozen triples) of tie_set(n)."""
    cells = tie_set(n)
    pairs = list(itertools.combinations(cells, 2))
    triples = list(itertools.combinations(cells, 3))
    return pairs, triples[::max(1, len(triples) // 12)][:12]


@functools.lru_cache(maxsize=None)
def ties(kernel, S, ch):
    n = S * S
    pairs, triples = tie_groups(n)
    hot = [list(p) for p in pairs] + [list(t) for t in triples]
    tags = ["pair"] * len(pairs) + ["triple"] * len(triples) + ["all-equal", "saturated"]
    maps = np.concatenate([logit_maps(hot, S, ch), logit_maps([range(n)], S, ch, hi=1.25), logit_maps([range(n)], S, ch, hi=SAT)])
    B = maps.shape[0]
    if kernel == "tr":
        S_lp, cls_lp, loc_lp = _filler_lp(B, ch)
        return Family(f"ties-tr-S{S}-ch{ch}", "ties", "tr", ch, 0.0, S, TO.hanning_window(S), maps, loc_c_maps(B, S), S_lp, cls_lp, loc_lp, tags)
    S_t, cls, loc_c = _filler_tr(B, ch)
    return Family(f"ties-lp-S{S}-ch{ch}", "ties", "lp", ch, 0.0, S_t, np.zeros(S_t * S_t), cls, loc_c, S, maps, loc_lp_maps(B, S), tags)


@functools.lru_cache(maxsize=None)
def gates(ch):
    """Translation at S = 25 with the Hanning window at window_influence 0.03, log-polar at S = 13.  Per record: (translation winner cell, its
    blended score or None = a clear +6), (log-polar winner cell, its score or None), and whether d0 / d2 of the log-polar winner are zero."""
    S, S_lp, keep = 25, 13, float(np.float32(1.0 - GATE_WI))
    win = TO.hanning_window(S)
    a, c = GATE_OFFSETS
    recs = [  # tag, tr cell, tr blended target, lp cell, lp score target, d0 zero, d2 zero
        ("tr+a lp+a", 312, 0.05 + a, 84, 0.25 + a, 0, 0), ("tr+c lp-a", 287, 0.05 + c, 70, 0.25 - a, 0, 0),
        ("tr-a lp-by-stop", 313, 0.05 - a, 85, None, 0, 0), ("tr-c lp-c", 262, 0.05 - c, 98, 0.25 - c, 0, 0),
        ("tr lp+c", 140, None, 45, 0.25 + c, 0, 0), ("d0=0 d2=0", 200, None, 31, None, 1, 1), ("d0=0", 201, None, 100, None, 1, 0),
        ("d2=0", 450, None, 127, None, 0, 1), ("d0 d2", 451, None, 150, None, 0, 0)]
    B = len(recs)
    cls, cls_lp = logit_maps([[] for _ in recs], S, ch, lo=-12.0), logit_maps([[] for _ in recs], S_lp, ch)
    loc_c, loc_lp = loc_c_maps(B, S, per_record=True), loc_lp_maps(B, S_lp, per_record=True)
    pts_lp = TO.generate_points(8, S_lp)
    for b, (_, ct, pt, cl, sl, z0, z2) in enumerate(recs):
        x = HI if pt is None else logit_of((pt - win[ct] * GATE_WI) / keep)
        cls.reshape(B, ch, -1)[b, ch - 1, ct] = x
        cls_lp.reshape(B, ch, -1)[b, ch - 1, cl] = HI if sl is None else logit_of(sl)
        if z0:
            loc_lp.reshape(B, 4, -1)[b, 0, cl] = pts_lp[cl, 0] / 8.0
        if z2:
            loc_lp.reshape(B, 4, -1)[b, 2, cl] = pts_lp[cl, 1] / 8.0
    f = Family(f"gates-ch{ch}", "gates", "both", ch, GATE_WI, S, win, cls, loc_c, S_lp, cls_lp, loc_lp, [r[0] for r in recs])
    f.targets = [(r[2], r[4]) for r in recs]
    f.zero_d = [(r[5], r[6]) for r in recs]
    return f


def _nonfinite_maps(S, ch, peak, before, after, inf_cell):
    """-> (maps [B,ch,S,S], tags, rows without a non-finite value).  NaN goes into the class-1 plane (the single plane) unless said otherwise."""
    n, nan = S * S, np.float32(np.nan)
    tags = ["clean", "nan-before", "nan-after", "clean", "nan-two", "nan-last", "inf-both", "all-nan", "clean"]
    maps = logit_maps([[peak], [peak], [peak], [peak + 1], [peak], [peak], [peak], [peak], [peak - 1]], S, ch)
    m = maps.reshape(len(tags), ch, n)
    m[1, ch - 1, before] = nan
    m[2, ch - 1, after] = nan
    m[4, 0, before], m[4, ch - 1, after] = nan, nan        # ch = 2: the earlier one in the class-0 plane
    m[5, ch - 1, n - 1] = nan
    m[6, :, inf_cell] = np.inf                             # softmax: inf - inf = NaN; sigmoid: exactly 1
    m[7] = nan
    return maps, tags, [0, 3, 8]


@functools.lru_cache(maxsize=None)
def nonfinite(ch, idle=False):
    """Production sizes (S = 25 / 13, NaNs at cells 77 and 400 around the peak at 310), or S = 7 for both kernels: n = 49 < 64, idle lanes in the butterfly."""
    if idle:
        S, S_lp, cells, cells_lp = 7, 7, (30, 20, 41, 10), (25, 5, 47, 33)
    else:
        S, S_lp, cells, cells_lp = 25, 13, (310, 77, 400, 130), (100, 30, 120, 50)
    cls, tags, clean = _nonfinite_maps(S, ch, *cells)
    cls_lp, _, _ = _nonfinite_maps(S_lp, ch, *cells_lp)
    B = len(tags)
    return Family(f"nonfinite-{'S7' if idle else 'prod'}-ch{ch}", "nonfinite", "both", ch, WI, S, TO.hanning_window(S), cls, loc_c_maps(B, S, True), S_lp,
                  cls_lp, loc_lp_maps(B, S_lp, True), tags, clean)


@functools.lru_cache(maxsize=None)
def nan_window(ch):
    """Finite logits, a NaN in the window table (cell 50): every record of the launch answers cell 50 with a finite best_score and a NaN pscore."""
    S = 25
    win = TO.hanning_window(S)
    win[50] = np.nan
    hot = [[300], [7], [50], [624]]
    S_lp, cls_lp, loc_lp = _filler_lp(len(hot), ch, 13)
    return Family(f"nonfinite-window-ch{ch}", "nonfinite", "tr", ch, WI, S, win, logit_maps(hot, S, ch), loc_c_maps(len(hot), S, True), S_lp, cls_lp, loc_lp,
                  ["nan-window"] * len(hot), [])


def finite_families():
    out = [sweep(S, ch) for S in TR_SWEEP_SIZES for ch in (2, 1)]
    out += [ties(k, S, ch) for k in ("tr", "lp") for S in TIE_SIZES[k] for ch in (2, 1)]
    return out + [gates(ch) for ch in (2, 1)]


def nonfinite_families():
    return [nonfinite(ch, idle) for idle in (False, True) for ch in (2, 1)] + [nan_window(ch) for ch in (2, 1)]


# ------------------------------------------------------------------------------------------------------------------------------------ the kernel, in numpy
def kernel_argmax(V, variant=None):
    """csrc/similarity.hip's argmax of every row of V [B, n] (float64 as the kernel compares): lane l starts from cell l (an idle lane of n < 64 from
    cell 0), scans l + 64, l + 128, ..., six __shfl_xor steps 32 ... 1 merge the lanes, lane 0 answers.  -> int64 [B].  variant: one of WRONG
    ('plane' is not an argmax mistake: restate() applies it)."""
    V = np.atleast_2d(np.asarray(V, np.float64))
    B, n = V.shape
    lanes = np.arange(WAVE)
    old = variant == "nan_skipped"            # the kernel before the fix: -inf / no cell to start from, `>` alone

    def scan_takes(ov, v):
        if old:
            return ov > v
        first_nan = np.isnan(ov) & ~np.isnan(v)
        return first_nan | ((ov >= v) if variant == "scan_ge" else (ov > v))

    def merge_takes(ov, oi, v, i):
        lower = (oi > i) if variant == "tiebreak_reversed" else (oi < i)
        if variant == "no_tiebreak":
            lower = np.zeros_like(lower)
        finite = (ov > v) | ((ov == v) & lower)
        if old:
            return finite
        on, vn = np.isnan(ov), np.isnan(v)
        return np.where(on | vn, on & (~vn | lower), finite)

    if old:
        v, i = np.full((B, WAVE), -np.inf), np.full((B, WAVE), NO_CELL, np.int64)
    else:
        i = np.broadcast_to(np.where(lanes < n, lanes, 0), (B, WAVE)).astype(np.int64)
        v = V[:, i[0]].copy()
    limit = n - n % WAVE if variant == "scan_short" else n
    for r in range(0 if old else 1, -(-n // WAVE)):
        c = lanes + WAVE * r
        ov = V[:, np.minimum(c, n - 1)]
        t = (c < limit)[None, :] & scan_takes(ov, v)
        v, i = np.where(t, ov, v), np.where(t, c[None, :], i)
    s = WAVE // 2
    while s >= 1:
        ov, oi = v[:, lanes ^ s], i[:, lanes ^ s]
        t = merge_takes(ov, oi, v, i)
        v, i = np.where(t, ov, v), np.where(t, oi, i)
        s //= 2
    return i[:, 0]


def restate(f, variant=None):
    """What the two kernels, restated, answer for the family: dict of best_idx, delta [B,2] (translation), best_idx_lp, rot_delta (log-polar).  The
    blended scores are the oracle's own maps; only the argmax and the reads that follow it are restated.  An index outside the map gives NaN fields."""
    e = f.expected()
    n, n_lp = f.S * f.S, f.S_lp * f.S_lp
    second, second_lp = (0, 0) if variant == "plane" else (n, 2 * n_lp)       # 'plane': the second regression value read from the first plane
    idx, idx_lp = kernel_argmax(e["pscore_map"], variant), kernel_argmax(e["score_lp_map"], variant)
    delta, rot = np.full((f.B, 2), np.nan), np.full(f.B, np.nan)
    for b in range(f.B):
        i, j = int(idx[b]), int(idx_lp[b])
        stop = 0
        if 0 <= i < n:
            stop = int(e["pscore_map"][b][i] < 0.05)
            loc = f.loc_c[b].reshape(-1)
            px = f.points[i, 0] - loc[i] * np.float32(8)
            py = f.points[i, 1] - loc[second + i] * np.float32(8)
            delta[b] = (0.0, 0.0) if stop else (np.float64(px) / (EXEMPLAR / f.seq[b, 2]), np.float64(py) / (EXEMPLAR / f.seq[b, 2]))
        if 0 <= j < n_lp:
            if stop or e["score_lp_map"][b][j] < 0.25:
                rot[b] = 0.0
            else:
                d2 = f.points_lp[j, 1] - f.loc_lp[b].reshape(-1)[second_lp + j] * np.float32(8)
                rot[b] = np.float64(np.float32(d2) * np.float32(ROT_UNIT))
    return {"best_idx": idx, "delta": delta, "best_idx_lp": idx_lp, "rot_delta": rot}


def rejects(f, variant):
    """Does the family tell the restated kernel with `variant` from the expectation?  -> the first differing (field, record) or None."""
    e, r = f.expected(), restate(f, variant)
    for k in ("best_idx", "best_idx_lp", "delta", "rot_delta"):
        same = np.isclose(np.asarray(r[k], np.float64), np.asarray(e[k], np.float64), rtol=0, atol=0, equal_nan=True)
        if not same.all():
            return k, int(np.argwhere(~same.reshape(f.B, -1).all(1))[0, 0])
    return None


def where(i):
    """A cell as the kernel meets it: (lane, round)."""
    i = int(i)
    return f"cell {i} (lane {i % WAVE}, round {i // WAVE})" if 0 <= i < NO_CELL else f"cell {i} (no cell of the map)"


def mismatch(kernel, f, b, want, got):
    S = f.S if kernel == "translation" else f.S_lp
    return f"{kernel} kernel, {f.name} [{f.tags[b]}], S = {S}, cls_channels = {f.ch}, record {b}: expected {where(want)}, got {where(got)}"
