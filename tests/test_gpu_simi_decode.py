"""csrc/similarity.hip through the raw C ABI (-m gpu).

The decode kernels (hdn_similarity_translation_f32 then hdn_similarity_logpolar_f32) run every fixture of tests/simi_decode_cases.py - the maximum in
every cell, exact ties placed on the kernel's lane structure, both gates from both sides, non-finite scores - against what the oracle's decode answers
(proven on the CPU by tests/test_simi_decode_host.py).  Indices, gates and the float32-only rotation are exact; the bounds on scores (1e-6), scale
(1e-6 relative to max(1, |scale|)), centre (1e-12) and H_sim (1e-12 at the device's own scale and rotation) are test_similarity_decode_golden's.

The one-lane-per-sequence kernels (hdn_simi_track_update_f64, its ragged form, hdn_track_prepare_f64, hdn_track_accumulate_f64) run at B = 63, 64, 65
and 130 - one workgroup short of full, full, and more than one - with every row bit-equal to the same row through a B = 1 call; the accumulate kernel's
w == 0 / eps edge, NaN score and float32 rounding of the points are checked against oracle.tracker_oracle.track_accumulate."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import simi_decode_cases as C  # noqa: E402

STATE = 48
UNWRITTEN = (14, 15, 29, 30, 31, 38, 39)          # doubles of a state record that neither decode kernel writes
PATTERN = 0x7FF8C0DE00000000                      # (a NaN payload: a float compare of it with anything is false, its bits are compared)
WORST = {"score": 0.0, "scale_rel": 0.0, "H_sim_own": 0.0, "H_sim_ref": 0.0, "center": 0.0}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _pattern(rows, cols, dev, base=PATTERN):
    return (base + torch.arange(rows * cols, dtype=torch.int64, device=dev)).view(rows, cols).view(torch.float64)


def _decode(dev, f):
    """Both kernels over the family's B records, into rows 1 ... B of a (B + 2)-row state that starts as a bit pattern -> int64 bits [B + 2, 48] (host).
    Asserts that no input changed and that the records before and after the batch and the unwritten doubles keep the pattern."""
    from hdn_amd import _lib
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = {k: d(getattr(f, k)) for k in ("cls", "loc_c", "window", "points", "seq", "cls_lp", "loc_lp", "points_lp")}
    before = {k: _bits(v).clone() for k, v in t.items()}
    state = _pattern(f.B + 2, STATE, dev)
    start = _bits(state).clone()
    p = lambda k: _lib.ptr(t[k])
    with _lib.device_guard(dev):
        _lib.check(lib.hdn_similarity_translation_f32(p("cls"), p("loc_c"), p("window"), p("points"), p("seq"), _lib.ptr(state[1]), f.B, f.S, f.wi, C.STRIDE,
                                                      C.EXEMPLAR, f.ch, st), "translation decode")
        _lib.check(lib.hdn_similarity_logpolar_f32(p("cls_lp"), p("loc_lp"), p("points_lp"), p("seq"), _lib.ptr(state[1]), f.B, f.S_lp, C.STRIDE, C.MAG,
                                                   C.ROT_UNIT, f.ch, st), "log-polar decode")
    torch.cuda.synchronize()
    for k, v in t.items():
        assert torch.equal(_bits(v), before[k]), f"{f.name}: the kernels changed their input {k}"
    got = _bits(state)
    assert torch.equal(got[0], start[0]) and torch.equal(got[-1], start[-1]), f"{f.name}: a record outside the batch was written"
    assert torch.equal(got[:, list(UNWRITTEN)], start[:, list(UNWRITTEN)]), f"{f.name}: a double no kernel owns was written"
    written = [q for q in range(STATE) if q not in UNWRITTEN]
    assert not (got[1:-1][:, written] == start[1:-1][:, written]).any(), f"{f.name}: a double of a record was left unwritten"
    return got.cpu().numpy()


def _close(name, f, got, want, tol):
    """|got - want| <= tol per record, NaN fields compared as NaN."""
    got, want, tol = np.asarray(got, np.float64), np.asarray(want, np.float64), np.broadcast_to(np.asarray(tol, np.float64), np.shape(want))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{f.name}: {name} NaN in records {np.flatnonzero((np.isnan(got) != nan).reshape(f.B, -1).any(1))[:8]}"
    err = np.where(nan, 0.0, np.abs(np.where(nan, 0.0, got) - np.where(nan, 0.0, want)))
    bad = err > tol
    assert not bad.any(), f"{f.name}: {name} off in records {np.flatnonzero(bad.reshape(f.B, -1).any(1))[:8]}, worst {err.max():.3e}"
    return float(err.max())


def _check(f, bits):
    from oracle import tracker_oracle as TO
    e, s = f.expected(), bits[1:-1].view(np.float64)
    for kernel, col, key in (("translation", 6, "best_idx"), ("log-polar", 18, "best_idx_lp")):
        got = s[:, col]
        for b in np.flatnonzero(got != e[key]):
            raise AssertionError(C.mismatch(kernel, f, int(b), int(e[key][b]), int(got[b]) if np.isfinite(got[b]) else C.NO_CELL))
    for name, col, key in (("stop", 4, "stop"), ("state[47]", 47, "gated"), ("rot_delta", 17, "rot_delta")):
        bad = np.flatnonzero(s[:, col] != e[key])
        assert bad.size == 0, f"{f.name}: {name} of record {bad[0]} [{f.tags[bad[0]]}]: expected {e[key][bad[0]]!r}, got {s[bad[0], col]!r}"
    WORST["score"] = max(WORST["score"], _close("best_score", f, s[:, 5], e["best_score"], 1e-6), _close("pscore", f, s[:, 7], e["pscore"], 1e-6),
                         _close("score_lp", f, s[:, 19], e["score_lp"], 1e-6))
    tol = 1e-6 * np.maximum(1.0, np.abs(e["scale_delta"]))
    WORST["scale_rel"] = max(WORST["scale_rel"], float((np.abs(s[:, 16] - e["scale_delta"]) / np.maximum(1.0, np.abs(e["scale_delta"]))).max()))
    _close("scale_delta", f, s[:, 16], e["scale_delta"], tol)
    _close("state[46]", f, s[:, 46], e["sim0"], 1e-6 * np.maximum(1.0, np.abs(e["sim0"])))
    gated = e["gated"] == 1
    assert (s[gated, 16] == 1.0).all() and (s[gated, 46] == 1.0).all() and (s[gated, 17] == 0.0).all()
    WORST["center"] = max(WORST["center"], _close("delta", f, s[:, 0:2], e["delta"], 1e-12 + 1e-12 * np.abs(e["delta"])),
                          _close("center", f, s[:, 2:4], e["center"], 1e-12 + 1e-12 * np.abs(e["center"])))
    for b in range(f.B):
        cx, cy, sd, rd = s[b, 2], s[b, 3], s[b, 16], s[b, 17]
        H = TO.rot_scale_around_center_shift_tran(e["center"][b][0], e["center"][b][1], e["rot_delta"][b], e["scale_delta"][b], e["delta"][b][0], e["delta"][b][1])
        H_own = TO.rot_scale_around_center_shift_tran(cx, cy, rd, sd, s[b, 0], s[b, 1])
        scale = max(1.0, np.abs(H).max())
        own, ref = np.abs(s[b, 20:29].reshape(3, 3) - H_own).max() / scale, np.abs(s[b, 20:29].reshape(3, 3) - H).max() / scale
        WORST["H_sim_own"], WORST["H_sim_ref"] = max(WORST["H_sim_own"], own), max(WORST["H_sim_ref"], ref)
        # (the distance from the oracle's H_sim inherits scale_delta's float32 ulp times the centre, as in test_similarity_decode_golden: measured, printed)
        assert own <= 1e-12, f"{f.name}: H_sim of record {b} [{f.tags[b]}]: {own:.3e} from rot_scale_around_center_shift_tran at its own scale / rotation"
        cc, ss = np.cos(-rd), np.sin(-rd)
        np.testing.assert_allclose(s[b, 32:38], [cc, -ss, cx - cx * cc + cy * ss, ss, cc, cy - cy * cc - cx * ss], rtol=0, atol=1e-10, err_msg=f"{f.name} {b}")
        np.testing.assert_allclose(s[b, 8:14], [cx, cy, f.seq[b, 3], 10.0, 20.0, 30.0], rtol=0, atol=0, err_msg=f"{f.name} {b}")
        np.testing.assert_allclose(s[b, 40:46], [cx, cy, f.seq[b, 4] * sd, 10.0, 20.0, 30.0], rtol=1e-15, atol=0, err_msg=f"{f.name} {b}")


def _run(dev, f):
    bits = _decode(dev, f)
    _check(f, bits)
    assert np.array_equal(_decode(dev, f), bits), f"{f.name}: two calls differ"
    return bits


@pytest.mark.parametrize("ch", [2, 1])
@pytest.mark.parametrize("S", C.TR_SWEEP_SIZES)
def test_every_cell_wins_once(dev, S, ch):
    """B = n = S * S records, record b's maximum in cell b: best_idx = b for both kernels, stop = 0, centre = (points[b] - 8 loc[:, b]) / (127 / s_z)."""
    f = C.sweep(S, ch)
    bits = _run(dev, f)
    assert bits[1:-1].view(np.float64)[:, 6].tolist() == list(range(S * S))
    print(f"{f.name}: worst so far {WORST}")


@pytest.mark.parametrize("ch", [2, 1])
@pytest.mark.parametrize("kernel,S", [(k, S) for k in ("tr", "lp") for S in C.TIE_SIZES[k]])
def test_exact_ties_keep_the_lowest_index(dev, kernel, S, ch):
    """Equal bits in cells chosen by lane and round: a lane's own two rounds, lane 0's partner at every xor distance with the lower index in either
    lane, idle lanes (n = 49), all cells equal, all cells saturated at exactly 1.0f."""
    _run(dev, C.ties(kernel, S, ch))


@pytest.mark.parametrize("ch", [2, 1])
def test_both_gates_from_both_sides(dev, ch):
    """Winners 2e-4 and 5e-3 either side of 0.05 and 0.25 (a hundred times the 1e-6 bound on a device score at the least); a log-polar record gated by
    `stop` alone; scale exactly 1 and rotation exactly 0 in an un-gated record, each alone and together (both branches of H_sim skipped and taken)."""
    f = C.gates(ch)
    s = _run(dev, f)[1:-1].view(np.float64)
    for b, (z0, z2) in enumerate(f.zero_d):
        if z0:
            assert s[b, 46] == 1.0 and s[b, 47] == 0.0 and s[b, 16] == 1.0
        if z0 and z2:
            np.testing.assert_array_equal(s[b, 20:29], [1, 0, s[b, 0], 0, 1, s[b, 1], 0, 0, 1])
    print(f"{f.name}: worst so far {WORST}")


@pytest.mark.parametrize("ch", [2, 1])
@pytest.mark.parametrize("which", ["prod", "S7", "window"])
def test_nonfinite_scores_follow_numpy_argmax(dev, which, ch):
    """NaN before / after the finite peak, two NaNs, a NaN in the last cell, in an idle-lane map, +inf in both classes, an all-NaN map, a NaN in the
    window table: the first NaN's cell (0 for the all-NaN map), stop = 0, its finite regression values decoded, NaN scores, the log-polar record decoded and
    not gated.  The clean records of the mixed batch are bit-equal to the same records launched without the others."""
    f = C.nan_window(ch) if which == "window" else C.nonfinite(ch, idle=which == "S7")
    bits = _run(dev, f)
    s = bits[1:-1].view(np.float64)
    n, n_lp = f.S * f.S, f.S_lp * f.S_lp
    assert ((0 <= s[:, 6]) & (s[:, 6] < n)).all() and ((0 <= s[:, 18]) & (s[:, 18] < n_lp)).all()
    if f.clean:
        alone = _run(dev, f.subset(f.clean))
        written = [q for q in range(STATE) if q not in UNWRITTEN]          # (the other doubles hold the start pattern of the row's position)
        assert np.array_equal(alone[1:-1][:, written], bits[1:-1][f.clean][:, written]), f"{f.name}: a clean record depends on its neighbours"


# --------------------------------------------------------------------------------------------- the one-lane-per-sequence kernels at more than one workgroup
BS = (63, 64, 65, 130)
DIMS = [(360, 640), (20, 640), (360, 30), (9, 70), (48, 160), (17, 65)]       # (H_b, W_b), as tests/test_gpu_simi_update_ragged.py
CAP = (360, 640)
BOXES = [(50, 40), (52, 38), (48, 42), (50, 40), (46, 44), (58, 36)]
SCALES = [1.0, 1.1, 0.95, 1.2, 1.15, 1.15]
THRESH, CONTEXT, RATIO = 0.5, 0.5, 2.0
NPTS, GATE = 4, 2.5


def _consts(zc):
    from hdn_amd.tracker import TRACK_CONST_DOUBLES
    k = np.zeros((len(zc), TRACK_CONST_DOUBLES))
    for b, z in enumerate(zc):
        S = np.diag([127 / (z[2] - z[0] + 1), 127 / (z[3] - z[1] + 1), 1.0]).astype(np.float32)
        Sh = np.array([[1, 0, -z[0]], [0, 1, -z[1]], [0, 0, 1]], np.float32)
        k[b, 0:9], k[b, 9:18] = np.linalg.inv(S).reshape(-1), S.reshape(-1)
        k[b, 18:27], k[b, 27:36], k[b, 36] = np.linalg.inv(Sh).reshape(-1), Sh.reshape(-1), GATE
    return k


def _lane_inputs(B):
    """Host inputs of the four kernels for B sequences, generated as tests/test_gpu_simi_update_ragged.py and
    test_track_bookkeeping_kernels_vs_restatement generate theirs."""
    from hdn_amd.simi_tracker import sequence_records
    from hdn_amd.similarity import TrackerConfig
    g = np.random.default_rng(20261020)
    state = g.uniform(-1.0, 1.0, (B, STATE))
    state[:, 2:4] = g.uniform(20.0, 300.0, (B, 2))
    state[:, 5], state[:, 7] = g.uniform(0.2, 1.0, B), g.uniform(0.2, 1.0, B)
    state[:, 17] = g.uniform(-0.2, 0.2, B)
    state[:, 46] = [SCALES[b % 6] for b in range(B)]
    state[:, 47] = g.integers(0, 2, B)
    tr, seq = [], []
    for b in range(B):
        w, h = BOXES[b % 6][0] + g.uniform(-0.5, 0.5), BOXES[b % 6][1] + g.uniform(-0.5, 0.5)
        cx, cy = g.uniform(60, 200, 2)
        t, s, _, _ = sequence_records([cx, cy, w, h, float(g.uniform(-0.3, 0.3))], (cx - w / 2, cy - h / 2), g.uniform(90, 130, 3), TrackerConfig())
        tr.append(t), seq.append(s)
    Ht = np.eye(3)[None] + g.normal(0, 0.05, (B, 3, 3)); Ht[:, 2, :2] *= 1e-3; Ht[:, :2, 2] *= 100
    Ht[2::7] = 0.0; Ht[2::7, 0, 0] = 1.0                                       # singular -> identity
    H_comp = np.eye(3)[None] + g.normal(0, 0.02, (B, 3, 3)); H_comp[:, 2, :2] *= 1e-2
    H_sim = np.eye(3)[None] + g.normal(0, 0.03, (B, 3, 3)); H_sim[:, 2] = [0, 0, 1]; H_sim[:, :2, 2] *= 200
    acc_state = np.zeros((B, STATE)); acc_state[:, 20:29] = H_sim.reshape(B, 9); acc_state[:, 5] = g.uniform(0, 1, B)
    score = np.resize(np.array([0.3, 2.4999, 2.5, 2.5001, 9.0, 1.0, np.nan], np.float32), B)
    zc = [np.array([100.0 + 3 * (b % 9), 50.0 + (b % 9), 300.0 + 5 * (b % 9), 180.0 + 2 * (b % 9)]) for b in range(B)]
    return {"state": state, "tr": np.stack(tr), "seq": np.stack(seq), "dims": np.array([DIMS[b % 6] for b in range(B)], np.int32),
            "Ht": Ht.reshape(B, 9), "H_comp": H_comp.reshape(B, 9), "acc_state": acc_state, "score": score, "consts": _consts(zc),
            "pts": g.uniform(0, 700, (B, NPTS, 2))}


def _lane_kernels(dev, x, rows, sentinel):
    """The four kernels (update, ragged update, prepare, accumulate) over the records `rows` in ONE call each -> dict of output bits, one row per record
    (+ one sentinel row behind the batch when asked, which must come back as it went in)."""
    from hdn_amd import _lib
    lib, st, B = _lib.load(), _lib.stream_ptr(dev), len(rows)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a[rows])).to(dev)
    extra = 1 if sentinel else 0

    def padded(a, base):          # the records, then a row of pattern
        t = _pattern(B + extra, a.shape[1], dev, base)
        t[:B] = d(a)
        return t

    out = {}
    with _lib.device_guard(dev):
        state = d(x["state"])
        for name in ("update", "ragged"):
            tr, seq, o = padded(x["tr"], PATTERN), padded(x["seq"], PATTERN + 4096), _pattern(B + extra, 20, dev, PATTERN + 8192)
            if name == "update":
                _lib.check(lib.hdn_simi_track_update_f64(_lib.ptr(state), _lib.ptr(tr), _lib.ptr(seq), _lib.ptr(o), B, CAP[1], CAP[0], THRESH, CONTEXT, RATIO, st), name)
            else:
                dims = d(x["dims"])
                _lib.check(lib.hdn_simi_track_update_ragged_f64(_lib.ptr(state), _lib.ptr(tr), _lib.ptr(seq), _lib.ptr(o), _lib.ptr(dims), B, CAP[0], CAP[1], THRESH,
                                                                CONTEXT, RATIO, st), name)
            out[name + ".tr"], out[name + ".seq"], out[name + ".out"] = tr, seq, o
        H_total, keep, inv = d(x["Ht"]), _pattern(B + extra, 9, dev), _pattern(B + extra, 9, dev, PATTERN + 4096)
        _lib.check(lib.hdn_track_prepare_f64(_lib.ptr(H_total), _lib.ptr(keep), _lib.ptr(inv), B, st), "prepare")
        out["prepare.Ht"], out["prepare.Hinv"] = keep, inv
        a = [d(x[k]) for k in ("acc_state", "H_comp", "score", "consts", "pts")]
        H_out = _pattern(B + extra, 9, dev, PATTERN + 8192)
        pts_out = _pattern(B + extra, 2 * NPTS + 1, dev).view(torch.int64).to(torch.int32).view(torch.float32)       # (low words of the pattern)
        _lib.check(lib.hdn_track_accumulate_f64(_lib.ptr(keep), _lib.ptr(a[0]), _lib.ptr(a[1]), _lib.ptr(a[2]), _lib.ptr(a[3]), _lib.ptr(a[4]), NPTS,
                                                _lib.ptr(H_out), _lib.ptr(pts_out), B, st), "accumulate")
        out["accumulate.H"], out["accumulate.out"] = H_out, pts_out
        torch.cuda.synchronize()
    if sentinel:
        fresh = {"update.tr": PATTERN, "update.seq": PATTERN + 4096, "update.out": PATTERN + 8192, "ragged.tr": PATTERN, "ragged.seq": PATTERN + 4096,
                 "ragged.out": PATTERN + 8192, "prepare.Ht": PATTERN, "prepare.Hinv": PATTERN + 4096, "accumulate.H": PATTERN + 8192}
        for k, base in fresh.items():
            assert torch.equal(_bits(out[k])[B], _bits(_pattern(B + 1, out[k].shape[1], dev, base))[B]), f"{k}: the row behind a batch of {B} was written"
        want = _pattern(B + 1, 2 * NPTS + 1, dev).view(torch.int64).to(torch.int32)[B]
        assert torch.equal(_bits(out["accumulate.out"])[B], want), f"accumulate.out: the row behind a batch of {B} was written"
    return {k: _bits(v)[:B].cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def lane_rows(dev):
    """Every record of the largest batch through B = 1 calls: computed once, never written."""
    x = _lane_inputs(max(BS))
    one = [_lane_kernels(dev, x, [b], sentinel=False) for b in range(max(BS))]
    return x, {k: np.concatenate([r[k] for r in one]) for k in one[0]}


@pytest.mark.parametrize("B", BS)
def test_one_lane_kernels_rows_equal_single_calls(dev, lane_rows, B):
    """One workgroup with an idle lane, exactly one, one lane of a second, and three: every row bit-equal to the same row through a B = 1 call, the
    row behind the batch untouched."""
    x, ref = lane_rows
    got = _lane_kernels(dev, x, list(range(B)), sentinel=True)
    for k, v in got.items():
        bad = np.flatnonzero((v != ref[k][:B]).reshape(B, -1).any(1))
        assert bad.size == 0, f"{k}: rows {bad[:8]} of a batch of {B} differ from their B = 1 call"
    # the rows are not trivially equal: the update moved every record, the singular H_total rows were reset, both sides of the score gate occur
    assert (got["update.tr"] != _bits(torch.from_numpy(x["tr"][:B])).numpy()).any(1).all()
    assert (got["update.out"] != got["ragged.out"]).any(1).sum() >= B // 2          # the ragged form clamps at each row's own frame
    eye = np.eye(3).reshape(-1).view(np.int64)
    assert all((got["prepare.Ht"][b] == eye).all() for b in range(2, B, 7))


@pytest.mark.parametrize("n_points", [1, 7])
def test_accumulate_edges_vs_oracle(dev, n_points):
    """hdn_track_accumulate_f64 against oracle.tracker_oracle.track_accumulate within test_track_bookkeeping_kernels_vs_restatement's bounds: w == 0 exactly
    and w = 2^-52 project to (0, 0), w = 2^-51 does not; a NaN homo_score is not above the gate (the residual is multiplied in); points that are not
    float32 numbers are projected from their float32 roundings."""
    from hdn_amd import _lib
    from oracle.tracker_oracle import perspective_transform, track_accumulate
    g = np.random.default_rng(20261021)
    rows = ["w=0", "w=2^-52", "w=2^-51", "nan-score", "f32-points", "plain"]
    B = len(rows)
    Ht = np.eye(3)[None] + g.normal(0, 0.05, (B, 3, 3)); Ht[:, 2, :2] *= 1e-3; Ht[:, :2, 2] *= 100
    Ht[0] = [[1, 0, 0], [0, 1, 0], [-0.25, 0, 1]]
    Ht[1] = [[1, 0, 0], [0, 1, 0], [-0.25, 2.0 ** -52, 1]]
    Ht[2] = [[1, 0, 0], [0, 1, 0], [-0.25, 2.0 ** -51, 1]]
    Ht[4] = [[64, 0, -44800], [0, 1, 0], [0, 0, 1]]
    H_sim = np.repeat(np.eye(3)[None], B, 0)
    H_sim[3] += g.normal(0, 0.03, (3, 3)); H_sim[3, 2] = [0, 0, 1]
    H_comp = np.eye(3)[None] + g.normal(0, 0.02, (B, 3, 3)); H_comp[:, 2, :2] *= 1e-2
    score = np.array([9.0, 9.0, 9.0, np.nan, 9.0, 1.0], np.float32)          # 9 > 2.5: the gate is closed, H = H_total @ H_sim
    pts = g.uniform(0, 700, (B, n_points, 2)).astype(np.float32).astype(np.float64)
    pts[0, 0] = [4.0, 33.0]
    pts[1, 0] = pts[2, 0] = [4.0, 1.0]
    pts[4, 0] = [700.0 + 3 * 2.0 ** -16, 123.0]                                # float32 spacing at 700 is 2^-14: rounds up by 2^-16
    zc = [np.array([100.0 + 3 * b, 50.0 + b, 300.0 + 5 * b, 180.0 + 2 * b]) for b in range(B)]
    state = np.zeros((B, STATE)); state[:, 20:29] = H_sim.reshape(B, 9); state[:, 5] = g.uniform(0, 1, B)
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = [d(Ht), d(state), d(H_comp), d(score), d(_consts(zc)), d(pts)]
    H_out = torch.empty((B, 9), dtype=torch.float64, device=dev)
    out = torch.empty((B, 2 * n_points + 1), dtype=torch.float32, device=dev)
    with _lib.device_guard(dev):
        _lib.check(lib.hdn_track_accumulate_f64(*[_lib.ptr(v) for v in t], n_points, _lib.ptr(H_out), _lib.ptr(out), B, st), "accumulate")
    torch.cuda.synchronize()
    H_out, out = H_out.cpu().numpy(), out.cpu().numpy()
    for b, tag in enumerate(rows):
        H_ref, p_ref = track_accumulate(Ht[b], H_sim[b], H_comp[b], score[b], zc[b], pts[b], GATE)
        np.testing.assert_allclose(H_out[b].reshape(3, 3), H_ref, rtol=1e-12, atol=1e-12 * np.abs(H_ref).max(), err_msg=tag)
        got = out[b, :2 * n_points].reshape(n_points, 2)
        np.testing.assert_allclose(got, p_ref, rtol=3e-7, atol=1e-4, err_msg=tag)
        assert out[b, 2 * n_points] == np.float32(state[b, 5])
        if tag in ("w=0", "w=2^-52"):
            assert (got[0] == 0).all() and (p_ref[0] == 0).all(), (tag, got[0])
        if tag == "w=2^-51":
            assert got[0].tolist() == [4 * 2.0 ** 51, 2.0 ** 51], got[0]
        if tag == "nan-score":      # with the gate closed the answer would be H_total @ H_sim: far from what both computed
            closed = Ht[b] @ H_sim[b]
            assert np.abs(H_ref - closed / closed[2, 2]).max() > 1e-3 * np.abs(H_ref).max()
        if tag == "f32-points":     # the projection of the float64 point itself is outside the bound: the float32 rounding was projected
            exact = 64.0 * pts[b, 0, 0] - 44800.0
            assert abs(exact - float(p_ref[0, 0])) > 1e-4 + 3e-7 * abs(float(p_ref[0, 0])) and float(p_ref[0, 0]) == 64.0 * 2.0 ** -14
            assert abs(float(got[0, 0]) - exact) > 1e-4 + 3e-7 * abs(exact)
    assert perspective_transform(np.array([[4.0, 1.0]]), Ht[1]).tolist() == [[0.0, 0.0]]
