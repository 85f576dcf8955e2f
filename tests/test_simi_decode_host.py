"""No GPU: the fixtures of tests/simi_decode_cases.py are proven on the CPU before tests/test_gpu_simi_decode.py runs them on the device.

    * every expectation is the oracle's (decode_translation / decode_logpolar), and where the design allows it plain index arithmetic;
    * the margins that make the expectations independent of the device's expf hold;
    * the tie sets are built on the kernel's lane structure, the sweep sizes cover idle lanes, exactly one wave and a ragged last round;
    * the kernel's argmax restated in numpy (per-lane strided scan + six-step xor butterfly) passes every family, and each wrong version of
      simi_decode_cases.WRONG is rejected by the families named in REJECTED_BY - the finite families alone all pass the NaN-skipping version,
      which is the kernel as it stood before it followed np.argmax;
    * the entry points' error codes for S = 1025 and a NaN exemplar_size, from host pointers (no launch)."""
import ctypes

import numpy as np
import pytest

import simi_decode_cases as C
from oracle import tracker_oracle as TO

# wrong version -> the family kinds that must reject it (some family of each named kind does); every kind not named passes it
REJECTED_BY = {
    "no_tiebreak": {"ties", "nonfinite"},          # lane 0 keeps its own later cell against another lane's equal, earlier one (two NaNs are such a tie)
    "tiebreak_reversed": {"ties", "nonfinite"},
    "scan_ge": {"ties"},                           # only a lane that meets two equal cells: n > 64
    "scan_short": {"sweep", "ties", "gates", "nonfinite"},   # every family with a winner in the ragged last round
    "plane": {"sweep", "ties", "gates", "nonfinite"},
    "nan_skipped": {"nonfinite"},
}


def _families():
    return C.finite_families() + C.nonfinite_families()


def test_sweep_expectations_are_index_arithmetic_and_hold_a_margin():
    """Record b answers cell b, un-gated, with centre (points[b] - 8 loc[:, b]) / (127 / s_z); the winner leads the runner-up's blended score by >= 0.66."""
    sizes = {S * S for S in C.TR_SWEEP_SIZES}
    assert any(n < C.WAVE for n in sizes) and C.WAVE in sizes and any(n > C.WAVE and n % C.WAVE for n in sizes)
    assert {S * S for S in C.LP_SWEEP_SIZES} & {1, 4, 49, 64, 81, 169} == {1, 4, 49, 64, 81, 169}
    for ch in (2, 1):
        for S in C.TR_SWEEP_SIZES:
            f, n = C.sweep(S, ch), S * S
            e = f.expected()
            assert f.B == n and e["best_idx"].tolist() == list(range(n)) and not e["stop"].any(), f
            loc = f.loc_c.reshape(n, 2, n)
            b = np.arange(n)
            pred = np.stack([f.points[:, 0] - 8 * loc[b, 0, b], f.points[:, 1] - 8 * loc[b, 1, b]], 1)
            assert pred.dtype == np.float32
            np.testing.assert_array_equal(e["delta"], pred.astype(np.float64) / (127.0 / f.seq[:, 2:3]))
            np.testing.assert_array_equal(e["center"], e["delta"] + f.seq[:, 0:2])
            if n > 1:
                m = np.stack(e["pscore_map"])
                lead = m[b, b] - np.where(np.eye(n, dtype=bool), -np.inf, m).max(1)
                assert lead.min() >= 0.66, (f, lead.min())
            if S in C.LP_SWEEP_SIZES:
                assert e["best_idx_lp"].tolist() == list(range(n)) and not e["gated"].any(), f
                d2 = f.points_lp[:, 1] - 8 * f.loc_lp.reshape(n, 4, n)[b, 2, b]
                np.testing.assert_array_equal(e["rot_delta"], (d2 * np.float32(C.ROT_UNIT)).astype(np.float64))
                if n > 1:
                    m = np.stack(e["score_lp_map"])
                    assert (m[b, b] - np.where(np.eye(n, dtype=bool), -np.inf, m).max(1)).min() >= 0.99
            # another cell or the other plane is another number: the regression values at the winner differ between the planes somewhere
            assert n == 1 or (loc[0, 0] != loc[0, 1]).any()


def test_tie_sets_follow_the_lane_structure():
    """For every xor distance a tied pair whose lower index sits in the lower lane and (n > 64) one whose lower index sits in the higher lane; the
    same lane one round and nine rounds later; the last cell.  The expected cell of every tie record is the smallest tied index."""
    for kernel, sizes in C.TIE_SIZES.items():
        for S in sizes:
            n = S * S
            cells = C.tie_set(n)
            pairs, triples = C.tie_groups(n)
            assert n - 1 in cells and len(triples) == 12 and len(pairs) == len(cells) * (len(cells) - 1) // 2
            for s in (1, 2, 4, 8, 16, 32):
                meet = [(a, b) for a, b in pairs if (a % C.WAVE) ^ (b % C.WAVE) == s]          # a < b
                assert any(a % C.WAVE < b % C.WAVE for a, b in meet), (n, s)
                if n > C.WAVE:
                    assert any(a % C.WAVE > b % C.WAVE for a, b in meet), (n, s)
            if n > C.WAVE:
                assert (0, 64) in pairs          # one lane, two rounds
            else:
                assert n < C.WAVE                # idle lanes take part in the butterfly
            for ch in (2, 1):
                f = C.ties(kernel, S, ch)
                e = f.expected()
                want = [min(g) for g in pairs + triples] + [0, 0]
                got = e["best_idx"] if kernel == "tr" else e["best_idx_lp"]
                assert got.tolist() == want and f.wi == 0.0, f
                assert not e["stop"].any() and not e["gated"].any()
                # the tied scores are equal bits in the oracle's map, and the saturated map is exactly 1
                maps = e["pscore_map"] if kernel == "tr" else e["score_lp_map"]
                for b, g in enumerate(pairs + triples):
                    assert len({maps[b][c] for c in g}) == 1 and maps[b][g[0]] > np.delete(maps[b], list(g)).max()
                assert (maps[-1] == 1.0).all() and len(set(maps[-2])) == 1
    assert (0, 576) in C.tie_groups(625)[0] and 624 in C.tie_set(625)      # nine rounds later; the last cell


def test_gate_fixtures_sit_beside_the_gates():
    lo, hi = 1e-4, 1e-2
    for ch in (2, 1):
        f = C.gates(ch)
        e = f.expected()
        sides_t, sides_l = set(), set()
        for b, (pt, sl) in enumerate(f.targets):
            if pt is not None:
                d = e["pscore"][b] - 0.05
                assert lo <= abs(d) <= hi and abs(e["pscore"][b] - pt) <= 1e-6, (f, b, d)
                assert e["stop"][b] == int(d < 0)
                sides_t.add(d > 0)
                # the winner is far from the runner-up: the 0.03 floor of the window blend at the map's centre
                assert e["pscore"][b] - np.delete(e["pscore_map"][b], e["best_idx"][b]).max() >= 0.01
            if sl is not None:
                d = e["score_lp"][b] - 0.25
                assert lo <= abs(d) <= hi and abs(e["score_lp"][b] - sl) <= 1e-6, (f, b, d)
                assert e["gated"][b] == int(d < 0 or e["stop"][b])
                sides_l.add(d > 0)
        assert sides_t == sides_l == {True, False}
        by_stop = f.tags.index("tr-a lp-by-stop")
        assert e["stop"][by_stop] == 1 and e["score_lp"][by_stop] > 0.9 and e["gated"][by_stop] == 1
        assert (e["delta"][by_stop] == 0).all() and e["scale_delta"][by_stop] == 1.0 and e["rot_delta"][by_stop] == 0.0
        # un-gated answers with scale exactly 1 and / or rotation exactly 0: both branches of H_sim skipped and taken
        combos = set()
        for b, (z0, z2) in enumerate(f.zero_d):
            if f.tags[b].startswith("d"):
                assert e["gated"][b] == 0 and (e["sim0"][b] == 1.0) == bool(z0) and (e["scale_delta"][b] == 1.0) == bool(z0), (f, b)
                assert (e["rot_delta"][b] == 0.0) == bool(z2), (f, b)
                combos.add((z0, z2))
        assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_nonfinite_expectations_are_numpys():
    """np.argmax: the first NaN, else the maximum; an all-NaN map answers 0; a NaN winner is decoded, never gated."""
    assert int(np.argmax([1, np.nan, 5, np.nan])) == 1 and int(np.argmax(np.full(5, np.nan))) == 0
    for f in C.nonfinite_families():
        e = f.expected()
        assert not e["stop"].any() and not e["gated"].any(), f
        assert np.isfinite(e["delta"]).all() and np.isfinite(e["scale_delta"]).all() and np.isfinite(e["rot_delta"]).all()
        for b, tag in enumerate(f.tags):
            for idx, m, sc in ((e["best_idx"][b], e["pscore_map"][b], e["pscore"][b]), (e["best_idx_lp"][b], e["score_lp_map"][b], e["score_lp"][b])):
                nans = np.flatnonzero(np.isnan(m))
                if nans.size:
                    assert idx == nans[0] and np.isnan(sc), (f, b, tag)
                else:
                    assert idx == int(np.argmax(m)) and np.isfinite(sc) and np.sort(m)[-1] - np.sort(m)[-2] > 1e-3, (f, b, tag)
            if tag == "all-nan":
                assert e["best_idx"][b] == 0 and e["best_idx_lp"][b] == 0 and np.isnan(e["best_score"][b])
            if tag == "clean":
                assert np.isfinite(f.cls[b]).all() and np.isfinite(f.cls_lp[b]).all() and np.isfinite(e["pscore"][b])
            if tag == "nan-window":
                assert e["best_idx"][b] == 50 and np.isnan(e["pscore"][b]) and np.isfinite(e["best_score"][b])
        if f.clean:
            assert [f.tags[b] for b in f.clean] == ["clean"] * len(f.clean) and 0 < len(f.clean) < f.B
    tags = set(C.nonfinite(2).tags)
    assert {"nan-before", "nan-after", "nan-two", "nan-last", "inf-both", "all-nan"} <= tags
    f = C.nonfinite(2)
    e = f.expected()
    assert e["best_idx"][f.tags.index("nan-two")] == 77 and e["best_idx"][f.tags.index("nan-last")] == 624
    assert np.isnan(e["pscore"][f.tags.index("inf-both")])          # softmax of (inf, inf): NaN


def test_restated_kernel_passes_every_family():
    for f in _families():
        assert C.rejects(f, None) is None, f


@pytest.mark.parametrize("variant", C.WRONG)
def test_wrong_versions_are_rejected_by_the_named_families(variant):
    hits = {}
    for f in _families():
        r = C.rejects(f, variant)
        if r is not None:
            hits.setdefault(f.kind, []).append((f.name,) + r)
    print(variant, "rejected by", {k: [h[0] for h in v] for k, v in hits.items()})
    assert set(hits) == REJECTED_BY[variant], (variant, hits)
    if variant == "nan_skipped":
        # the kernel as it stood: every finite family passes it, every non-finite family rejects it
        assert all(C.rejects(f, variant) is None for f in C.finite_families())
        assert all(C.rejects(f, variant) is not None for f in C.nonfinite_families())
        # and on an all-NaN map it holds no cell at all
        assert int(C.kernel_argmax(np.full((1, 625), np.nan), variant)[0]) == C.NO_CELL
    if variant in ("no_tiebreak", "tiebreak_reversed", "scan_ge"):
        assert all(C.rejects(C.sweep(S, 2), variant) is None for S in C.TR_SWEEP_SIZES)      # a sweep has no ties: it cannot see these
    if variant == "scan_short":
        assert all(C.rejects(C.sweep(S, 2), variant) is not None for S in (9, 13, 25, 31))      # n mod 64 != 0 and n > 64


def test_restated_argmax_is_numpys_on_random_maps_with_ties_and_nans():
    g = np.random.default_rng(20261020)
    for n in (1, 5, 49, 63, 64, 65, 128, 169, 625, 961):
        V = g.integers(0, 4, (40, n)).astype(np.float64)          # many exact ties
        V[g.random((40, n)) < 0.02] = np.nan
        V[0], V[1] = np.nan, -np.inf
        np.testing.assert_array_equal(C.kernel_argmax(V), np.argmax(V, 1))


def test_entry_points_refuse_bad_sizes_before_any_launch():
    from hdn_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    assert lib.hdn_similarity_translation_f32(one, one, one, one, one, one, 1, 1025, 0.16, 8.0, 127.0, 2, None) == -3          # HDN_E_LIMIT
    assert lib.hdn_similarity_logpolar_f32(one, one, one, one, one, 1, 1025, 8.0, 0.03, 0.05, 2, None) == -3
    assert lib.hdn_similarity_translation_f32(one, one, one, one, one, one, 1, 25, 0.16, 8.0, float("nan"), 2, None) == -2     # HDN_E_SHAPE
    assert lib.hdn_similarity_translation_f32(one, one, one, one, one, one, 1, 25, 0.16, 8.0, 0.0, 1, None) == -2
