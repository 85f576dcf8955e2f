"""Host side of tests/test_gpu_geometry_fwd.py: everything the GPU tests of the geometry forwards rely on, proven without a device.  The launch
constants restated in tests/geometry_fwd_cases.py stand in the sources and the case tables reach both sides of each of them; every "exact" fixture is
exact (float64 == fp32 == the oracle, bit for bit, on fp32 values); the position pattern's theta list is derived; every fixture reaches the branch it
is there for (counted, never zero); the fp32 restatement of the kernel's coordinates rounds every operation once; every r_ref is measured and printed."""
import numpy as np
import torch

import cv_semantics as S
import geometry_bwd_cases as GC
import geometry_fwd_cases as FC
from oracle import hdn_oracle as O


def _eq_nan(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


# ------------------------------------------------------------------------------------------------------------------------ constants, coverage
def test_restated_constants_stand_in_the_sources():
    for name, text in FC.SOURCE_FACTS:
        assert text in FC.source(name), (name, text)
    assert FC.WARP_PX_PER_BLOCK == 1024 and FC.L1_PASS == 16384 and FC.DLT_PER_WAVE == 8 and FC.DLT_PER_BLOCK == 32
    assert FC.rw_blocks(127, 127) == (FC.RW_BW, FC.RW_BH)


def test_case_tables_reach_both_sides_of_every_constant():
    px = [h * w for h, w in FC.WARP_FWD_SHAPES]
    assert min(px) < FC.HDN_BLOCK < sorted(px)[1] and any(FC.HDN_BLOCK < p < FC.WARP_PX_PER_BLOCK for p in px)
    assert sum(p > FC.WARP_PX_PER_BLOCK for p in px) >= 5 and any(p > 2 * FC.WARP_PX_PER_BLOCK for p in px)
    assert {(33, 33), (17, 65), (65, 33), (129, 9), (9, 129)} <= set(FC.WARP_FWD_SHAPES)
    assert all(h in (5, 9, 17, 33, 65, 129) and w in (5, 9, 17, 33, 65, 129) for h, w in FC.WARP_FWD_SHAPES + FC.POSITION_SHAPES)
    edge = [h * w for h, w in FC.WARP_EDGE_SHAPES]
    assert {FC.WARP_PX_PER_BLOCK - 1, FC.WARP_PX_PER_BLOCK, FC.WARP_PX_PER_BLOCK + 1, 127 * 127} == set(edge)
    assert any(H * W > FC.WARP_PX_PER_BLOCK and (H * W) % FC.WARP_PX_PER_BLOCK for H, W in FC.POSITION_SHAPES)
    # solve: either side of a lane group's wave (8 samples) and of a workgroup (32 samples), and several workgroups
    for edge in (FC.DLT_PER_WAVE, FC.DLT_PER_BLOCK):
        assert {edge - 1, edge, edge + 1} <= set(FC.DLT_FWD_BATCHES)
    assert 1 in FC.DLT_FWD_BATCHES and max(FC.DLT_FWD_BATCHES) > 8 * FC.DLT_PER_BLOCK
    # sampler: S S either side of one workgroup, and many workgroups
    ss = [FC.LOGPOLAR_DYADIC[0][0] ** 2, FC.LOGPOLAR_DYADIC[1][0] ** 2] + [c[4] ** 2 for c in FC.LOGPOLAR_FWD_RANDOM]
    assert FC.HDN_BLOCK in ss and FC.HDN_BLOCK + 33 in ss and min(ss) < FC.HDN_BLOCK and max(ss) > 60 * FC.HDN_BLOCK
    # refinement warp: the second grid-stride pass, and a block walk wider than 64
    cap = FC.RW_CAP * FC.HDN_BLOCK
    over = [(H, W) for H, W in FC.REFINE_SHAPES if H * W > cap]
    print(f"GEOMETRY-FWD refine_warp: shapes with a second grid-stride pass (H W > {cap}): {over}")
    assert over == [(129, 128)] and 127 * 127 < cap and (129, 128) in FC.REFINE_PROJECTIVE_SHAPES
    assert FC.rw_grid(129, 128) == FC.RW_CAP and FC.rw_grid(127, 127) == 64 and FC.rw_grid(8, 200) == 7 and FC.rw_grid(1, 1) == 1
    bws = {s: FC.rw_blocks(*s)[0] for s in FC.REFINE_SHAPES}
    assert bws[(8, 200)] == 128 and bws[(3, 300)] == 300 and bws[(127, 127)] == 64 and bws[(129, 128)] == 64 and bws[(1, 1)] == 1
    assert any(W > 64 and FC.rw_blocks(H, W)[0] != 64 for H, W in FC.REFINE_PROJECTIVE_SHAPES)
    # score: either side of a wave, the workgroup, and one 16-per-thread pass; three passes
    for edge in (FC.HDN_WAVE, FC.L1_THREADS, FC.L1_PASS):
        assert {edge - 1, edge, edge + 1} <= set(FC.L1_SIZES)
    assert 1 in FC.L1_SIZES and max(FC.L1_SIZES) > 2 * FC.L1_PASS and 127 * 127 in FC.L1_SIZES
    assert 16 * max(FC.L1_SIZES) < 2 ** 24 and {p for _, p in FC.L1_BATCH} == {0, 1, 37} and {b for b, _ in FC.L1_BATCH} == {1, 3, 5}
    assert any(n > FC.L1_PASS for n in FC.L1_BATCH_SIZES) and any(n < FC.L1_THREADS for n in FC.L1_BATCH_SIZES)


# ------------------------------------------------------------------------------------------------------------------------ warp
def _all_warp_fixtures():
    for si in range(len(FC.WARP_FWD_SHAPES)):
        for gi in range(len(FC.WARP_FWD_GROUPS)):
            U, theta = FC.warp_exact_fwd(si, gi)[:2]
            yield f"exact {si}/{gi}", U, theta
    for H, W in FC.POSITION_SHAPES:
        U, theta, _ = FC.position_problem(H, W)
        yield f"position {H}x{W}", U, theta
    for H, W in FC.WARP_DEGENERATE_SHAPES:
        U, theta, _ = FC.warp_degenerate_problem(H, W)
        yield f"degenerate {H}x{W}", U, theta
    for H, W in FC.WARP_EDGE_SHAPES:
        U, theta = FC.warp_random_fwd(H, W)[:2]
        yield f"random {H}x{W}", U, theta


def test_fp32_restatement_of_the_coordinates_is_single_rounded():
    """grid_coord32 is torch.linspace.  No float64 sum inside warp_xy32's restated fma lands on an fp32 tie on any fixture, so every operation is
    rounded once, as on the device, whatever this CPU is.  Against warp_coords in fp32 (the oracle's sgemm and elementwise path): the same bits,
    NaN equal to NaN, on the exact, position and degenerate fixtures (exact arithmetic: no order of additions matters); on the random ones a BLAS
    may add the three terms in another order, so only closeness is asked (printed: how many coordinates differ)."""
    for n in (2, 5, 9, 17, 25, 31, 32, 33, 41, 65, 127, 129):
        assert torch.equal(torch.from_numpy(FC.grid_coord32(n)), torch.linspace(-1.0, 1.0, n)), n
    FC.FMA_TIES[0] = 0
    for name, U, theta in _all_warp_fixtures():
        B, _, H, W = U.shape
        t, x, y = FC.warp_xy32(theta.numpy(), H, W)
        c = GC.warp_coords(theta, B, H, W, torch.float32)
        if name.startswith("random"):
            differ = int((torch.from_numpy(x) != c[5]).sum() + (torch.from_numpy(y) != c[6]).sum())
            print(f"GEOMETRY-FWD warp {name}: coordinates that differ from torch's fp32 path: {differ} of {2 * x.size}")
            assert torch.allclose(torch.from_numpy(x), c[5], rtol=1e-5, atol=1e-5) and torch.allclose(torch.from_numpy(y), c[6], rtol=1e-5, atol=1e-5), name
        else:
            assert _eq_nan(t, c[2]) and _eq_nan(x, c[5]) and _eq_nan(y, c[6]), name
    assert FC.FMA_TIES[0] == 0, FC.FMA_TIES


def test_warp_exact_fixtures_are_exact():
    """float64 transformer_rs == its fp32 evaluation == the oracle's transformer == warp_expect (the rule-based taps), bit for bit; the count too.
    Between them the fixtures push pixels past each border, clamp both taps to one index, and cancel there exactly."""
    past = np.zeros(4, np.int64)
    both = 0
    for si, (H, W) in enumerate(FC.WARP_FWD_SHAPES):
        for gi in range(len(FC.WARP_FWD_GROUPS)):
            U, theta, want, count = FC.warp_exact_fwd(si, gi)
            ref, cond = O.transformer(U, theta.reshape(-1, 3, 3), (H, W))
            assert _eq_nan(ref, want) and _eq_nan(GC.transformer_rs(U, theta, torch.float32), want), (si, gi)
            assert int(cond) == count == 3 * H * W
            assert _eq_nan(want.float(), want)
            exp = FC.warp_expect(U, theta)
            assert _eq_nan(exp["out"], want) and exp["count"] == count
            x, y = exp["xy"]
            past += np.array([(x < 0).sum(), (x >= W).sum(), (y < 0).sum(), (y >= H).sum()])
            x0, x1, y0, y1 = exp["taps"]
            same = (x0 == x1) | (y0 == y1)
            both += int(same.sum())
            finite = ~want.isnan().reshape(3, H * W, -1).any(2).numpy()
            assert bool((want.reshape(3, H * W, -1).numpy()[same & finite] == 0).all())           # both taps on one index: exactly 0
            if None in FC.WARP_FWD_GROUPS[gi]:
                b = FC.WARP_FWD_GROUPS[gi].index(None)
                assert bool(want[b].isnan().all()) and not bool(want[:b].isnan().any())            # samples do not mix
    print(f"GEOMETRY-FWD warp exact fixtures: pixels past left / right / top / bottom {past.tolist()}, with both taps of an axis on one index {both}")
    assert bool((past > 0).all()) and both > 0


def test_position_theta_list_is_derived():
    """Of the candidate shifts (in half grid steps) exactly those stay under which this CPU's fp32 evaluation of the pattern equals the integer
    arithmetic; the identity, whole and half steps must be among them, and a tap one position off must change the expectation."""
    for H, W in FC.POSITION_SHAPES:
        keep = FC.position_shifts(H, W)
        print(f"GEOMETRY-FWD position fixture {H}x{W}: exact under shifts (half grid steps) {keep}")
        assert {(0, 0), (2, 0), (0, -2), (1, 0), (0, 1), (2, -4)} <= set(keep)
        P = FC.pattern_planes(2, H, W)
        for c in range(2):
            p = P[c]
            assert bool((p[:, 1:] != p[:, :-1]).all()) and bool((p[1:] != p[:-1]).all()) and bool((p[1:, 1:] != p[:-1, :-1]).all())
            assert bool((p[1:, :-1] != p[:-1, 1:]).all())
        U, theta, want = FC.position_problem(H, W)
        assert _eq_nan(FC.warp_expect(U, theta)["out"], want)                                    # the rule-based float64 truth is the integer arithmetic
        assert not torch.equal(want[0, :, 1:], want[0, :, :-1])


def test_warp_degenerate_fixtures_reach_their_branches():
    """Counted on the fp32 coordinates: a nudged column, INT_MIN coordinates (out of range and NaN), |t| between the kernel's threshold and ten times
    it, |t| on the threshold.  The oracle's fp32 transformer gives the same count, and its r_ref is measured."""
    names = [n for n, _ in FC.WARP_DEGENERATE]
    for H, W in FC.WARP_DEGENERATE_SHAPES:
        U, theta, exp = FC.warp_degenerate_problem(H, W)
        gx = FC.grid_coord32(W)
        nudged = int((gx == 0).sum()) * H
        assert nudged == H and bool((exp["t"][names.index("nudge")].reshape(H, W)[:, W // 2] == np.float32(1e-6)).all())
        x, y = exp["xy"]
        with np.errstate(all="ignore"):
            out_of_range = ~((np.floor(x) >= -2147483648.0) & (np.floor(x) < 2147483648.0)) | ~((np.floor(y) >= -2147483648.0) & (np.floor(y) < 2147483648.0))
        n_min = {n: int(out_of_range[names.index(n)].sum()) for n in names}
        print(f"GEOMETRY-FWD warp degenerate {H}x{W}: nudged pixels {nudged}, pixels with an INT_MIN coordinate {n_min}")
        assert n_min["huge"] > 0 and n_min["nan_y"] == H * W and n_min["nan_t"] == H * W and n_min["nudge"] == 0 and n_min["tiny"] == 0
        assert int((FC.f2i_x86(np.floor(x[names.index("huge")])) == FC.INT_MIN).sum()) > 0
        assert FC.f2i_x86(np.array([np.nan, np.inf, -np.inf, 2147483648.0, -2147483648.0, -2147483904.0, 2147483520.0, -0.5])).tolist() == \
            [FC.INT_MIN, FC.INT_MIN, FC.INT_MIN, FC.INT_MIN, FC.INT_MIN, FC.INT_MIN, 2147483520, 0]
        assert FC._inc32(np.array([FC.INT_MIN, -1, 2 ** 31 - 1])).tolist() == [FC.INT_MIN + 1, 0, FC.INT_MIN]
        x0, x1, y0, y1 = exp["taps"]
        assert bool((x0[out_of_range] * 0 == 0).all()) and bool((y0[names.index("nan_y")] == 0).all()) and bool((y1[names.index("nan_y")] == 0).all())
        want_count = {"nudge": H * W, "zero_row": H * W, "huge": H * W, "nan_y": H * W, "nan_t": 0, "tiny": H * W, "edge": 0}
        assert {n: int(exp["per_sample_count"][i]) for i, n in enumerate(names)} == want_count
        assert 1e-7 < FC.TINY < 1e-6 and float(np.abs(exp["t"][names.index("tiny")]).max()) == FC.TINY
        assert float(np.abs(exp["t"][names.index("edge")]).max()) == FC.T_EDGE == float(np.float32(1e-7))
        ref, cond = O.transformer(U, theta.reshape(-1, 3, 3), (H, W))
        assert int(cond) == exp["count"] == sum(want_count.values())
        r = FC.km_check(ref, exp["out"], exp["M"], 0.0)
        print(f"GEOMETRY-FWD warp degenerate {H}x{W}: r_ref {r[0]:.3e} -> K = {FC.k_bound(r[0]):.3e}; irregular elements that differ from the oracle: {r[1]}")
        assert r[0] <= FC.k_bound(r[0]) and r[0] < 1e-6 and r[1] == 0
        # the tiny sample is exact: float64 transformer_rs gives the truth's bits and fp32 the same
        i = names.index("tiny")
        assert torch.equal(GC.transformer_rs(U[i:i + 1].double(), theta[i:i + 1].double())[0], exp["out"][i]) and torch.equal(ref[i].double(), exp["out"][i])


def test_warp_reference_ratios_on_random_data():
    for H, W in FC.WARP_EDGE_SHAPES:
        U, theta, exp, r = FC.warp_random_fwd(H, W)
        print(f"GEOMETRY-FWD warp N(0,1) {H}x{W}: r_ref {r:.3e} -> K = {FC.k_bound(r):.3e}")
        assert 0 < r < 1e-3 and bool(exp["out"].isfinite().all()) and exp["count"] == 2 * H * W
        # the fp32 restatement of the whole pixel against the oracle's fp32 transformer on this CPU: informational (a BLAS may order the sgemm's
        # additions otherwise); what is asserted is that the restatement lies as near to float64 as the oracle does
        r32 = FC.warp_expect32(U, theta)
        n = int((r32 != O.transformer(U, theta.reshape(-1, 3, 3), (H, W))[0]).sum())
        print(f"GEOMETRY-FWD warp N(0,1) {H}x{W}: elements of the fp32 restatement that differ from the oracle's fp32 output: {n} of {r32.numel()}")
        assert FC.km_check(r32, exp["out"], exp["M"], 0.0)[0] <= FC.k_bound(r)


def test_fp32_output_restatements_on_the_exact_fixtures():
    """warp_expect32 and logpolar_expect32 (numpy, every operation rounded once in the kernels' order) give the float64 truths' bits wherever fp32
    is exact, NaN for NaN, and the degenerate fixture's oracle bits (exact arithmetic or single operations: no order matters there)."""
    for si in range(len(FC.WARP_FWD_SHAPES)):
        for gi in range(len(FC.WARP_FWD_GROUPS)):
            U, theta, want, _ = FC.warp_exact_fwd(si, gi)
            assert _eq_nan(FC.warp_expect32(U, theta), want), (si, gi)
    for H, W in FC.POSITION_SHAPES:
        U, theta, want = FC.position_problem(H, W)
        assert _eq_nan(FC.warp_expect32(U, theta), want)
    for H, W in FC.WARP_DEGENERATE_SHAPES:
        U, theta, exp = FC.warp_degenerate_problem(H, W)
        assert _eq_nan(FC.warp_expect32(U, theta), O.transformer(U, theta.reshape(-1, 3, 3), (H, W))[0]), (H, W)
    for i in range(FC.N_LOGPOLAR_EXACT):
        x, polar, tabs, want, _ = FC.logpolar_exact_fwd(i)
        assert torch.equal(FC.logpolar_expect32(x, polar, tabs).double(), want), i
    for i in range(len(FC.LOGPOLAR_EXACT), FC.N_LOGPOLAR_EXACT):
        for x, polar, tabs in (FC.logpolar_poisoned(i, float("nan"), -1, -1), FC.logpolar_poisoned(i, float("inf"), None, FC.logpolar_inf_row(i))):
            assert _eq_nan(FC.logpolar_expect32(x, polar, tabs), FC.logpolar_expect(x, polar, tabs)[0]), i


def test_fused_reference_ratios():
    """r_ref of the fused kernel's warp: theta = normalise_rs(fp32(float64 dlt_rs)) (the device's H lies within one rounding of it), the oracle's
    fp32 transformer against float64 on the fp32 cells."""
    for H, W in FC.FUSED_SHAPES:
        h4p, off, img = FC.fused_problem(H, W)
        theta = FC.normalise_rs(FC.dlt_truth(h4p, off).float().numpy(), H, W)
        U = img.reshape(-1, 1, H, W)
        exp = FC.warp_expect(U, theta)
        r = FC.warp_r_ref(U, theta, exp)
        print(f"GEOMETRY-FWD fused warp N(0,1) {H}x{W}: r_ref {r:.3e} -> K = {FC.k_bound(r):.3e}")
        assert 0 < r < 1e-3 and FC.km_check(FC.warp_expect32(U, theta), exp["out"], exp["M"], 0.0)[0] <= FC.k_bound(r)


def test_fused_theta_restatement():
    """normalise_rs (single roundings on fractions) against torch's fp32 bmm chain: equal on the identity and within 2 ulp of it elsewhere (the
    kernel's order is the restated one); round32 rounds ties to even."""
    assert float(FC.round32(FC.Fraction(1) + FC.Fraction(1, 2 ** 24))) == 1.0 and float(FC.round32(FC.Fraction(1) + FC.Fraction(3, 2 ** 24))) == 1.0 + 2.0 ** -22
    for H, W in ((33, 33), (25, 41), (127, 127)):
        Hm = torch.tensor([[1, 0, 0, 0, 1, 0, 0, 0, 1], [1.01, 0.02, -1.5, 0.03, 0.98, 2.25, 1e-4, -1e-4, 1]], dtype=torch.float32)
        th = FC.normalise_rs(Hm.numpy(), H, W).double()
        M = torch.tensor([[W / 2, 0, W / 2], [0, H / 2, H / 2], [0, 0, 1]], dtype=torch.float64)
        want = torch.linalg.inv(M) @ Hm.double().reshape(-1, 3, 3) @ M
        assert float((th.reshape(-1, 3, 3) - want).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------------------------------ DLT solve
def test_dlt_fixtures_and_the_elimination():
    """The known maps come back from float64 dlt_rs; the float64 restatement of the kernel's elimination errs by less than 1e-3 of the bound; the
    production corners force row swaps; production and the tie quad meet ties in the pivot search, and either tie rule stays inside the bound."""
    names, src, off = FC.dlt_fixture_rows()
    truth = FC.dlt_truth(src, off)
    for i, (name, quad, Hm) in enumerate(FC.DLT_KNOWN):
        assert float((truth[i] - torch.tensor(Hm, dtype=torch.float64)).abs().max()) < 1e-11, name
        assert torch.equal((src[i] + off[i]).double(), torch.from_numpy(FC._apply(Hm, quad))), name
    # each corner displaced alone moves its own two rows: the four solutions differ, and differ from the identity
    corners = truth[len(FC.DLT_KNOWN):len(FC.DLT_KNOWN) + 4]
    assert all(float((corners[p] - corners[q]).abs().max()) > 1e-3 for p in range(4) for q in range(p))
    n_swaps, n_ties, worst = {}, {}, 0.0
    for i, name in enumerate(names):
        low, swaps, ties = FC.dlt_eliminate(src[i], off[i], "low")
        high, _, _ = FC.dlt_eliminate(src[i], off[i], "high")
        n_swaps[name], n_ties[name] = len(swaps), len(ties)
        for h in (low, high):
            got = torch.cat([torch.from_numpy(h), torch.ones(1, dtype=torch.float64)]).reshape(1, 9)
            worst = max(worst, FC.dlt_excess(got, truth[i:i + 1])[1])
    print(f"GEOMETRY-FWD DLT fixtures: row swaps {n_swaps}; pivot searches that met a tie {n_ties}; the float64 elimination's own error is "
          f"{worst:.3e} of the bound")
    assert worst < 1e-3                                                                           # the bound is the rounding to fp32
    assert n_swaps["production_random"] > 0 and n_swaps["shift_whole"] > 0
    assert n_ties["production_random"] > 0 and n_ties["tie_random"] > 0 and n_ties["shift_tie"] > 0
    low, s_low, _ = FC.dlt_eliminate(src[names.index("tie_random")], off[names.index("tie_random")], "low")
    high, s_high, _ = FC.dlt_eliminate(src[names.index("tie_random")], off[names.index("tie_random")], "high")
    assert s_low != s_high                                                                        # the tie rule changes the elimination's path
    # ... and its values: where H is exactly 0 the elimination leaves float64 residues that depend on the path.  At least one fixture's fp32 H
    # differs under the other tie rule, and at least one under the other point order, so bit-equality with dlt_restated pins both on the device
    low32 = FC.dlt_restated(src, off)
    by_tie = {n: int((FC.dlt_restated(src[i:i + 1], off[i:i + 1], tie="high") != low32[i:i + 1]).sum()) for i, n in enumerate(names)}
    by_order = {n: int((FC.dlt_restated(src[i:i + 1], off[i:i + 1], point=(0, 1, 2, 3)) != low32[i:i + 1]).sum()) for i, n in enumerate(names)}
    print(f"GEOMETRY-FWD DLT fixtures: fp32 values that change with ties to the highest row {by_tie}; with the point order (0, 1, 2, 3) {by_order}")
    assert by_tie["shift_tie"] > 0 and by_order["scale_order"] > 0
    assert FC.dlt_excess(low32, truth)[0] <= 0
    for B in (33, 65):                                                                            # the batches in which the GPU test meets them
        nm = FC.dlt_fwd_problem(B)[0]
        assert "shift_tie" in nm and "scale_order" in nm, (B, nm)
    for B in FC.DLT_FWD_BATCHES:
        nm, s, o, Ht = FC.dlt_fwd_problem(B)
        assert s.shape == (B, 8) and bool(Ht.isfinite().all()) and bool((Ht[:, 8] == 1).all())
    s, o = FC.dlt_degenerate_problem()
    assert bool((s[FC.DEGENERATE_AT].reshape(4, 2) == s[FC.DEGENERATE_AT, :2]).all()) and 0 < FC.DEGENERATE_AT < s.shape[0] - 1
    h = FC.dlt_eliminate(s[FC.DEGENERATE_AT], o[FC.DEGENERATE_AT])[0]
    assert not bool(np.isfinite(h).all())


# ------------------------------------------------------------------------------------------------------------------------ sampler
def test_sampler_exact_fixtures_are_exact():
    """float64 grid_sample == fp32 grid_sample == the rule-based truth (logpolar_expect) bit for bit, the grid too; every batched fixture has samples
    past each of the four borders; masked east and south taps are counted."""
    masked = np.zeros(2, np.int64)
    for i in range(FC.N_LOGPOLAR_EXACT):
        x, polar, tabs, want, grid = FC.logpolar_exact_fwd(i)
        B, C, H, W = x.shape
        assert torch.equal(GC.logpolar_rs(x, polar, tabs, torch.float32).double(), want), i
        assert torch.equal(FC.logpolar_expect(x, polar, tabs, torch.float32)[0], want) and torch.equal(FC.logpolar_expect(x, polar, tabs, torch.float64)[0], want), i
        assert torch.equal(FC.logpolar_grid32(polar, tabs, H, W).double(), grid) and torch.equal(want.float().double(), want)
        pxu, pyu = GC.logpolar_coords(polar, tabs, H, W, torch.float64)
        past = [int((pxu < 0).sum()), int((pxu > W - 1).sum()), int((pyu < 0).sum()), int((pyu > H - 1).sum())]
        _, _, e_ok, s_ok = FC.logpolar_cells(polar, tabs, H, W)
        masked += np.array([int((~e_ok).sum()), int((~s_ok).sum())])
        if B > 1:
            assert all(p > 0 for p in past), (i, past)
        if i >= len(FC.LOGPOLAR_EXACT):
            S = tabs[0].numel()
            print(f"GEOMETRY-FWD sampler dyadic fixture S={S} on {H}x{W}: samples past left / right / top / bottom {past}, "
                  f"masked east {int((~e_ok).sum())}, south {int((~s_ok).sum())}")
            assert H != W and int((~e_ok).sum()) > 0 and int((~s_ok).sum()) > 0 and int((~e_ok & s_ok).sum()) > 0
            assert bool((tabs[0] * 4 == (tabs[0] * 4).round()).all()) and set(tabs[1].tolist()) | set(tabs[2].tolist()) <= {0.0, 0.5, -0.5, 1.0, -1.0}
    assert bool((masked > 0).all())


def test_sampler_nan_reaches_only_the_unmasked_taps():
    """A NaN column at x = W - 1 and a NaN row at y = H - 1: float64 grid_sample is NaN exactly on logpolar_reach, the set computed from the tap
    rule; the set is neither empty nor everything.  With +inf in row logpolar_inf_row instead, the rule-based truth is grid_sample's (NaN equal to NaN) and
    holds +-inf where a masked south-east tap, if read with its weight 0, would turn it into NaN."""
    for i in range(len(FC.LOGPOLAR_EXACT), FC.N_LOGPOLAR_EXACT):
        x, polar, tabs = FC.logpolar_poisoned(i, float("nan"), -1, -1)
        H, W = x.shape[2:]
        reach = FC.logpolar_reach(polar, tabs, H, W, col=W - 1, row=H - 1)
        ref = GC.logpolar_rs(x.double(), polar.double(), tabs)
        assert torch.equal(ref.isnan(), reach.unsqueeze(1).expand_as(ref)) and 0 < int(reach.sum()) < reach.numel()
        assert _eq_nan(FC.logpolar_expect(x, polar, tabs)[0], ref)
        r = FC.logpolar_inf_row(i)
        x, polar, tabs = FC.logpolar_poisoned(i, float("inf"), None, r)
        want = FC.logpolar_expect(x, polar, tabs)[0]
        assert _eq_nan(want, GC.logpolar_rs(x.double(), polar.double(), tabs))
        x0, y0, e_ok, s_ok = FC.logpolar_cells(polar, tabs, H, W)
        at = (~e_ok & s_ok & (y0 + 1 == r)).unsqueeze(1).expand_as(want)
        print(f"GEOMETRY-FWD sampler fixture {i}: outputs whose masked south-east tap lies in the inf row {r}: {int(at.sum())}, of them infinite {int(want[at].isinf().sum())}")
        assert int(want[at].isinf().sum()) > 0


def test_sampler_reference_ratios_on_random_data():
    for case in FC.LOGPOLAR_FWD_RANDOM:
        x, polar, tabs, out, M, r = FC.logpolar_random_fwd(*case)
        B, C, H, W = x.shape
        print(f"GEOMETRY-FWD sampler N(0,1) {case}: r_ref {r:.3e} -> K = {FC.k_bound(r):.3e}")
        assert 0 < r < 1e-2 and bool(out.isfinite().all())
        rho, c, s = tabs
        gx = ((rho.unsqueeze(0) * c.unsqueeze(1)).unsqueeze(0) + polar[:, 0].reshape(B, 1, 1)) / (H // 2)
        gy = ((rho.unsqueeze(0) * s.unsqueeze(1)).unsqueeze(0) + polar[:, 1].reshape(B, 1, 1)) / (W // 2)
        assert torch.equal(FC.logpolar_grid32(polar, tabs, H, W), torch.stack([gx, gy], dim=3))


# ------------------------------------------------------------------------------------------------------------------------ refinement warp
def test_refine_exact_fixtures_are_exact():
    """Translations by multiples of 1/32 px on integer images: the oracle's refine_step == float64 bilinear-replicate == cv_semantics' ideal warp,
    bit for bit; a whole shift is index arithmetic; the shifts replicate all four borders; H_comp in the kernel's order is numpy's product to 1e-15."""
    sides = np.zeros(4, np.int64)
    for H, W in FC.REFINE_SHAPES:
        for B in (1, 5):
            Hm, img, want = FC.refine_exact_problem(H, W, B)
            for b in range(B):
                tx, ty = FC.REFINE_SHIFTS[b]
                w, _ = O.refine_step(Hm[b].reshape(3, 3).numpy(), img[b].numpy(), np.eye(3))
                assert np.array_equal(w.astype(np.float64), want[b].numpy()), (H, W, b)
                ideal, _ = S.warp_perspective(img[b].numpy(), Hm[b].reshape(3, 3).numpy().astype(np.float64))
                assert np.array_equal(ideal, want[b].numpy())
                if tx == int(tx) and ty == int(ty):
                    assert np.array_equal(FC.shifted_index(img[b].numpy(), tx, ty), want[b].numpy())
                sides += np.array([tx > 0, tx < 0, ty > 0, ty < 0])
            assert bool((img[0] == FC.pattern(H, W)).all())
    assert bool((sides > 0).all())
    for H, W in FC.REFINE_PROJECTIVE_SHAPES:
        Hm, img, Hc = FC.refine_projective_problem(H, W)
        for b in range(Hm.shape[0]):
            Hhm, _ = FC.refine_chain(Hm[b].numpy())
            np.testing.assert_allclose(FC.hcomp_product(Hc[b], Hhm), Hc[b] @ Hhm.astype(np.float64), rtol=1e-15, atol=0)
            np.testing.assert_array_equal(O.refine_step(Hm[b].reshape(3, 3).numpy(), img[b].numpy(), Hc[b])[1], Hc[b] @ Hhm.astype(np.float64))


def test_refine_projective_seed_keeps_the_oracle_inside_the_bar():
    """On the projective fixtures the oracle's restatement stays within cv_semantics.bar_float of the float64 ideal on every pixel but at most 16
    per call (the cap of the existing test), so the cap is a fair condition for the kernel against the oracle."""
    for H, W in FC.REFINE_PROJECTIVE_SHAPES:
        Hm, img, Hc = FC.refine_projective_problem(H, W)
        n_out, moved = 0, 0
        for b in range(Hm.shape[0]):
            _, M = FC.refine_chain(Hm[b].numpy())
            ref, L = S.warp_perspective(img[b].numpy(), M.astype(np.float64), ring=1)
            w, _ = O.refine_step(Hm[b].reshape(3, 3).numpy(), img[b].numpy(), Hc[b])
            n_out += int(S.violations(w, ref, S.bar_float(ref, L)).sum())
            moved += int((np.abs(w - img[b].numpy()) > 1e-3).sum())
        print(f"GEOMETRY-FWD refine_warp projective {H}x{W} seed {FC.REFINE_SEED}: oracle pixels outside bar_float {n_out} (cap 16)")
        assert n_out <= 16 and moved > H * W


def test_refine_tie_fixture_depends_on_the_block_walk():
    """On the tie fixture the restated walk is the oracle's at the rule's bw = 128 and differs from it, by more than 1e-5, on more than 16 pixels
    per sample when bw is held at 64: a kernel that walks the wrong blocks cannot stay inside the cap."""
    Hm, img = FC.refine_tie_problem()
    H, W = FC.REFINE_TIE_SHAPE
    assert FC.rw_blocks(H, W)[0] == 128
    for b in range(Hm.shape[0]):
        _, M = FC.refine_chain(Hm[b].numpy())
        ref = O.warp_perspective_replicate(img[b].numpy(), M.astype(np.float64))
        assert np.array_equal(FC.warp_perspective_bw(img[b].numpy(), M.astype(np.float64)), ref)
        n = int((np.abs(FC.warp_perspective_bw(img[b].numpy(), M.astype(np.float64), 64) - ref) > 1e-5).sum())
        ideal, L = S.warp_perspective(img[b].numpy(), M.astype(np.float64), ring=1)
        print(f"GEOMETRY-FWD refine_warp tie fixture sample {b}: pixels that bw = 64 moves: {n}")
        assert n > 16 and not S.violations(ref, ideal, S.bar_float(ideal, L)).any()


# ------------------------------------------------------------------------------------------------------------------------ score
def test_score_fixtures_are_exact_in_any_order():
    for n in FC.L1_SIZES:
        a, b0, b1, truth = FC.l1_problem(n)
        d = (a - b0).abs()
        assert float(d.double().sum()) < 2 ** 24 and float(d.max()) <= 16 and bool((d == d.round()).all())
        assert torch.equal(truth.float().double(), truth) and (float(truth[0, 0]) != float(truth[0, 1]) or n == 1)
        assert float(d.flip(1).cumsum(1)[0, -1]) * FC.L1_SCALE == float(truth[0, 0])              # another order, in fp32
    assert FC.L1_SCALE == 2.0 ** -7
