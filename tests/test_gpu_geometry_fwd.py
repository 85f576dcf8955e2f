"""The geometry forwards on the device through the raw C ABI - hdn_warp_count_f32 / hdn_warp_f32 / hdn_dlt_warp_strided_f32 / hdn_dlt_solve_f32 /
hdn_l1_score*_f32 (csrc/dlt_warp.hip), hdn_logpolar_sample_f32 (csrc/logpolar.hip) and hdn_refine_warp_f32 (csrc/refine_warp.hip) - against the
float64 truths of tests/geometry_fwd_cases.py: torch.equal on the fixtures on which fp32 is exact, every pixel inside K M on random data, exact tap
rules in the degenerate branches; from base pointers aligned and at odd float offsets, every output starting as NaN inside 0xA5 margins, the inputs
compared bit for bit afterwards.  tests/test_geometry_fwd_host.py proves on the CPU what these tests rely on."""
import numpy as np
import pytest
import torch

import cv_semantics as S
import geometry_fwd_cases as FC
from oracle import hdn_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _nhwc(H, W, C=None):
    def where(at):
        b, i, j = at[:3]
        return f"sample {b}, pixel ({i}, {j})" + (f", channel {at[3]}" if len(at) > 3 else "") + ", " + FC.where_warp(i * W + j)
    return where


def _inside(what, got, truth, M, K, where):
    r, n_bad, at = FC.km_check(got, truth, M, K)
    print(f"FORMS geometry forward {what}: worst |hip - f64| / M = {r:.3e} (K = {K:.3e}); irregular elements that differ: {n_bad}")
    assert r <= K and n_bad == 0, (what, r, K, n_bad, at, float(got[at]), float(truth[at]), where(at))
    return r


# ------------------------------------------------------------------------------------------------------------------------------ 1. warp
@pytest.mark.parametrize("si", range(len(FC.WARP_FWD_SHAPES)), ids=lambda i: "%dx%d" % FC.WARP_FWD_SHAPES[i])
def test_warp_exact_fixtures(dev, si):
    """Integer images, the eight dyadic thetas in calls of three samples (one sample all NaN): the NHWC output and the count equal float64
    transformer_rs; hdn_warp_f32 gives the bits of hdn_warp_count_f32 and leaves the count's place alone."""
    H, W = FC.WARP_FWD_SHAPES[si]
    for gi in range(len(FC.WARP_FWD_GROUPS)):
        U, theta, want, count = FC.warp_exact_fwd(si, gi)
        for off in FC.OFFSETS:
            got, n, clean, same = FC.run_warp(U, theta, dev, off)
            tag = ("hdn_warp_count_f32", (H, W), "thetas", FC.WARP_FWD_GROUPS[gi], "offsets", off)
            assert FC.difference(got, want, _nhwc(H, W), nan_equal=True) is None, (tag, FC.difference(got, want, _nhwc(H, W), nan_equal=True))
            assert n == count, (tag, n, count)
            assert clean and same, (tag, "written outside the results" if not clean else "an input changed")
            plain, _, clean, same = FC.run_warp(U, theta, dev, off, count=False)
            assert FC.difference(plain, got, _nhwc(H, W), nan_equal=True) is None and clean and same, ("hdn_warp_f32",) + tag[1:]


@pytest.mark.parametrize("H,W", FC.POSITION_SHAPES, ids=lambda v: str(v))
def test_warp_position_fixture(dev, H, W):
    """Patterns whose neighbours all differ under the identity and whole / half grid-step shifts: the output is index arithmetic on integers."""
    U, theta, want = FC.position_problem(H, W)
    for off in FC.OFFSETS:
        got, n, clean, same = FC.run_warp(U, theta, dev, off)
        d = FC.difference(got, want, _nhwc(H, W))
        assert d is None, ("hdn_warp_count_f32", (H, W), "shifts", FC.position_shifts(H, W), "offsets", off, d)
        assert n == U.shape[0] * H * W and clean and same


@pytest.mark.parametrize("H,W", FC.WARP_DEGENERATE_SHAPES, ids=lambda v: str(v))
def test_warp_degenerate_branches(dev, H, W):
    """The nudge (t == 0 on the centre column; an all-zero third row), coordinates beyond int32, NaN in theta, |t| between 1e-7 and 1e-6 and |t| ==
    1e-7f: the count, per sample, is the rule's; the values lie inside K M of float64 on the taps that the restated f2i_x86 / clamp rule picks, bit
    for bit where the truth is not finite or M is 0; the 2^-21 sample is exact."""
    U, theta, exp = FC.warp_degenerate_problem(H, W)
    K = FC.k_bound(FC.warp_r_ref(U, theta, exp))
    names = [n for n, _ in FC.WARP_DEGENERATE]
    for off in FC.OFFSETS:
        got, n, clean, same = FC.run_warp(U, theta, dev, off)
        assert clean and same, off
        assert n == exp["count"], ("hdn_warp_count_f32 count", (H, W), off, n, exp["count"])
        _inside(f"warp degenerate {H}x{W} offsets {off}", got, exp["out"], exp["M"], K, _nhwc(H, W))
        d = FC.difference(got, FC.warp_expect32(U, theta), _nhwc(H, W), nan_equal=True)
        assert d is None, ("hdn_warp_count_f32 against the fp32 restatement", (H, W), off, d)
        i = names.index("tiny")
        assert FC.difference(got[i], exp["out"][i]) is None, ("tiny", FC.difference(got[i], exp["out"][i]))
    for b, name in enumerate(names):
        one, n, clean, same = FC.run_warp(U[b:b + 1], theta[b:b + 1], dev, FC.OFFSETS[1])
        assert n == int(exp["per_sample_count"][b]), (name, n, int(exp["per_sample_count"][b]))
        assert FC.difference(one[0], got[b], nan_equal=True) is None and clean and same, name


@pytest.mark.parametrize("H,W", FC.WARP_EDGE_SHAPES, ids=lambda v: str(v))
def test_warp_block_and_tail_edges(dev, H, W):
    """1,023 / 1,024 / 1,025 pixels and the production plane, B = 2, C = 3, N(0,1) data, theta = I + 0.08 N(0,1): every pixel inside K M on the
    cells the fp32 coordinates pick, K = max(4 r_ref, 2e-6) with r_ref the oracle's fp32 transformer at the same shape, and bit-equal to
    warp_expect32, the numpy restatement of the kernel's own roundings."""
    U, theta, exp, r_ref = FC.warp_random_fwd(H, W)
    for off in FC.OFFSETS:
        got, n, clean, same = FC.run_warp(U, theta, dev, off)
        assert clean and same and n == exp["count"], (off, n)
        _inside(f"warp N(0,1) {H}x{W} (r_ref {r_ref:.3e}) offsets {off}", got, exp["out"], exp["M"], FC.k_bound(r_ref), _nhwc(H, W))
        d = FC.difference(got, FC.warp_expect32(U, theta), _nhwc(H, W))                           # sharper than K M: the kernel's own roundings
        assert d is None, ("hdn_warp_count_f32 against the fp32 restatement", (H, W), off, d)


@pytest.mark.parametrize("H,W", FC.FUSED_SHAPES, ids=lambda v: str(v))
def test_fused_solve_and_warp(dev, H, W):
    """hdn_dlt_warp_strided_f32, planes packed and 5 NaN floats apart: H_out has the bits of hdn_dlt_solve_f32 and lies inside the solve's bound;
    the warped plane has the bits of hdn_warp_count_f32 at theta = normalise_H(H_out) (restated with single roundings: W / 2 is no power of two, so
    this theta is not dyadic and float64 equality is not to be had) and lies inside K M of float64 on the fp32 cells."""
    h4p, off, img = FC.fused_problem(H, W)
    B = img.shape[0]
    truth = FC.dlt_truth(h4p, off)
    Hs, clean, same = FC.run_dlt(h4p, off, dev, FC.OFFSETS[1])
    assert clean and same and FC.dlt_excess(Hs, truth)[0] <= 0
    theta = FC.normalise_rs(Hs.numpy(), H, W)
    U = img.reshape(B, 1, H, W)
    exp = FC.warp_expect(U, theta)
    r_ref = FC.warp_r_ref(U, theta, exp)
    alone = FC.run_warp(U, theta, dev, FC.OFFSETS[1])[0].reshape(B, H, W)
    d = FC.difference(alone, FC.warp_expect32(U, theta).reshape(B, H, W), _nhwc(H, W))
    assert d is None, ("hdn_warp_count_f32 against the fp32 restatement", (H, W), d)
    for offs in FC.OFFSETS:
        for gap in (0, 5):
            Hf, warped, clean, same = FC.run_dlt_warp(h4p, off, img, dev, offs, gap)
            tag = ("hdn_dlt_warp_strided_f32", (H, W), "offsets", offs, "gap", gap)
            assert clean and same, tag
            assert torch.equal(Hf, Hs), (tag, FC.difference(Hf, Hs, lambda at: f"sample {at[0]}, " + FC.where_solve(at[0])))
            d = FC.difference(warped, alone, _nhwc(H, W))
            assert d is None, (tag, "against hdn_warp_count_f32", d)
            _inside(f"fused warp {H}x{W} (r_ref {r_ref:.3e}) offsets {offs} gap {gap}", warped.reshape(B, H, W, 1), exp["out"], exp["M"], FC.k_bound(r_ref), _nhwc(H, W))


# ------------------------------------------------------------------------------------------------------------------------------ 2. solve
@pytest.mark.parametrize("B", FC.DLT_FWD_BATCHES)
def test_dlt_solve_batches(dev, B):
    """Known maps, single displaced corners, production / skewed / tie quads under random offsets, at batch sizes either side of the lane group, the
    wave and the workgroup: both solvers inside 2^-23 |truth| + 2^-23 max|truth| of float64 dlt_rs, bit-equal to each other and to
    fp32(dlt_eliminate), the host's operation-for-operation restatement (ties to the lowest row, dlt_point's order: the host test shows fixtures whose
    fp32 values change under either mutation), H[8] == 1.0, the nine floats of sample B - 1 end at the sentinel."""
    names, src, off, truth = FC.dlt_fwd_problem(B)
    img = FC.pattern(5, 9).repeat(B, 1, 1)
    where = lambda at: f"sample {at[0]} ({names[at[0]]}), " + FC.where_solve(at[0])
    for offs in FC.OFFSETS:
        got, clean, same = FC.run_dlt(src, off, dev, offs)
        excess, ratio = FC.dlt_excess(got, truth)
        print(f"FORMS geometry forward DLT B={B} offsets {offs}: worst error {ratio:.3f} of the bound")
        worst = int(((got.double() - truth).abs() - 2.0 ** -23 * (truth.abs() + truth.abs().amax(1, keepdim=True))).amax(1).argmax())
        assert clean and same, ("hdn_dlt_solve_f32", B, offs)
        assert excess <= 0, ("hdn_dlt_solve_f32", B, offs, ratio, where((worst,)), got[worst], truth[worst])
        assert bool((got[:, 8] == 1.0).all())
        d = FC.difference(got, FC.dlt_fwd_restated(B), where)                                     # the elimination's path: point order, pivot ties
        assert d is None, ("hdn_dlt_solve_f32 against the restated elimination", B, offs, d)
        fused, _, clean, same = FC.run_dlt_warp(src, off, img, dev, offs)
        assert clean and same and torch.equal(fused, got), ("hdn_dlt_warp_strided_f32", B, offs, FC.difference(fused, got, where))
    known = {name: Hm for name, _, Hm in FC.DLT_KNOWN}
    for b, name in enumerate(names):
        if name in known:                                                                         # the map the fixture was built from
            assert FC.dlt_excess(got[b:b + 1], torch.tensor([known[name]], dtype=torch.float64))[0] <= 0, (name, got[b])


def test_dlt_degenerate_sample_stays_in_its_place(dev):
    """Sample 4 of 9 has four equal source corners (a singular system).  Its H may be anything; every other sample keeps the bits it has when run
    alone, in both solvers; nothing outside the results is written; the fused warp's other planes keep their bits too.
    Bounds: warp_pixel forms every index through f2i_x86 (NaN and out of range -> INT_MIN) and clampi to [0, W - 1] / [0, H - 1] before it reads
    pl[y * W + x], and writes only out[(i W + j) C + c] of its own pixel, so a non-finite H cannot move a load or a store out of the plane."""
    src, off = FC.dlt_degenerate_problem()
    B, k = src.shape[0], FC.DEGENERATE_AT
    img = FC.pattern(9, 17).repeat(B, 1, 1)
    got, clean, same = FC.run_dlt(src, off, dev, FC.OFFSETS[1])
    assert clean and same
    fused, warped, clean, same = FC.run_dlt_warp(src, off, img, dev, FC.OFFSETS[1], gap=3)
    assert clean and same
    print(f"FORMS geometry forward DLT degenerate sample: H = {got[k].tolist()}")
    for b in range(B):
        if b == k:
            continue
        one = FC.run_dlt(src[b:b + 1], off[b:b + 1], dev)[0]
        f1, w1, _, _ = FC.run_dlt_warp(src[b:b + 1], off[b:b + 1], img[b:b + 1], dev)
        assert torch.equal(one[0], got[b]) and torch.equal(f1[0], fused[b]) and torch.equal(fused[b], got[b]), (b, FC.where_solve(b))
        assert torch.equal(w1[0], warped[b]) and bool(warped[b].isfinite().all()), b
    assert FC.dlt_excess(torch.cat([got[:k], got[k + 1:]]), FC.dlt_truth(torch.cat([src[:k], src[k + 1:]]), torch.cat([off[:k], off[k + 1:]])))[0] <= 0


# ------------------------------------------------------------------------------------------------------------------------------ 3. sampler
def _bcss(S):
    return lambda at: f"sample {at[0]}, channel {at[1]}, angle row {at[2]}, radius column {at[3]}, " + FC.where_sampler(at[2] * S + at[3])


@pytest.mark.parametrize("i", range(FC.N_LOGPOLAR_EXACT))
def test_sampler_exact_fixtures(dev, i):
    """The five dyadic fixtures of the backward suite and the two dyadic-table ones (S = 16 and 17 on oblong crops, samples past every border): out
    and grid torch.equal to float64; with grid_or_null NULL the same out bits and the grid's place untouched."""
    x, polar, tabs, want, grid = FC.logpolar_exact_fwd(i)
    S = tabs[0].numel()
    for off in FC.OFFSETS:
        out, g, clean, same = FC.run_logpolar(x, polar, tabs, dev, off)
        tag = ("hdn_logpolar_sample_f32", tuple(x.shape), "S", S, "offsets", off)
        assert FC.difference(out, want, _bcss(S)) is None, (tag, FC.difference(out, want, _bcss(S)))
        assert FC.difference(g, grid, lambda at: f"sample {at[0]}, " + FC.where_sampler(at[1] * S + at[2])) is None, (tag, "grid")
        assert clean and same, tag
        out2, g2, clean, same = FC.run_logpolar(x, polar, tabs, dev, off, want_grid=False)
        assert g2 is None and torch.equal(out2, out) and clean and same, (tag, "grid_or_null NULL")


@pytest.mark.parametrize("i", range(len(FC.LOGPOLAR_EXACT), FC.N_LOGPOLAR_EXACT))
def test_sampler_masked_taps_are_not_read(dev, i):
    """A NaN column at x = W - 1 and a NaN row at y = H - 1 reach exactly the outputs whose unmasked taps include them; +inf in the south row of the
    outputs at the east border stays +-inf (a masked south-east tap read with its weight of 0 would make it NaN)."""
    S = FC.logpolar_exact_fwd(i)[2][0].numel()
    for name, (x, polar, tabs) in (("NaN column and row", FC.logpolar_poisoned(i, float("nan"), -1, -1)),
                                   ("inf row", FC.logpolar_poisoned(i, float("inf"), None, FC.logpolar_inf_row(i)))):
        want = FC.logpolar_expect(x, polar, tabs)[0]
        for off in FC.OFFSETS:
            out, _, clean, same = FC.run_logpolar(x, polar, tabs, dev, off)
            d = FC.difference(out, want, _bcss(S), nan_equal=True)
            assert d is None and clean and same, ("hdn_logpolar_sample_f32", name, tuple(x.shape), off, d)
    H, W = x.shape[2:]
    x, polar, tabs = FC.logpolar_poisoned(i, float("nan"), -1, -1)
    out = FC.run_logpolar(x, polar, tabs, dev)[0]
    assert torch.equal(out.isnan(), FC.logpolar_reach(polar, tabs, H, W, col=W - 1, row=H - 1).unsqueeze(1).expand_as(out))


@pytest.mark.parametrize("B,C,H,W,S", FC.LOGPOLAR_FWD_RANDOM, ids=lambda v: str(v))
def test_sampler_real_tables_random_data(dev, B, C, H, W, S):
    """The module's own tables on N(0,1) crops, origins that push samples past every border: grid bit-equal to the numpy fp32 restatement of its two
    statements, out inside K M on the fp32 cells, K = max(4 r_ref, 2e-6) with r_ref of F.grid_sample in fp32 on the CPU at the same shape, and
    bit-equal to logpolar_expect32, the numpy restatement of the kernel's own roundings (F.grid_sample itself rounds otherwise in a few per cent of
    the elements: printed)."""
    x, polar, tabs, want, M, r_ref = FC.logpolar_random_fwd(B, C, H, W, S)
    for off in FC.OFFSETS:
        out, g, clean, same = FC.run_logpolar(x, polar, tabs, dev, off)
        assert clean and same, off
        d = FC.difference(g, FC.logpolar_grid32(polar, tabs, H, W), lambda at: f"sample {at[0]}, " + FC.where_sampler(at[1] * S + at[2]))
        assert d is None, ("hdn_logpolar_sample_f32 grid", (B, C, H, W, S), off, d)
        _inside(f"sampler S={S} on {H}x{W} (r_ref {r_ref:.3e}) offsets {off}", out, want, M, FC.k_bound(r_ref), _bcss(S))
        d = FC.difference(out, FC.logpolar_expect32(x, polar, tabs), _bcss(S))                    # sharper than K M: the kernel's own roundings
        assert d is None, ("hdn_logpolar_sample_f32 against the fp32 restatement", (B, C, H, W, S), off, d)
        ncpu = int((out != FC.logpolar_rs(x, polar, tabs, torch.float32)).sum())
        print(f"FORMS geometry forward sampler S={S} on {H}x{W}: elements that differ from F.grid_sample in fp32 on this CPU: {ncpu} of {out.numel()}")


# ------------------------------------------------------------------------------------------------------------------------------ 4. refinement warp
def _bhw(H, W):
    return lambda at: f"sample {at[0]}, pixel ({at[1]}, {at[2]}), " + FC.where_refine(at[1] * W + at[2], H, W)


@pytest.mark.parametrize("H,W", FC.REFINE_SHAPES, ids=lambda v: str(v))
def test_refine_warp_exact_translations(dev, H, W):
    """Translations by whole, half and n/32 pixels on integer images (sample 0: the position pattern under a whole shift), B = 1 and 5: torch.equal
    to float64 bilinear-replicate sampling and, for whole shifts, to index arithmetic; H_comp (dyadic, so the product is exact in any order) updated to 1e-15 of numpy's float64 product for every
    sample and ending at its sentinel; the image bits the same with H_comp_or_null NULL."""
    for B in (1, 5):
        Hm, img, want = FC.refine_exact_problem(H, W, B)
        Hc0 = np.stack([np.array([[1.5, 0.25, 3.0], [0.125, 0.75, 2.0], [2.0 ** -10, 2.0 ** -9, 1.0]]) * (b + 1) for b in range(B)])
        for off in FC.OFFSETS:
            got, Hc, clean, same = FC.run_refine(Hm, img, Hc0, dev, off)
            tag = ("hdn_refine_warp_f32", (B, H, W), "offsets", off)
            d = FC.difference(got, want, _bhw(H, W))
            assert d is None, (tag, d)
            assert clean and same, tag
            for b in range(B):
                tx, ty = FC.REFINE_SHIFTS[b]
                if tx == int(tx) and ty == int(ty):
                    assert np.array_equal(got[b].numpy(), FC.shifted_index(img[b].numpy(), tx, ty)), (tag, b)
                np.testing.assert_allclose(Hc[b], Hc0[b] @ FC.refine_chain(Hm[b].numpy())[0].astype(np.float64), rtol=1e-15, atol=0, err_msg=str((tag, b)))
            null, none, clean, same = FC.run_refine(Hm, img, None, dev, off)
            assert none is None and torch.equal(null, got) and clean and same, (tag, "H_comp_or_null NULL")


@pytest.mark.parametrize("H,W", FC.REFINE_PROJECTIVE_SHAPES, ids=lambda v: str(v))
def test_refine_warp_projective(dev, H, W):
    """Projective H on N(0,1) images at 127 x 127, 129 x 128 (the grid-stride loop's second pass) and 8 x 200 (bw = 128): every pixel within
    cv_semantics.bar_float of the float64 ideal, and at most 16 pixels per call more than 1e-5 from oracle.hdn_oracle.refine_step."""
    Hm, img, Hc0 = FC.refine_projective_problem(H, W)
    B = Hm.shape[0]
    got, Hc, clean, same = FC.run_refine(Hm, img, Hc0, dev, FC.OFFSETS[1])
    assert clean and same
    n_diff = 0
    for b in range(B):
        Hhm, M = FC.refine_chain(Hm[b].numpy())
        ref, L = S.warp_perspective(img[b].numpy(), M.astype(np.float64), ring=1)
        bad = ~(np.abs(got[b].numpy().astype(np.float64) - ref) <= S.bar_float(ref, L))             # (a NaN left in the output is a violation)
        assert not bad.any(), ("hdn_refine_warp_f32 against the float64 ideal", (H, W), b, int(bad.sum()), _bhw(H, W)((b,) + tuple(np.argwhere(bad)[0])))
        wr, Hr = O.refine_step(Hm[b].reshape(3, 3).numpy(), img[b].numpy(), Hc0[b])
        n_diff += int((~(np.abs(got[b].numpy() - wr) <= 1e-5)).sum())
        np.testing.assert_allclose(Hc[b], Hc0[b] @ Hhm.astype(np.float64), rtol=1e-15, atol=0)
    print(f"FORMS geometry forward refine_warp projective {H}x{W}: pixels more than 1e-5 from the oracle: {n_diff} (cap 16)")
    assert n_diff <= 16, n_diff


def test_refine_warp_block_walk_decides_ties(dev):
    """8 x 200 (bw = 128) under a scale of 5 (3, sheared) and a shift of 3/64 px: every fifth (third) column lies on a cvRound tie in exact
    arithmetic, so the float64 roundings of X0 = M0 bx + M1 y + M2 decide it and a walk in other blocks moves some 100 pixels by 1/32 px (the
    host test counts them).  At most 16 pixels per call may differ from the oracle by more than 1e-5; every pixel stays within bar_float."""
    Hm, img = FC.refine_tie_problem()
    H, W = FC.REFINE_TIE_SHAPE
    for off in FC.OFFSETS:
        got, _, clean, same = FC.run_refine(Hm, img, None, dev, off)
        assert clean and same
        n_diff, where = 0, ""
        for b in range(Hm.shape[0]):
            _, M = FC.refine_chain(Hm[b].numpy())
            ref, L = S.warp_perspective(img[b].numpy(), M.astype(np.float64), ring=1)
            assert not (~(np.abs(got[b].numpy().astype(np.float64) - ref) <= S.bar_float(ref, L))).any(), b
            wr = O.refine_step(Hm[b].reshape(3, 3).numpy(), img[b].numpy(), np.eye(3))[0]
            far = ~(np.abs(got[b].numpy() - wr) <= 1e-5)
            n_diff += int(far.sum())
            if far.any() and not where:
                where = _bhw(H, W)((b,) + tuple(np.argwhere(far)[0]))
        print(f"FORMS geometry forward refine_warp tie fixture offsets {off}: pixels more than 1e-5 from the oracle: {n_diff} (cap 16)")
        assert n_diff <= 16, ("hdn_refine_warp_f32", (H, W), off, n_diff, where)


# ------------------------------------------------------------------------------------------------------------------------------ 5. score
@pytest.mark.parametrize("n", FC.L1_SIZES)
def test_l1_score_exact(dev, n):
    """Integers in [-8, 8], scale 2^-7: hdn_l1_score_f32 and both entries of hdn_l1_score2_f32 torch.equal to float64, a sentinel behind each."""
    a, b0, b1, truth = FC.l1_problem(n)
    for off in FC.OFFSETS:
        one, clean, same = FC.run_l1(a, b0, b1, dev, off, "one")
        assert FC.difference(one, truth[0, :1]) is None and clean and same, ("hdn_l1_score_f32", n, off, one, truth[0, :1])
        two, clean, same = FC.run_l1(a, b0, b1, dev, off, "pair")
        assert FC.difference(two, truth[0]) is None and clean and same, ("hdn_l1_score2_f32", n, off, two, truth[0])


@pytest.mark.parametrize("n", FC.L1_BATCH_SIZES)
def test_l1_score_batch_exact(dev, n):
    """hdn_l1_score2_batch_f32 at B = 1, 3, 5 with plane_stride n, n + 1 and n + 37, the gaps NaN: entry s equals float64 and the pair call on
    sample s alone; out[2 B] is the sentinel."""
    for B, pad in FC.L1_BATCH:
        a, b0, b1, truth = FC.l1_problem(n, B)
        for off in FC.OFFSETS:
            got, clean, same = FC.run_l1(a, b0, b1, dev, off, "batch", pad)
            tag = ("hdn_l1_score2_batch_f32", n, "B", B, "plane_stride", n + pad, "offsets", off)
            assert FC.difference(got, truth, lambda at: f"sample {at[0]}, score {at[1]}") is None, (tag, got, truth)
            assert clean and same, tag
        for s in range(B):
            two = FC.run_l1(a[s:s + 1], b0[s:s + 1], b1[s:s + 1], dev, FC.OFFSETS[1], "pair")[0]
            assert torch.equal(two, got[s]), (tag, s)
