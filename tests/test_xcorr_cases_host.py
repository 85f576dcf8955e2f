"""Host side of tests/test_gpu_xcorr_forms.py: the fixtures of tests/xcorr_cases.py are what they claim (exact in fp32, closed forms equal to the float64
direct sum, separated by four bounds), the bound has a yardstick that is not the code under test (fp32 torch.fft), the restated grouping rules still
match csrc/xcorr.hip and csrc/xcorr_fft.hip, and the case tables reach every path.  No GPU, no kernel."""
import os
import re

import pytest
import torch

import xcorr_cases as XC

CSRC = os.path.join(XC.ROOT, "hdn_amd", "csrc")


def table_problems():
    """Every (kind, planes, tag) of the exact fixture that a table of tests/xcorr_cases.py asks for."""
    seen = set()
    for kind, (counts, _) in XC.SINGLE.items():
        seen |= {(kind, P, 0) for P in counts}
    for kind, rows in XC.MULTI.items():
        seen |= {(kind, P, tag) for n, P in rows for tag in range(n)}
    for kind in ("north_direct", "north_fft"):
        for case in XC.CHILD_CASES:
            n, P = XC.parse_child_case(case)
            seen |= {(kind, P, tag) for tag in range(n)}
    for kind, counts in XC.GUARD.items():
        seen |= {(kind, P, tag) for P in counts for tag in range(2)}
    seen |= {(kind, XC.GENERIC_PLANES, 0) for kind in XC.GENERIC}
    return sorted(seen)


def test_exact_fixture_is_exact_in_fp32():
    """Small signed integers with exact zeros (31 x 31: zero rows, a zero plane, a -0.0 tap); for every table entry the largest sum|x k| is far below
    2^24 and 2e-6 of it below 0.25; the fp32 and the float64 direct sum agree bit for bit."""
    worst = {}
    for kind, P, tag in table_problems():
        K = XC.KINDS[kind]
        x, k, truth, M = XC.exact_problem(kind, P, tag)
        assert x.shape == (P, K.Hx, K.Wx) and k.shape == (P, K.Hk, K.Wk) and x.dtype == k.dtype == torch.float32
        assert truth.shape == (P,) + XC.out_size(K) and truth.dtype == torch.float64
        for t in (x, k):
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 3
        assert float(x.abs().max()) == 3
        assert K.Hk * K.Wk * 9 < 2 ** 24 / 1024 and XC.REL_TOL * K.Hk * K.Wk * 9 < 0.25        # the largest POSSIBLE sum|x k| of the value range
        head, rel = XC.exactness_headroom(x, k, K.circular)
        assert head < 2.0 ** -10 and rel < 0.25 and rel == XC.REL_TOL * float(M.max())
        worst[kind] = max(worst.get(kind, (0, 0)), (head, rel))
        if k.numel() >= 25:
            assert bool((k == 0).any()) and bool((k != 0).any())
        if (K.Hk, K.Wk) == (31, 31):
            assert bool(torch.signbit(k[0, 2, 3])) and float(k[0, 2, 3]) == 0
            for p in range(P):
                live = [u for u in range(31) if bool(k[p, u].any())]
                assert all(u % 5 != p % 5 for u in live)                                        # whole zero rows ...
                assert live or (P >= 3 and p == P - 2)                                          # ... and one all-zero plane
                if live:
                    assert bool((k[p, live] == 0).any()) and bool((k[p, live] != 0).any())      # the zero-tap branch taken and not taken in a row
            assert (P < 3) or not bool(k[P - 2].any())
        r32 = XC.direct_sum(x, k, K.circular, dtype=torch.float32)
        assert r32.dtype == torch.float32 and torch.equal(r32.double(), truth) and torch.equal(truth, truth.round())
    for kind, (head, rel) in worst.items():
        print(f"XCORR exact fixture {kind}: largest sum|x k| = {head:.3e} of 2^24, 2e-6 of it = {rel:.4f} (< 0.25)")


POSITION_KINDS = XC.SPECIALISED + XC.GENERIC_SMALL + ("gen_123x124_109x1",)


@pytest.mark.parametrize("kind", [k for k in POSITION_KINDS if k != "north_fft"])
def test_position_closed_forms_equal_the_float64_direct_sum(kind):
    """x-impulse and k-impulse: the index arithmetic equals the float64 direct sum at every position (north_direct and north_fft share the shape)."""
    K = XC.KINDS[kind]
    for name, x, k, want in XC.position_fixtures(kind):
        assert x.dtype == k.dtype == want.dtype == torch.float32 and bool((x >= 0).all()) and bool((k >= 0).all())
        imp, P = (x, K.Hx * K.Wx) if name == "x-impulse" else (k, K.Hk * K.Wk)
        assert torch.equal(imp.sum(dim=(1, 2)), torch.ones(imp.shape[0])) and float(imp.max()) == 1
        if K.Hx * K.Wx <= 4096 or name == "k-impulse":
            assert imp.shape[0] == P and torch.equal(imp.reshape(P, P), torch.eye(P))           # plane p: position p, every position once
        truth = XC.direct_sum(x, k, K.circular)
        assert torch.equal(want.double(), truth), (kind, name, (want.double() != truth).nonzero()[:4].tolist())
        assert float(want.amax(dim=(1, 2)).min()) > 0                                           # every plane reaches a result


@pytest.mark.parametrize("kind", ["north_fft", "circ13"])
def test_position_fixtures_are_separated_by_four_bounds(kind):
    """The smallest difference between a pattern value and a neighbour (or 0) is at least four times the largest bound of the fixture: a result that is
    one position off cannot hide inside the bound.  (x, k >= 0: M is the largest result of the plane.)"""
    K = XC.KINDS[kind]
    for name, x, k, want in XC.position_fixtures(kind):
        pat = k if name == "x-impulse" else x
        for p in range(pat.shape[0]):
            assert pat[p].unique().numel() == pat[p].numel()
        sep, b = XC.separation(pat), float(XC.bound(K, want.amax(dim=(1, 2)).double()).max())
        print(f"XCORR {kind} {name}: separation {sep:.6f} = {sep / b:.1f} x the largest bound {b:.3e}, largest value {float(pat.max()):.4f}")
        assert float(pat.max()) <= 32 and sep >= 4 * b


@pytest.mark.parametrize("kind", ["north_fft", "circ13"])
def test_fp32_fft_yardstick_stays_within_a_quarter_of_the_bound(kind):
    """An independent fp32 transform of the same correlation (torch.fft on the CPU) stays within a quarter of 1e-4 + 2e-6 M on every fixture the GPU
    tests give the transform kernels: the bound is wide enough for an fp32 transform, by a factor that is printed (docs/KERNELS.md records it)."""
    K = XC.KINDS[kind]
    fft32 = XC.fft32_plain if kind == "north_fft" else XC.fft32_circ13
    worst = 0.0
    for knd, P, tag in table_problems():
        if knd != kind:
            continue
        x, k, truth, M = XC.exact_problem(kind, P, tag)
        y = fft32(x, k)
        ratio = XC.worst_ratio(K, y, truth, M)
        worst = max(worst, ratio)
        assert ratio <= 0.25 and torch.equal(y.round().double(), truth), (P, tag, ratio)
    print(f"XCORR yardstick {kind} exact fixture: fp32 torch.fft error at most {worst:.4f} of the bound")
    for name, x, k, want in XC.position_fixtures(kind):
        ratio = XC.worst_ratio(K, fft32(x, k), want, want.amax(dim=(1, 2)))
        print(f"XCORR yardstick {kind} {name}: fp32 torch.fft error at most {ratio:.4f} of the bound")
        assert ratio <= 0.25, (name, ratio)


def test_pair_bound_and_references_on_a_tiny_case():
    """pair_max pairs (0, 1), (2, 3) and leaves an odd last plane alone; pad_circular wraps rows and clamps columns."""
    assert XC.pair_max(torch.tensor([1.0, 5.0, 7.0, 2.0, 3.0])).tolist() == [5, 5, 7, 7, 3]
    assert XC.pair_max(torch.tensor([4.0])).tolist() == [4]
    x = torch.arange(12.0).view(1, 4, 3)
    xp = XC.pad_circular(x)
    assert xp.shape == (1, 8, 5) and xp[0, :, 2].tolist() == [7, 10, 1, 4, 7, 10, 1, 4] and xp[0, 2].tolist() == [0, 0, 1, 2, 2]
    k = torch.zeros(1, 2, 2)
    k[0, 1, 0] = 2
    assert torch.equal(XC.direct_sum(x, k, False), 2 * x[:, 1:, :2].double())


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _ints(pattern, text, count=1):
    found = re.findall(pattern, text)
    assert len(found) == count, (pattern, found)
    return [int(v) for v in (found if isinstance(found[0], str) else found[0])]


def test_restated_constants_match_the_sources():
    """The grouping constants of tests/xcorr_cases.py, read out of csrc/xcorr.hip, csrc/xcorr_fft.hip and csrc/hdn_common.h as text."""
    xc, fft, common = _read("xcorr.hip"), _read("xcorr_fft.hip"), _read("hdn_common.h")
    block, = _ints(r"#define HDN_BLOCK (\d+)", common)
    wave, = _ints(r"#define HDN_WAVE (\d+)", common)
    assert (block, wave) == (256, 64)
    prod29 = xc[xc.index("namespace prod29 {"):xc.index("}  // namespace prod29")]
    cfg5 = xc[xc.index("namespace cfg5 {"):xc.index("}  // namespace cfg5")]
    assert _ints(r"constexpr int PPB = (\d+);", prod29) == [XC.PPB] and _ints(r"constexpr int PPB = (\d+), TH = \d+;", cfg5) == [XC.PPB]
    assert block // wave == XC.PPB                                                              # one wave per plane
    for ns, text in (("prod29", prod29), ("cfg5", cfg5)):
        hx, wx, hk, wk, ho, wo = _ints(r"constexpr int HX = (\d+), WX = (\d+), HK = (\d+), WK = (\d+), HO = (\d+), WO = (\d+);", text)
        K = XC.KINDS[ns]
        assert (hx, wx, hk, wk) == (K.Hx, K.Wx, K.Hk, K.Wk) and (ho, wo) == XC.out_size(K)
        assert (XC.PPB * hx * wx) % 4 == 0 and (XC.PPB * ho * wo) % 4 == 0                      # wide_copy: a group is a multiple of 16 bytes
    assert len(re.findall(r"if \(np == PPB && aligned16\(xg\)\)", xc)) == 2 and len(re.findall(r"if \(np == PPB && aligned16\(og\)\)", xc)) == 2
    # the direct 61 x 61 kernel: 4 waves of one plane each, grid capped at 512 / n
    assert _ints(r"const int gw = blockIdx\.x \* (\d+) \+ wave;", xc) == [XC.NORTH_WAVES] and _ints(r"const int nw = gridDim\.x \* (\d+);", xc) == [XC.NORTH_WAVES]
    assert _ints(r"const int per_problem = max\(1, min\(cdiv\(planes, (\d+)\), cap / n\)\);", xc) == [XC.NORTH_WAVES]
    direct, fftc = xc[xc.index("static int launch_north("):xc.index("g_last_variant = \"north_61x61_31x31\";")], xc[xc.index("if (v == HDN_NORTH_FFT_COL) {"):]
    assert _ints(r'static const int cap = env_positive\("%s", (\d+)\);' % XC.CAP_ENV, direct) == [XC.CAP_DIRECT]
    assert _ints(r'static const int cap = env_positive\("%s", (\d+)\);' % XC.CAP_ENV, fftc) == [XC.CAP_FFT]
    assert len(re.findall(r'"%s"' % XC.CAP_ENV, xc)) == 2 and "getenv(name);" in common       # (read nowhere else; env_positive reads it)
    assert "const int v = e ? atoi(e) : 0;\n  return v > 0 ? v : fallback;" in common[common.index("inline int env_positive(const char* name, int fallback) {"):]
    # the FFT kernel: pairs, nmain workers + one tail worker, 4 workers per workgroup, the stagger condition, the prefetch index
    assert len(re.findall(r"xcorr_north_fft4_kernel<%d>" % XC.FFT_WPG, fft)) == 3 and len(re.findall(r"xcorr_north_fft4_kernel<\d+>", fft)) == 3
    assert len(re.findall(r"dim3\(\(workers \+ 3\) / 4\), dim3\(256\)", fft)) == 2
    assert _ints(r"wave > 0 && npairs >= (\d+) \* nmain", fft) == [XC.FFT_STAGGER_PASSES]
    assert "const int pn = min(p + nmain, npairs - 1);" in fft and "for (; p < npairs; p += nmain)" in fft
    assert "const int npairs = (planes + 1) / 2, nfast = planes / 2;" in fft and "const int nmain = nfast < max_blocks ? nfast : max_blocks;" in fft
    assert "const int tail_worker = nfast < npairs ? nmain : -1;" in fft and "if (nfast == 0) return launch_north_fft(" in fft
    # the circular kernel: 9 planes per wave, 4 waves per workgroup, one flat grid over the problems
    assert _ints(r"constexpr int N = 13, PL = N \* N, NF = 7, PPW = (\d+), WAVES = HDN_BLOCK / 64;", xc) == [XC.CIRC_PPW] and block // 64 == XC.CIRC_WAVES
    assert "const int prob = g / groups_per_problem, p0 = (g - prob * groups_per_problem) * PPW, np = min(PPW, planes - p0);" in xc
    assert "const int g = blockIdx.x * WAVES + wave;" in xc and "const int gpp = cdiv(planes, circ13f::PPW);" in xc
    # the generic kernel's switch and the problems of one launch
    a, b = _ints(r"if \(lds <= (\d+) \* (\d+)\) \{", xc)
    assert a * b == XC.GENERIC_LDS_BYTES and "const size_t lds = (size_t(HP) * WP + size_t(Hk) * Wk) * sizeof(float);" in xc
    assert _ints(r"constexpr int XC_MAX_PROBLEMS = (\d+);", xc) == [XC.MAX_PROBLEMS]
    for K in XC.KINDS.values():
        if K.name.startswith("gen"):
            assert XC.generic_variant(K) == K.variant, K.name


def test_tables_reach_every_path():
    """The restated rules evaluated over the tables: every np of every kernel, both sides of each alignment branch for x and for out, the FFT kernel's
    tail worker with and without interior pairs, a circular workgroup spanning two problems, several passes and the stagger under the cap."""
    # ---- the two 4-plane kernels
    for kind in ("prod29", "cfg5"):
        counts, offsets = XC.SINGLE[kind]
        assert {np_ for P in counts for _, np_ in XC.groups4(P)} == {1, 2, 3, 4}
        assert max(len(XC.groups4(P)) for P in counts) == 3                                     # a first, a middle and a last workgroup
        x_side = {(XC.wide_copy(np_, ox), np_ == XC.PPB) for P in counts for _, np_ in XC.groups4(P) for ox, _, _ in offsets}
        o_side = {(XC.wide_copy(np_, oo), np_ == XC.PPB) for P in counts for _, np_ in XC.groups4(P) for _, _, oo in offsets}
        for side in (x_side, o_side):
            assert side == {(True, True), (False, True), (False, False)}                        # wide; full group on a misaligned pointer; tail group
        both = {(ox % 4 == 0, oo % 4 == 0) for ox, _, oo in offsets}
        assert both == {(True, True), (False, True), (True, False), (False, False)}             # x and out decide independently
        assert any(ok % 4 for _, ok, _ in offsets)
        # the multi table: the slices of one stacked buffer start at every residue, with tail groups
        HO, WO = XC.out_size(XC.KINDS[kind])
        starts = {(i * P * HO * WO) % 4 for n, P in XC.MULTI[kind] for i in range(n)}
        assert starts == {0, 1, 2, 3} and {n for n, _ in XC.MULTI[kind]} == set(XC.MULTI_N) and {P for _, P in XC.MULTI[kind]} == {5, 6}
    # ---- the direct 61 x 61 kernel
    counts, _ = XC.SINGLE["north_direct"]
    plans = [XC.north_direct_plan(P) for P in counts]
    assert {p["live_waves"] % XC.NORTH_WAVES for p in plans} == {0, 1, 2, 3} and {p["workgroups"] for p in plans} >= {1, 2, 3, 9}
    assert all(p["passes"] == 1 for p in plans)                                                 # several passes need the cap: the child
    # ---- the FFT kernel
    counts, offsets = XC.SINGLE["north_fft"]
    plans = {P: XC.fft4_plan(P) for P in counts}
    assert plans[1]["v1_alone"] and not any(p["v1_alone"] for P, p in plans.items() if P > 1)
    assert plans[3]["tail"] and plans[3]["nmain"] == 1 and plans[9]["tail"] and plans[9]["nmain"] == 4 and not plans[2]["tail"] and not plans[8]["tail"]
    assert {p["surplus"] for p in plans.values() if not p["v1_alone"]} == {0, 1, 2, 3} and max(p["workgroups"] for p in plans.values()) >= 2
    assert {p["workers"] % XC.FFT_WPG for p in plans.values()} == {0, 1, 2, 3}
    assert {(ox % 4 == 0, oo % 4 == 0) for ox, _, oo in offsets} == {(True, True), (False, True), (True, False), (False, False)}
    # ---- the circular kernel
    counts, offsets = XC.SINGLE["circ13"]
    assert {np_ for P in counts for wg in XC.circ_groups(P) for _, _, np_ in wg} == set(range(1, XC.CIRC_PPW + 1))
    assert {sum(len(wg) for wg in XC.circ_groups(P)) for P in counts} == {1, 2, 3, 5}
    assert max(len(XC.circ_groups(P)) for P in counts) == 2                                     # a second workgroup
    assert {o[0] % 4 for o in offsets} == {o[2] % 4 for o in offsets} == {o[1] % 4 for o in offsets} == {0, 1, 2, 3}
    spanning = [(n, P) for n, P in XC.MULTI["circ13"] if any(len({prob for prob, _, _ in wg}) > 1 for wg in XC.circ_groups(P, n))]
    assert (3, 10) in spanning and (8, 1) in spanning
    assert [len({prob for prob, _, _ in wg}) for wg in XC.circ_groups(1, 8)] == [4, 4] and [[g[0] for g in wg] for wg in XC.circ_groups(10, 3)] == [[0, 0, 1, 1], [2, 2]]
    # ---- the multi table of the 61 x 61 kernels
    for kind in ("north_direct", "north_fft"):
        assert {n for n, _ in XC.MULTI[kind]} == set(XC.MULTI_N) and {P for _, P in XC.MULTI[kind]} == {3, 4}
    assert max(XC.MULTI_N) == XC.MAX_PROBLEMS
    # ---- the capped grids of the child
    cap = XC.CHILD_BLOCKS
    cases = [XC.parse_child_case(c) for c in XC.CHILD_CASES]
    assert cases == [(1, 37), (1, 38), (3, 9)]
    f = {c: XC.fft4_plan(P, cap) for c, (n, P) in zip(XC.CHILD_CASES, cases)}
    assert all(p["nmain"] == cap and p["passes"] >= 2 and p["prefetch_next"] and p["prefetch_clamped"] for p in f.values())
    assert f["37"]["stagger"] and f["37"]["tail"] and f["38"]["stagger"] and not f["38"]["tail"] and f["3x9"]["tail"] and not f["3x9"]["stagger"]
    assert f["37"]["passes"] == 6 and f["38"]["passes"] == 7 and not any(XC.fft4_plan(P)["stagger"] for P in XC.SINGLE["north_fft"][0])
    d = {c: XC.north_direct_plan(P, n, cap) for c, (n, P) in zip(XC.CHILD_CASES, cases)}
    assert d["37"]["workgroups"] == 3 and d["37"]["passes"] == 4 and d["38"]["passes"] == 4
    assert d["3x9"]["workgroups"] == cap // 3 == 1 and d["3x9"]["passes"] == 3
    # ---- the generic kernel
    gen = [XC.KINDS[n] for n in XC.GENERIC]
    for circ in (False, True):
        mine = [K for K in gen if K.circular == circ]
        assert {K.variant for K in mine} == {"generic_lds", "generic_l2"}
        assert any(K.Wk == 1 for K in mine) and any(XC.out_size(K) == (1, 1) for K in mine)
        assert {(K.Hx % 2, K.Wx % 2) for K in mine} >= {(0, 1), (1, 0)} and any(K.Hx % 2 and K.Wx % 2 for K in mine)
        floats = lambda K: (XC.out_size(K)[0] + K.Hk - 1) * (XC.out_size(K)[1] + K.Wk - 1) + K.Hk * K.Wk
        assert XC.GENERIC_LDS_BYTES // 4 in {floats(K) for K in mine} and XC.GENERIC_LDS_BYTES // 4 + 1 in {floats(K) for K in mine}
    # ---- the guard tables: every kernel at a tail count and at an unaligned offset
    assert set(XC.SPECIALISED) <= set(XC.GUARD) and {XC.KINDS[n].variant for n in XC.GUARD} >= {"generic_lds", "generic_l2"}
    assert any(XC.KINDS[n].circular and n.startswith("gen") for n in XC.GUARD)
    for kind in ("prod29", "cfg5"):
        assert all(P % XC.PPB for P in XC.GUARD[kind])
    assert all(P % XC.CIRC_PPW for P in XC.GUARD["circ13"]) and any(P % 2 for P in XC.GUARD["north_fft"]) and any(P % 4 for P in XC.GUARD["north_direct"])
    assert any(all(o % 4 for o in off) for off in XC.GUARD_OFFSETS) and (0, 0, 0) in XC.GUARD_OFFSETS
