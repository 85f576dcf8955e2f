"""The depthwise correlation kernels on the device (csrc/xcorr.hip: xcorr_prod29_kernel, xcorr_cfg5_kernel, xcorr_north_kernel, xcorr_circ13f_kernel,
xcorr_generic_kernel; csrc/xcorr_fft.hip: xcorr_north_fft4_kernel and its guarded v1 path) at every tail plane count, alignment of the three base
pointers and launch form, against the float64 direct sum of tests/xcorr_cases.py on fixtures on which fp32 is exact: the direct kernels must be
torch.equal to it, the two transform kernels inside the project's bound 1e-4 + 2e-6 M and round to it.  The host side, tests/test_xcorr_cases_host.py,
proves that the fixtures are exact, that the tables reach every path and that an independent fp32 transform needs less than a quarter of the bound."""
import json
import os
import subprocess
import sys

import pytest
import torch

import xcorr_cases as XC

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT_S = 240      # a child imports torch, opens the GPU and runs three small launches with their float64 references: seconds


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def where(kind, planes, plane, n=1, cap=None):
    """Which workgroup, wave or worker of the launch a plane belongs to."""
    if kind in ("prod29", "cfg5"):
        return f"workgroup {plane // XC.PPB} (np = {XC.groups4(planes)[plane // XC.PPB][1]}), wave {plane % XC.PPB}"
    if kind == "circ13":
        return f"group {plane // XC.CIRC_PPW} of the problem (np = {min(XC.CIRC_PPW, planes - plane // XC.CIRC_PPW * XC.CIRC_PPW)}), plane {plane % XC.CIRC_PPW} of it"
    if kind == "north_fft":
        plan = XC.fft4_plan(planes, cap or XC.CAP_FFT)
        pair = plane // 2
        if plan["v1_alone"] or (plan["tail"] and pair == planes // 2):
            return f"pair {pair}, half {plane % 2}: the guarded v1 path"
        return f"pair {pair}, half {plane % 2}: worker {pair % plan['nmain']}, pass {pair // plan['nmain']}"
    if kind == "north_direct":
        waves = XC.north_direct_plan(planes, n, cap or XC.CAP_DIRECT)["waves"]
        return f"wave {plane % waves}, pass {plane // waves}"
    return "one workgroup per plane"


def explain(kind, planes, offsets, d, n=1, cap=None):
    """The message of a mismatch: the kernel, the plane count, the offsets, the first (plane, row, column) and where() of it."""
    K = XC.KINDS[kind]
    if "plane" not in d:
        return f"{kind} at {planes} planes, offsets {offsets}: {d['how']}"
    extra = "".join(f", {key} {d[key]:.3e}" for key in ("bound", "worst_error_over_bound") if key in d)
    return (f"{K.variant} at {n} x {planes} planes, float offsets (x, k, out) = {offsets}: {d['count']} of {d['of']} outputs {d['how']}"
            + (f" in problem {d['problem']}" if "problem" in d else "") + f"; first (plane, row, column) = ({d['plane']}, {d['row']}, {d['column']}): got "
            f"{d['got']!r}, want {d['want']!r}{extra}; " + where(kind, planes, d["plane"], n, cap))


def single_cases(kind):
    if kind.startswith("gen"):
        return [(XC.GENERIC_PLANES, off) for off in ((0, 0, 0), (1, 2, 3))]
    counts, offsets = XC.SINGLE[kind]
    return [(P, off) for P in counts for off in offsets]


@pytest.mark.parametrize("kind", XC.SPECIALISED + XC.GENERIC)
def test_exact_fixture_every_plane_count(dev, kind):
    """Every entry of the single-call tables (XC.SINGLE: plane counts x offsets of the base pointers; the generic cases at 3 planes): the dispatched
    kernel is the intended one and every plane matches the float64 direct sum, from an output buffer that held NaN."""
    failures, ratios = [], []
    for planes, offsets in single_cases(kind):
        d, worst = XC.check_exact_case(kind, planes, dev, offsets)
        if d is not None:
            failures.append(explain(kind, planes, offsets, d))
        ratios.append(worst)
    if not XC.KINDS[kind].exact:
        print(f"XCORR {kind} exact fixture: error at most {max(ratios):.4f} of the bound over {len(ratios)} cases")
    assert not failures, f"{len(failures)} of {len(single_cases(kind))} cases: " + " | ".join(failures[:6])


@pytest.mark.parametrize("kind", XC.SPECIALISED + XC.GENERIC_SMALL + ("gen_123x124_109x1",))
def test_every_input_pixel_meets_every_tap(dev, kind):
    """x-impulse (plane p: a single 1 at input position p over taps that all differ) and k-impulse (plane p: a single 1 at tap position p over pixels that
    all differ), one launch each, against the closed forms of XC.x_impulse / XC.k_impulse; the 123 x 124 plane of generic_l2 gets sampled input
    positions and every tap position."""
    K = XC.KINDS[kind]
    for name, x, k, want in XC.position_fixtures(kind):
        got, variant = XC.run(kind, x, k, dev)
        assert variant == K.variant, (name, variant)
        M = want.amax(dim=(1, 2))
        if not K.exact:
            print(f"XCORR {kind} {name}: error at most {XC.worst_ratio(K, got, want, M):.4f} of the bound over {x.shape[0]} planes")
        d = XC.first_difference(K, got, want, M, False)
        if d is not None:
            p = d["plane"]
            imp = (x if name == "x-impulse" else k)[p]
            r, c = (imp == 1).nonzero()[0].tolist()
            pytest.fail(f"{name}, the 1 at (row, column) = ({r}, {c}): " + explain(kind, x.shape[0], (0, 0, 0), d))


@pytest.mark.parametrize("kind", XC.SPECIALISED)
def test_multi_problem_launches_into_one_stacked_buffer(dev, kind):
    """XC.MULTI through xcorr_depthwise_multi(..., outs = the slices of one stacked buffer that held NaN): each problem is torch.equal to its single call
    on plain tensors and matches the float64 direct sum; a circular workgroup then holds waves of two problems, the slices start at every residue of a
    16-byte line."""
    import hdn_amd
    from hdn_amd import xcorr as X
    K = XC.KINDS[kind]
    single = hdn_amd.xcorr_depthwise_circular if K.circular else hdn_amd.xcorr_depthwise
    for n, planes in XC.MULTI[kind]:
        for off in ((0, 0, 0), (0, 0, 1)):
            probs = [XC.exact_problem(kind, planes, tag) for tag in range(n)]
            got, (xd, kd, outs) = XC.run_multi(kind, [p[0] for p in probs], [p[1] for p in probs], dev, off)
            assert XC.last["variant"] == K.variant
            assert all(outs[i].data_ptr() - outs[0].data_ptr() == 4 * i * outs[0].numel() for i in range(n))
            for i, (y, (x, k, truth, M)) in enumerate(zip(got, probs)):
                d = XC.first_difference(K, y, truth, M, True)
                assert d is None, f"problem {i}: " + explain(kind, planes, off, d, n)
                if K.north:
                    with X.north_variant(K.north):
                        alone = single(xd[i], kd[i])
                else:
                    alone = single(xd[i], kd[i])
                assert X.last_variant() == K.variant
                assert torch.equal(alone.cpu().view_as(y), y), f"problem {i} of {n} x {planes} planes of {kind} differs from its single call"


SENTINEL = -12345.678


def guard_cases():
    return [(kind, P, off) for kind, counts in XC.GUARD.items() for P in counts for off in XC.GUARD_OFFSETS]


@pytest.mark.parametrize("kind,planes,offsets", guard_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_no_stray_writes_and_inputs_untouched(dev, kind, planes, offsets):
    """Two problems in one launch, x, k and out each in the middle of a larger buffer with more than a plane of margin on both sides: NaN around the
    inputs, a sentinel around the results.  Afterwards the sentinels and the input buffers are bit-unchanged, and the results are finite and torch.equal
    to the same launch on plain tensors.  (The margins are allocated memory: a stray access shows, it does not fault.)"""
    K = XC.KINDS[kind]
    HO, WO = XC.out_size(K)
    probs = [XC.exact_problem(kind, planes, tag) for tag in range(2)]
    bits = lambda t: t.cpu().view(torch.int32)
    mx, mk, mo = (-(-n // 4) * 4 + 4 for n in (K.Hx * K.Wx, K.Hk * K.Wk, HO * WO))      # more than a plane, a multiple of 16 bytes
    xs = [XC.at_offset(p[0], offsets[0], dev, mx, float("nan")) for p in probs]
    ks = [XC.at_offset(p[1], offsets[1], dev, mk, float("nan")) for p in probs]
    outs = [XC.at_offset(planes * HO * WO, offsets[2], dev, mo, SENTINEL) for _ in probs]
    assert all(v.data_ptr() % 16 == 4 * o for vs, o in zip((xs, ks, outs), offsets) for v, _ in vs)
    before = [bits(b) for _, b in xs + ks]
    XC.launch(K, [v.view(1, planes, K.Hx, K.Wx) for v, _ in xs], [v.view(1, planes, K.Hk, K.Wk) for v, _ in ks],
              [v.view(1, planes, HO, WO) for v, _ in outs])
    torch.cuda.synchronize()
    assert XC.last["variant"] == K.variant
    for name, (_, b), was in zip(["x0", "x1", "k0", "k1"], xs + ks, before):
        assert torch.equal(bits(b), was), f"the buffer of {name} changed"
    sentinel = bits(torch.full((1,), SENTINEL))
    for i, (v, b) in enumerate(outs):
        whole = b.cpu()
        lo = mo + offsets[2]
        for name, part in (("before", whole[:lo]), ("behind", whole[lo + v.numel():])):
            wrong = (bits(part) != sentinel).nonzero().flatten()
            assert part.numel() > HO * WO and wrong.numel() == 0, \
                f"{wrong.numel()} sentinels {name} the results of problem {i} were overwritten, first at {int(wrong[0])} of {part.numel()}"
    plain, _ = XC.run_multi(kind, [p[0] for p in probs], [p[1] for p in probs], dev, stacked=False)    # (after the sentinels: nothing strayed)
    for i, (v, _) in enumerate(outs):
        y = v.cpu().view(planes, HO, WO)
        assert bool(torch.isfinite(y).all()), f"problem {i}: {int((~torch.isfinite(y)).sum())} results are not finite: " + str((~torch.isfinite(y)).nonzero()[:4].tolist())
        assert torch.equal(y, plain[i]), f"problem {i}: differs from the launch on plain tensors at " + str((y != plain[i]).nonzero()[:4].tolist())
        d = XC.first_difference(K, y, probs[i][2], probs[i][3], True)
        assert d is None, explain(kind, planes, offsets, d, 2)


@pytest.mark.parametrize("kind", list(XC.GUARD))
def test_a_nan_plane_stays_in_its_plane(dev, kind):
    """One plane of x, then one plane of k, all NaN, at the first, a middle and the last plane of a tail count: every other plane is torch.equal to the
    clean run - except, for the FFT kernel, the partner of the pair, which shares the transform (docs/KERNELS.md); the 9-plane groups of the circular
    kernel share nothing.  The NaN plane itself is NaN wherever the reference is (the direct 61 x 61 kernel skips zero taps: not checked)."""
    K = XC.KINDS[kind]
    planes = max(XC.GUARD[kind])
    x, k, truth, M = XC.exact_problem(kind, planes)
    clean, _ = XC.run(kind, x, k, dev)
    assert XC.first_difference(K, clean, truth, M, True) is None
    for victim in sorted({0, planes // 2, planes - 1}):
        for which in ("x", "k"):
            xn, kn = x.clone(), k.clone()
            (xn if which == "x" else kn)[victim] = float("nan")
            got, variant = XC.run(kind, xn, kn, dev)
            assert variant == K.variant
            exempt = {victim} | ({victim ^ 1} if kind == "north_fft" else set())
            keep = [p for p in range(planes) if p not in exempt]
            moved = [p for p in keep if not torch.equal(got[p], clean[p])]
            assert not moved, f"{K.variant}, {planes} planes, {which}[{victim}] = NaN: planes {moved} moved; " + where(kind, planes, moved[0])
            if kind != "north_direct":
                assert bool(torch.isnan(got[victim]).all()), f"{K.variant}: plane {victim} with a NaN {which} holds {int((~torch.isnan(got[victim])).sum())} numbers"


_child_fault = []          # a child that died of a signal or ran into its time limit: nothing more is started on the device by this test


@pytest.mark.parametrize("kind", ["north_fft", "north_direct"])
def test_capped_persistent_grids_in_a_child_process(dev, kind):
    """HDN_NORTH_BLOCKS = 3 (read once per process: one fresh child per 61 x 61 kernel, one after the other): 37 and 38 planes through the single call and
    3 problems of 9 planes in one launch, so that every worker makes several passes, the FFT kernel hands its prefetch over, takes the staggered start
    and the odd tail, and the direct kernel's grid is one workgroup per problem.  The child checks every plane as test_exact_fixture_every_plane_count."""
    if _child_fault:
        pytest.fail(f"not started: {_child_fault[0]}")
    cmd = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "xcorr_cases.py"), kind, *XC.CHILD_CASES]
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S, env=dict(os.environ, **{XC.CAP_ENV: str(XC.CHILD_BLOCKS)}))
    except subprocess.TimeoutExpired as e:
        _child_fault.append(f"the child of {kind} did not end within {CHILD_TIMEOUT_S} s")
        pytest.fail(_child_fault[0] + ": " + str(e.stderr)[-1500:])
    tail = res.stdout[-1500:] + res.stderr[-1500:]
    if res.returncode < 0:
        _child_fault.append(f"the child of {kind} ended with signal {-res.returncode}")
        pytest.fail(_child_fault[0] + ": " + tail)
    assert res.returncode == 0, tail
    answer = json.loads(res.stdout.strip().splitlines()[-1])
    assert answer["kind"] == kind and answer["blocks"] == str(XC.CHILD_BLOCKS) and [c["case"] for c in answer["cases"]] == list(XC.CHILD_CASES), answer
    for c in answer["cases"]:
        n, planes = XC.parse_child_case(c["case"])
        assert c["variant"] == XC.KINDS[kind].variant, c
        assert c["first"] is None, f"under {XC.CAP_ENV}={XC.CHILD_BLOCKS}: " + explain(kind, planes, (0, 0, 0), c["first"], n, XC.CHILD_BLOCKS)
