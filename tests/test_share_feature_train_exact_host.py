"""CPU side of tests/test_gpu_share_feature_train_exact.py: the exact fixtures of tests/share_feature_train_exact_cases.py are exact in fp32 in any
order (so torch.equal is the right demand on the device), the committed seed offsets are the first accepted ones, the one-hot sets meet every tap,
the stage checker accepts a host model of the kernels and rejects one wrong element, and each of five wrong kernels, restated in numpy, is rejected
by a named fixture.  No device is touched."""
import math

import numpy as np
import pytest
import torch

import share_feature_train_cases as C
import share_feature_train_exact_cases as E

SMALL = [s for s in E.DYADIC_CASES if s[0] * s[1] * s[2] <= 4096]
MUTANT_SHAPES = [(1, 15, 17), (1, 3, 683), (3, 33, 65)]


def stock32(fix):
    ref = C.stock(fix, torch.float32, train=False, running=C.running_of(fix), eps=E.EPS_DYADIC)
    ref["saved"] = E.saved_of(ref["c"])
    return ref


# ------------------------------------------------------------------------------------------------------------------------ A1
@pytest.mark.parametrize("shape", list(E.DYADIC_CASES))
def test_dyadic_fixture_is_exact_in_fp32_and_its_offset_the_first_accepted(shape):
    off = E.DYADIC_CASES[shape]
    assert E.first_dyadic_offset(shape) == off
    fix, truth = E.dyadic_problem(shape, off)
    assert E.shares_ok(truth["z"]) and E.order_free_margin(fix) < 1.0
    if shape[1] * shape[2] > 1:
        assert all(E.SHARE[0] <= s <= E.SHARE[1] for s in E.shares(truth["z"]))
    # the fixture is what the docstring says
    for name, lo, hi in (("x", -4, 4), ("g", -3, 3), ("w1", -2, 2), ("w2", -2, 2), ("w3", -2, 2), ("bias", -2, 2), ("rmean", -2, 2)):
        v = fix[name]
        assert torch.equal(v, v.round()) and lo <= float(v.min()) and float(v.max()) <= hi
    assert set(fix["gamma"].tolist()) <= {0.5, 1.0, 2.0}
    var = fix["rvar"].double() + E.EPS_DYADIC
    assert set(var[:12].tolist()) <= {1.0, 4.0, 16.0, 64.0} and float(var[12]) == 256.0
    assert torch.equal(truth["stats01"][13:], 1.0 / torch.sqrt(var)) and torch.equal(truth["stats01"][13:].float().double(), truth["stats01"][13:])
    # exact without the kernel: the stock fp32 layers equal the float64 ones bit for bit, and so does the order-free restatement
    ref, own = stock32(fix), E.chain_of(fix, E.EPS_DYADIC)
    for name in E.EXACT_TENSORS:
        if name == "stats01":
            continue
        t = truth[name].reshape(-1)
        assert torch.equal(ref[name].double().reshape(-1), t), name
        assert np.array_equal(own[name].reshape(-1), t.numpy()), name
        assert torch.equal(t.float().double(), t), name


@pytest.mark.parametrize("shape", [(3, 33, 65), (1, 3, 683), (2, 127, 127)])
def test_dyadic_weight_gradients_are_exact_in_any_order(shape):
    """sum |dc a| 2^r < 2^24 per weight, 2^-r the terms' resolution: every partial sum of the terms, in any order and through any fma chain, is a
    multiple of 2^-r below 2^24 2^-r, an fp32 number.  S1 and S2 are float64 sums in the kernel, rounded once: 2^53 there, and the truth is an fp32
    number (asserted with the fixture)."""
    fix, truth = E.dyadic_problem(shape, E.DYADIC_CASES[shape])
    d = {k: fix[k].double().numpy() for k in ("x", "g", "w1", "w2", "w3")}
    d.update(E.frozen_tables(fix, E.EPS_DYADIC))
    B, H, W = shape
    worst = 0.0

    def exact_in_any_order(terms, bits=24):
        nonlocal worst
        if not (terms != 0).any():
            return True
        r = 0
        while not np.array_equal(np.ldexp(terms, r), np.rint(np.ldexp(terms, r))):
            r += 1
            assert r < 64
        total = float(np.abs(np.ldexp(terms, r)).sum())
        if bits == 24:
            worst = max(worst, total / 2.0 ** 24)
        return total < 2.0 ** bits

    out = E.chain(d)
    grad = d["g"]
    acts = [d["x"]] + [np.maximum(z, 0) for z in out["z"][:2]]
    for l in (2, 1, 0):
        lo, hi = C.LAYERS[l]
        per = lambda v: v[lo:hi].reshape(1, -1, 1, 1)
        c = out["saved"][{0: slice(0, 4 * B * H * W), 1: slice(4 * B * H * W, 12 * B * H * W), 2: slice(12 * B * H * W, None)}[l]].reshape(B, hi - lo, H, W)
        dz = grad * (out["z"][l] > 0)
        xh = (c - per(d["mean"])) * per(d["invstd"])
        dc = per(d["alpha"]) * dz
        ap = np.zeros((B, acts[l].shape[1], H + 2, W + 2))
        ap[:, :, 1:H + 1, 1:W + 1] = acts[l]
        for co in range(hi - lo):
            assert exact_in_any_order(dz[:, co], 53) and exact_in_any_order(dz[:, co] * xh[:, co], 53), (l, co)
            for ci in range(acts[l].shape[1]):
                for k in range(9):
                    assert exact_in_any_order(dc[:, co] * ap[:, ci, k // 3:k // 3 + H, k % 3:k % 3 + W]), (l, co, ci, k)
        grad = E.shift_conv(dc, np.ascontiguousarray(d["w%d" % (l + 1)].transpose(1, 0, 2, 3)), -1)
    assert np.array_equal(grad, truth["gx"].numpy())
    print(f"{shape}: worst sum|term| 2^r / 2^24 = {worst:.4f}")


def test_dyadic_fixtures_decide_the_kink():
    """About 3 % of layer 1's pre-activations are exactly zero at every shape of some size."""
    for shape in [(1, 15, 17), (3, 33, 65), (2, 127, 127)]:
        z = E.dyadic_problem(shape, E.DYADIC_CASES[shape])[1]["z"]
        assert 0.01 <= float((z[0] == 0).double().mean()) <= 0.08 and int((z[1] == 0).sum()) > 0


def test_case_lists_sit_on_both_sides_of_every_launch_boundary():
    hw = {s[1] * s[2] for s in E.DYADIC_CASES if s[0] == 1}
    assert {1, 2, 255, 256, 257, 1023, 1024, 1025, 2049} <= hw
    assert any(s[1] == 1 and s[2] > 1 for s in E.DYADIC_CASES) and any(s[2] == 1 and s[1] > 1 for s in E.DYADIC_CASES)
    wg = {C.workgroups(*s) for s in E.DYADIC_CASES}
    assert {1, 2, 3, 64, 65, 256, 257} <= wg
    assert (3, 33, 65) in E.DYADIC_CASES and C.workgroups(3, 33, 65) == 9 and (2, 127, 127) in E.DYADIC_CASES and C.workgroups(2, 127, 127) == 32
    assert set(E.A3_CASES) <= set(E.DYADIC_CASES) and (2, 127, 127) in E.A3_CASES and (2, 127, 127) in E.STAGE_CASES
    assert any(C.workgroups(*s) > s[0] and s[1] * s[2] % 1024 for s in E.ONEHOT_SHAPES)


# ------------------------------------------------------------------------------------------------------------------------ A2
def test_onehot_sets_meet_every_tap_of_all_three_layers():
    met = [set(), set(), set()]
    for s in range(E.ONEHOT_SETS):
        ws = E.onehot_weights(s)
        assert [int(w.sum()) for w in ws] == [4, 8, 8]
        assert (ws[0].sum(axis=(1, 2, 3)) == 1).all() and (ws[1].sum(axis=(1, 2, 3)) == 1).all() and (ws[2].sum(axis=(0, 2, 3)) == 1).all()
        for l, w in enumerate(ws):
            met[l] |= {tuple(int(v) for v in i) for i in zip(*np.nonzero(w.reshape(w.shape[0], w.shape[1], 9)))}
    assert [len(m) for m in met] == [36, 288, 72]
    assert all((a == b).all() for a, b in zip(E.onehot_weights(E.BETA_SET), E.onehot_weights(0)))


@pytest.mark.parametrize("shape", E.ONEHOT_SHAPES)
def test_onehot_truth_is_float64_autograd_and_exact_in_fp32(shape):
    B, H, W = shape
    for s in (0, 7, 35, E.BETA_SET):
        fix, truth, ints = E.onehot_problem(s, shape)
        auto = C.stock(fix, torch.float64, train=False, running=C.running_of(fix), eps=E.EPS_DYADIC)
        auto["saved"] = E.saved_of(auto["c"])
        for name in E.EXACT_TENSORS:
            if name != "stats01":
                assert np.array_equal(auto[name].numpy().reshape(-1), truth[name].reshape(-1).astype(np.float64)), (s, name)
        # every sum of absolute terms is below 2^24: fp32 is exact on the set in any order
        acts = [np.abs(ints["x"])] + [np.maximum(z, 0) for z in truth["z"][:2]]
        grad = np.abs(ints["g"])
        for l in (2, 1, 0):
            mag = E.shift_dot(grad * np.ones_like(truth["z"][l]), acts[l])
            assert int(mag.max()) < 2 ** 24 and int(np.abs(truth["saved"]).max()) * int(grad.max()) * B * H * W < 2 ** 53
            assert int((grad * np.abs(truth["z"][l])).sum(axis=(0, 2, 3)).max()) < 2 ** 24             # S2
            grad = E.shift_conv(grad * np.ones_like(truth["z"][l]), np.ascontiguousarray(ints["w%d" % (l + 1)].transpose(1, 0, 2, 3)), -1)
        assert int(np.abs(truth["y"]).max()) < 2 ** 24
        if s != E.BETA_SET:                                                                           # the kink, in layers 1 and 2
            assert all(int((z == 0).sum()) > 0 for z in truth["z"][:2])
    # the codes name the pixel: no two pixels of a 3 x 3 neighbourhood share one
    x = np.abs(E.onehot_problem(0, shape)[2]["x"])[:, 0]
    for dy in range(0, min(3, H)):
        for dx in range(-min(2, W - 1), min(3, W)):
            if (dy, dx) > (0, 0):
                assert (x[:, dy:, max(dx, 0):W + min(dx, 0)] != x[:, :H - dy, max(-dx, 0):W - max(dx, 0)]).all()


# ------------------------------------------------------------------------------------------------------------------------ C. five wrong kernels
def rejected(fix, truth, mutant):
    """The names of the A1 / A2 tensors on which the wrong kernel differs from the truth."""
    if "alpha" in fix:
        wrong = E.chain(fix, np.int64, mutant)
    else:
        wrong = E.chain_of(fix, E.EPS_DYADIC, mutant=mutant)
    as_np = lambda v: v.numpy() if torch.is_tensor(v) else v
    return [n for n in E.EXACT_TENSORS if n != "stats01" and not np.array_equal(wrong[n].reshape(-1).astype(np.float64), as_np(truth[n]).reshape(-1))]


@pytest.mark.parametrize("shape", MUTANT_SHAPES)
def test_wrong_kernels_are_rejected_by_the_dyadic_fixture(shape):
    fix, truth = E.dyadic_problem(shape, E.DYADIC_CASES[shape])
    assert rejected(fix, truth, None) == []
    # 1. padding read as relu(beta): every plane behind layer 1 and every gradient
    assert {"y", "saved", "gx", "gw2", "gw3"} <= set(rejected(fix, truth, "padding"))
    # 2. mask >=: only gradients, and only because a zero pre-activation exists
    hit = rejected(fix, truth, "mask")
    assert hit and "y" not in hit and "saved" not in hit and any((z == 0).any() for z in truth["z"])
    # 3. the data adjoint gathers at p + k
    hit = rejected(fix, truth, "adjoint")
    assert "gx" in hit and "y" not in hit and "gw3" not in hit
    # 5. the last workgroup's partial left out of the S1 / S2 finish, of the weight finish
    hit = rejected(fix, truth, "drop-bn")
    assert hit and set(hit) <= {"gb1", "gb2", "gb3", "gg1", "gg2", "gg3"}
    hit = rejected(fix, truth, "drop-weight")
    assert hit and set(hit) <= {"gw1", "gw2", "gw3"}


def test_mask_mutant_fails_only_where_a_zero_pre_activation_exists():
    seen = {True: 0, False: 0}
    for shape in SMALL:
        fix, truth = E.dyadic_problem(shape, E.DYADIC_CASES[shape])
        zero = any(bool((z == 0).any()) for z in truth["z"])
        hit = rejected(fix, truth, "mask")
        assert not hit or zero, shape                       # never without a zero
        seen[zero] += 1
        if not zero:
            assert hit == [], shape
    assert seen[True] >= 8 and seen[False] >= 2             # fixtures of both kinds exist
    big = (3, 33, 65)
    assert rejected(*E.dyadic_problem(big, E.DYADIC_CASES[big]), "mask")


@pytest.mark.parametrize("shape", E.ONEHOT_SHAPES)
def test_wrong_kernels_are_rejected_by_the_onehot_sets(shape):
    B, H, W = shape
    for s in (0, 13, E.BETA_SET):
        _, truth, ints = E.onehot_problem(s, shape)
        assert rejected(ints, truth, None) == []
        assert "gx" in rejected(ints, truth, "adjoint")
        assert bool(rejected(ints, truth, "mask")) == any(bool((z == 0).any()) for z in truth["z"]) == (s != E.BETA_SET)
        hit = rejected(ints, truth, "padding")
        assert (s == E.BETA_SET) == bool(hit), "with beta = 0 the padding reads relu(0) = 0 either way"
    # the beta set: wrong by a whole integer on every border pixel of c2 whose tap looks outside
    _, truth, ints = E.onehot_problem(E.BETA_SET, shape)
    n = B * H * W
    wrong = E.chain(ints, np.int64, "padding")["saved"][4 * n:12 * n].reshape(B, 8, H, W)
    diff = wrong - truth["saved"][4 * n:12 * n].reshape(B, 8, H, W)
    assert set(np.unique(diff)) == {0, 3} and (diff[:, :, 1:-1, 1:-1] == 0).all()
    for co, (ci, k) in enumerate(E.onehot_taps(E.BETA_SET)[1]):
        outside = np.zeros((H, W), bool)
        if k // 3 != 1:
            outside[0 if k // 3 == 0 else H - 1, :] = True
        if k % 3 != 1:
            outside[:, 0 if k % 3 == 0 else W - 1] = True
        assert ((diff[:, co] == 3) == outside).all(), co


@pytest.mark.parametrize("shape", E.A3_CASES)
def test_wrong_statistics_are_rejected_by_the_integer_fixture(shape):
    fix = E.dyadic_problem(shape, E.DYADIC_CASES[shape])[0]
    c1, rows = E.layer1_batch_stats(fix, E.EPS_A3[0])
    assert np.array_equal(c1.reshape(-1), E.chain_of(fix, E.EPS_DYADIC)["saved"][:c1.size])
    # 4. the unbiased factor dropped: row 2 and nothing else
    wrong = E.layer1_batch_stats(fix, E.EPS_A3[0], "unbiased")[1]
    assert np.array_equal(wrong[:2], rows[:2]) and (wrong[2] != rows[2])[rows[2] != 0].all() and (rows[2] != 0).any()
    # 5. the last workgroup's partial left out of the statistics finish
    wrong = E.layer1_batch_stats(fix, E.EPS_A3[0], "drop-stats")[1]
    assert wrong.tobytes() != rows.tobytes()
    # another eps: invstd and nothing else
    other = E.layer1_batch_stats(fix, E.EPS_A3_PERMUTED[0])[1]
    assert (other[1] != rows[1]).all() and np.array_equal(other[[0, 2]], rows[[0, 2]])


# ------------------------------------------------------------------------------------------------------------------------ B. the stage checker
def test_fma32_is_the_correctly_rounded_fma():
    rng = np.random.default_rng(3)
    a, b, c = (rng.standard_normal(2000).astype(np.float32) for _ in range(3))
    got = E.fma32(a, b, c)
    from fractions import Fraction
    for i in range(0, 2000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        assert abs(exact - Fraction(float(got[i]))) <= min(abs(exact - Fraction(float(lo))), abs(exact - Fraction(float(hi))))
    # an inexact tie: c = 1 + 2^-23, a b = 2^-24 (1 + 2^-23)(1 - 2^-23) = 2^-24 - 2^-70.  The exact sum lies just below the midpoint of c and
    # 1 + 2^-22 and rounds DOWN to c; float64 rounds it to the midpoint, which ties-to-even would then round UP
    before = E.FMA_TIES[0]
    c2, a2, b2 = np.float32(1.0 + 2.0 ** -23), np.float32(2.0 ** -24 * (1.0 + 2.0 ** -23)), np.float32(1.0 - 2.0 ** -23)
    mid = float(np.float64(a2) * np.float64(b2) + np.float64(c2))
    assert mid == 1.0 + 2.0 ** -23 + 2.0 ** -24 and np.float32(mid) == np.float32(1.0 + 2.0 ** -22)
    assert E.fma32(a2, b2, c2) == c2 and E.FMA_TIES[0] == before + 1
    assert E.fma32(-a2, b2, -c2) == -c2 and E.FMA_TIES[0] == before + 2
    assert E.fma32(np.float32(2.0 ** -24), np.float32(1), c2) == np.float32(1.0 + 2.0 ** -22) and E.FMA_TIES[0] == before + 2      # an exact tie: to even


def test_enclosures():
    lo, hi = E.enclose_sum(np.arange(-5.0, 100.0))
    assert lo == hi == float(np.arange(-5.0, 100.0).sum())
    t = np.random.default_rng(5).standard_normal(1000).astype(np.float32).astype(np.float64)
    lo, hi = E.enclose_sum(t)
    assert lo < math.fsum(t) < hi and hi - lo < 1e-9
    for order in (t, t[::-1], np.sort(t)):
        s = 0.0
        for v in order:
            s += v
        assert lo <= s <= hi
    enc = E.enclose_stats(t, t.size, 1e-5)
    got = E.stats_statements(t.sum(), (t * t).sum(), t.size, 1e-5)[:3]
    assert all(a <= g <= b for g, (a, b) in zip(got, enc))
    ints = np.arange(1.0, 50.0)
    enc = E.enclose_stats(ints, ints.size, 1e-3)
    assert all(a == b for a, b in enc)
    assert tuple(a for a, _ in enc) == E.stats_statements(ints.sum(), (ints * ints).sum(), ints.size, 1e-3)[:3]


@pytest.mark.parametrize("shape, frozen", [((2, 5, 7), False), ((2, 5, 7), True), ((1, 25, 41), False), ((1, 1, 2), False), ((1, 1, 1), True)])
def test_stage_checker_accepts_the_host_model_and_rejects_one_wrong_element(shape, frozen):
    fix = E.stage_fixture(shape)
    model = E.emulate(fix, frozen, C.EPS3)
    rep = E.check_stages(fix, E.device_dict(model), frozen, C.EPS3)
    assert not rep.bad, rep.bad
    assert rep.gw_ratio <= 1.0 and rep.enclosures == 39 + 26
    if frozen:
        assert rep.not_points <= 26                          # the frozen statistics are statements on exactly known numbers
    # the model is the operation: inside the bound tests' bound of the float64 truth
    truth = C.restatement(fix, eps=C.EPS3) if not frozen else C.stock(fix, torch.float64, train=False, running=C.running_of(fix), eps=C.EPS3)
    got = E.device_dict(model)
    if shape[0] * shape[1] * shape[2] > 2:
        for name in ("y", "gx", "gw1", "gw2", "gw3", "gb1", "gg2"):
            t = truth[name].double()
            assert float((got[name].double().reshape(t.shape) - t).abs().max()) <= 1e-4 * max(1.0, float(t.abs().max())), name
    # one element one ulp off, anywhere, is named
    n = shape[0] * shape[1] * shape[2]
    for key, i in (("saved", 0), ("saved", 4 * n + n // 2), ("saved", 13 * n - 1), ("y", n - 1), ("gx", n // 2), ("stats", 13), ("stats", 25), ("gp", 400), ("gp", 421)):
        if frozen and key == "stats":
            continue
        wrong = {k: v.clone() for k, v in model.items()}
        v = wrong[key].reshape(-1)
        v[i] = float(np.nextafter(np.float32(v[i]), np.float32(np.inf))) if float(v[i]) != 0 else 1e-3
        assert E.check_stages(fix, E.device_dict(wrong), frozen, C.EPS3).bad, (key, i)
    # a permutation of the three eps leaves the enclosures
    swapped = E.emulate(fix, frozen, (C.EPS3[1], C.EPS3[2], C.EPS3[0]))
    assert E.check_stages(fix, E.device_dict(swapped), frozen, C.EPS3).bad


def test_a3_eps_permutation_moves_every_invstd_in_the_host_model():
    for shape in [s for s in E.A3_CASES if s[0] * s[1] * s[2] <= 7000]:
        fix = E.dyadic_problem(shape, E.DYADIC_CASES[shape])[0]
        a, b = (E.emulate(fix, False, eps)["stats"].numpy() for eps in (E.EPS_A3, E.EPS_A3_PERMUTED))
        rows = E.layer1_batch_stats(fix, E.EPS_A3[0])[1]
        assert a[0:4].tobytes() == rows[0].tobytes() and a[13:17].tobytes() == rows[1].tobytes() and a[26:30].tobytes() == rows[2].tobytes()
        assert (a[13:17] != b[13:17]).all() and (a[17:25] != b[17:25]).all() and a[25] != b[25]
