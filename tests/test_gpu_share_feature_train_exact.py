"""PreShareFeature's training kernels (csrc/share_feature_train.hip) on the device, exactly: the order-free fixtures of
tests/share_feature_train_exact_cases.py against float64 / int64 truths with torch.equal (A1 - A3), and every stage recomputed from the device's
own upstream outputs on N(0, 1) data, bit for bit or inside an a-priori enclosure (B).  A mismatch names its first wrong element.  The host side,
tests/test_share_feature_train_exact_host.py, proves without a device that the fixtures are exact and which wrong kernel each one rejects."""
import numpy as np
import pytest
import torch

import share_feature_train_cases as C
import share_feature_train_exact_cases as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRADS = tuple(n for n in E.EXACT_TENSORS if n[0] == "g")


def raw_clean(fix, offsets, frozen, eps):
    got, clean = E.run_raw(fix, DEV, offsets, frozen=frozen, eps=eps)
    assert clean, "bytes outside an output were written"
    for k, v in got.items():
        assert not torch.isnan(v).any(), f"{k} not fully overwritten"
    return got


# ------------------------------------------------------------------------------------------------------------------------ A1. dyadic, frozen
@pytest.mark.parametrize("offsets", C.OFFSETS)
@pytest.mark.parametrize("shape", list(E.DYADIC_CASES))
def test_dyadic_fixture_through_the_c_abi_equals_float64(shape, offsets):
    fix, truth = E.dyadic_problem(shape, E.DYADIC_CASES[shape])
    got = raw_clean(fix, offsets, True, E.EPS_DYADIC)
    bad = E.compare_exact(got, truth, E.EXACT_TENSORS, shape)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape", list(E.DYADIC_CASES))
def test_dyadic_fixture_through_the_module_in_eval_mode_equals_float64(shape):
    fix, truth = E.dyadic_problem(shape, E.DYADIC_CASES[shape])
    running = C.running_of(fix)
    got = C.run_module(fix, DEV, train=False, running=running, eps=E.EPS_DYADIC)
    assert got["grad_fn"]
    bad = E.compare_exact(got, truth, ("y",) + GRADS, shape)
    assert not bad, "\n".join(bad)
    for l, (lo, hi) in enumerate(C.LAYERS, start=1):
        assert torch.equal(got["rm%d" % l], running[0][lo:hi]) and torch.equal(got["rv%d" % l], running[1][lo:hi]) and got["nbt%d" % l] == 0


# ------------------------------------------------------------------------------------------------------------------------ A2. one-hot sets
@pytest.mark.parametrize("shape", E.ONEHOT_SHAPES)
def test_onehot_sets_meet_every_tap_exactly(shape):
    """36 sets + the beta > 0 set: every plane, gx and every weight gradient equal the int64 index arithmetic.  In the beta set a kernel that
    normalises the padding is wrong by a whole integer on every border pixel."""
    bad = []
    for s in list(range(E.ONEHOT_SETS)) + [E.BETA_SET]:
        fix, truth, _ = E.onehot_problem(s, shape)
        got = raw_clean(fix, C.OFFSETS[s % 2], True, E.EPS_DYADIC)
        bad += [f"set {s}: {m}" for m in E.compare_exact(got, truth, E.EXACT_TENSORS, shape, E.onehot_tap_names(s))]
    assert not bad, "\n".join(bad[:20])


# ------------------------------------------------------------------------------------------------------------------------ A3. batch statistics
@pytest.mark.parametrize("shape", E.A3_CASES)
def test_integer_fixture_batch_statistics_of_layer_1_are_the_float64_statements(shape):
    fix = E.dyadic_problem(shape, E.DYADIC_CASES[shape])[0]
    n = shape[0] * shape[1] * shape[2]
    runs = {}
    for eps in (E.EPS_A3, E.EPS_A3_PERMUTED):
        got = raw_clean(fix, C.OFFSETS[0], False, eps)
        c1, rows = E.layer1_batch_stats(fix, eps[0])
        m = E.first_mismatch("saved", got["saved"][:4 * n].numpy(), c1, (shape[0], shape[1], shape[2]))
        assert m is None, m
        stats = got["stats"].numpy()
        for row, what in enumerate(("mean", "invstd", "unbiased variance")):
            have = stats[13 * row:13 * row + 4]
            assert have.tobytes() == rows[row].tobytes(), f"eps {eps}: layer 1 {what}: got {have!r} want {rows[row]!r}"
        runs[eps] = stats
    a, b = runs[E.EPS_A3], runs[E.EPS_A3_PERMUTED]
    # another eps moves every invstd of its own layer ...
    assert (a[13:17] != b[13:17]).all() and (a[17:25] != b[17:25]).all() and a[25] != b[25]
    # ... and neither mean nor unbiased variance of layer 1, which sees no eps at all
    assert np.array_equal(a[0:4], b[0:4]) and np.array_equal(a[26:30], b[26:30])


# ------------------------------------------------------------------------------------------------------------------------ B. device-fed stages
# (one value per channel has no batch statistics: the C ABI refuses it, the host tests assert that)
@pytest.mark.parametrize("shape, frozen", [(s, f) for s in E.STAGE_CASES for f in (False, True) if f or s != (1, 1, 1)])
def test_every_stage_from_the_devices_own_upstream_outputs(shape, frozen):
    """y, the 13 saved planes and gx bit for bit; stats, gb, gg inside their enclosures; gw inside GW_ROUNDINGS 2^-24 sum |dc a| per weight.
    Three different eps, so a permutation of them leaves the enclosures."""
    fix = E.stage_fixture(shape)
    got = raw_clean(fix, C.OFFSETS[0], frozen, C.EPS3)
    rep = E.check_stages(fix, got, frozen, C.EPS3)
    print(f"stages {shape} {'frozen' if frozen else 'batch'}: worst gw error / bound {rep.gw_ratio:.4f}, {rep.not_points} of {rep.enclosures} "
          f"enclosures not points, fma ties {E.FMA_TIES[0]}")
    assert not rep.bad, "\n".join(rep.bad[:20])
    assert rep.gw_ratio <= 1.0
