"""The oracle and the cases of the gated, clipped AMSGrad step (tests/opt_step_cases.py), and hdn_amd.optim's argument validation - no GPU.

  - the float64 restatement against the reference's own formulation (is_valid_number, stock clip_grad_norm_ and Adam(amsgrad=True), float64, CPU);
  - the case inputs: the sizes, magnitudes, gate values and the distance of every case from the clamp norm == max_norm;
  - fourteen simulated wrong kernels, each of which must leave the bound on at least one case;
  - GatedAMSGrad / grad_norm refusing CPU tensors and bad hyper-parameters with the package's errors."""
import math

import numpy as np
import pytest
import torch

import opt_step_cases as C
from hdn_amd import GatedAMSGrad, grad_norm, optim
from hdn_amd._lib import HdnHipError

CASES = C.all_cases()


def test_the_cases_restate_the_modules_constants():
    assert (C.CHUNK, C.TENSORS_PER_LAUNCH) == (optim.CHUNK, optim.TENSORS_PER_LAUNCH)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_oracle_agrees_with_stock_float64(c):
    """Stock PyTorch in float64 and the restatement differ by float64 rounding only: a step is a few dozen operations of relative error 1.1e-16
    each, three steps and a norm over at most 2 10^4 elements stay below 1e-12 relative (no quantity cancels in these cases); status and
    counters are exact.  A non-finite gradient norm is the one place where the stock lines are not followed (they write NaN everywhere)."""
    want, got = C.oracle(c), C.stock_steps(c, torch.float64)
    assert got["status"] == want["status"] and np.array_equal(got["steps"], want["steps"])
    qg, qw = C.compared(got, clipped=True), C.compared(want, clipped=True)
    for k in qw:
        for a, b in zip(qg[k], qw[k]):
            assert (a is None) == (b is None), (c.name, k)
            if a is None:
                continue
            a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
            fin = np.isfinite(b)
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)]), (c.name, k)
            rel = np.abs(a[fin] - b[fin]) / np.maximum(np.abs(b[fin]), 1e-300)
            assert rel.size == 0 or rel.max() <= 1e-12, (c.name, k, rel.max())


def test_case_inputs():
    """What the device tests rely on: the sizes, the magnitudes, fp32-exact gate values with the statuses they must give, both sides of the clamp
    and no case within rounding of it, fewer than a million elements, and an fp32 reference that is a few ulps from the oracle (so the bound
    means something)."""
    names = {c.name for c in CASES}
    assert len(names) == len(CASES)
    sizes = C.case("sizes").sizes
    assert set(sizes) >= {1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, C.CHUNK - 1, C.CHUNK, C.CHUNK + 1, 2 * C.CHUNK + 3}
    assert C.case("many").sizes == (1,) * (C.TENSORS_PER_LAUNCH + 1)
    assert sum(sum(c.sizes) for c in CASES) < 1_000_000
    assert len(set(C.case("many").lrs)) == 3 and len(set(C.case("sizes").lrs)) == 2
    assert float(np.float32(C.LOSS_LIMIT)) == C.LOSS_LIMIT and C.NEXT_AFTER_LIMIT > C.LOSS_LIMIT
    assert float(np.float32(C.NEXT_AFTER_LIMIT)) == C.NEXT_AFTER_LIMIT
    clamped = set()
    for c in CASES:
        want, d_ref = C.references(c)
        for k in range(C.K):
            loss = c.losses[k]
            assert loss is None or math.isnan(loss) or float(np.float32(loss)) == loss, (c.name, "the loss is not exact in fp32")
            for i, g in enumerate(c.grads()[k]):
                if g is not None and (k, i) not in c.poison:
                    assert 2.5e-4 <= np.abs(g).min() and np.abs(g).max() <= 2e3          # scales 1e-3 .. 1e3 times a factor in [0.3, 1.95]
            norm = want["grad_norm"][k]
            if c.max_norm is not None and math.isfinite(norm):
                assert abs(norm / c.max_norm - 1.0) > 1e-3, (c.name, k, "within rounding of the clamp")
                clamped.add(norm < c.max_norm)
        for p in c.params0():
            assert 0.5 <= np.abs(p).min() and np.abs(p).max() <= 2.0
        for k, d in d_ref.items():
            assert d < 64.0, (c.name, k, d)                                    # ulps: no cancellation inflates the bound
        if c.name.startswith("gate_"):
            assert want["status"] == [0, C.GATE_STATUS[c.name[5:]], 0]
            assert list(want["steps"]) == [3.0 if want["status"][1] == 0 else 2.0] * 2
    assert clamped == {True, False}
    assert C.oracle(C.case("absent"))["steps"].tolist() == [3.0, 2.0, 3.0]
    w = C.case("warm").state0()
    assert all((a > b).all() for a, b in zip(w["max_exp_avg_sq"], w["exp_avg_sq"]))


def _leaves_the_bound(res, c):
    want, d_ref = C.references(c)
    if list(res["status"]) != want["status"] or not np.array_equal(res["steps"], want["steps"]):
        return True
    got, exp = C.compared(res, clipped=True), C.compared(want, clipped=True)
    return any(C.distance(got[k], exp[k]) > C.bound(d_ref[k]) for k in got)


def test_the_references_themselves_stay_inside_the_bound():
    for c in CASES:
        assert not _leaves_the_bound(C.oracle(c), c)
        assert not _leaves_the_bound(C.stock32(c), c), c.name               # inside 4 d_ref trivially


@pytest.mark.parametrize("mutation", C.MUTATIONS)
def test_a_simulated_wrong_kernel_leaves_the_bound(mutation):
    caught = [c.name for c in CASES if _leaves_the_bound(C.oracle(c, mutation), c)]
    print(f"OPT_STEP mutation {mutation}: caught by {caught}")
    assert caught, mutation


# ------------------------------------------------------------------------------------------------------------------- validation, CPU tensors
def _param(n=4, dtype=torch.float32):
    return torch.nn.Parameter(torch.ones(n, dtype=dtype))


def test_cpu_parameters_are_refused_without_a_fallback():
    with pytest.raises(HdnHipError, match="no CPU fallback"):
        GatedAMSGrad([_param()], lr=2e-4)
    with pytest.raises(HdnHipError, match="no CPU fallback"):
        GatedAMSGrad([{"params": [_param()], "lr": 2e-4}, {"params": [_param(3)], "lr": 2e-5}], weight_decay=1e-4, max_norm=10.0)
    with pytest.raises(HdnHipError, match="no CPU fallback"):
        grad_norm([torch.ones(3)])


@pytest.mark.parametrize("kw", [dict(lr=-1.0), dict(lr=float("nan")), dict(lr="1e-3"), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)),
                                dict(betas=(0.9,)), dict(eps=-1e-8), dict(weight_decay=-1e-4), dict(max_norm=0.0), dict(max_norm=-1.0),
                                dict(max_norm=float("inf")), dict(loss_limit=float("nan")), dict(loss_limit=None),
                                dict(clip_grads_in_place=1)], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_bad_hyper_parameters_raise_before_anything_else(kw):
    with pytest.raises(ValueError, match="GatedAMSGrad"):
        GatedAMSGrad([_param()], **kw)


def test_groups_share_betas_eps_and_weight_decay():
    with pytest.raises(ValueError, match="only lr is per group"):
        GatedAMSGrad([{"params": [_param()]}, {"params": [_param(3)], "weight_decay": 0.5}])
    with pytest.raises(ValueError, match="lr"):
        GatedAMSGrad([{"params": [_param()], "lr": -2.0}])


def test_grad_norm_needs_a_tensor():
    with pytest.raises(ValueError, match="no tensor"):
        grad_norm([None])
