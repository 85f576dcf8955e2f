"""tests/conv3x3_train_cases.py checked without a GPU: the float64 truths against autograd, the full-correlation identity behind the dgrad kernel, the
exponent rule and the piece bound of the gradient split, the integer problems' range, the case lists against the library's own form answers (host
queries), and — the point of the emulation — that each simulated wrong kernel fails the checks the device results have to pass while the right one passes."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv3x3_train_cases as TC  # noqa: E402


def test_truths_equal_float64_autograd():
    g = torch.Generator().manual_seed(0)
    for (B, S, CI, CO) in ((2, 3, 4, 5), (3, 7, 6, 2), (1, 6, 3, 3)):
        x = torch.randn(B, CI, S, S, generator=g, dtype=torch.float64, requires_grad=True)
        w = torch.randn(CO, CI, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
        dy = torch.randn(B, CO, S - 2, S - 2, generator=g, dtype=torch.float64)
        y = F.conv2d(x, w)
        y.backward(dy)
        xd, wd = x.detach(), w.detach()
        assert (TC.conv_truth(xd, wd) - y.detach()).abs().max() < 1e-12
        assert (TC.gx_truth(dy, wd, S) - x.grad).abs().max() < 1e-12
        assert (TC.gw_truth(xd, dy) - w.grad).abs().max() < 1e-12
        # the identity the dgrad kernel computes: a VALID convolution of the padding-2 dy with w'[ci][co][ky][kx] = w[co][ci][2-ky][2-kx]
        assert (TC.conv_truth(TC.pad2(dy), TC.w_dgrad(wd)) - x.grad).abs().max() < 1e-12
        # K slices partition the pixels
        m = torch.zeros(B, S - 2, S - 2, dtype=torch.bool)
        m[:, : (S - 2) // 2] = True
        assert (TC.gw_truth(xd, dy, m) + TC.gw_truth(xd, dy, ~m) - w.grad).abs().max() < 1e-12


def test_exponent_rule():
    for k in range(-126, 127, 7):
        for m in (1.0, 1.5, 1.9999999):
            a = m * 2.0 ** k
            e = TC.exponent_rule(a)
            assert 2.0 ** 14 <= float(torch.tensor(a, dtype=torch.float32)) * 2.0 ** e < 2.0 ** 15, (a, e)
            assert TC.exponent_rule(a * 2.0 ** 5) == e - 5 or k + 5 > 127           # a power of two shifts e and nothing else
            assert TC.exponent_rule(m * 2.0 ** k) == TC.exponent_rule(1.0 * 2.0 ** k)   # the exponent field only
    assert TC.exponent_rule(0.0) == 0 and TC.exponent_rule(float("inf")) == 0 and TC.exponent_rule(float("nan")) == 0
    assert TC.exponent_rule(1e-40) == 140                                           # subnormal: as the smallest normal
    g = torch.tensor([1e-7, -3e-6, 0.0])
    assert TC.grad_exponent(g) == TC.exponent_rule(3e-6) and TC.grad_exponent(torch.tensor([1.0, float("nan")])) == 0


def test_float16_split_meets_the_piece_bound():
    """Every element v of a gradient is carried by its two pieces within max(2^-22 |v|, 2^-50 amax), at magnitudes from 1e-30 to 1e20."""
    g = torch.Generator().manual_seed(1)
    for mag in (1e-30, 1e-20, 1e-10, 1e-7, 1e-3, 1.0, 1e4, 1e10, 1e20):
        v = (torch.randn(4096, generator=g) * mag).float()
        v[:64] *= torch.logspace(-12, 0, 64)                 # a wide range below amax
        v[100] = 0.0
        amax = float(v.abs().max())
        e = TC.grad_exponent(v)
        assert 2.0 ** 14 <= amax * 2.0 ** e < 2.0 ** 15
        p0, p1 = TC.split16(v.double(), e)
        assert torch.isfinite(p0).all() and torch.isfinite(p1).all()
        err = (TC.joined(p0, p1, e) - v.double()).abs()
        assert bool((err <= TC.piece_bound(v, amax)).all()), (mag, float((err / TC.piece_bound(v, amax)).max()))
    # ... and the activations' fixed 2^-8 does NOT, at a gradient's magnitude: the reason for the data-chosen scale
    v = (torch.randn(4096, generator=g) * 1e-7).float()
    p0, p1 = TC.split16(v.double(), -8)
    assert not bool(((TC.joined(p0, p1, -8) - v.double()).abs() <= TC.piece_bound(v, float(v.abs().max()))).all())


def test_integer_problems_are_exact_in_fp32():
    for c in TC.EXACT_CASES:
        assert TC.integer_sum_limit(*c) < 2 ** 24, c
    x, w, dy, y, gx, gw = TC.integer_problem(3, 7, 96, 32)
    assert max(int(y.abs().max()), int(gx.abs().max()), int(gw.abs().max())) <= TC.integer_sum_limit(3, 7, 96, 32)
    assert int(x.abs().max()) == 4 and int(w.abs().max()) == 2 and int(dy.abs().max()) == 3


def _lib_or_skip():
    from hdn_amd import _lib
    return _lib.load()          # host queries only: the library loads without a GPU


def test_case_lists_name_their_launch_form():
    lib = _lib_or_skip()
    for name, cases in TC.DGRAD_CASES.items():
        for c in cases:
            assert TC.dgrad_form_name(lib.hdn_conv3x3v_dgrad_form(*c)) == name, (c, name)
    for name, cases in TC.WGRAD_CASES.items():
        for c in cases:
            v = lib.hdn_conv3x3v_wgrad_form(*c)
            assert TC.wgrad_form_name(v) == name, (c, name, TC.wgrad_form_name(v))
            W, units, ups, Z = TC.wgrad_plan(*c)
            assert (v & 0xffff, v >> 16) == (W, Z) and lib.hdn_conv3x3v_wgrad_workspace_bytes(*c) == (36 * Z * c[2] * c[3] if Z > 1 else 0)
    assert set(TC.DGRAD_CASES) == {"A", "A split", "B", "B split", "C"}
    assert set(TC.WGRAD_CASES) == {"W1", "W2", "W4", "W1 split", "W2 split", "W4 split"}
    # the plan reads (B, S, CI, CO) only, and the dgrad schedule is the forward kernel's at the same M, N, K
    assert lib.hdn_conv3x3v_dgrad_form(2, 31, 256, 256) == lib.hdn_conv3x3d_form(2, 31, 256, 256, 1)
    assert lib.hdn_conv3x3v_dgrad_form(2, 2, 32, 32) < 0 and lib.hdn_conv3x3v_wgrad_form(2, 5, 48, 32) < 0


def _emulated(fault):
    def factory():
        calls = [0]

        def fn(x, w, dy):
            calls[0] += 1
            return TC.emulate(x, w, dy, fault, call=calls[0] - 1)
        return fn
    return factory


def test_the_emulated_kernels_pass_every_check():
    assert TC.all_checks(_emulated(None)) == {"exact": True, "bound": True, "repeatable": True}


# which check has to catch which wrong kernel
CAUGHT_BY = {
    "unflipped taps": "exact", "untransposed weights": "exact", "missing halo row": "exact", "missing halo column": "exact",
    "slice boundary off by one": "exact", "dropped lo": "bound", "fixed 2^-8 gradient split": "bound", "slice order by arrival": "repeatable",
}


@pytest.mark.parametrize("fault", TC.FAULTS)
def test_each_simulated_wrong_kernel_fails_its_check(fault):
    assert set(CAUGHT_BY) == set(TC.FAULTS)
    check = CAUGHT_BY[fault]
    if check == "exact":
        cases = [(3, 7, 32, 32)] if fault == "untransposed weights" else [(2, 5, 32, 96), (9, 5, 32, 32)]
        assert not TC.check_exact(_emulated(fault)(), cases)
    elif check == "bound":
        assert not TC.check_random(_emulated(fault)(), [(2, 5, 32, 96)], dy_scale=1e-7)
    else:
        assert not TC.check_repeatable(_emulated(fault)(), (9, 5, 32, 32))
