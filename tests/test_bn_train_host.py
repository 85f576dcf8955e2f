"""The training BatchNorm + ReLU without a GPU: the builders of tests/bn_train_cases.py against float64 autograd, the case list against
hdn_bn_relu_train_form, the workspace query, every error code of the raw ABI (they are checked before the first HIP call) and bn_train.qualifies."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bn_train_cases as BC  # noqa: E402
from hdn_amd import _lib, bn_train as BT  # noqa: E402  (without the feature nothing here is collected)

OK, E_NULL, E_SHAPE, E_LIMIT, E_ALIAS = 0, -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------------------------- the builders
@pytest.mark.parametrize("case", BC.EXACT_CASES)
def test_exact_expectations_are_float64_autograd(case):
    prob, expect = BC.exact_problem(*case)
    for relu in (0, 1):
        ref = BC.reference(prob, *case, relu, eps=BC.EXACT_EPS, momentum=BC.EXACT_MOMENTUM)
        for name in ("y", "dc", "dgamma", "dbeta", "mean", "invstd", "rm", "rv"):
            assert torch.equal(expect[relu][name].float(), ref[name].float()), (case, relu, name)
        dc = expect[relu]["dc"]
        assert torch.equal(dc * 2, torch.round(dc * 2)) and float(dc.abs().max()) < 2 ** 22          # exact half-integers, exact in fp32


@pytest.mark.parametrize("case", [(2, 1, 32), (2, 169, 96)])
def test_pytorch_fp32_reproduces_the_exact_forward(case):
    prob, expect = BC.exact_problem(*case)
    for relu in (0, 1):
        got = BC.reference(prob, *case, relu, eps=BC.EXACT_EPS, momentum=BC.EXACT_MOMENTUM, dtype=torch.float32)
        assert torch.equal(got["y"], expect[relu]["y"].float())


def test_random_and_large_mean_problems_keep_the_margin():
    for case in BC.CASES:
        c, gamma, beta = BC.random_problem(*case)[:3]
        assert BC.min_abs_z(c, gamma, beta) >= BC.MARGIN, case
    for case in BC.LARGE_MEAN_CASES:
        c, gamma, beta = BC.large_mean_problem(*case)[:3]
        assert BC.min_abs_z(c, gamma, beta) >= BC.MARGIN, case
        assert float(c.mean()) > 990.0


# ---------------------------------------------------------------------------------------------------------------------------------- the forms
def test_the_cases_reach_every_form_and_sit_on_the_threshold(lib):
    form = lambda case: lib.hdn_bn_relu_train_form(*case)
    for cases in (BC.CASES, BC.EXACT_CASES):
        assert {form(c) for c in cases} == {0, 1}
    (b_last, P, C), (b_first, _, _) = BC.THRESHOLD_CASES
    assert b_first == b_last + 1
    walked = [form((B, P, C)) for B in range(1, 4 * b_first)]
    assert walked == sorted(walked) and set(walked) == {0, 1}                      # one switch as B is walked
    assert walked.index(1) + 1 == b_first and form((b_last, P, C)) == 0            # the last batch of form 0, the first of form 1
    assert b_last * P <= BC.FUSED_MAX_ROWS < b_first * P
    # the threshold is one on N: other (P, C) switch at the same row count
    for P2, C2 in ((1, 32), (169, 64), (841, 2048)):
        for B in (BC.FUSED_MAX_ROWS // P2, BC.FUSED_MAX_ROWS // P2 + 1):
            if B >= 1 and B * P2 >= 2:
                assert form((B, P2, C2)) == int(B * P2 > BC.FUSED_MAX_ROWS), (B, P2, C2)


def test_workspace_bytes_are_what_the_form_needs(lib):
    for case in BC.CASES + BC.EXACT_CASES:
        n = lib.hdn_bn_relu_train_workspace_bytes(*case)
        if lib.hdn_bn_relu_train_form(*case) == 0:
            assert n == 0, case
        else:
            B, P, C = case
            assert n > 0 and n % 16 == 0 and n >= 8 * C + 16 * C, case             # S1 / N, S2 / N and at least one partial of 2 C doubles
    for bad, rc in (((0, 25, 32), E_SHAPE), ((2, 25, 48), E_SHAPE), ((1, 1, 32), E_SHAPE), ((2, 25, 4096), E_LIMIT), ((1 << 16, 1 << 10, 64), E_LIMIT)):
        assert lib.hdn_bn_relu_train_workspace_bytes(*bad) == rc and lib.hdn_bn_relu_train_form(*bad) == rc, bad


# ---------------------------------------------------------------------------------------------------------------------------- the error codes
class _Args:
    """Host buffers standing in for device memory: every check below is made before the first HIP call, so nothing is dereferenced."""

    def __init__(self, lib, B=41, P=25, C=64):
        self.lib, self.B, self.P, self.C = lib, B, P, C
        n = B * P * C
        self.ws_bytes = max(int(lib.hdn_bn_relu_train_workspace_bytes(B, P, C)), 0)
        self.keep = {}
        for name, floats in (("c", n), ("y", n), ("dy", n), ("dc", n), ("gamma", C), ("beta", C), ("stats", 2 * C), ("rm", C), ("rv", C), ("dgamma", C),
                             ("dbeta", C), ("ws", self.ws_bytes // 4 + 8)):
            self.keep[name] = torch.zeros(floats + 8)
        self.p = {k: self._aligned(v) for k, v in self.keep.items()}

    @staticmethod
    def _aligned(t):
        return t.data_ptr() + (-t.data_ptr() % 16)

    def fwd(self, momentum=0.1, eps=1e-5, relu=1, layout=1, B=None, P=None, C=None, ws_bytes=None, **ptrs):
        p = dict(self.p, **ptrs)
        v = lambda k: ctypes.c_void_p(p[k]) if p[k] else None
        return self.lib.hdn_bn_relu_train_fwd_f32(v("c"), v("gamma"), v("beta"), v("y"), v("stats"), v("rm"), v("rv"), momentum, eps, v("ws"),
                                                  self.ws_bytes if ws_bytes is None else ws_bytes, self.B if B is None else B,
                                                  self.P if P is None else P, self.C if C is None else C, relu, layout, None)

    def bwd(self, relu=1, layout=1, B=None, P=None, C=None, ws_bytes=None, **ptrs):
        p = dict(self.p, **ptrs)
        v = lambda k: ctypes.c_void_p(p[k]) if p[k] else None
        return self.lib.hdn_bn_relu_train_bwd_f32(v("dy"), v("c"), v("gamma"), v("beta"), v("stats"), v("dc"), v("dgamma"), v("dbeta"), v("ws"),
                                                  self.ws_bytes if ws_bytes is None else ws_bytes, self.B if B is None else B,
                                                  self.P if P is None else P, self.C if C is None else C, relu, layout, None)


def test_every_error_code_comes_through_the_raw_abi(lib):
    a = _Args(lib)
    assert a.ws_bytes > 0                                                           # form 1: the workspace checks are live
    for name in ("c", "gamma", "beta", "y", "stats", "ws"):
        assert a.fwd(**{name: 0}) == E_NULL, name
    for name in ("dy", "c", "gamma", "beta", "stats", "ws"):
        assert a.bwd(**{name: 0}) == E_NULL, name
    for call in (a.fwd, a.bwd):
        for kw in (dict(B=0), dict(P=0), dict(C=0), dict(B=-1), dict(C=48), dict(B=1, P=1), dict(relu=2), dict(layout=2), dict(layout=-1)):
            assert call(**kw) == E_SHAPE, (call.__name__, kw)
        assert call(C=4096) == E_LIMIT and call(B=1 << 16, P=1 << 10) == E_LIMIT
        assert call(c=a.p["c"] + 4) == E_LIMIT and call(ws=a.p["ws"] + 4) == E_LIMIT and call(ws_bytes=a.ws_bytes - 1) == E_LIMIT
    for kw in (dict(eps=0.0), dict(eps=-1e-5), dict(momentum=-0.1), dict(momentum=1.5), dict(eps=float("nan"))):
        assert a.fwd(**kw) == E_SHAPE, kw
    assert a.bwd(dc=a.p["dc"] + 4) == E_LIMIT
    assert a.bwd(dc=0, dgamma=0, dbeta=0) == E_SHAPE
    assert a.fwd(y=a.p["y"] + 4, layout=0) == E_LIMIT and a.bwd(dy=a.p["dy"] + 4, layout=0) == E_LIMIT   # a channels-last y / dy is read as float4
    n4 = a.B * a.P * a.C * 4
    for kw in (dict(y=a.p["c"]), dict(y=a.p["c"] + n4 - 4), dict(stats=a.p["gamma"]), dict(rm=a.p["beta"]), dict(rv=a.p["rm"]), dict(ws=a.p["c"]),
               dict(stats=a.p["y"] + 16), dict(rm=a.p["stats"] + 4 * a.C)):
        assert a.fwd(**kw) == E_ALIAS, kw
    for kw in (dict(dc=a.p["dy"]), dict(dc=a.p["c"]), dict(dgamma=a.p["dbeta"]), dict(dbeta=a.p["stats"]), dict(dgamma=a.p["gamma"]), dict(ws=a.p["dy"]),
               dict(dgamma=a.p["dc"] + 64)):
        assert a.bwd(**kw) == E_ALIAS, kw
    # a form without a workspace takes NULL
    small = _Args(lib, B=2, P=25, C=32)
    assert small.ws_bytes == 0 and small.fwd(ws=0, c=0) == E_NULL and small.fwd(ws=0, y=small.p["c"]) == E_ALIAS


def test_the_wrappers_raise_pytorchs_words_for_one_value_per_channel():
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        BT._dims(torch.zeros(1, 32, 1, 1))
    with pytest.raises(Exception):
        BT.batchnorm_relu_train(torch.zeros(2, 32, 3, 3), torch.ones(32), torch.zeros(32))          # host tensors: no CPU fallback


# ----------------------------------------------------------------------------------------------------------------------------------- qualifies
def test_restates_on_and_off_each_condition():
    assert BT.restates(nn.BatchNorm2d(64))
    assert BT.restates(nn.BatchNorm2d(2048)) and BT.restates(nn.BatchNorm2d(32, track_running_stats=False))
    assert not BT.restates(nn.BatchNorm2d(64, affine=False))
    assert not BT.restates(nn.BatchNorm2d(64).double()) and not BT.restates(nn.BatchNorm2d(64).half())
    assert not BT.restates(nn.BatchNorm2d(64, momentum=None))
    assert not BT.restates(nn.BatchNorm2d(48)) and not BT.restates(nn.BatchNorm2d(2048 + 32))
    assert not BT.restates(nn.BatchNorm1d(64)) and not BT.restates(nn.GroupNorm(2, 64)) and not BT.restates(nn.Identity())
    half = nn.BatchNorm2d(64)
    half.track_running_stats = False                  # buffers kept but not tracked: F.batch_norm would then normalise by them; not restated
    assert not BT.restates(half)
    assert not BT.qualifies(nn.BatchNorm2d(64))       # on the host: the device condition is off
    assert not BT.qualifies(nn.BatchNorm2d(64), torch.zeros(2, 64, 3, 3))
