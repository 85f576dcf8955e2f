"""CPU tests of PreShareFeature's training path: the float64 truth, the fixtures' ReLU margins, the C ABI's argument checks (no device is touched),
and the routing of the module and of install(train=True).  The device tests are tests/test_gpu_share_feature_train.py."""
import copy
import ctypes
import types

import pytest
import torch

import share_feature_train_cases as C
import hdn_amd
from hdn_amd import _lib, install as hinstall, share_feature as SF


def rel(a, b):
    b = b.double()
    return float((a.double().reshape(b.shape) - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("shape, momentum, calls", [((3, 9, 11), 0.1, 1), ((2, 5, 7), 0.1, 2), ((1, 2, 3), None, 2), ((2, 17, 130), 0.3, 1)])
def test_restatement_is_float64_autograd_through_the_stock_layers(shape, momentum, calls):
    fix = C.draw(*shape, C.SEED)
    truth, auto = C.restatement(fix, momentum, calls), C.stock(fix, torch.float64, momentum=momentum, calls=calls)
    for name in C.TENSORS:
        assert rel(truth[name], auto[name]) <= 1e-12, name
    for zt, za in zip(truth["z"], auto["z"]):
        assert rel(zt, za) <= 1e-12
    assert [truth["nbt%d" % l] for l in (1, 2, 3)] == [auto["nbt%d" % l] for l in (1, 2, 3)] == [calls] * 3


@pytest.mark.parametrize("shape", list(C.TRAIN_CASES))
def test_train_fixtures_keep_the_relu_margin_and_the_reference_its_own_bound(shape):
    off = C.TRAIN_CASES[shape]
    assert C.first_offset(shape) == off, "the committed offset is the first that satisfies the margin rule"
    assert shape[0] * shape[1] * shape[2] <= 110_000
    _, truth, ref = C.problem(shape, off)
    assert C.margin_ok(truth["z"], ref["z"])
    for name in C.TENSORS:
        err, bound = C.excess(ref, truth, ref, name)
        assert err <= bound, name


@pytest.mark.parametrize("mode, shape", list(C.EPS3_CASES))
def test_three_eps_fixtures_keep_the_relu_margin_and_feel_a_permutation(mode, shape):
    off = C.EPS3_CASES[mode, shape]
    assert len(set(C.EPS3)) == 3 and C.first_offset(shape, mode, C.EPS3) == off
    fix, truth, ref = C.problem(shape, off, mode, C.EPS3)
    assert C.margin_ok(truth["z"], ref["z"])
    swapped = C.problem(shape, off, mode, (C.EPS3[1], C.EPS3[2], C.EPS3[0]))[1]        # what a kernel that permutes the three eps computes
    for name in ("y", "gx", "gw1", "gw2", "gw3"):
        err, bound = C.excess(swapped, truth, ref, name)
        assert err > 10 * bound, name


def test_restatement_with_three_momenta_is_float64_autograd():
    assert None in C.MOMENTA3 and len(set(C.MOMENTA3)) == 3
    fix = C.draw(3, 9, 11, C.SEED)
    truth, auto = C.restatement(fix, C.MOMENTA3, 2), C.stock(fix, torch.float64, momentum=C.MOMENTA3, calls=2)
    for name in C.TENSORS:
        assert rel(truth[name], auto[name]) <= 1e-12, name


@pytest.mark.parametrize("shape", list(C.FROZEN_CASES))
def test_frozen_fixtures_keep_the_relu_margin(shape):
    assert C.first_offset(shape, "frozen") == C.FROZEN_CASES[shape]
    _, truth, ref = C.problem(shape, C.FROZEN_CASES[shape], "frozen")
    assert C.margin_ok(truth["z"], ref["z"])
    for l in (1, 2, 3):       # eval mode leaves the buffers alone
        assert truth["nbt%d" % l] == 0


def test_step_fixture_keeps_the_margins_in_all_three_calls():
    shape, off = C.STEP_CASE
    assert C.first_offset(shape, "step") == off
    _, truth, ref = C.step_problem(shape, off)
    assert len(truth["z"]) == 9 and C.step_margin_ok(truth, ref)
    assert all(truth["nbt%d" % l] == 3 for l in (1, 2, 3))


def test_case_list_sits_on_both_sides_of_every_launch_boundary():
    """One launch form (no form query): the boundaries are the thread's pixel stride (256), the workgroup's pixels (1024), the weight finish's stride
    (64 workgroups) and the statistics finish's (256 workgroups)."""
    hw = {s[1] * s[2] for s in C.TRAIN_CASES if s[0] == 1}
    assert {256, 257, 1024, 1025} <= hw
    wg = {C.workgroups(*s) for s in C.TRAIN_CASES}
    assert {1, 2, 64, 65, 256, 257} <= wg
    assert any(C.workgroups(*s) > s[0] for s in C.TRAIN_CASES), "more than one workgroup per image"
    assert (2, 127, 127) not in C.TRAIN_CASES


def test_size_queries():
    lib = _lib.load()
    for q in (lib.hdn_share_feature_train_workspace_bytes, lib.hdn_share_feature_train_saved_bytes):
        base = q(2, 17, 33)
        assert base > 0
        assert q(3, 17, 33) > base and q(2, 18, 33) > base and q(2, 17, 64) > base
        for bad in ((0, 5, 5), (1, 0, 5), (1, 5, 0), (-1, 5, 5)):
            assert q(*bad) == -2
        assert q(13, 4096, 4096) == -3        # 13 N beyond 2^31 - 1
    assert lib.hdn_share_feature_train_saved_bytes(2, 5, 7) == 13 * 70 * 4
    assert lib.hdn_share_feature_train_workspace_bytes(2, 5, 7) % 16 == 0


def _ptrs(n, stride=1 << 20):
    return [ctypes.c_void_p(4096 + i * stride) for i in range(n)]


def test_forward_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    f = lib.hdn_share_feature_train_fwd_f32
    B, H, W = 2, 5, 7
    need = lib.hdn_share_feature_train_workspace_bytes(B, H, W)
    img, w1, w2, w3, gamma, bias, mv, out, saved, stats, ws = _ptrs(11)

    def call(img=img, w1=w1, w2=w2, w3=w3, gamma=gamma, bias=bias, mv=None, mode=0, out=out, saved=saved, stats=stats, ws=ws, nbytes=need, B=B, H=H, W=W):
        return f(img, w1, w2, w3, gamma, bias, mv, 1e-5, 1e-5, 1e-5, mode, out, saved, stats, ws, nbytes, B, H, W, None)

    for name in ("img", "w1", "w2", "w3", "gamma", "bias", "out", "saved", "stats", "ws"):
        assert call(**{name: None}) == -1, name
    assert call(mode=1, mv=None) == -1
    assert call(B=0) == -2 and call(H=0) == -2 and call(W=-3) == -2 and call(mode=2) == -2
    assert call(B=1, H=1, W=1, nbytes=1 << 30) == -2                    # one value per channel has no batch statistics
    assert call(B=13, H=4096, W=4096, nbytes=1 << 62) == -3
    assert call(nbytes=need - 1) == -3
    assert call(ws=ctypes.c_void_p(ws.value + 4)) == -3                 # the workspace is 16-byte aligned
    assert call(out=img) == -4 and call(saved=img) == -4 and call(stats=gamma) == -4 and call(ws=w2) == -4
    assert call(out=ctypes.c_void_p(saved.value + 4 * 13 * B * H * W - 4)) == -4     # the last float of saved
    assert call(mode=1, mv=mv, stats=ctypes.c_void_p(mv.value + 100)) == -4


def test_backward_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    f = lib.hdn_share_feature_bwd_f32
    B, H, W = 2, 5, 7
    need = lib.hdn_share_feature_train_workspace_bytes(B, H, W)
    img, w1, w2, w3, gamma, bias, saved, stats, gout, gimg, gpar, ws = _ptrs(12)

    def call(img=img, w1=w1, w2=w2, w3=w3, gamma=gamma, bias=bias, saved=saved, stats=stats, gout=gout, gimg=gimg, gpar=gpar, ws=ws, nbytes=need,
             mode=0, B=B, H=H, W=W):
        return f(img, w1, w2, w3, gamma, bias, saved, stats, gout, gimg, gpar, ws, nbytes, mode, B, H, W, None)

    for name in ("img", "w1", "w2", "w3", "gamma", "bias", "saved", "stats", "gout", "ws"):
        assert call(**{name: None}) == -1, name
    assert call(gimg=None, gpar=None) == -2                              # no gradient asked for
    assert call(B=0) == -2 and call(H=-1) == -2 and call(W=0) == -2 and call(mode=-1) == -2
    assert call(B=1, H=1, W=1) == -2
    assert call(B=13, H=4096, W=4096, nbytes=1 << 62) == -3
    assert call(nbytes=need - 1) == -3 and call(ws=ctypes.c_void_p(ws.value + 8)) == -3
    assert call(gimg=img) == -4 and call(gimg=gout) == -4 and call(gpar=w2) == -4 and call(gpar=stats) == -4 and call(ws=saved) == -4
    assert call(gimg=ctypes.c_void_p(gpar.value + 4 * 421)) == -4        # the last float of grad_params
    assert call(gimg=None, gpar=ctypes.c_void_p(saved.value + 16)) == -4


# ------------------------------------------------------------------------------------------------------------------------ routing
class _Spy(torch.nn.Module):
    """Counts the calls that reach the stock layers."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.calls = inner, 0

    def forward(self, x):
        self.calls += 1
        return self.inner(x)


def _spied(module):
    spy = _Spy(module.ShareFeature)
    module.__dict__["_modules"]["ShareFeature"] = spy      # forward() resolves self.ShareFeature here; the parameter names are not what is tested
    return spy


def test_classes_and_attribute():
    a, b = hdn_amd.PreShareFeature(), hdn_amd.PreShareFeatureTrain()
    assert a.hip_train is False and b.hip_train is True and isinstance(b, hdn_amd.PreShareFeature)
    assert list(a.state_dict()) == list(b.state_dict())
    assert "hip_train" in b.__dict__                                   # a plain attribute
    c = copy.deepcopy(b)
    assert c.hip_train is True and c.double().ShareFeature[0].weight.dtype == torch.float64
    b.load_state_dict(a.state_dict())


def test_default_module_in_train_mode_runs_the_stock_layers():
    m = hdn_amd.PreShareFeature().train()
    spy = _spied(m)
    y = m(torch.randn(2, 1, 5, 7))
    assert spy.calls == 1 and y.grad_fn is not None


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_hip_train_with_a_cpu_or_float64_tensor_runs_the_stock_layers(dtype):
    m = hdn_amd.PreShareFeatureTrain().to(dtype).train()
    x = torch.randn(2, 1, 5, 7, dtype=dtype)
    assert m._hip_train_mode(x) == 0
    spy = _spied(m)
    y = m(x)
    assert spy.calls == 1 and y.dtype == dtype and y.grad_fn is not None


def test_one_value_per_channel_raises_pytorchs_own_error():
    m = hdn_amd.PreShareFeatureTrain().train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        m(torch.randn(1, 1, 1, 1))


def test_install_train_binds_what_the_measurement_says():
    pre = types.SimpleNamespace(head={"PreShareFeature": "the reference's"})
    mods = {hinstall._DLT + ".preprocess": pre}
    assert isinstance(hinstall.SHARE_FEATURE_TRAIN_BOUND, bool)
    try:
        hinstall.install(modules=mods, train=True)
        want = hdn_amd.PreShareFeatureTrain if hinstall.SHARE_FEATURE_TRAIN_BOUND else hdn_amd.PreShareFeature
        assert pre.head["PreShareFeature"] is want
        hinstall.uninstall()
        assert pre.head["PreShareFeature"] == "the reference's"
        hinstall.install(modules=mods)
        assert pre.head["PreShareFeature"] is hdn_amd.PreShareFeature
    finally:
        hinstall.uninstall()
    assert pre.head["PreShareFeature"] == "the reference's"


def test_function_signature_is_the_ten_differentiable_inputs_first():
    import inspect
    names = list(inspect.signature(SF._ShareFeatureTrain.forward).parameters)
    assert names[1:11] == ["x", "w1", "g1", "b1", "w2", "g2", "b2", "w3", "g3", "b3"]
