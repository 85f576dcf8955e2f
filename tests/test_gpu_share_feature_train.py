"""PreShareFeature's training path on the device (csrc/share_feature_train.hip, hdn_amd.PreShareFeatureTrain) against the float64 truth of
tests/share_feature_train_cases.py, per tensor: |got - truth| <= 4 e_ref + 1e-5 max|truth|, e_ref = the stock fp32 nn.Sequential's own error on the
CPU.  The fixtures keep every pre-activation away from the ReLU's kink (the host test asserts it)."""
import pytest
import torch

import share_feature_train_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRADS = tuple(n for n in C.TENSORS if n[0] == "g")


def check_bound(got, truth, ref, names, what):
    worst = {}
    for name in names:
        err, bound = C.excess(got, truth, ref, name)
        worst[name] = err / bound
        print(f"{what} {name}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (what, bad)


# ------------------------------------------------------------------------------------------------------------------------ 1. batch statistics
@pytest.mark.parametrize("shape", list(C.TRAIN_CASES))
def test_batch_statistics_every_tensor_within_the_bound(shape):
    fix, truth, ref = C.problem(shape, C.TRAIN_CASES[shape])
    got = C.run_module(fix, DEV)
    assert got["grad_fn"] and [got["nbt%d" % l] for l in (1, 2, 3)] == [1, 1, 1]
    check_bound(got, truth, ref, C.TENSORS, f"train {shape}")


@pytest.mark.parametrize("mode, shape", list(C.EPS3_CASES))
def test_three_different_eps_every_tensor_within_the_bound(mode, shape):
    """eps1, eps2, eps3 all different: a permutation between the layers (the three stats_finish launches, table_kernel's selection) moves every
    tensor far beyond the bound."""
    fix, truth, ref = C.problem(shape, C.EPS3_CASES[mode, shape], mode, C.EPS3)
    if mode == "train":
        got = C.run_module(fix, DEV, eps=C.EPS3)
        check_bound(got, truth, ref, C.TENSORS, f"three eps train {shape}")
    else:
        got = C.run_module(fix, DEV, train=False, running=C.running_of(fix), eps=C.EPS3)
        check_bound(got, truth, ref, ("y",) + GRADS, f"three eps frozen {shape}")
    assert got["grad_fn"]


@pytest.mark.parametrize("shape, momentum", [((3, 9, 11), 0.1), ((5, 13, 33), None), ((3, 9, 11), C.MOMENTA3)])
def test_running_buffers_after_two_calls(shape, momentum):
    fix = C.problem(shape, C.TRAIN_CASES[shape])[0]
    truth, ref = C.restatement(fix, momentum, calls=2), C.stock(fix, torch.float32, momentum=momentum, calls=2)
    got = C.run_module(fix, DEV, momentum=momentum, calls=2)
    assert [got["nbt%d" % l] for l in (1, 2, 3)] == [2, 2, 2]
    check_bound(got, truth, ref, C.TENSORS, f"two calls {shape} momentum {momentum}")


# ------------------------------------------------------------------------------------------------------------------------ 2. frozen statistics
@pytest.mark.parametrize("shape", list(C.FROZEN_CASES))
def test_frozen_statistics(shape):
    import hdn_amd
    fix, truth, ref = C.problem(shape, C.FROZEN_CASES[shape], "frozen")
    running = C.running_of(fix)
    got = C.run_module(fix, DEV, train=False, running=running)
    assert got["grad_fn"]
    check_bound(got, truth, ref, ("y",) + GRADS, f"frozen {shape}")
    for l, (lo, hi) in enumerate(C.LAYERS, start=1):     # buffers bit-unchanged
        assert torch.equal(got["rm%d" % l], running[0][lo:hi]) and torch.equal(got["rv%d" % l], running[1][lo:hi]) and got["nbt%d" % l] == 0
    # eval mode without grad is the fused kernel, same bits as before
    m = C.load_params(hdn_amd.PreShareFeatureTrain(), fix, running).to(DEV).eval()
    x = fix["x"].to(DEV)
    with torch.no_grad():
        y = m(x)
    for p in m.parameters():
        p.requires_grad_(False)
    y2 = m(x)
    folded = hdn_amd.fold_params(m.ShareFeature.state_dict(), prefix="").to(DEV)
    want = hdn_amd.share_feature.share_feature(x, folded)
    assert torch.equal(y, want) and torch.equal(y2, want) and y.grad_fn is None and y2.grad_fn is None


# ------------------------------------------------------------------------------------------------------------------------ 3. determinism
@pytest.mark.parametrize("shape", [(5, 13, 33), (1, 127, 127)])
def test_two_calls_are_bit_equal(shape):
    fix = C.problem(shape, C.TRAIN_CASES[shape])[0]
    a, b = C.run_module(fix, DEV), C.run_module(fix, DEV)
    for name in C.TENSORS:
        assert torch.equal(a[name], b[name]), name


# ------------------------------------------------------------------------------------------------------------------------ 4. requested outputs
def test_requested_output_combinations():
    shape = (3, 9, 11)
    fix = C.problem(shape, C.TRAIN_CASES[shape])[0]
    full = C.run_module(fix, DEV)
    no_x = C.run_module(fix, DEV, x_grad=False)
    assert "gx" not in no_x
    for name in GRADS[1:]:
        assert torch.equal(no_x[name], full[name]), name
    no_p = C.run_module(fix, DEV, p_grad=False)
    assert torch.equal(no_p["gx"], full["gx"]) and not any(n in no_p for n in GRADS[1:])
    none = C.run_module(fix, DEV, x_grad=False, p_grad=False)
    assert not none["grad_fn"] and torch.equal(none["y"], full["y"])
    for l in (1, 2, 3):
        assert none["nbt%d" % l] == 1 and torch.equal(none["rm%d" % l], full["rm%d" % l]) and torch.equal(none["rv%d" % l], full["rv%d" % l])


def test_double_backward_raises():
    import hdn_amd
    fix = C.problem((2, 5, 7), 0)[0]
    m = C.load_params(hdn_amd.PreShareFeatureTrain(), fix).to(DEV).train()
    x = fix["x"].to(DEV).requires_grad_(True)
    (gx,) = torch.autograd.grad(m(x).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


# ------------------------------------------------------------------------------------------------------------------------ 5. memory discipline
@pytest.mark.parametrize("offsets", C.OFFSETS)
@pytest.mark.parametrize("frozen", [False, True])
def test_memory_discipline_through_the_c_abi(offsets, frozen):
    shape = (3, 9, 11)
    fix, truth, ref = C.problem(shape, 0, "frozen" if frozen else "train")
    res, clean = C.run_raw(fix, DEV, offsets, frozen=frozen)
    assert clean, "bytes outside an output were written"
    for k in ("y", "saved", "stats", "gx", "gp"):
        assert not torch.isnan(res[k]).any(), f"{k} not fully overwritten"
    got = dict(C.split_params(res["gp"]), y=res["y"], gx=res["gx"])
    check_bound(got, truth, ref, ("y",) + GRADS, f"raw {offsets} frozen {frozen}")
    # the unaligned call has the bits of the aligned one
    if offsets != C.OFFSETS[0]:
        base, _ = C.run_raw(fix, DEV, C.OFFSETS[0], frozen=frozen)
        for k in ("y", "saved", "stats", "gx", "gp"):
            assert torch.equal(base[k], res[k]), k
    for need_x, need_params in ((True, False), (False, True)):
        part, clean = C.run_raw(fix, DEV, offsets, frozen=frozen, need_x=need_x, need_params=need_params)
        assert clean
        if need_x:
            assert part["gp"] is None and torch.equal(part["gx"], res["gx"])
        else:
            assert part["gx"] is None and torch.equal(part["gp"], res["gp"])


# ------------------------------------------------------------------------------------------------------------------------ 6. sample coupling
def test_samples_couple_through_the_statistics_only():
    shape = (3, 9, 11)
    fix = C.problem(shape, 0, "frozen")[0]
    one = {k: (v[:1].clone() if k in ("x", "g") else v) for k, v in fix.items()}
    running = C.running_of(fix)
    # grad_x only: the parameter gradients are sums over the batch in either mode
    fb, f1 = C.run_module(fix, DEV, train=False, running=running, p_grad=False), C.run_module(one, DEV, train=False, running=running, p_grad=False)
    assert torch.equal(fb["y"][:1], f1["y"]) and torch.equal(fb["gx"][:1], f1["gx"])
    tb, t1 = C.run_module(fix, DEV, p_grad=False), C.run_module(one, DEV, p_grad=False)
    assert not torch.equal(tb["y"][:1], t1["y"]) and not torch.equal(tb["gx"][:1], t1["gx"])
    assert not torch.equal(tb["y"], fb["y"])


# ------------------------------------------------------------------------------------------------------------------------ 7. the step's pattern
def test_three_calls_in_one_graph_under_the_triplet_loss():
    import hdn_amd
    shape, off = C.STEP_CASE
    fix, truth, ref = C.step_problem(shape, off)
    m = C.load_params(hdn_amd.PreShareFeatureTrain(), fix).to(DEV).train()
    got = C.step_run(m, fix, torch.float32, DEV)
    assert [got["nbt%d" % l] for l in (1, 2, 3)] == [3, 3, 3]
    check_bound(got, truth, ref, C.TENSORS + ("loss",), "step")


# ------------------------------------------------------------------------------------------------------------------------ 8. one value per channel
def test_one_value_per_channel_raises_pytorchs_own_error():
    import hdn_amd
    m = hdn_amd.PreShareFeatureTrain().to(DEV).train()
    x = torch.randn(1, 1, 1, 1, device=DEV)
    assert m._hip_train_mode(x) == 0
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        m(x)          # through the stock layers (mode 0 above): none of the train kernels is launched
