"""Host side of tests/test_gpu_triplet.py: the two entry points of csrc/triplet_loss.hip exist in the library, the header and the binding (ABI still
10), their validation codes come in the order of the other entry points (made-up addresses: nothing is launched), the numpy restatement of
tests/triplet_cases.py equals float64 autograd, PyTorch's own fp32 loss lies inside the bound on every case, every mutation breaks it, the excluded
rows stay under the cap, and hdn_amd.triplet / install(train=True) / HomoModelBuilder.training_forward route as documented.  No GPU, no kernel."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import triplet_cases as TC

E_NULL, E_SHAPE, E_LIMIT, E_ALIAS = -1, -2, -3, -4
NEW = {"hdn_triplet_l1_f32": 12, "hdn_triplet_l1_bwd_f32": 15}
SITES = ("hdn.models.model_builder_e2e_unconstrained_v2", "homo_estimator.Deep_homography.Oneline_DLTv1.models.homo_model_builder")


def _lib():
    from hdn_amd import _lib as L
    return L


def test_symbols_in_the_library_the_header_and_the_binding():
    L = _lib()
    lib = L.load()
    assert lib.hdn_abi_version() == L.ABI_VERSION == 10
    with open(os.path.join(TC.ROOT, "include", "hdn_hip.h")) as f:
        header = f.read()
    assert "#define HDN_ABI_VERSION 10" in header
    for name, nargs in NEW.items():
        assert hasattr(lib, name) and name in L.SIGNATURES
        res, args = L.SIGNATURES[name]
        assert len(args) == nargs and res is ctypes.c_int
        decl = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == nargs
        assert args[-1] is ctypes.c_void_p and "void* stream" in decl.group(1).split(",")[-1]
        assert args[-3] is ctypes.c_float and args[-2] is ctypes.c_float and "float margin" in decl.group(1) and "float eps" in decl.group(1)
    for text in ("d_ap = sum_j |(a_j - p_j) + eps|", "d_an = sum_j |(a_j - n_j) + eps|", "v = (margin + d_ap) - d_an", "loss = v if v >= 0, 0 if v < 0",
                 "A NaN v", "grad_a = g (s_ap - s_an)", "grad_p = -g s_ap", "grad_n = g s_an", "sgn(0) = 0", "active iff v >= 0", "no atomics",
                 "outside [0, N)"):
        assert text in header, text
    import hdn_amd
    assert hdn_amd.triplet_l1 is hdn_amd.triplet.triplet_l1 and hdn_amd.triplet_l1_backward is hdn_amd.triplet.triplet_l1_backward
    assert hdn_amd.TripletMarginLossL1 is hdn_amd.triplet.TripletMarginLossL1
    import __graft_entry__ as G
    assert "triplet_loss.hip" in G.HIP_SOURCES


def test_validation_codes_in_order():
    """Made-up host addresses: every call here is refused before a launch.  NULL -> -1, then shape (no gradient asked for included) -> -2, then the
    limits -> -3, then the aliases -> -4."""
    lib = _lib().load()
    a = [ctypes.c_void_p(v << 34) for v in range(1, 12)]
    m, e = 1.0, 1e-6
    # ---- forward: anchor, positive, negative, ids, loss | N R D n_ids | margin eps
    f = lib.hdn_triplet_l1_f32
    ok = (3, 5, 7, 0)
    for i in (0, 1, 2, 4):
        ptrs = [a[0], a[1], a[2], None, a[4]]
        ptrs[i] = None
        assert f(*ptrs, *ok, m, e, None) == E_NULL and f(*ptrs, 0, 5, 7, 0, m, e, None) == E_NULL, i            # NULL before shape
    for k in range(3):
        dims = list(ok)
        dims[k] = 0
        assert f(a[0], a[1], a[2], None, a[4], *dims, m, e, None) == E_SHAPE, dims
        assert f(a[0], a[1], a[2], None, a[0], *dims, m, e, None) == E_SHAPE, dims                              # shape before alias
    assert f(a[0], a[1], a[2], a[3], a[4], 3, 5, 7, 0, m, e, None) == E_SHAPE                                    # ids without entries
    assert f(a[0], a[1], a[2], a[3], a[4], 3, 5, 7, -1, m, e, None) == E_SHAPE
    assert f(a[0], a[1], a[2], None, a[4], 1 << 16, 1 << 15, 7, 0, m, e, None) == E_LIMIT                        # N R > 2^30
    assert f(a[0], a[1], a[2], a[3], a[4], 3, 1 << 15, 7, 1 << 16, m, e, None) == E_LIMIT                        # n_ids R > 2^30
    assert f(a[0], a[1], a[2], None, a[4], 3, 5, (1 << 20) + 1, 0, m, e, None) == E_LIMIT
    assert f(a[0], a[1], a[2], None, a[0], 3, 5, (1 << 20) + 1, 0, m, e, None) == E_LIMIT                        # limit before alias
    for out in (a[0], a[1], a[2]):
        assert f(a[0], a[1], a[2], None, out, *ok, m, e, None) == E_ALIAS
    assert f(a[0], a[1], a[2], a[3], a[3], 3, 5, 7, 2, m, e, None) == E_ALIAS                                    # loss on ids
    assert f(a[0], a[1], a[2], None, ctypes.c_void_p((1 << 34) + 3 * 5 * 7 * 4 - 4), *ok, m, e, None) == E_ALIAS  # the last float of anchor
    # ---- backward: anchor, positive, negative, ids, grad_loss | ga gp gn | N R D n_ids | margin eps
    f = lib.hdn_triplet_l1_bwd_f32
    ins = [a[0], a[1], a[2], None, a[4]]
    for i in (0, 1, 2, 4):
        bad = list(ins)
        bad[i] = None
        assert f(*bad, a[5], a[6], a[7], *ok, m, e, None) == E_NULL, i
        assert f(*bad, None, None, None, 0, 5, 7, 0, m, e, None) == E_NULL, i                                    # NULL before shape
    assert f(*ins, None, None, None, *ok, m, e, None) == E_SHAPE                                                 # no gradient asked for
    for k in range(3):
        dims = list(ok)
        dims[k] = 0
        assert f(*ins, a[5], a[6], a[7], *dims, m, e, None) == E_SHAPE, dims
        assert f(*ins, a[0], a[6], a[7], *dims, m, e, None) == E_SHAPE, dims                                     # ... although an output aliases
    assert f(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], 3, 5, 7, 0, m, e, None) == E_SHAPE
    assert f(*ins, a[5], a[6], a[7], 1 << 16, 1 << 15, 7, 0, m, e, None) == E_LIMIT
    assert f(*ins, a[0], a[6], a[7], 3, 5, (1 << 20) + 1, 0, m, e, None) == E_LIMIT                              # limit before alias
    for ga, gp, gn in ((a[0], a[6], a[7]), (a[5], a[1], a[7]), (a[5], a[6], a[2]), (a[4], None, None), (None, a[4], None), (None, None, a[4]),
                       (a[5], a[5], None), (a[5], None, a[5]), (None, a[6], a[6]), (None, None, a[0])):
        assert f(*ins, ga, gp, gn, *ok, m, e, None) == E_ALIAS, (ga, gp, gn)
    assert f(a[0], a[1], a[2], a[3], a[4], None, a[3], None, 3, 5, 7, 2, m, e, None) == E_ALIAS                  # a gradient on ids
    # the three inputs may alias each other: refused for no other reason than the one asked about (here: no gradient)
    assert f(a[0], a[0], a[0], None, a[4], None, None, None, *ok, m, e, None) == E_SHAPE


# ------------------------------------------------------------------------------------------------------------------------ reference, bound, mutations
@pytest.mark.parametrize("name", TC.NAMES)
def test_restatement_equals_float64_autograd_and_fp32_pytorch_is_inside_tol(name):
    c = TC.CASES[name]
    a, p, n = c.gathered()
    loss64, ga, gp, gn = TC.autograd64(a, p, n, c.g, c.margin, c.eps)
    r = TC.closed(a.numpy(), p.numpy(), n.numpy(), c.margin, c.eps, g=c.g.numpy())
    scale = float(np.abs(r["d_ap"]).max() + np.abs(r["d_an"]).max() + abs(c.margin))
    assert float(np.abs(r["loss"] - loss64.numpy()).max()) <= 1e-13 * scale
    t = c.truth()
    near = (t["v64"].abs() <= 1e-13 * scale).unsqueeze(-1)                                   # (float64 against float64: only a v at rounding distance of 0 may differ)
    for got, want in ((r["ga"], ga), (r["gp"], gp), (r["gn"], gn)):
        assert bool(((torch.from_numpy(got) == want) | near).all())
    # PyTorch's own fp32 on this CPU: inside tol on every row of every case
    loss32 = TC.torch_loss(a, p, n, c.margin, c.eps)
    err = (loss32.double() - loss64).abs()
    worst = float((err / t["tol"]).max())
    print(f"TRIPLET {name}: PyTorch fp32 worst |err| / tol = {worst:.3f}; rows left out of the gradient comparison: {t['excluded']} of {loss64.numel()}")
    assert bool((err <= t["tol"]).all()), worst
    # the rows left out of the gradient comparison stay under the cap (zero with these seeds on N(0,1) data)
    assert t["excluded"] <= TC.EXCLUDED_CAP * loss64.numel(), t["excluded"]
    if c.exact:                                                                              # order-independent rows: fp32 PyTorch is the fp32 restatement bit for bit
        assert torch.equal(loss32, t["loss"])


@pytest.mark.parametrize("variant", sorted(TC.MUTATIONS))
def test_mutations_break_the_bound(variant):
    """Each mistake, restated in numpy, leaves tol on every row of its fixture, while the unmutated restatement at the same precision stays inside."""
    c = TC.CASES[TC.MUTATIONS[variant]]
    a, p, n = (x.numpy() for x in c.gathered())
    t = c.truth()
    dtypes = (np.float32,) if variant == "order" else (np.float32, np.float64)               # a reassociation is invisible in float64
    for dt in dtypes:
        good = TC.closed(a, p, n, c.margin, dt(c.eps), dtype=dt)["loss"].astype(np.float64)
        bad = TC.closed(a, p, n, c.margin, dt(c.eps), variant=variant, dtype=dt)["loss"].astype(np.float64)
        want, tl = t["loss"].double().numpy(), t["tol"].numpy()
        assert bool((np.abs(good - want) <= tl).all()), (variant, dt)
        assert bool((np.abs(bad - want) > tl).all()), (variant, dt, np.abs(bad - want) / tl)
        assert bool((want > tl).all())                                                        # the fixture's rows are active: the loss feels every term


def test_boundary_rows_are_what_the_issue_states():
    for D in TC.BOUNDARY_DS:
        c = TC.CASES[f"boundary_D{D}"]
        t = c.truth()
        loss = t["loss"]
        assert bool((loss[:, 0] == 0).all()) and bool((loss[:, 1] > 0).all()) and bool((loss[:, 2] == 0).all())
        v32 = TC.closed(c.a.numpy(), c.p.numpy(), c.n.numpy(), c.margin, np.float32(c.eps), dtype=np.float32)["v"]
        assert bool((v32[:, 0] == 0).all()) and bool((v32[:, 2] < 0).all())
        for got, want in zip(t["grads"], TC.expected_boundary(c, D)):
            assert torch.equal(got, want)
        # ... and PyTorch's fp32 autograd on this CPU agrees, at the boundary too (clamp_min passes the gradient at exactly 0)
        _, ga, gp, gn = TC.autograd64(c.a, c.p, c.n, c.g, c.margin, c.eps, torch.float32)
        for got, want in zip((ga, gp, gn), t["grads"]):
            assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------------------------------ Python layer
def test_no_fallback_and_input_rules():
    import hdn_amd
    from hdn_amd import _lib
    a, p, n = torch.zeros(2, 3, 7), torch.zeros(2, 3, 7), torch.zeros(2, 3, 7)
    with pytest.raises(_lib.HdnHipError):                                                     # a CPU tensor: no fallback
        hdn_amd.triplet_l1(a, p, n)
    ag = a.clone().requires_grad_(True)
    for args in ((ag, p, n), (a, ag, n), (a, p, ag)):
        with pytest.raises(RuntimeError, match="inference-only.*uninstall"):                   # refused before any device check
            hdn_amd.triplet_l1(*args)
        with torch.no_grad(), pytest.raises(_lib.HdnHipError):                                # not recording: goes on to the device check
            hdn_amd.triplet_l1(*args)
        with pytest.raises(_lib.HdnHipError):                                                 # differentiable: no longer refuses, reaches the device check
            hdn_amd.triplet_l1(*args, differentiable=True)
        with pytest.raises(_lib.HdnHipError):
            hdn_amd.TripletMarginLossL1()(*args)
    for bad in (torch.zeros(2, 3, 8), torch.zeros(2, 1, 7), torch.zeros(3, 7), torch.zeros(1, 3, 7)):    # no broadcasting
        with pytest.raises(ValueError):
            hdn_amd.triplet_l1(a, bad, n)
        with pytest.raises(ValueError):
            hdn_amd.triplet_l1(a, p, bad, differentiable=True)
    with pytest.raises(ValueError):
        hdn_amd.triplet_l1(a, p, n, ids=torch.tensor([0.0]))                                   # ids are int64
    with pytest.raises(ValueError):
        hdn_amd.triplet_l1_backward(a, p, n, torch.zeros(2, 3), need_anchor=False, need_positive=False, need_negative=False)
    with pytest.raises(ValueError):
        hdn_amd.triplet_l1_backward(a, p, n, torch.zeros(2, 4))
    with pytest.raises(_lib.HdnHipError):
        hdn_amd.triplet_l1_backward(a, p, n, torch.zeros(2, 3))
    m = hdn_amd.TripletMarginLossL1(margin=0.5, eps=1e-5)
    assert (m.margin, m.eps) == (0.5, 1e-5) and not list(m.parameters())


def _site(loss):
    mods = {}
    for name in SITES:
        mods[name] = types.ModuleType(name)
        if loss is not None:
            mods[name].triplet_loss = loss
    return mods


def test_install_train_routes_by_the_constant_and_uninstall_restores(monkeypatch):
    import hdn_amd
    import hdn_amd.install as hinstall
    assert isinstance(hinstall.TRIPLET_TRAIN_BOUND, bool)
    orig = nn.TripletMarginLoss(margin=1.0, p=1, reduce=False, size_average=False)          # the reference's own line
    assert orig.reduction == "none"
    default = hinstall.install(modules=_site(None))
    hinstall.uninstall()
    assert default and not any(attr == "triplet_loss" for _, attr in default)
    for bound in (True, False):
        monkeypatch.setattr(hinstall, "TRIPLET_TRAIN_BOUND", bound)
        for train in (True, False):
            mods = _site(orig)
            done = hinstall.install(modules=mods, train=train) if train else hinstall.install(modules=mods)
            try:
                for name in SITES:
                    if train and bound:
                        got = mods[name].triplet_loss
                        assert isinstance(got, hdn_amd.TripletMarginLossL1) and (got.margin, got.eps) == (1.0, orig.eps) and (name, "triplet_loss") in done
                    else:
                        assert mods[name].triplet_loss is orig and (name, "triplet_loss") not in done
            finally:
                hinstall.uninstall()
            assert all(mods[name].triplet_loss is orig for name in SITES)                     # the identical object is back
    monkeypatch.setattr(hinstall, "TRIPLET_TRAIN_BOUND", True)
    # a loss the kernel does not restate is left alone; so is a module without the attribute, which must not gain one
    for other in (nn.TripletMarginLoss(margin=1.0, p=2, reduction="none"), nn.TripletMarginLoss(margin=1.0, p=1, swap=True, reduction="none"),
                  nn.TripletMarginLoss(margin=1.0, p=1), nn.L1Loss(reduction="none"), None):
        mods = _site(other)
        try:
            done = hinstall.install(modules=mods, train=True)
            for name in SITES:
                assert (name, "triplet_loss") not in done
                assert (mods[name].triplet_loss is other) if other is not None else not hasattr(mods[name], "triplet_loss")
        finally:
            hinstall.uninstall()
        assert all(not hasattr(mods[name], "triplet_loss") for name in SITES) if other is None else True
    # margin and eps travel
    mods = _site(nn.TripletMarginLoss(margin=0.25, p=1, eps=1e-4, reduction="none"))
    try:
        hinstall.install(modules=mods, train=True)
        assert all((mods[name].triplet_loss.margin, mods[name].triplet_loss.eps) == (0.25, 1e-4) for name in SITES)
    finally:
        hinstall.uninstall()
    # the default install is what it was: the sites are no part of REBINDINGS
    for bound in (True, False):
        monkeypatch.setattr(hinstall, "TRIPLET_TRAIN_BOUND", bound)
        assert hinstall.install(modules=_site(orig)) == default
        hinstall.uninstall()
    assert not any(attr == "triplet_loss" for _, attr, _ in hinstall.REBINDINGS)


def test_the_committed_constant_is_what_the_measurement_says():
    import hdn_amd.install as hinstall
    with open(os.path.join(TC.ROOT, "profiles", "triplet_train.json")) as f:
        res = json.load(f)
    assert isinstance(res["ahead"], bool) and hinstall.TRIPLET_TRAIN_BOUND is res["ahead"]
    spread = max(res[s]["max"] - res[s]["min"] for s in ("hip", "library"))
    assert res["ahead"] == (res["library"]["ms_per_step"] - res["hip"]["ms_per_step"] > spread)
    assert res["rounds"] >= 5 and res["window_seconds"] >= 0.5 and "hip_fused_ids" in res


def test_training_forward_refuses_a_share_feature_that_detaches():
    import hdn_amd
    net = hdn_amd.HomoModelBuilder().eval()
    assert callable(net.training_forward) and net.ShareFeature.hip_train is False
    with pytest.raises(RuntimeError, match="ShareFeature.*eval.*hip_train"):                  # before any device work: the data is never looked at
        net.training_forward({})
    net.ShareFeature.hip_train = True
    with pytest.raises(KeyError):                                                             # past the refusal: now the data is looked at
        net.training_forward({})
    net.ShareFeature.hip_train = False
    net.train()
    with pytest.raises(KeyError):
        net.training_forward({})
