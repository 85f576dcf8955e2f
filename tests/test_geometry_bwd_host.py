"""Host side of tests/test_gpu_geometry_bwd.py: the entry points of csrc/geometry_bwd.hip exist in the library, the header and the binding (ABI still 10),
their validation codes are provoked with made-up addresses (nothing is launched), the closed forms of tests/geometry_bwd_cases.py equal float64 autograd
through the restatements, the restated transformer's fp32 forward is the oracle's bit for bit, the exact fixtures are exact in fp32, the bound fixtures
keep their coordinate margin and the reference formulations' own fp32 ratios r_ref are measured and printed, and install(train=True) binds
STN_PolarTrain on stand-in modules.  No GPU, no kernel."""
import ctypes
import os
import re
import types

import pytest
import torch

import geometry_bwd_cases as GC

E_NULL, E_SHAPE, E_LIMIT, E_ALIAS = -1, -2, -3, -4
NEW = {"hdn_logpolar_sample_bwd_f32": 16, "hdn_dlt_solve_bwd_f32": 7, "hdn_warp_bwd_f32": 12, "hdn_logpolar_sample_bwd_workspace_bytes": 2,
       "hdn_warp_bwd_workspace_bytes": 3}


def _lib():
    from hdn_amd import _lib as L
    return L


def test_symbols_in_the_library_the_header_and_the_binding():
    L = _lib()
    lib = L.load()
    assert lib.hdn_abi_version() == L.ABI_VERSION == 10
    with open(os.path.join(GC.ROOT, "include", "hdn_hip.h")) as f:
        header = f.read()
    assert "#define HDN_ABI_VERSION 10" in header
    for name, nargs in NEW.items():
        assert hasattr(lib, name) and name in L.SIGNATURES
        res, args = L.SIGNATURES[name]
        assert len(args) == nargs and res is (ctypes.c_longlong if name.endswith("_bytes") else ctypes.c_int)
        decl = re.search(r"(?:int|long long) %s\(([^;]*)\);" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == nargs
        if not name.endswith("_bytes"):
            assert args[-1] is ctypes.c_void_p and "void* stream" in decl.group(1).split(",")[-1]
    for text in ("d out / d px = s (I_ne - I_nw) + n (I_se - I_sw)", "(W/2) / (H//2)", "clip_coordinates_set_grad", "A^T lambda = grad_H[0:8]",
                 "grad_A = -lambda h^T", "d out / d x = (Ic - Ia)(y1 - y) + (Id - Ib)(y - y0)", "NOT\n *     bit-reproducible"):
        assert text in header, text
    import hdn_amd
    assert hdn_amd.dlt_solve_backward is hdn_amd.homography.dlt_solve_backward
    assert hdn_amd.transformer_backward is hdn_amd.homography.transformer_backward
    assert hdn_amd.logpolar_sample_backward is hdn_amd.logpolar.logpolar_sample_backward
    assert issubclass(hdn_amd.STN_PolarTrain, hdn_amd.STN_Polar)
    import __graft_entry__ as G
    assert "geometry_bwd.hip" in G.HIP_SOURCES


def test_validation_codes_in_order():
    """Made-up host addresses: every call here is refused before a launch.  NULL -> -1, then shape (no gradient asked for included) -> -2, then the
    limits -> -3, then the workspace and the aliases."""
    lib = _lib().load()
    a = [ctypes.c_void_p(v << 34) for v in range(1, 12)]
    # ---- sampler: img, polar, rho, cos, sin, gout | gpolar, gimg | ws, ws_bytes | B C H W S
    f = lib.hdn_logpolar_sample_bwd_f32
    ins, ok = a[:6], (2, 3, 31, 29, 15, None)
    need = lib.hdn_logpolar_sample_bwd_workspace_bytes(2, 15)
    assert need == 2 * 1 * 2 * 4 and lib.hdn_logpolar_sample_bwd_workspace_bytes(3, 127) == 3 * 64 * 2 * 4
    assert lib.hdn_logpolar_sample_bwd_workspace_bytes(0, 15) == E_SHAPE and lib.hdn_logpolar_sample_bwd_workspace_bytes(70000, 15) == E_LIMIT
    for i in range(6):
        bad = list(ins)
        bad[i] = None
        assert f(*bad, a[6], a[7], a[8], need, *ok) == E_NULL, i
        assert f(*bad, None, None, a[8], need, 0, 3, 31, 29, 15, None) == E_NULL, i          # NULL before shape
    assert f(*ins, None, None, a[8], need, *ok) == E_SHAPE                                     # no gradient asked for
    for dims in ((0, 3, 31, 29, 15), (2, 0, 31, 29, 15), (2, 3, 1, 29, 15), (2, 3, 31, 1, 15), (2, 3, 31, 29, 0)):
        assert f(*ins, a[6], a[7], a[8], need, *dims, None) == E_SHAPE, dims
        assert f(*ins, a[0], a[7], a[8], need, *dims, None) == E_SHAPE, dims                  # ... although an output aliases
    assert f(*ins, a[6], a[7], a[8], need, 65536, 3, 31, 29, 15, None) == E_LIMIT
    assert f(*ins, a[6], a[7], None, 0, *ok) == E_NULL                                         # grad_polar needs the workspace
    assert f(*ins, a[6], a[7], a[8], need - 4, *ok) == E_LIMIT
    assert f(*ins, a[6], a[7], ctypes.c_void_p((9 << 34) + 4), need, *ok) == E_LIMIT           # not 16-byte aligned
    assert f(*ins, a[6], a[7], a[0], need, *ok) == E_ALIAS
    for gp, gi in ((a[0], a[7]), (a[6], a[5]), (a[6], a[6]), (a[8], a[7]), (a[1], None), (None, a[0])):
        assert f(*ins, gp, gi, a[8], need, *ok) == E_ALIAS, (gp, gi)
    # ---- DLT: src, off, gH | gsrc, goff | B
    f = lib.hdn_dlt_solve_bwd_f32
    for i in range(3):
        bad = list(a[:3])
        bad[i] = None
        assert f(*bad, a[3], a[4], 4, None) == E_NULL and f(*bad, None, None, 0, None) == E_NULL, i
    assert f(*a[:3], None, None, 4, None) == E_SHAPE and f(*a[:3], a[3], a[4], 0, None) == E_SHAPE and f(*a[:3], a[0], a[4], -1, None) == E_SHAPE
    assert f(*a[:3], a[3], a[4], (1 << 24) + 1, None) == E_LIMIT
    for gs, go in ((a[0], a[4]), (a[3], a[2]), (a[3], a[3]), (a[1], None), (None, a[2])):
        assert f(*a[:3], gs, go, 4, None) == E_ALIAS, (gs, go)
    # ---- warp: img, theta, gout | gtheta, gimg | ws, ws_bytes | B C H W
    f = lib.hdn_warp_bwd_f32
    ins, ok = a[:3], (2, 3, 11, 13, None)
    need = lib.hdn_warp_bwd_workspace_bytes(2, 11, 13)
    assert need == 2 * 1 * 9 * 4 and lib.hdn_warp_bwd_workspace_bytes(2, 127, 127) == 2 * 16 * 9 * 4 and lib.hdn_warp_bwd_workspace_bytes(1, 25, 41) == 72
    assert lib.hdn_warp_bwd_workspace_bytes(2, 1, 13) == E_SHAPE
    for i in range(3):
        bad = list(ins)
        bad[i] = None
        assert f(*bad, a[3], a[4], a[5], need, *ok) == E_NULL and f(*bad, None, None, a[5], need, 2, 3, 1, 13, None) == E_NULL, i
    assert f(*ins, None, None, a[5], need, *ok) == E_SHAPE
    for dims in ((0, 3, 11, 13), (2, 0, 11, 13), (2, 3, 1, 13), (2, 3, 11, 1)):
        assert f(*ins, a[3], a[4], a[5], need, *dims, None) == E_SHAPE and f(*ins, a[0], a[4], a[5], need, *dims, None) == E_SHAPE, dims
    assert f(*ins, a[3], a[4], a[5], need, 65536, 3, 11, 13, None) == E_LIMIT
    assert f(*ins, a[3], a[4], a[5], need, 2, 1 << 12, 1 << 10, 1 << 10, None) == E_LIMIT     # C H W > 2^31 - 1
    assert f(*ins, a[3], a[4], None, 0, *ok) == E_NULL and f(*ins, a[3], a[4], a[5], need - 4, *ok) == E_LIMIT
    for gt, gi in ((a[0], a[4]), (a[3], a[2]), (a[3], a[3]), (a[5], a[4]), (a[1], None)):
        assert f(*ins, gt, gi, a[5], need, *ok) == E_ALIAS, (gt, gi)


# ------------------------------------------------------------------------------------------------------------------------ closed forms
def _close(a, b, what, rel=1e-11):
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    assert err <= rel * max(scale, 1.0), (what, err, scale)


def test_sampler_closed_form_equals_float64_autograd():
    for kw in (GC.LOGPOLAR_BOUND, dict(B=3, C=2, H=24, W=37, S=16)):
        x, polar, tabs, g, gp, Mp, gx, Mx = GC.logpolar_random_problem(**kw)
        assert GC.logpolar_margin(polar, tabs, kw["H"], kw["W"]) > GC.MARGIN
        ap, ax = GC.logpolar_autograd(x, polar, tabs, g, torch.float64)
        _close(gp, ap, "grad_polar")
        _close(gx, ax, "grad_x")
        assert bool((Mp >= gp.abs() * (1 - 1e-12)).all()) and bool((Mx >= gx.abs() * (1 - 1e-12)).all())
        # the border rule and the masked taps take part: some samples are past a border on every side
        pxu, pyu = GC.logpolar_coords(polar, tabs, kw["H"], kw["W"], torch.float64)
        assert bool((pxu <= 0).any() or (pyu <= 0).any()) and bool((pxu >= kw["W"] - 1).any() or (pyu >= kw["H"] - 1).any())
        # the fp32 restatement picks the same cells on a fixture that keeps the margin
        same = GC.logpolar_closed(x, polar, tabs, g, torch.float32)
        assert all(torch.equal(p, q) for p, q in zip(same, (gp, Mp, gx, Mx)))


def test_sampler_exact_fixtures_are_exact():
    """Dyadic tables and origins, integers in [-3, 3]: the float64 closed forms equal float64 AND fp32 CPU autograd bit for bit, are fp32 values, and
    every batched fixture has samples past every border (H != W in two of them: a swap of H//2 and W//2 changes the result)."""
    for i, (H, W, C, _) in enumerate(GC.LOGPOLAR_EXACT):
        x, polar, tabs, g, gp, gx = GC.logpolar_exact_problem(i)
        for dt in (torch.float64, torch.float32):
            ap, ax = GC.logpolar_autograd(x, polar, tabs, g, dt)
            assert torch.equal(ap.double(), gp) and torch.equal(ax.double(), gx), (i, dt)
        assert torch.equal(gp.float().double(), gp) and torch.equal(gx.float().double(), gx)
        pxu, pyu = GC.logpolar_coords(polar, tabs, H, W, torch.float64)
        past = [bool((pxu <= 0).any()), bool((pxu >= W - 1).any()), bool((pyu <= 0).any()), bool((pyu >= H - 1).any())]
        assert sum(past) >= 2 and (polar.shape[0] == 1 or all(past)), (i, past)                # a batch: past every border; one sample: past two
        inside = (pxu > 0) & (pxu < W - 1) & (pyu > 0) & (pyu < H - 1)
        assert bool(inside.any()) and float(gp.abs().max()) > 0
    x, polar, tabs, g, gp, gx = GC.logpolar_exact_problem(3)                                   # H = 8, W = 16
    swapped = GC.logpolar_closed(x.transpose(2, 3).contiguous(), polar, tabs, g)[0]
    assert not torch.equal(swapped, gp)
    pxu, _ = GC.logpolar_coords(torch.tensor(GC.LOGPOLAR_EXACT[0][3]), tabs, 8, 8, torch.float64)
    assert bool((pxu == 0).any())                                                              # p == 0 exactly: derivative 0 by the rule


def test_dlt_closed_form_equals_float64_autograd():
    for kind in GC.DLT_CORNERS:
        for B in (1, 9):
            src, off, gH, gs, go = GC.dlt_problem(kind, B)
            assert float(off.abs().max()) <= 32
            a_s, a_o = GC.dlt_autograd(src, off, gH)
            _close(gs, a_s, "grad_src", 1e-9)
            _close(go, a_o, "grad_off", 1e-9)
            # the two float64 routes agree far inside the bound of the kernel (2^-23): the solve's own noise is orders below
            assert GC.dlt_excess(a_s, gs)[1] < 1e-3 and GC.dlt_excess(a_o, go)[1] < 1e-3
    # grad_H[8] is ignored
    src, off, gH, gs, go = GC.dlt_problem("production", 7)
    g2 = gH.clone()
    g2[:, 8] += 5.0
    assert torch.equal(GC.dlt_closed(src, off, g2)[0], gs)


def test_transformer_restatement_is_the_oracle_bit_for_bit():
    from oracle import hdn_oracle as O
    for kw in (GC.WARP_BOUND, dict(B=1, C=2, H=25, W=41)):
        U, theta, g = GC.warp_random_problem(**kw, cells32=True)[:3]
        want, _ = O.transformer(U, theta.reshape(-1, 3, 3), (kw["H"], kw["W"]))
        assert torch.equal(GC.transformer_rs(U, theta, torch.float32), want)
    for i in range(len(GC.WARP_EXACT)):
        U, theta, g, _, _ = GC.warp_exact_problem(i)
        want, _ = O.transformer(U, theta.reshape(-1, 3, 3), U.shape[2:])
        assert torch.equal(GC.transformer_rs(U, theta, torch.float32), want)
        assert torch.equal(GC.transformer_rs(U, theta, torch.float64), want.double())


def test_warp_closed_form_equals_float64_autograd():
    seeds = [s for s in range(6) if GC.warp_margin(GC._warp_random(s, **GC.WARP_BOUND)[1], GC.WARP_BOUND["B"], GC.WARP_BOUND["H"],
                                                   GC.WARP_BOUND["W"]) > GC.MARGIN]
    print(f"GEOMETRY-BWD warp bound fixture: seeds of 0-5 that keep the margin: {seeds}")
    assert seeds and GC.WARP_BOUND_SEED == seeds[0]
    U, theta, g, gth, Mth, gU, MU = GC.warp_random_problem(**GC.WARP_BOUND)
    at, aU = GC.warp_autograd(U, theta, g, torch.float64)
    _close(gth, at, "grad_theta")
    _close(gU, aU, "grad_U")
    assert bool((Mth >= gth.abs() * (1 - 1e-12)).all()) and bool((MU >= gU.abs() * (1 - 1e-12)).all())
    same = GC.warp_closed(U, theta, g, torch.float32)
    assert all(torch.equal(p, q) for p, q in zip(same, (gth, Mth, gU, MU)))
    # projective rows take part
    assert float(theta[:, 6:8].abs().min()) > 0 and float(gth[:, 6:].abs().min()) > 0


def test_warp_exact_fixtures_are_exact():
    for i, (H, W, C, B) in enumerate(GC.WARP_EXACT):
        assert H != W and H in (5, 9, 17) and W in (5, 9, 17)
        U, theta, g, gth, gU = GC.warp_exact_problem(i)
        for dt in (torch.float64, torch.float32):
            at, aU = GC.warp_autograd(U, theta, g, dt)
            assert torch.equal(at.double(), gth) and torch.equal(aU.double(), gU), (i, dt)
        assert torch.equal(gth.float().double(), gth) and torch.equal(gU.float().double(), gU)
        assert float(gth.abs().max()) > 0


def test_reference_ratios_and_the_bounds_they_give():
    """r_ref: the worst |fp32 CPU autograd - truth| / M of the reference formulation on the bound fixtures; K = max(4 r_ref, 2e-6).  The sums over a
    sample (grad_polar, grad_theta) come out near the fp32 unit roundoff.  The scattered image gradients do not: a bilinear weight is a difference
    px - floor(px) of an fp32 coordinate of size 10 - 30, so a weight of 0.05 carries a relative error of 1e-5 that M (absolute terms) does not
    see - which is why K is taken from the reference's own error and not from the number format alone."""
    for name, (r1, r2) in (("sampler (grad_polar, grad_x)", GC.logpolar_r_ref()), ("warp (grad_theta, grad_U)", GC.warp_r_ref())):
        print(f"GEOMETRY-BWD r_ref {name}: {r1:.3e}, {r2:.3e} -> K = {GC.k_bound(r1):.3e}, {GC.k_bound(r2):.3e}")
        assert 0 < r1 < 1e-5 and 0 < r2 < 1e-3


# ------------------------------------------------------------------------------------------------------------------------ Python layer
def test_install_train_binds_the_differentiable_sampler_and_uninstall_restores():
    import hdn_amd
    import hdn_amd.install as hinstall
    lp, mb = types.ModuleType("hdn.models.logpolar"), types.ModuleType("hdn.models.model_builder_e2e_unconstrained_v2")

    class Own:
        pass

    lp.STN_Polar = mb.STN_Polar = Own
    mods = {lp.__name__: lp, mb.__name__: mb}
    for train, want in ((False, hdn_amd.STN_Polar), (True, hdn_amd.STN_PolarTrain)):
        done = hinstall.install(modules=mods, train=train) if train else hinstall.install(modules=mods)
        try:
            assert lp.STN_Polar is want and mb.STN_Polar is want
            assert (lp.__name__, "STN_Polar") in done and (mb.__name__, "STN_Polar") in done
            assert lp.STN_Polar(30).differentiable is train
        finally:
            assert hinstall.uninstall() >= 2
        assert lp.STN_Polar is Own and mb.STN_Polar is Own


def test_differentiable_switch_reaches_the_device_check():
    """STN_Polar's default still refuses a grad-carrying input before any device check; STN_PolarTrain and the attribute switch go on to the device
    check (HdnHipError on the CPU) - they no longer refuse."""
    import hdn_amd
    from hdn_amd import _lib
    x, polar = torch.zeros(2, 3, 31, 31), torch.zeros(2, 2, requires_grad=True)
    m = hdn_amd.STN_Polar(31)
    assert m.differentiable is False
    with pytest.raises(RuntimeError, match="inference-only.*uninstall"):
        m(x, polar)
    m.differentiable = True
    for mod in (m, hdn_amd.STN_PolarTrain(31), hdn_amd.STN_Polar(31, differentiable=True)):
        with pytest.raises(_lib.HdnHipError):
            mod(x, polar)
    assert "differentiable" not in dict(m.named_buffers()) and "differentiable" not in dict(m.named_parameters())
    with pytest.raises(ValueError):
        hdn_amd.dlt_solve_backward(torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(2, 9), need_src=False, need_off=False)
    with pytest.raises(ValueError):
        hdn_amd.transformer_backward(torch.zeros(1, 1, 4, 4), torch.zeros(1, 9), torch.zeros(1, 4, 4, 1), need_U=False, need_theta=False)
    with pytest.raises(ValueError):
        hdn_amd.logpolar_sample_backward(x, polar, GC.real_tables(15), torch.zeros(2, 3, 15, 15), need_x=False, need_polar=False)
