"""Host side of tests/test_gpu_affine_stn.py: the three entry points of csrc/affine_stn.hip exist in the library, the header and the binding (ABI still
10), their validation codes come in the order of the other geometry backwards (made-up addresses: nothing is launched), the closed form of
tests/affine_stn_cases.py equals float64 autograd through F.affine_grid + F.grid_sample at 1e-12 of M, the numpy restatement of the kernel's forward
lies inside the bound, the bound fixtures keep their coordinate margin, the 'classes' fixtures populate every zeros-padding class, PyTorch's own fp32
ratios r_ref are measured and printed, and hdn_amd.affine / install(train=True) route as documented.  No GPU, no kernel."""
import ctypes
import os
import re
import types

import pytest
import torch

import affine_stn_cases as AC
import geometry_bwd_cases as GC

E_NULL, E_SHAPE, E_LIMIT, E_ALIAS = -1, -2, -3, -4
NEW = {"hdn_affine_sample_f32": 10, "hdn_affine_sample_bwd_workspace_bytes": 3, "hdn_affine_sample_bwd_f32": 14}
MB = "hdn.models.model_builder_e2e_unconstrained_v2"


def _lib():
    from hdn_amd import _lib as L
    return L


def test_symbols_in_the_library_the_header_and_the_binding():
    L = _lib()
    lib = L.load()
    assert lib.hdn_abi_version() == L.ABI_VERSION == 10
    with open(os.path.join(AC.ROOT, "include", "hdn_hip.h")) as f:
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
    for text in ("X_j = (2j+1)/Wo - 1", "px = ((gx+1) W - 1)/2", "d out / d px = (1-n)(I_ne - I_nw) + n (I_se - I_sw)",
                 "d out / d py = (1-w)(I_sw - I_nw) + w (I_se - I_ne)", "strictly inside (-1, W)", "before any conversion to an integer",
                 "NOT bit-reproducible between calls"):
        assert text in header, text
    import hdn_amd
    assert hdn_amd.affine_sample is hdn_amd.affine.affine_sample
    import __graft_entry__ as G
    assert "affine_stn.hip" in G.HIP_SOURCES


def test_validation_codes_in_order():
    """Made-up host addresses: every call here is refused before a launch.  NULL -> -1, then shape (no gradient asked for included) -> -2, then the
    limits -> -3, then the workspace and the aliases."""
    lib = _lib().load()
    a = [ctypes.c_void_p(v << 34) for v in range(1, 12)]
    q = lib.hdn_affine_sample_bwd_workspace_bytes
    assert q(2, 5, 7) == 2 * 1 * 6 * 4 and q(2, 19, 23) == 2 * 2 * 6 * 4 and q(32, 127, 127) == 32 * 64 * 6 * 4 and q(1, 16, 16) == 24
    assert q(0, 5, 7) == E_SHAPE and q(2, 0, 7) == E_SHAPE and q(2, 5, -1) == E_SHAPE and q(70000, 5, 7) == E_LIMIT and q(1, 1 << 16, 1 << 15) == E_LIMIT
    # ---- forward: img, theta, out | B C H W Ho Wo
    f = lib.hdn_affine_sample_f32
    ok = (2, 3, 9, 11, 5, 7, None)
    for i in range(3):
        bad = list(a[:3])
        bad[i] = None
        assert f(*bad, *ok) == E_NULL and f(*bad, 0, 3, 9, 11, 5, 7, None) == E_NULL, i                # NULL before shape
    for k in range(6):
        dims = list(ok[:6])
        dims[k] = 0
        assert f(*a[:3], *dims, None) == E_SHAPE and f(a[0], a[1], a[0], *dims, None) == E_SHAPE, dims     # shape before alias
    assert f(*a[:3], 65536, 3, 9, 11, 5, 7, None) == E_LIMIT and f(*a[:3], 2, 3, 1 << 16, 1 << 15, 5, 7, None) == E_LIMIT
    assert f(*a[:3], 2, 3, 9, 11, 1 << 15, 1 << 16, None) == E_LIMIT
    assert f(a[0], a[1], a[0], 65536, 3, 9, 11, 5, 7, None) == E_LIMIT                                  # limit before alias
    assert f(a[0], a[1], a[0], *ok) == E_ALIAS and f(a[0], a[1], a[1], *ok) == E_ALIAS
    # ---- backward: img, theta, gout | gtheta, gimg | ws, ws_bytes | B C H W Ho Wo
    f = lib.hdn_affine_sample_bwd_f32
    ins = a[:3]
    need = q(2, 5, 7)
    for i in range(3):
        bad = list(ins)
        bad[i] = None
        assert f(*bad, a[3], a[4], a[5], need, *ok) == E_NULL, i
        assert f(*bad, None, None, a[5], need, 0, 3, 9, 11, 5, 7, None) == E_NULL, i                    # NULL before shape
    assert f(*ins, None, None, a[5], need, *ok) == E_SHAPE                                              # no gradient asked for
    for k in range(6):
        dims = list(ok[:6])
        dims[k] = 0
        assert f(*ins, a[3], a[4], a[5], need, *dims, None) == E_SHAPE, dims
        assert f(*ins, a[0], a[4], a[5], need, *dims, None) == E_SHAPE, dims                            # ... although an output aliases
    assert f(*ins, a[3], a[4], a[5], need, 65536, 3, 9, 11, 5, 7, None) == E_LIMIT
    assert f(*ins, a[3], a[4], None, 0, 65536, 3, 9, 11, 5, 7, None) == E_LIMIT                         # limit before the workspace
    assert f(*ins, a[3], a[4], None, 0, *ok) == E_NULL                                                  # grad_theta needs the workspace
    assert f(*ins, a[3], a[4], a[5], need - 4, *ok) == E_LIMIT
    assert f(*ins, a[3], a[4], ctypes.c_void_p((9 << 34) + 4), need, *ok) == E_LIMIT                    # not 16-byte aligned
    assert f(*ins, a[3], a[4], a[0], need, *ok) == E_ALIAS                                              # the workspace on img
    assert f(*ins, a[0], a[4], None, 0, *ok) == E_NULL                                                  # workspace before the output aliases
    for gt, gi in ((a[0], a[4]), (a[3], a[2]), (a[3], a[3]), (a[5], a[4]), (a[1], None), (None, a[0]), (None, a[1])):
        assert f(*ins, gt, gi, a[5], need, *ok) == E_ALIAS, (gt, gi)


# ------------------------------------------------------------------------------------------------------------------------ closed form and fixtures
@pytest.mark.parametrize("shape", AC.SHAPES, ids=str)
def test_closed_form_equals_float64_autograd_at_1e_12_of_M(shape):
    """Per element at 1e-12 of M at the small shapes (every kind; the identity's exact integer coordinates included).  At 255 -> 127 the two float64
    routes form px ~ 255 differently (affine_grid scales a linspace and multiplies matrices) and differ by some 1e-13 in it, while a weight - and with
    it an element's M - can be as small as the fixture's margin (7e-7; 0 for the identity): there grad_theta, a sum over the sample, is held to
    1e-12 of M per element, out and grad_img to 1e-11 of the largest M."""
    B, C, H, W, Ho, Wo = shape
    for kind in AC.KINDS:
        x, theta, g, truth = AC.problem(kind, shape)
        o, t, xg = AC.autograd(x, theta, (B, 1, Ho, Wo), g, torch.float64)                   # size[1] is not read, as in the reference's call
        for name, got in (("out", o), ("theta", t), ("img", xg)):
            val, M = truth[name]
            if shape in AC.SMALL_SHAPES or name == "theta":
                r = GC.worst_ratio(got, val, M)
            else:
                r = float((got - val).abs().max()) / float(M.max()) / 10.0
            assert r <= 1e-12, (kind, name, r)
            assert bool((M >= val.abs() * (1 - 1e-12)).all())


def test_bound_fixtures_keep_the_margin_and_classes_are_populated():
    for shape in AC.SMALL_SHAPES:
        B, C, H, W, Ho, Wo = shape
        for kind in ("similarity", "classes"):
            m = AC.margin(AC.make_theta(kind, shape), H, W, Ho, Wo)
            print(f"AFFINE-STN margin {kind} {shape}: {m:.3e}")
            assert m > AC.MARGIN, (kind, shape, m)
    for shape in AC.CLASS_SHAPES:
        B, C, H, W, Ho, Wo = shape
        theta = AC.make_theta("classes", shape)
        for dt in (torch.float64, torch.float32):
            got = AC.classes_present(theta, H, W, Ho, Wo, dt)
            assert set(AC.REQUIRED_CLASSES) <= got, (shape, dt, got)
        # and the random similarity stays what combine_affine_c0_v2 builds: a = d, b = -c, a scale of about one half
        t = AC.make_theta("similarity", shape)
        assert torch.equal(t[:, 0, 0], t[:, 1, 1]) and torch.equal(t[:, 0, 1], -t[:, 1, 0])
        sc = (t[:, 0, 0] ** 2 + t[:, 1, 0] ** 2).sqrt()
        assert bool(((sc > 0.39) & (sc < 0.63)).all())


def test_poisoned_samples_are_dead_in_the_closed_form_too():
    """A shift of 1e30, NaN and inf entries: every sample of that batch entry is dead (class 'dead' only), in float64 and in fp32."""
    shape = AC.SHAPES[0]
    B, C, H, W, Ho, Wo = shape
    for how in ("shift", "nan", "inf"):
        t = AC.poisoned(AC.make_theta("similarity", shape), 1, how)
        for dt in (torch.float64, torch.float32):
            _, _, px, py = AC.coords(t, H, W, Ho, Wo, dt)
            dead = (AC.axis_class(px, W) == 3) | (AC.axis_class(py, H) == 3)
            assert bool(dead[1].all()) and not bool(dead[0].any()), (how, dt)
        x, _, g, _ = AC.problem("similarity", shape)
        out = AC.kernel_forward_np(x, t, Ho, Wo)
        assert bool((out[1] == 0).all()) and torch.equal(out[0], AC.kernel_forward_np(x, AC.make_theta("similarity", shape), Ho, Wo)[0])
        tr = AC.closed(x, t, Ho, Wo, g)
        assert all(bool((tr[k][0][1] == 0).all()) and bool((tr[k][1][1] == 0).all()) for k in ("out", "theta", "img"))
        if how == "shift":                                                                   # a finite position far outside: PyTorch's CPU path gives 0 too
            assert bool((AC.stn_rs(x, t, (B, C, Ho, Wo), torch.float32)[1] == 0).all())


@pytest.mark.parametrize("shape", AC.SHAPES, ids=str)
def test_reference_ratios_and_the_restated_forward_inside_the_bound(shape):
    """r_ref of PyTorch's own fp32 CPU path per fixture, printed; the numpy restatement of the kernel's forward (which the kernel must equal bit for
    bit) lies inside K M of the truth, K = max(4 r_ref, 2e-6)."""
    B, C, H, W, Ho, Wo = shape
    for kind in AC.KINDS:
        r = AC.r_ref(kind, shape)
        x, theta, g, truth = AC.problem(kind, shape)
        rs = GC.worst_ratio(AC.kernel_forward_np(x, theta, Ho, Wo), *truth["out"])
        print(f"AFFINE-STN r_ref {kind} {shape}: out {r['out']:.3e}, grad_theta {r['theta']:.3e}, grad_img {r['img']:.3e}; restated forward {rs:.3e}")
        assert all(v >= 0 for v in r.values())
        assert rs <= GC.k_bound(r["out"]), (kind, rs, r["out"])


# ------------------------------------------------------------------------------------------------------------------------ Python layer
class _Builder:
    """A stand-in ModelBuilder that owns the reference's three-line method."""

    def stn_with_theta(self, x, theta, size):
        theta = theta.view(-1, 2, 3)
        grid = torch.nn.functional.affine_grid(theta, size)
        x = torch.nn.functional.grid_sample(x, grid)
        return x


def test_install_train_routes_by_the_constant_and_uninstall_restores(monkeypatch):
    import hdn_amd.install as hinstall
    from hdn_amd import affine
    assert isinstance(hinstall.AFFINE_STN_TRAIN_BOUND, bool)
    mb = types.ModuleType(MB)
    mb.ModelBuilder = _Builder
    orig = _Builder.__dict__["stn_with_theta"]
    site = (MB, "ModelBuilder.stn_with_theta")
    for bound in (True, False):
        monkeypatch.setattr(hinstall, "AFFINE_STN_TRAIN_BOUND", bound)
        for train in (True, False):
            done = hinstall.install(modules={MB: mb}, train=train) if train else hinstall.install(modules={MB: mb})
            try:
                if train and bound:
                    assert _Builder.__dict__["stn_with_theta"] is affine.stn_with_theta and site in done
                else:
                    assert _Builder.__dict__["stn_with_theta"] is orig and site not in done
            finally:
                hinstall.uninstall()
            assert _Builder.__dict__["stn_with_theta"] is orig
    # a ModelBuilder without the method of its own is left alone
    monkeypatch.setattr(hinstall, "AFFINE_STN_TRAIN_BOUND", True)
    mb2 = types.ModuleType(MB)
    mb2.ModelBuilder = type("Bare", (), {})
    try:
        assert site not in hinstall.install(modules={MB: mb2}, train=True)
        assert "stn_with_theta" not in mb2.ModelBuilder.__dict__
    finally:
        hinstall.uninstall()


def test_the_committed_constant_is_what_the_measurement_says():
    import json
    import hdn_amd.install as hinstall
    with open(os.path.join(AC.ROOT, "profiles", "affine_stn_train.json")) as f:
        res = json.load(f)
    assert isinstance(res["ahead"], bool) and hinstall.AFFINE_STN_TRAIN_BOUND is res["ahead"]
    spread = max(res[s]["max"] - res[s]["min"] for s in ("hip", "library"))
    assert res["ahead"] == (res["library"]["ms_per_step"] - res["hip"]["ms_per_step"] > spread)


def test_no_fallback_and_input_rules():
    import hdn_amd
    from hdn_amd import _lib, affine
    x, theta = torch.zeros(2, 3, 9, 11), torch.zeros(2, 2, 3)
    size = (2, 1, 5, 7)
    with pytest.raises(_lib.HdnHipError):                                                     # a CPU tensor: no fallback
        hdn_amd.affine_sample(x, theta, size)
    tg = theta.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference-only.*uninstall"):                       # refused before any device check
        hdn_amd.affine_sample(x, tg, size)
    with pytest.raises(RuntimeError, match="inference-only.*uninstall"):
        hdn_amd.affine_sample(x.clone().requires_grad_(True), theta, size)
    with torch.no_grad(), pytest.raises(_lib.HdnHipError):                                    # not recording: goes on to the device check
        hdn_amd.affine_sample(x, tg, size)
    with pytest.raises(_lib.HdnHipError):                                                     # differentiable: no longer refuses, reaches the device check
        hdn_amd.affine_sample(x, tg, size, differentiable=True)
    with pytest.raises(_lib.HdnHipError):
        affine.stn_with_theta(None, x, tg.view(2, 6), size)
    with pytest.raises(ValueError):
        hdn_amd.affine_sample(x, theta, (3, 1, 5, 7))                                          # size[0] is not the batch
    with pytest.raises(ValueError):
        hdn_amd.affine_sample(x, torch.zeros(3, 6), size)                                      # theta's batch
    with pytest.raises(ValueError):
        hdn_amd.affine_sample(x[0], theta, size)
    with pytest.raises(RuntimeError):
        hdn_amd.affine_sample(x, torch.zeros(2, 3, 2).transpose(1, 2), size)                   # what .view(-1, 2, 3) refuses is refused
    with pytest.raises(ValueError):
        hdn_amd.affine_sample_backward(x, theta, size, torch.zeros(2, 3, 5, 7), need_x=False, need_theta=False)
    with pytest.raises(ValueError):
        hdn_amd.affine_sample_backward(x, theta, size, torch.zeros(2, 3, 5, 8))
    with pytest.raises(_lib.HdnHipError):
        hdn_amd.affine_sample_backward(x, theta, size, torch.zeros(2, 3, 5, 7))
