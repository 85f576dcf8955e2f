"""The backward of the depthwise correlations on the device (csrc/xcorr_bwd.hip through hdn_xcorr_depthwise_bwd_f32, hdn_amd.xcorr.xcorr_depthwise_backward
and the autograd Function behind xcorr_depthwise / xcorr_depthwise_circular) against float64 autograd through tests/xcorr_cases.py:direct_sum: exactly
on integer and position fixtures in both launch forms, inside 1e-4 + 2e-6 M on random data, bit for bit between calls, plane counts and requested
outputs, through autograd, through the training-mode head modules, and through install() on a stand-in of the reference's head module.  The host side is
tests/test_xcorr_bwd_host.py."""
import copy
import types

import pytest
import torch
import torch.nn as nn

import xcorr_bwd_cases as BC
import xcorr_cases as XC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def lib_form(S):
    from hdn_amd import _lib
    return _lib.load().hdn_xcorr_bwd_form(int(S.circular), S.Hx, S.Wx, S.Hk, S.Wk)


def check_exact(kind, planes, dev, offsets):
    """None, or what is wrong with the exact fixture at `planes` planes and these pointer offsets (results from NaN, margins of 0xA5 around them)."""
    S = BC.SHAPES[kind]
    x, k, g, gx, gk = BC.exact_problem(kind, planes)
    got_x, got_k, (bx, bk) = BC.run(kind, x, k, g, dev, offsets)
    for name, got, truth, buf, off in (("gx", got_x, gx, bx, offsets[3]), ("gk", got_k, gk, bk, offsets[4])):
        d = BC.first_difference(got, truth)
        if d is not None:
            return f"{kind} ({'circular' if S.circular else 'plain'}, form {BC.form(S)}) at {planes} planes, offsets {offsets}: {name}: {d}"
        if not BC.untouched(buf, 8 + off, 8 + off + got.numel()):
            return f"{kind} at {planes} planes, offsets {offsets}: a write outside {name}"
    return None


# ------------------------------------------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("kind", BC.EXACT_KINDS)
def test_exact_fixture_every_plane_count(dev, kind):
    """Integer x, k, g in [-3, 3]: gx and gk torch.equal to float64 at 1 .. 9 planes (19 too for the two training shapes), the five base pointers
    aligned and at float offsets (1, 2, 3, 1, 2), from output buffers that held NaN."""
    assert lib_form(BC.SHAPES[kind]) == BC.form(BC.SHAPES[kind]) == BC.FORM_LDS
    cases = [(P, off) for P in BC.plane_counts(kind) for off in BC.OFFSETS]
    failures = [f for f in (check_exact(kind, P, dev, off) for P, off in cases) if f is not None]
    assert not failures, f"{len(failures)} of {len(cases)} cases: " + " | ".join(failures[:4])


def test_exact_fixture_on_both_sides_of_the_form_switch(dev):
    """One plain and one circular shape at exactly 60 KiB (LDS form) and one float above (global form), 2 planes each: all four (form, variant) pairs
    occur, by the library's own answer, and each is torch.equal to float64."""
    pairs = set()
    failures = []
    for kind in BC.SWITCH_KINDS:
        S = BC.SHAPES[kind]
        pairs.add((lib_form(S), S.circular))
        for off in BC.OFFSETS:
            f = check_exact(kind, BC.SWITCH_PLANES, dev, off)
            if f is not None:
                failures.append(f)
    assert pairs == {(0, False), (1, False), (0, True), (1, True)}
    assert not failures, " | ".join(failures[:4])


# ------------------------------------------------------------------------------------------------------------------------------ 2. positions
@pytest.mark.parametrize("kind", BC.POSITION_KINDS)
def test_every_output_position_reaches_its_taps_and_pixels(dev, kind):
    """One plane per output position (i, j), g a single 1 there: gk[u][v] == xp[i + u][j + v] and gx == the taps scattered through the preimage rule,
    both built by index arithmetic, torch.equal."""
    x, k, g, want_gx, want_gk = BC.position_problem(kind)
    got_x, got_k, _ = BC.run(kind, x, k, g, dev)
    for name, got, want in (("gx", got_x, want_gx), ("gk", got_k, want_gk)):
        d = BC.first_difference(got, want)
        assert d is None, f"{kind} {name} (plane = output position, row-major): {d}"


# ------------------------------------------------------------------------------------------------------------------------------ 3. random data
@pytest.mark.parametrize("S", BC.RANDOM_SHAPES, ids=lambda S: S.name)
def test_random_data_inside_the_project_bound(dev, S):
    """relu(N(0, 1)) features, N(0, 1) g, 128 planes: |hip - f64| <= 1e-4 + 2e-6 M per plane, M the same backward on the absolute values; no element
    may be outside.  (The reference's own fp32 CPU gradients use at most 0.03 of this bound on such inputs.)"""
    x, k, g, gx, gk, mx, mk = BC.random_problem(S.name)
    got_x, got_k, _ = BC.run(S.name, x, k, g, dev)
    rx, rk = BC.worst_ratio(got_x, gx, mx), BC.worst_ratio(got_k, gk, mk)
    print(f"FORMS xcorr backward {S.name}: worst |hip - f64| / (1e-4 + 2e-6 M): gx {rx:.4f}, gk {rk:.4f} over {BC.RANDOM_PLANES} planes")
    for name, got, truth, M in (("gx", got_x, gx, mx), ("gk", got_k, gk, mk)):
        bad = ~((got.double() - truth).abs() <= BC.bound(M).view(-1, 1, 1))
        assert not bool(bad.any()), (S.name, name, int(bad.sum()), bad.nonzero()[0].tolist(), rx, rk)


# ------------------------------------------------------------------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("kind", ["prod29", "circ13", "genc_6x7_4x6", "gen_96x97_35x1"])
def test_bit_equal_between_calls_plane_counts_and_requested_outputs(dev, kind):
    """Random data: two calls are bit-equal; plane p of a 9-plane call equals that plane run alone; gx only and gk only give the bits of the joint
    call while the buffer that was not asked for (0xA5 everywhere) and the margins around both outputs stay untouched."""
    S = BC.SHAPES[kind]
    P = 9
    _, _, _, _, Ho, Wo = BC.geometry(S)
    gen = torch.Generator().manual_seed(BC.SEED + S.Hx)
    x, k, g = (torch.randn(P, h, w, generator=gen) for h, w in ((S.Hx, S.Wx), (S.Hk, S.Wk), (Ho, Wo)))
    ax, ak, (bx, bk) = BC.run(kind, x, k, g, dev, (1, 2, 3, 1, 2))
    assert BC.untouched(bx, 8 + 1, 8 + 1 + ax.numel()) and BC.untouched(bk, 8 + 2, 8 + 2 + ak.numel())
    assert not bool(ax.isnan().any()) and not bool(ak.isnan().any())
    bx2, bk2, _ = BC.run(kind, x, k, g, dev, (1, 2, 3, 1, 2))
    assert torch.equal(ax, bx2) and torch.equal(ak, bk2)
    for p in range(P):
        px, pk, _ = BC.run(kind, x[p:p + 1], k[p:p + 1], g[p:p + 1], dev)
        assert torch.equal(px[0], ax[p]) and torch.equal(pk[0], ak[p]), (kind, p)
    ox, none_k, (b1, b2) = BC.run(kind, x, k, g, dev, (1, 2, 3, 1, 2), need_k=False)
    assert none_k is None and torch.equal(ox, ax) and BC.untouched(b1, 8 + 1, 8 + 1 + ax.numel()) and BC.untouched(b2, 0, 0)
    none_x, ok, (b1, b2) = BC.run(kind, x, k, g, dev, (1, 2, 3, 1, 2), need_x=False)
    assert none_x is None and torch.equal(ok, ak) and BC.untouched(b1, 0, 0) and BC.untouched(b2, 8 + 2, 8 + 2 + ak.numel())


# ------------------------------------------------------------------------------------------------------------------------------ 5. autograd
@pytest.mark.parametrize("circular", [False, True])
def test_autograd_through_the_drop_ins(dev, circular, monkeypatch):
    from hdn_amd import _lib, xcorr as X
    fn = X.xcorr_depthwise_circular if circular else X.xcorr_depthwise
    Hx, Hk = (13, 13) if circular else (29, 5)
    gen = torch.Generator().manual_seed(BC.SEED + circular)
    x0, k0 = torch.randn(2, 5, Hx, Hx, generator=gen).to(dev), torch.randn(2, 5, Hk, Hk, generator=gen).to(dev)
    with torch.no_grad():
        y0 = fn(x0.clone().requires_grad_(True), k0)
    assert y0.grad_fn is None and not y0.requires_grad
    y1 = fn(x0, k0)                                              # grad mode on, no input requires grad
    assert y1.grad_fn is None and not y1.requires_grad and torch.equal(y1, y0)
    go = torch.randn(y0.shape, generator=gen).to(dev)
    want_x, want_k = X.xcorr_depthwise_backward(x0, k0, go, circular)
    assert want_x.shape == x0.shape and want_k.shape == k0.shape

    x, k = x0.clone().requires_grad_(True), k0.clone().requires_grad_(True)
    y = fn(x, k)
    assert y.grad_fn is not None and torch.equal(y.detach(), y0)  # the forward's bits are those of the no_grad path
    y.backward(go)
    assert torch.equal(x.grad, want_x) and torch.equal(k.grad, want_k)

    # a permuted grad_out is the same gradient
    gx_p, gk_p = X.xcorr_depthwise_backward(x0, k0, go.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), circular)
    assert torch.equal(gx_p, want_x) and torch.equal(gk_p, want_k)

    # only x requires grad: the entry point gets gk = NULL
    lib = _lib.load()
    real, calls = lib.hdn_xcorr_depthwise_bwd_f32, []

    def spy(*args):
        calls.append(args)
        return real(*args)

    monkeypatch.setattr(lib, "hdn_xcorr_depthwise_bwd_f32", spy)
    x, k = x0.clone().requires_grad_(True), k0.clone()
    fn(x, k).backward(go)
    assert k.grad is None and torch.equal(x.grad, want_x)
    assert len(calls) == 1 and calls[0][4] is None and calls[0][3] is not None
    x, k = x0.clone(), k0.clone().requires_grad_(True)
    fn(x, k).backward(go)
    assert x.grad is None and torch.equal(k.grad, want_k) and len(calls) == 2 and calls[1][3] is None and calls[1][4] is not None
    monkeypatch.undo()

    # a stride-0 grad_out
    x, k = x0.clone().requires_grad_(True), k0.clone().requires_grad_(True)
    fn(x, k).sum().backward()
    ones_x, ones_k = X.xcorr_depthwise_backward(x0, k0, torch.ones_like(y0), circular)
    assert torch.equal(x.grad, ones_x) and torch.equal(k.grad, ones_k)

    # first order only
    x = x0.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(fn(x, k0).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()

    # argument errors of the wrapper
    with pytest.raises(ValueError):
        X.xcorr_depthwise_backward(x0, k0, go[:, :, 1:], circular)
    with pytest.raises(ValueError):
        X.xcorr_depthwise_backward(x0, k0, go, circular, need_x=False, need_k=False)


# ------------------------------------------------------------------------------------------------------------------------------ 6. / 7. modules
def twin_grads(box, circular, z, x, wc, wl, dtype):
    """The gradients of loss = sum(cls wc) + sum(loc wl) for a CPU copy of `box` (.cls / .loc with conv_kernel, conv_search, head) in `dtype`, in
    training mode, its correlation being xcorr_cases.direct_sum: {parameter name | 'z' | 'x': gradient}."""
    t = copy.deepcopy(box).cpu().to(dtype).train()
    zz, xx = z.detach().cpu().to(dtype).requires_grad_(True), x.detach().cpu().to(dtype).requires_grad_(True)
    outs = []
    for br in (t.cls, t.loc):
        kf, sf = br.conv_kernel(zz), br.conv_search(xx)
        B, C = kf.shape[:2]
        f = XC.direct_sum(sf.flatten(0, 1), kf.flatten(0, 1), circular, dtype=dtype)
        outs.append(br.head(f.view(B, C, f.shape[1], f.shape[2])))
    ((outs[0] * wc.cpu().to(dtype)).sum() + (outs[1] * wl.cpu().to(dtype)).sum()).backward()
    grads = {n: p.grad for n, p in t.named_parameters()}
    grads["z"], grads["x"] = zz.grad, xx.grad
    return grads


def assert_inside_conv_bound(what, got, g64, g32):
    """err <= 4 e_ref + 1e-5 scale for every tensor: e_ref the error of the fp32 CPU twin, scale the largest |float64 gradient| of the tensor."""
    assert set(got) == set(g64) == set(g32)
    worst = (0.0, None)
    failures = []
    for name in sorted(got):
        assert got[name] is not None, f"{what}: {name} received no gradient"
        t = g64[name]
        err = float((got[name].detach().cpu().double() - t).abs().max())
        e_ref, scale = float((g32[name].double() - t).abs().max()), float(t.abs().max())
        b = 4 * e_ref + 1e-5 * scale
        worst = max(worst, (err / b if b > 0 else float(err > 0), name))
        if not err <= b:
            failures.append(f"{name}: err {err:.3e}, e_ref {e_ref:.3e}, scale {scale:.4g}, bound {b:.3e}")
    print(f"FORMS xcorr backward {what}: worst err / (4 e_ref + 1e-5 scale) = {worst[0]:.4f} at {worst[1]} over {len(got)} tensors")
    assert not failures, f"{what}: " + " | ".join(failures)


def seeded_inputs(circular, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    zs, xs = (15, 15) if circular else (7, 31)
    z = torch.randn(2, 16, zs, zs, generator=gen).to(dev).requires_grad_(True)
    x = torch.randn(2, 16, xs, xs, generator=gen).to(dev).requires_grad_(True)
    so = 13 if circular else 25
    wc, wl = torch.randn(2, 2, so, so, generator=gen).to(dev), torch.randn(2, 4 if circular else 2, so, so, generator=gen).to(dev)
    return z, x, wc, wl


@pytest.mark.parametrize("circular", [False, True])
def test_training_mode_head_modules(dev, circular):
    """heads.DepthwiseBAN (z 7 x 7, x 31 x 31) and heads.DepthwiseCircBAN (15 x 15 both) in .train() mode, 16 channels, B = 2: the gradients of every
    parameter and of both inputs for a seeded weighted sum of both outputs, against the float64 CPU twin."""
    from hdn_amd import heads
    torch.manual_seed(BC.SEED + 6 + circular)
    box = (heads.DepthwiseCircBAN if circular else heads.DepthwiseBAN)(16, 16, 2).to(dev).train()
    z, x, wc, wl = seeded_inputs(circular, dev, BC.SEED + 60 + circular)
    g64, g32 = (twin_grads(box, circular, z, x, wc, wl, dt) for dt in (torch.float64, torch.float32))
    cls, loc = box(z, x)
    assert cls.grad_fn is not None and loc.grad_fn is not None
    ((cls * wc).sum() + (loc * wl).sum()).backward()
    got = {n: p.grad for n, p in box.named_parameters()}
    got["z"], got["x"] = z.grad, x.grad
    assert_inside_conv_bound("DepthwiseCircBAN" if circular else "DepthwiseBAN", got, g64, g32)


def test_training_step_through_install_on_a_stand_in_head_module(dev):
    """A stand-in hdn.models.head.ban whose DepthwiseXCorr resolves the module-level xcorr_depthwise at call time (ban.py:76) and whose MultiBAN has a
    forward of its own: after install() a .train() forward + backward leaves a gradient on conv_kernel / conv_search (upstream of the correlation)
    inside the bound of the module test."""
    import hdn_amd.install as hinstall
    from hdn_amd import heads, xcorr as X
    ban = types.ModuleType("hdn.models.head.ban")

    def cpu_only(x, kernel):
        raise AssertionError("the stand-in's own xcorr_depthwise was called: install() did not rebind it")

    ban.xcorr_depthwise = cpu_only

    class DepthwiseXCorr(heads.DepthwiseXCorr):
        def forward(self, kernel, search):
            return self.head(ban.xcorr_depthwise(self.conv_search(search), self.conv_kernel(kernel)))

    class DepthwiseBAN(heads.DepthwiseBAN):
        _xcorr = DepthwiseXCorr

    class MultiBAN(nn.Module):
        def __init__(self):
            super().__init__()
            self.box2 = DepthwiseBAN(16, 16, 2)

        def forward(self, z_fs, x_fs):
            return self.box2(z_fs[0], x_fs[0])

    ban.MultiBAN = MultiBAN
    torch.manual_seed(BC.SEED + 7)
    m = MultiBAN().to(dev).train()
    z, x, wc, wl = seeded_inputs(False, dev, BC.SEED + 70)
    g64, g32 = (twin_grads(m.box2, False, z, x, wc, wl, dt) for dt in (torch.float64, torch.float32))
    hinstall.install(modules={"hdn.models.head.ban": ban})
    try:
        assert ban.xcorr_depthwise is X.xcorr_depthwise and "_hdn_orig_forward" in MultiBAN.__dict__
        cls, loc = m([z], [x])
        ((cls * wc).sum() + (loc * wl).sum()).backward()
    finally:
        hinstall.uninstall()
    assert ban.xcorr_depthwise is cpu_only
    upstream = m.box2.cls.conv_kernel[0].weight
    assert upstream.grad is not None and float(upstream.grad.abs().max()) > 0
    got = {n: p.grad for n, p in m.box2.named_parameters()}
    got["z"], got["x"] = z.grad, x.grad
    assert_inside_conv_bound("install() stand-in MultiBAN", got, g64, g32)
