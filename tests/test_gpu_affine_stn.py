"""The affine spatial transformer on the device (csrc/affine_stn.hip through its entry points, hdn_amd.affine and the autograd Function behind
stn_with_theta) against tests/affine_stn_cases.py: the forward bit-equal to the numpy restatement of the kernel's own statements; out, grad_theta and
grad_img inside K M of the float64 closed form, K = max(4 r_ref, 2e-6) with r_ref of PyTorch's own fp32 CPU path on the same fixture; guarded
(1e30 / NaN / inf) samples exactly 0 and the rest of their batch unchanged; every requested-output combination, raw and through autograd; grad_theta bit
for bit between calls and batch sizes; 0xA5 padding around misaligned outputs intact; non-contiguous inputs; and end to end through
install(train=True) on a stand-in ModelBuilder.  The host side is tests/test_affine_stn_host.py."""
import types

import pytest
import torch
import torch.nn.functional as F

import affine_stn_cases as AC
import geometry_bwd_cases as GC

pytestmark = pytest.mark.gpu
MISALIGNED = GC.OFFSETS[1]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def assert_inside(what, got, pair, K):
    truth, M = pair
    r = GC.worst_ratio(got, truth, M)
    print(f"FORMS affine stn {what}: worst |hip - f64| / M = {r:.3e} (K = {K:.3e})")
    assert not bool(got.isnan().any()) and r <= K, (what, r, K)
    return r


# ------------------------------------------------------------------------------------------------------------------------------ 1. bounds
@pytest.mark.parametrize("kind", AC.KINDS)
@pytest.mark.parametrize("shape", AC.SHAPES, ids=str)
def test_forward_and_backward_inside_the_bound(dev, shape, kind):
    """Every shape and theta kind, the base pointers aligned and at float offsets (1, 2, 3, 1, 2), outputs from NaN inside 0xA5 margins: the forward
    bit-equal to the restated kernel, everything inside K M, nothing written outside the outputs (so the zero-fill of grad_img covers exactly it)."""
    B, C, H, W, Ho, Wo = shape
    x, theta, g, truth = AC.problem(kind, shape)
    r = AC.r_ref(kind, shape)
    print(f"FORMS affine stn {kind} {shape} r_ref: out {r['out']:.3e}, grad_theta {r['theta']:.3e}, grad_img {r['img']:.3e}")
    want = AC.kernel_forward_np(x, theta, Ho, Wo)
    for off in GC.OFFSETS:
        out, clean = AC.run_forward(x, theta, Ho, Wo, dev, off)
        assert clean, f"the forward wrote outside out at offsets {off}"
        assert GC.first_difference(out, want.double()) is None, (off, GC.first_difference(out, want.double()))
        gt, gx, clean = AC.run_backward(x, theta, g, dev, off)
        assert clean, f"the backward wrote outside its outputs at offsets {off}"
        assert_inside(f"{kind} {shape} out", out, truth["out"], GC.k_bound(r["out"]))
        assert_inside(f"{kind} {shape} grad_theta", gt, truth["theta"], GC.k_bound(r["theta"]))
        assert_inside(f"{kind} {shape} grad_img", gx, truth["img"], GC.k_bound(r["img"]))


# ------------------------------------------------------------------------------------------------------------------------------ 2. the guard
@pytest.mark.parametrize("how", ["shift", "nan", "inf"])
@pytest.mark.parametrize("shape", [AC.SHAPES[0], AC.SHAPES[1], AC.SHAPES[4]], ids=str)
def test_a_guarded_sample_is_zero_and_leaves_its_batch_alone(dev, shape, how):
    """One sample of the batch with a shift of 1e30, NaN entries or inf entries: its out, grad_theta and grad_img are exactly 0; the other samples'
    out and grad_theta are bit-equal to the same batch without it, their grad_img (fp32 atomics, three or more colliding taps in no fixed order) equal
    within 1e-5 of its largest value."""
    B, C, H, W, Ho, Wo = shape
    x, theta, g, _ = AC.problem("similarity", shape)
    out0, _ = AC.run_forward(x, theta, Ho, Wo, dev)
    gt0, gx0, _ = AC.run_backward(x, theta, g, dev)
    for b in (0, B - 1):
        bad = AC.poisoned(theta, b, how)
        out, clean = AC.run_forward(x, bad, Ho, Wo, dev, MISALIGNED)
        gt, gx, clean2 = AC.run_backward(x, bad, g, dev, MISALIGNED)
        assert clean and clean2
        assert bool((out[b] == 0).all()) and bool((gt[b] == 0).all()) and bool((gx[b] == 0).all()), (how, b)
        for o in range(B):
            if o != b:
                assert torch.equal(out[o], out0[o]) and torch.equal(gt[o], gt0[o]), (how, b, o)
                assert float((gx[o] - gx0[o]).abs().max()) <= 1e-5 * float(gx0.abs().max())
        only_t, none_x, clean = AC.run_backward(x, bad, g, dev, MISALIGNED, need_x=False)
        assert clean and none_x is None and torch.equal(only_t, gt)


# ------------------------------------------------------------------------------------------------------------------------------ 3. requested outputs, determinism
@pytest.mark.parametrize("shape", [AC.SHAPES[0], AC.SHAPES[4], AC.LARGE_SHAPE], ids=str)
def test_requested_outputs_and_determinism(dev, shape):
    """grad_theta: two calls bit-equal, sample b of the batch bit-equal to that sample run alone, and asked for alone bit-equal to the joint call
    while the other buffer (0xA5 everywhere) stays untouched; grad_img asked for alone: the same sum (atomics), grad_theta's buffer untouched."""
    x, theta, g, _ = AC.problem("classes", shape)
    B = shape[0]
    a_t, a_x, clean = AC.run_backward(x, theta, g, dev, MISALIGNED)
    assert clean
    b_t, _, _ = AC.run_backward(x, theta, g, dev)
    assert torch.equal(a_t, b_t)
    for b in range(B):
        alone = AC.run_backward(x[b:b + 1], theta[b:b + 1], g[b:b + 1], dev)[0]
        assert torch.equal(alone[0], a_t[b]), b
    o_t, none_x, clean = AC.run_backward(x, theta, g, dev, MISALIGNED, need_x=False)
    assert none_x is None and clean and torch.equal(o_t, a_t)
    none_t, o_x, clean = AC.run_backward(x, theta, g, dev, MISALIGNED, need_theta=False)
    assert none_t is None and clean and not bool(o_x.isnan().any())
    assert float((o_x - a_x).abs().max()) <= 1e-5 * float(a_x.abs().max())


# ------------------------------------------------------------------------------------------------------------------------------ 4. Python layer
def test_autograd_in_every_needs_input_grad_combination(dev):
    import hdn_amd
    from hdn_amd import affine
    shape = AC.SHAPES[0]
    B, C, H, W, Ho, Wo = shape
    x, theta, g, _ = AC.problem("similarity", shape)
    xd, td, gd = x.to(dev), theta.to(dev), g.to(dev)
    size = torch.Size([B, 1, Ho, Wo])                                                          # the reference passes one channel for a 3-channel image
    with torch.no_grad():
        y0 = hdn_amd.affine_sample(xd, td.clone().requires_grad_(True), size)
    y1 = hdn_amd.affine_sample(xd, td, size, differentiable=True)                              # plain inputs: no graph either
    assert y0.grad_fn is None and y1.grad_fn is None and torch.equal(y0, y1) and y0.shape == (B, C, Ho, Wo)
    assert torch.equal(y0.cpu(), AC.kernel_forward_np(x, theta, Ho, Wo))
    with pytest.raises(RuntimeError, match="inference-only.*uninstall"):
        hdn_amd.affine_sample(xd, td.clone().requires_grad_(True), size)
    with pytest.raises(TypeError):
        hdn_amd.affine_sample(xd.double(), td.double(), size)                                  # fp32 only
    want_x, want_t = hdn_amd.affine_sample_backward(xd, td, size, gd)
    assert want_t.shape == (B, 2, 3) and want_x.shape == xd.shape
    only = hdn_amd.affine_sample_backward(xd, td, size, gd, need_x=False)
    assert only[0] is None and torch.equal(only[1], want_t)
    only = hdn_amd.affine_sample_backward(xd, td, size, gd, need_theta=False)
    assert only[1] is None and float((only[0] - want_x).abs().max()) <= 1e-5 * float(want_x.abs().max())
    for need_x, need_t in ((True, True), (False, True), (True, False)):
        xr, tr = xd.clone().requires_grad_(need_x), td.clone().requires_grad_(need_t)
        y = affine.stn_with_theta(None, xr, tr, size)
        assert y.grad_fn is not None and torch.equal(y.detach(), y0)
        y.backward(gd)
        assert (xr.grad is not None) == need_x and (tr.grad is not None) == need_t
        if need_t:
            assert torch.equal(tr.grad, want_t)
        if need_x:
            assert float((xr.grad - want_x).abs().max()) <= 1e-5 * float(want_x.abs().max())
    tr = td.clone().requires_grad_(True)                                                       # first order only
    (gt,) = torch.autograd.grad(hdn_amd.affine_sample(xd, tr, size, differentiable=True).sum(), tr, create_graph=True)
    with pytest.raises(RuntimeError):
        gt.sum().backward()


def test_non_contiguous_inputs(dev):
    """grad_out expanded (stride 0) and permuted, theta as [B,6] and as a non-contiguous slice that .view(-1, 2, 3) accepts, x a channel slice."""
    import hdn_amd
    shape = AC.SHAPES[4]
    B, C, H, W, Ho, Wo = shape
    x, theta, g, _ = AC.problem("similarity", shape)
    xd, td, gd = x.to(dev), theta.to(dev), g.to(dev)
    size = (B, C, Ho, Wo)
    want_x, want_t = hdn_amd.affine_sample_backward(xd, td, size, gd)
    g_perm = gd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)                           # the same values, NHWC strides
    assert not g_perm.is_contiguous()
    tr = td.reshape(B, 6).clone().requires_grad_(True)                                         # theta as [B,6]
    hdn_amd.affine_sample(xd, tr, size, differentiable=True).backward(g_perm)
    assert torch.equal(tr.grad.reshape(B, 2, 3), want_t)
    wide = torch.zeros(B, 8, device=dev)
    wide[:, :6] = td.reshape(B, 6)
    leaf = wide.requires_grad_(True)
    sl = leaf[:, :6]                                                                           # row stride 8: not contiguous, but .view(-1, 2, 3) takes it
    assert not sl.is_contiguous()
    y = hdn_amd.affine_sample(xd, sl, size, differentiable=True)
    y.backward(g_perm)
    assert torch.equal(leaf.grad[:, :6].reshape(B, 2, 3), want_t) and bool((leaf.grad[:, 6:] == 0).all())
    tr = td.clone().requires_grad_(True)                                                       # an expanded grad_out: sum() backward has stride 0
    hdn_amd.affine_sample(xd, tr, size, differentiable=True).sum().backward()
    ones = hdn_amd.affine_sample_backward(xd, td, size, torch.ones(B, C, Ho, Wo, device=dev), need_x=False)[1]
    assert torch.equal(tr.grad, ones)
    big = torch.randn(B, C + 2, H, W, device=dev)                                              # a non-contiguous image
    big[:, 1:C + 1] = xd
    assert torch.equal(hdn_amd.affine_sample(big[:, 1:C + 1], td, size), hdn_amd.affine_sample(xd, td, size))


# ------------------------------------------------------------------------------------------------------------------------------ 5. end to end
class Builder:
    """A stand-in ModelBuilder: the reference's three-line stn_with_theta (restated) and the pattern of its training step's three calls
    (model_builder_e2e_unconstrained_v2.py:407, :408, :418), each followed by the channel mean the reference takes."""

    def stn_with_theta(self, x, theta, size):
        theta = theta.view(-1, 2, 3)
        grid = F.affine_grid(theta, size)
        x = F.grid_sample(x, grid)
        return x

    def step(self, search_hm, search_window, affine_m, affine_aug, size, gs):
        a = self.stn_with_theta(search_hm, affine_m, size).mean(1, keepdim=True)
        b = self.stn_with_theta(search_hm, affine_aug, size).mean(1, keepdim=True)
        c = self.stn_with_theta(search_window, affine_m, size)
        return (a * gs[0]).sum() + (b * gs[1]).sum() + (c * gs[2]).sum()


def test_the_steps_three_calls_through_install_train(dev, monkeypatch):
    """install(modules=..., train=True) with AFFINE_STN_TRAIN_BOUND on rebinds the class's method; a scalar loss over the step's three calls (two
    images, two thetas, one theta shared by two calls and requiring grad, built from a [B,6] leaf) gives that leaf a gradient inside K M of float64:
    the loss is linear in the three outputs, so truth and M are the sums of the two calls' closed forms, and r_ref is PyTorch's fp32 CPU autograd of the
    same loss.  After uninstall() the class attribute is the original object."""
    import hdn_amd.install as hinstall
    from hdn_amd import affine
    shape = AC.SHAPES[4]
    B, C, H, W, Ho, Wo = shape
    hm, theta, _, _ = AC.problem("similarity", shape)
    aug = AC.make_theta("classes", shape)
    gen = torch.Generator().manual_seed(AC.SEED + 5)
    window = torch.randn(B, 1, H, W, generator=gen)
    gs = [torch.randn(B, 1, Ho, Wo, generator=gen) for _ in range(3)]
    size = torch.Size([B, 1, Ho, Wo])
    t0 = AC.closed(hm, theta, Ho, Wo, (gs[0] / C).expand(B, C, Ho, Wo))["theta"]
    t2 = AC.closed(window, theta, Ho, Wo, gs[2])["theta"]
    truth, M = (t0[0] + t2[0]).reshape(B, 6), (t0[1] + t2[1]).reshape(B, 6)
    leaf32 = theta.reshape(B, 6).clone().requires_grad_(True)
    Builder().step(hm, window, leaf32, aug, size, gs).backward()                               # PyTorch's own fp32 CPU path
    r = GC.worst_ratio(leaf32.grad, truth, M)
    leaf64 = theta.reshape(B, 6).double().requires_grad_(True)
    Builder().step(hm.double(), window.double(), leaf64, aug.double(), size, [t.double() for t in gs]).backward()
    assert GC.worst_ratio(leaf64.grad, truth, M) <= 1e-12
    print(f"FORMS affine stn step r_ref: {r:.3e}")

    mb = types.ModuleType("hdn.models.model_builder_e2e_unconstrained_v2")
    mb.ModelBuilder = Builder
    orig = Builder.__dict__["stn_with_theta"]
    monkeypatch.setattr(hinstall, "AFFINE_STN_TRAIN_BOUND", True)
    done = hinstall.install(modules={mb.__name__: mb}, train=True)
    try:
        assert Builder.__dict__["stn_with_theta"] is affine.stn_with_theta and (mb.__name__, "ModelBuilder.stn_with_theta") in done
        leaf = theta.reshape(B, 6).to(dev).requires_grad_(True)
        loss = Builder().step(hm.to(dev), window.to(dev), leaf, aug.to(dev), size, [t.to(dev) for t in gs])
        loss.backward()
    finally:
        hinstall.uninstall()
    assert Builder.__dict__["stn_with_theta"] is orig
    assert leaf.grad is not None and leaf.grad.shape == (B, 6)
    assert_inside("step grad of the shared theta", leaf.grad.cpu(), (truth, M), GC.k_bound(r))
