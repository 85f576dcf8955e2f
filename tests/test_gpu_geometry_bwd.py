"""The backward of the log-polar sampler, the DLT solve and the projective warp on the device (csrc/geometry_bwd.hip through its three entry points, the
*_backward wrappers and the autograd Functions behind STN_PolarTrain, DLT_solve, transformer and transform) against the float64 closed forms of
tests/geometry_bwd_cases.py: exactly on dyadic fixtures, at the block and tail edges, inside K M on random data, bit for bit between calls, batch sizes
and requested outputs, through autograd, and end to end through install(train=True) on stand-ins of the reference's two training branches.  The host
side is tests/test_geometry_bwd_host.py."""
import copy
import types

import pytest
import torch
import torch.nn as nn

import geometry_bwd_cases as GC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def assert_inside(what, got, truth, M, K):
    r = GC.worst_ratio(got, truth, M)
    print(f"FORMS geometry backward {what}: worst |hip - f64| / M = {r:.3e} (K = {K:.3e})")
    assert not bool(got.isnan().any()) and r <= K, (what, r, K)
    return r


# ------------------------------------------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("i", range(len(GC.WARP_EXACT)))
def test_warp_exact_fixtures(dev, i):
    """Integer image and grad_out, dyadic affine theta, W, H in {5, 9, 17}: grad_theta and grad_img torch.equal to float64, from buffers that held
    NaN inside 0xA5 margins, the base pointers aligned and at float offsets (1, 2, 3, 1, 2)."""
    U, theta, g, gth, gU = GC.warp_exact_problem(i)
    for off in GC.OFFSETS:
        got_t, got_U, clean = GC.run_warp(U, theta, g, dev, off)
        assert GC.first_difference(got_t, gth) is None, ("grad_theta", off, GC.first_difference(got_t, gth))
        assert GC.first_difference(got_U, gU) is None, ("grad_img", off, GC.first_difference(got_U, gU))
        assert clean, f"a write outside the outputs at offsets {off}"


@pytest.mark.parametrize("i", range(len(GC.LOGPOLAR_EXACT)))
def test_sampler_exact_fixtures(dev, i):
    """Dyadic tables and origins that push samples past the borders (zero-derivative rule, masked taps), H != W in two fixtures: the raw entry point
    and hdn_amd.logpolar.logpolar_sample with the test's own tables under autograd, both torch.equal to float64."""
    from hdn_amd import logpolar
    x, polar, tabs, g, gp, gx = GC.logpolar_exact_problem(i)
    for off in GC.OFFSETS:
        got_p, got_x, clean = GC.run_logpolar(x, polar, tabs, g, dev, off)
        assert GC.first_difference(got_p, gp) is None, ("grad_polar", off, GC.first_difference(got_p, gp))
        assert GC.first_difference(got_x, gx) is None, ("grad_x", off, GC.first_difference(got_x, gx))
        assert clean, f"a write outside the outputs at offsets {off}"
    xd, pd = x.to(dev).requires_grad_(True), polar.to(dev).requires_grad_(True)
    out, grid = logpolar.logpolar_sample(xd, pd, tuple(t.to(dev) for t in tabs), differentiable=True)
    assert torch.equal(out.detach().cpu().double(), GC.logpolar_rs(x.double(), polar.double(), tabs))
    out.backward(g.to(dev))
    assert GC.first_difference(pd.grad.cpu(), gp) is None and GC.first_difference(xd.grad.cpu(), gx) is None


# ------------------------------------------------------------------------------------------------------------------------------ 2. edges
WARP_EDGES = ((2, 2, 5, 9), (2, 2, 31, 33), (2, 2, 32, 32), (2, 2, 25, 41), (2, 1, 127, 127))     # B, C, H, W: 45, 1023, 1024, 1025 pixels; 16 blocks


@pytest.mark.parametrize("B,C,H,W", WARP_EDGES, ids=lambda v: str(v))
def test_warp_block_and_tail_edges(dev, B, C, H, W):
    """One pixel either side of the 1024-pixel block and the production plane, random data: inside K M of the float64 closed form on the cells the
    fp32 forward reads, K = max(4 r_ref, 2e-6) with r_ref measured at the same shape; NaN nowhere, nothing written outside."""
    U, theta, g, gth, Mth, gU, MU = GC.warp_random_problem(B, C, H, W, cells32=True)
    got_t, got_U, clean = GC.run_warp(U, theta, g, dev, (1, 2, 3, 1, 2))
    assert clean
    rt, rU = GC.warp_r_ref(B, C, H, W, True)                                     # the reference formulation's fp32 CPU autograd at this shape
    print(f"FORMS geometry backward warp {H}x{W} r_ref: grad_theta {rt:.3e}, grad_img {rU:.3e}")
    assert_inside(f"warp {H}x{W} grad_theta", got_t, gth, Mth, GC.k_bound(rt))
    assert_inside(f"warp {H}x{W} grad_img", got_U, gU, MU, GC.k_bound(rU))


SAMPLER_EDGES = tuple((2, 2, H, W, S) for (H, W) in ((31, 31), (24, 37)) for S in (15, 16, 17)) + ((1, 3, 255, 255, 127), (1, 3, 127, 127, 127))


@pytest.mark.parametrize("B,C,H,W,S", SAMPLER_EDGES, ids=lambda v: str(v))
def test_sampler_block_and_tail_edges(dev, B, C, H, W, S):
    """S * S = 225 (less than a block), 256, 289 on a square and an oblong crop, and S = 127 on the 255 x 255 search crop and on update_template's
    127 x 127 crop: inside K M of the float64 closed form on the cells the fp32 forward reads, K = max(4 r_ref, 2e-6) with r_ref at the same shape."""
    x, polar, tabs, g, gp, Mp, gx, Mx = GC.logpolar_random_problem(B, C, H, W, S, cells32=True)
    got_p, got_x, clean = GC.run_logpolar(x, polar, tabs, g, dev, (1, 2, 3, 1, 2))
    assert clean
    rp, rx = GC.logpolar_r_ref(B, C, H, W, S, True)                               # the reference formulation's fp32 CPU autograd at this shape
    print(f"FORMS geometry backward sampler S={S} on {H}x{W} r_ref: grad_polar {rp:.3e}, grad_x {rx:.3e}")
    assert_inside(f"sampler S={S} on {H}x{W} grad_polar", got_p, gp, Mp, GC.k_bound(rp))
    assert_inside(f"sampler S={S} on {H}x{W} grad_x", got_x, gx, Mx, GC.k_bound(rx))


def test_sampler_broadcast_origin_gives_the_batch_sum(dev):
    """polar [1,2] with B = 3: the gradient is the sum over the batch of the per-sample gradients (autograd sums the expand back)."""
    from hdn_amd import logpolar
    x, polar, tabs, g = GC.logpolar_random_problem(3, 2, 24, 37, 16)[:4]
    td = tuple(t.to(dev) for t in tabs)
    p1 = polar[:1].to(dev).requires_grad_(True)
    out, _ = logpolar.logpolar_sample(x.to(dev), p1, td, differentiable=True)
    out.backward(g.to(dev))
    _, each = logpolar.logpolar_sample_backward(x.to(dev), polar[:1].expand(3, 2).to(dev), td, g.to(dev), need_x=False)
    assert p1.grad.shape == (1, 2) and torch.equal(p1.grad, each.sum(0, keepdim=True))
    gp, Mp = GC.logpolar_closed(x, polar[:1].expand(3, 2), tabs, g)[:2]
    assert_inside("sampler broadcast origin", p1.grad.cpu(), gp.sum(0, keepdim=True), Mp.sum(0, keepdim=True), GC.k_bound(GC.logpolar_r_ref()[0]))


# ------------------------------------------------------------------------------------------------------------------------------ 3. bounds
def test_warp_random_data_inside_the_bound(dev):
    """The 11 x 13 bound fixture (theta = I + 0.08 N(0,1); no coordinate within 1e-4 of an integer): |hip - f64| <= K M, K = max(4 r_ref, 2e-6)."""
    U, theta, g, gth, Mth, gU, MU = GC.warp_random_problem(**GC.WARP_BOUND)
    got_t, got_U, clean = GC.run_warp(U, theta, g, dev)
    rt, rU = GC.warp_r_ref()
    print(f"FORMS geometry backward warp r_ref: grad_theta {rt:.3e}, grad_img {rU:.3e}")
    assert clean
    assert_inside("warp bound fixture grad_theta", got_t, gth, Mth, GC.k_bound(rt))
    assert_inside("warp bound fixture grad_img", got_U, gU, MU, GC.k_bound(rU))


def test_sampler_random_data_inside_the_bound(dev):
    x, polar, tabs, g, gp, Mp, gx, Mx = GC.logpolar_random_problem(**GC.LOGPOLAR_BOUND)
    got_p, got_x, clean = GC.run_logpolar(x, polar, tabs, g, dev)
    rp, rx = GC.logpolar_r_ref()
    print(f"FORMS geometry backward sampler r_ref: grad_polar {rp:.3e}, grad_x {rx:.3e}")
    assert clean
    assert_inside("sampler bound fixture grad_polar", got_p, gp, Mp, GC.k_bound(rp))
    assert_inside("sampler bound fixture grad_x", got_x, gx, Mx, GC.k_bound(rx))


@pytest.mark.parametrize("kind", sorted(GC.DLT_CORNERS))
def test_dlt_inside_one_fp32_rounding(dev, kind):
    """Production corners and a skewed quad, offsets uniform in +-32, B = 1, 7, 8, 9, 65 (either side of the 8-lane group and of the wave):
    |hip - f64| <= 2^-23 |truth| + 2^-23 max|truth| per sample, for grad_src and grad_off."""
    worst = 0.0
    for B in GC.DLT_BATCHES:
        src, off, gH, gs, go = GC.dlt_problem(kind, B)
        got_s, got_o, clean = GC.run_dlt(src, off, gH, dev, (1, 2, 3, 1, 2))
        assert clean
        for name, got, truth in (("grad_src", got_s, gs), ("grad_off", got_o, go)):
            excess, ratio = GC.dlt_excess(got, truth)
            worst = max(worst, ratio)
            assert not bool(got.isnan().any()) and excess <= 0, (kind, B, name, excess, ratio)
    print(f"FORMS geometry backward DLT {kind}: worst |hip - f64| / (2^-23 |t| + 2^-23 max|t|) = {worst:.4f}")


# ------------------------------------------------------------------------------------------------------------------------------ 4. determinism
def test_deterministic_outputs_are_bit_equal(dev):
    """grad_theta, grad_polar, grad_src, grad_off: two calls are bit-equal, sample b of a batch equals that sample run alone, and one gradient asked
    for alone has the bits of the joint call while the other buffer (0xA5 everywhere) stays untouched."""
    U, theta, g = GC.warp_random_problem(3, 2, 31, 33, cells32=True)[:3]
    a_t, a_U, _ = GC.run_warp(U, theta, g, dev, (1, 2, 3, 1, 2))
    b_t, _, _ = GC.run_warp(U, theta, g, dev)
    assert torch.equal(a_t, b_t)
    for b in range(3):
        assert torch.equal(GC.run_warp(U[b:b + 1], theta[b:b + 1], g[b:b + 1], dev)[0][0], a_t[b]), b
    o_t, none_U, clean = GC.run_warp(U, theta, g, dev, (1, 2, 3, 1, 2), need_U=False)
    assert none_U is None and clean and torch.equal(o_t, a_t)
    none_t, o_U, clean = GC.run_warp(U, theta, g, dev, (1, 2, 3, 1, 2), need_theta=False)
    assert none_t is None and clean and not bool(o_U.isnan().any())
    assert float((o_U - a_U).abs().max()) <= 1e-5 * float(a_U.abs().max())        # atomics: not bit-reproducible, the same sum

    x, polar, tabs, g = GC.logpolar_random_problem(3, 2, 24, 37, 17, cells32=True)[:4]
    a_p, a_x, _ = GC.run_logpolar(x, polar, tabs, g, dev, (1, 2, 3, 1, 2))
    assert torch.equal(a_p, GC.run_logpolar(x, polar, tabs, g, dev)[0])
    for b in range(3):
        assert torch.equal(GC.run_logpolar(x[b:b + 1], polar[b:b + 1], tabs, g[b:b + 1], dev)[0][0], a_p[b]), b
    o_p, none_x, clean = GC.run_logpolar(x, polar, tabs, g, dev, (1, 2, 3, 1, 2), need_x=False)
    assert none_x is None and clean and torch.equal(o_p, a_p)
    none_p, o_x, clean = GC.run_logpolar(x, polar, tabs, g, dev, (1, 2, 3, 1, 2), need_polar=False)
    assert none_p is None and clean and float((o_x - a_x).abs().max()) <= 1e-5 * float(a_x.abs().max())

    src, off, gH = GC.dlt_problem("skewed", 9)[:3]
    a_s, a_o, _ = GC.run_dlt(src, off, gH, dev, (1, 2, 3, 1, 2))
    b_s, b_o, _ = GC.run_dlt(src, off, gH, dev)
    assert torch.equal(a_s, b_s) and torch.equal(a_o, b_o)
    for b in range(9):
        p_s, p_o, _ = GC.run_dlt(src[b:b + 1], off[b:b + 1], gH[b:b + 1], dev)
        assert torch.equal(p_s[0], a_s[b]) and torch.equal(p_o[0], a_o[b]), b
    o_s, none_o, clean = GC.run_dlt(src, off, gH, dev, (1, 2, 3, 1, 2), need_off=False)
    assert none_o is None and clean and torch.equal(o_s, a_s)
    none_s, o_o, clean = GC.run_dlt(src, off, gH, dev, (1, 2, 3, 1, 2), need_src=False)
    assert none_s is None and clean and torch.equal(o_o, a_o)


# ------------------------------------------------------------------------------------------------------------------------------ 5. autograd
def test_autograd_through_dlt_solve_and_transformer(dev):
    from hdn_amd import homography as HG
    src, off, gH = (t.to(dev) for t in GC.dlt_problem("production", 7)[:3])
    with torch.no_grad():
        H0 = HG.DLT_solve(src.clone().requires_grad_(True), off)
    H1 = HG.DLT_solve(src, off)
    assert H0.grad_fn is None and H1.grad_fn is None and not H1.requires_grad and torch.equal(H0, H1) and H0.shape == (7, 1, 3, 3)
    want_s, want_o = HG.dlt_solve_backward(src, off, gH)
    s, o = src.clone().requires_grad_(True), off.clone().requires_grad_(True)
    H = HG.DLT_solve(s, o)
    assert H.grad_fn is not None and torch.equal(H.detach(), H0)
    H.backward(gH.view(7, 1, 3, 3))
    assert torch.equal(s.grad, want_s) and torch.equal(o.grad, want_o)
    o = off.clone().requires_grad_(True)                                         # the reference's case: only the regressor's output needs grad
    HG.DLT_solve(src, o).backward(gH.view(7, 1, 3, 3))
    assert torch.equal(o.grad, want_o)
    assert HG.dlt_solve_backward(src, off, gH, need_src=False)[0] is None
    (go,) = torch.autograd.grad(HG.DLT_solve(src, o).sum(), o, create_graph=True)
    with pytest.raises(RuntimeError):
        go.sum().backward()

    U, theta, g = (t.to(dev) for t in GC.warp_random_problem(**GC.WARP_BOUND)[:3])
    Hh, Ww = U.shape[2:]
    with torch.no_grad():
        y0, c0 = HG.transformer(U, theta.clone().requires_grad_(True), (Hh, Ww))
    y1, c1 = HG.transformer(U, theta.view(-1, 3, 3), (Hh, Ww))
    assert y0.grad_fn is None and y1.grad_fn is None and torch.equal(y0, y1) and torch.equal(c0, c1)
    want_U, want_t = HG.transformer_backward(U, theta, g)
    Ur, tr = U.clone().requires_grad_(True), theta.clone().view(-1, 3, 3).requires_grad_(True)
    y, cond = HG.transformer(Ur, tr, (Hh, Ww))
    assert y.grad_fn is not None and torch.equal(y.detach(), y0) and not cond.requires_grad and torch.equal(cond, c0)
    y.backward(g)
    assert torch.equal(tr.grad, want_t.view(-1, 3, 3)) and tr.grad.shape == (U.shape[0], 3, 3)
    assert float((Ur.grad - want_U).abs().max()) <= 1e-5 * float(want_U.abs().max())
    tr = theta.clone().requires_grad_(True)                                      # theta alone, a permuted and a stride-0 grad_out
    y, none_c = HG.transformer(U, tr, (Hh, Ww), want_condition=False)
    assert none_c is None
    y.backward(g.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1))
    assert torch.equal(tr.grad, want_t)
    tr = theta.clone().requires_grad_(True)
    HG.transformer(U, tr, (Hh, Ww))[0].sum().backward()
    assert torch.equal(tr.grad, HG.transformer_backward(U, theta, torch.ones_like(y0), need_U=False)[1])
    (gt,) = torch.autograd.grad(HG.transformer(U, tr, (Hh, Ww))[0].sum(), tr, create_graph=True)
    with pytest.raises(RuntimeError):
        gt.sum().backward()
    with pytest.raises(ValueError):
        HG.transformer_backward(U, theta, g[:, 1:])


def test_autograd_through_the_sampler_module(dev):
    import hdn_amd
    x, polar, tabs, g = (GC.logpolar_random_problem(**GC.LOGPOLAR_BOUND)[i] for i in range(4))
    xd, pd, gd = x.to(dev), polar.to(dev), g.to(dev)
    plain, train = hdn_amd.STN_Polar(30), hdn_amd.STN_PolarTrain(30)
    with torch.no_grad():
        y0, grid0 = plain(xd, pd.clone().requires_grad_(True))
    y1, grid1 = train(xd, pd)                                                    # plain inputs: no graph either
    assert y0.grad_fn is None and y1.grad_fn is None and torch.equal(y0, y1) and torch.equal(grid0, grid1)
    with pytest.raises(RuntimeError, match="inference-only.*uninstall"):
        plain(xd, pd.clone().requires_grad_(True))
    td = plain._tables(dev, 0.0)
    want_x, want_p = hdn_amd.logpolar_sample_backward(xd, pd, td, gd)
    for mod in (train, plain):
        mod.differentiable = True                                                # the attribute switch on a built module
        xr, pr = xd.clone().requires_grad_(True), pd.clone().requires_grad_(True)
        y, grid = mod(xr, pr)
        assert y.grad_fn is not None and torch.equal(y.detach(), y0) and torch.equal(grid, grid0) and not grid.requires_grad
        y.backward(gd)
        assert torch.equal(pr.grad, want_p) and float((xr.grad - want_x).abs().max()) <= 1e-5 * float(want_x.abs().max())
    pr = pd.clone().requires_grad_(True)
    (gp,) = torch.autograd.grad(train(xd, pr)[0].sum(), pr, create_graph=True)
    with pytest.raises(RuntimeError):
        gp.sum().backward()


# ------------------------------------------------------------------------------------------------------------------------------ 6. end to end
def assert_chain_bound(what, got, g64, g32):
    """Every parameter's gradient within max(4 d_ref, 1e-5) max|grad| of the float64 twin's; d_ref: the fp32 CPU twin's deviation over max|grad|."""
    assert set(got) == set(g64) == set(g32)
    for name in sorted(got):
        assert got[name] is not None, f"{what}: {name} received no gradient"
        t = g64[name]
        scale = float(t.abs().max())
        d_ref = float((g32[name].double() - t).abs().max()) / scale
        d = float((got[name].detach().cpu().double() - t).abs().max()) / scale
        print(f"FORMS geometry backward {what} {name}: d = {d:.3e}, d_ref = {d_ref:.3e}, bound {max(4 * d_ref, 1e-5):.3e}")
        assert d <= max(4 * d_ref, 1e-5), (what, name, d, d_ref)


class PolarBranch(nn.Module):
    """model_builder_e2e_unconstrained_v2.py:377-388 in small: a conv gives loc, polar is loc at the best cls position times the stride, the search
    crop goes through the sampler, a conv and an L1 loss follow."""

    def __init__(self, sampler):
        super().__init__()
        self.loc = nn.Conv2d(4, 2, 3, padding=1)
        self.logpolar_instance = sampler
        self.feat = nn.Conv2d(3, 2, 3)

    def forward(self, f, cls, search, target, sample=None):
        loc = self.loc(f)
        best = cls.flatten(1).argmax(1)
        polar = loc.flatten(2)[torch.arange(f.shape[0]), :, best] * 8.0
        x_lp = self.logpolar_instance(search, polar)[0] if sample is None else sample(search, polar)
        return (self.feat(x_lp) - target).abs().mean(), polar


def test_logpolar_branch_through_install_train(dev):
    import hdn_amd.install as hinstall
    lp = types.ModuleType("hdn.models.logpolar")
    lp.STN_Polar = type("Own", (), {})
    torch.manual_seed(GC.SEED + 61)
    f, cls, search = 0.3 * torch.randn(2, 4, 5, 5), torch.randn(2, 1, 5, 5), torch.randn(2, 3, 31, 29)
    target = torch.randn(2, 2, 13, 13)
    hinstall.install(modules={lp.__name__: lp}, train=True)
    try:
        m = PolarBranch(lp.STN_Polar(30))
        assert type(m.logpolar_instance).__name__ == "STN_PolarTrain"
        tabs = GC.real_tables(15)
        grads = {}
        for dt in (torch.float64, torch.float32):
            t = copy.deepcopy(m).to(dt)
            loss, polar = t(f.to(dt), cls, search.to(dt), target.to(dt), sample=lambda s, p: GC.logpolar_rs(s, p, tabs, dt))
            loss.backward()
            grads[dt] = {n: p.grad for n, p in t.named_parameters()}
            if dt is torch.float64:
                margin = GC.logpolar_margin(polar, tabs, 31, 29)
                print(f"FORMS geometry backward log-polar branch: coordinate margin of the twin {margin:.3e}")
                assert margin > GC.MARGIN
        m = m.to(dev)
        loss, _ = m(f.to(dev), cls.to(dev), search.to(dev), target.to(dev))
        loss.backward()
    finally:
        hinstall.uninstall()
    got = {n: p.grad for n, p in m.named_parameters()}
    assert float(got["loc.weight"].abs().max()) > 0
    assert_chain_bound("log-polar branch", got, grads[torch.float64], grads[torch.float32])


class HomoBranch(nn.Module):
    """homo_model_builder.py:154-197 in small: ShareFeature on both patches, a regressor (here one Linear) gives x, H = DLT_solve(h4p, x), the
    template image is warped by transform() and goes through ShareFeature, and the triplet loss compares the three feature maps."""

    def __init__(self, ns, hw, share):
        super().__init__()
        self.ns, self.hw = ns, hw
        self.ShareFeature = share
        self.fc = nn.Linear(2 * hw * hw, 8)
        nn.init.normal_(self.fc.weight, std=2e-3)
        nn.init.zeros_(self.fc.bias)

    def forward(self, org_imgs, input_tensors, h4p, patch_inds, identity_patch):
        B, _, H, W = org_imgs.shape
        ph, pw = input_tensors.shape[2:]
        dev = org_imgs.device
        batch_inds = torch.arange(0, B * H * W, H * W, device=dev).unsqueeze(1).expand(B, ph * pw).reshape(-1)
        M = torch.tensor([[W / 2.0, 0., W / 2.0], [0., H / 2.0, H / 2.0], [0., 0., 1.]], dtype=org_imgs.dtype, device=dev)
        M_tile, M_tile_inv = M.unsqueeze(0).expand(B, 3, 3), torch.inverse(M).unsqueeze(0).expand(B, 3, 3)
        patch_1 = self.ShareFeature(input_tensors[:, :1, ...])
        patch_2 = self.ShareFeature(input_tensors[:, 1:, ...])
        x = self.fc(torch.cat((patch_1, patch_2), dim=1).flatten(1))
        H_mat = self.ns.DLT_solve(h4p, x).squeeze(1)
        kw = {"assume_identity_patch": True} if identity_patch and self.ns.transform.__module__.startswith("hdn_amd") else {}
        pred_I2 = self.ns.transform(ph, pw, M_tile_inv, H_mat, M_tile, org_imgs[:, :1, ...], patch_inds, batch_inds, **kw)
        pred = self.ShareFeature(pred_I2)
        loss = nn.TripletMarginLoss(margin=1.0, p=1, reduction="none")(patch_2, pred, patch_1)
        return torch.sum(loss) / B / (H * W), x


def _twin_namespace(dt):
    """The float64 / fp32 CPU twin of the drop-ins, from the restatements of the cases module."""
    def transform(ph, pw, M_inv, H_mat, M, I1, pidx, base):
        B, C, H, W = I1.shape
        Hn = torch.matmul(torch.matmul(M_inv, H_mat), M)
        flat = GC.transformer_rs(I1, Hn.reshape(B, 9), dt).reshape(-1, C)
        return flat[pidx.reshape(-1).long() + base].reshape(B, ph, pw, C).permute(0, 3, 1, 2)
    return types.SimpleNamespace(DLT_solve=lambda s, o: GC.dlt_rs(s, o, dt).reshape(-1, 1, 3, 3), transform=transform)


HOMO_SEED = 66          # a seed at which the twin's warp coordinates keep GC.MARGIN on both paths (asserted below)


@pytest.mark.parametrize("path", ["full_patch", "gather"])
def test_homography_branch_through_install_train(dev, path):
    import hdn_amd
    import hdn_amd.install as hinstall
    utils = types.ModuleType("homo_estimator.Deep_homography.Oneline_DLTv1.models.homo_model_builder")
    utils.DLT_solve = utils.transform = None
    hw, B = 21, 2
    torch.manual_seed(GC.SEED + HOMO_SEED)
    share = hdn_amd.PreShareFeature().train()
    m = HomoBranch(None, hw, share).train()                                       # its namespace: the twins' restatements, then the stand-in module
    org, inp = torch.randn(B, 2, hw, hw), torch.randn(B, 2, hw, hw)
    h4p = torch.tensor([[0.0, 0.0, 0.0, hw, hw, hw, hw, 0.0]]).repeat(B, 1)
    if path == "full_patch":
        pidx = torch.arange(hw * hw, dtype=torch.float32).repeat(B, 1)
    else:                                                                         # a 15 x 15 patch at (3, 2) of the image
        ph = 15
        rows, cols = torch.arange(3, 3 + ph), torch.arange(2, 2 + ph)
        pidx = (rows.unsqueeze(1) * hw + cols.unsqueeze(0)).reshape(1, -1).float().repeat(B, 1)
        inp = inp[:, :, :ph, :ph].contiguous()
        m.fc = nn.Linear(2 * ph * ph, 8)
        nn.init.normal_(m.fc.weight, std=2e-3)
        nn.init.zeros_(m.fc.bias)
    grads = {}
    for dt in (torch.float64, torch.float32):
        t = copy.deepcopy(m).to(dt).train()
        t.ns = _twin_namespace(dt)
        loss, x = t(org.to(dt), inp.to(dt), h4p.to(dt), pidx, False)
        loss.backward()
        grads[dt] = {n: p.grad for n, p in t.named_parameters()}
        if dt is torch.float64:
            Hn = torch.matmul(torch.matmul(torch.inverse(torch.tensor([[hw / 2, 0, hw / 2], [0, hw / 2, hw / 2], [0, 0, 1.0]], dtype=dt)),
                                           GC.dlt_rs(h4p.to(dt), x.detach(), dt).reshape(B, 3, 3)),
                              torch.tensor([[hw / 2, 0, hw / 2], [0, hw / 2, hw / 2], [0, 0, 1.0]], dtype=dt))
            margin = GC.warp_margin(Hn.reshape(B, 9), B, hw, hw)
            print(f"FORMS geometry backward homography branch ({path}): coordinate margin of the twin {margin:.3e}, max |x| {float(x.detach().abs().max()):.3f}")
            assert margin > GC.MARGIN and float(x.detach().abs().max()) > 0.05
    hinstall.install(modules={utils.__name__: utils}, train=True)
    try:
        assert utils.DLT_solve is hdn_amd.DLT_solve and utils.transform is hdn_amd.transform
        m.ns = utils
        m = m.to(dev)
        loss, _ = m(org.to(dev), inp.to(dev), h4p.to(dev), pidx.to(dev), path == "full_patch")
        loss.backward()
    finally:
        hinstall.uninstall()
    got = {n: p.grad for n, p in m.named_parameters()}
    assert got["fc.weight"] is not None and float(got["fc.weight"].abs().max()) > 0      # the regressor hears the feature loss
    assert_chain_bound(f"homography branch ({path})", got, grads[torch.float64], grads[torch.float32])
