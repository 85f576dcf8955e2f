"""The L1 triplet rows on the device (csrc/triplet_loss.hip through its two entry points, hdn_amd.triplet's wrappers and autograd Function, the
install(train=True) rebinding and HomoModelBuilder.training_forward) against the float64 truth of tests/triplet_cases.py: every loss row inside tol,
every gradient exact, bit for bit between calls, written inside untouched margins at every float offset, for every subset of requested gradients,
through autograd, beside poisoned rows, with ids against the gathered copies, and end to end against a float64 CPU twin of the reference's training
forward.  The host side is tests/test_triplet_host.py."""
import copy
import itertools
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import geometry_bwd_cases as GC
import triplet_cases as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(x, y):
    return x.shape == y.shape and torch.equal(bits(x), bits(y))


def run_raw(c, dev, off=0, need=(True, True, True), ids="case", inputs=None):
    """Both entry points on case c with every float tensor at float offset `off` of its allocation; outputs start as NaN inside 0xA5 margins.
    -> (loss [n_sel,R] on the CPU, [ga, gp, gn] full size on the CPU or None, report): report holds what the caller asserts on."""
    from hdn_amd import _lib
    lib = _lib.load()
    ids = c.ids if ids == "case" else ids
    a, p, n = inputs if inputs is not None else (c.a, c.p, c.n)
    N, R, D = a.shape
    n_sel = N if ids is None else len(ids)
    dins = [GC.at_offset(t, off, dev) for t in (a, p, n)]
    dg = GC.at_offset(c.g if c.g.shape[0] == n_sel else torch.ones(n_sel, R), off, dev)
    dids = None if ids is None else torch.tensor(ids, dtype=torch.long, device=dev)
    n_ids = 0 if ids is None else len(ids)
    loss_v, loss_b = GC.at_offset(n_sel * R, off, dev, margin=GC.PAD, fill=GC.FILL)
    _lib.launch("triplet_l1", dev, lib.hdn_triplet_l1_f32, *[_lib.ptr(v) for v, _ in dins], _lib.opt(dids), _lib.ptr(loss_v), N, R, D, n_ids,
                c.margin, c.eps)
    outs = [GC.at_offset(N * R * D, off, dev, margin=GC.PAD, fill=GC.FILL) if w else (None, None) for w in need]
    _lib.launch("triplet_l1_backward", dev, lib.hdn_triplet_l1_bwd_f32, *[_lib.ptr(v) for v, _ in dins], _lib.opt(dids), _lib.ptr(dg[0]),
                *[_lib.opt(v) for v, _ in outs], N, R, D, n_ids, c.margin, c.eps)
    torch.cuda.synchronize()
    clean = GC.untouched(loss_b.cpu(), GC.PAD + off, GC.PAD + off + n_sel * R)
    for v, b in outs:
        if b is not None:
            clean = clean and GC.untouched(b.cpu(), GC.PAD + off, GC.PAD + off + N * R * D)
    unchanged = all(same_bits(v.cpu().reshape(t.shape), t) for (v, _), t in zip(dins, (a, p, n)))
    grads = [None if v is None else v.cpu().reshape(N, R, D) for v, _ in outs]
    return loss_v.cpu().reshape(n_sel, R), grads, {"clean": clean, "unchanged": unchanged}


def assert_case(c, loss, grads, what):
    t = c.truth()
    assert not bool(loss.isnan().any()), what
    if c.exact:
        assert torch.equal(loss, t["loss"]), what
    else:
        err = (loss.double() - t["loss"]).abs()
        assert bool((err <= t["tol"]).all()), (what, float((err / t["tol"]).max()))
    for name, got, want in zip(("grad_a", "grad_p", "grad_n"), grads, t["grads"]):
        if got is None:
            continue
        assert not bool(got.isnan().any()), (what, name)
        m = t["compared_full"]
        assert torch.equal(got[m], want[m]), (what, name, GC.first_difference(torch.where(m, got, want), want))


# ------------------------------------------------------------------------------------------------------------------------------ 1. every case
@pytest.mark.parametrize("name", TC.NAMES)
def test_every_case_through_the_raw_abi(dev, name):
    """Loss inside tol of float64 (bit-exact on the order-independent fixtures), gradients exact, two calls bit-equal, outputs written from NaN
    inside untouched 0xA5 margins, inputs bit-unchanged, every tensor at float offsets 0..3."""
    c = TC.CASES[name]
    first = None
    for off in range(4):
        loss, grads, rep = run_raw(c, dev, off)
        assert rep["clean"] and rep["unchanged"], (name, off, rep)
        assert_case(c, loss, grads, (name, off))
        if first is None:
            first = (loss, grads)
            loss, grads, _ = run_raw(c, dev, off)                                             # a second call: bit-equal
        assert same_bits(first[0], loss) and all(same_bits(x, y) for x, y in zip(first[1], grads)), (name, off)   # ... and so is every alignment
    err = ((first[0].double() - c.truth()["loss"]).abs() / c.truth()["tol"]).max()
    print(f"FORMS triplet {name}: worst |hip - f64| / tol = {float(err):.3f}; rows left out of the gradient comparison: {c.truth()['excluded']}")


@pytest.mark.parametrize("name", TC.NAMES)
def test_every_case_through_triplet_l1(dev, name):
    """hdn_amd.triplet_l1 / triplet_l1_backward and the autograd path give the raw ABI's bits, in the documented shapes."""
    import hdn_amd
    c = TC.CASES[name]
    raw_loss, raw_grads, _ = run_raw(c, dev)
    a, p, n = (t.to(dev) for t in (c.a, c.p, c.n))
    ids = None if c.ids is None else torch.tensor(c.ids, dtype=torch.long, device=dev)
    loss = hdn_amd.triplet_l1(a, p, n, margin=c.margin, eps=c.eps, ids=ids)
    assert tuple(loss.shape) == (c.n_sel, c.R) and not loss.requires_grad and same_bits(loss, raw_loss)
    grads = hdn_amd.triplet_l1_backward(a, p, n, c.g.to(dev), margin=c.margin, eps=c.eps, ids=ids)
    assert all(tuple(x.shape) == tuple(c.a.shape) and same_bits(x, y) for x, y in zip(grads, raw_grads))
    al, pl, nl = (t.clone().requires_grad_(True) for t in (a, p, n))
    out = hdn_amd.triplet_l1(al, pl, nl, margin=c.margin, eps=c.eps, ids=ids, differentiable=True)
    assert out.requires_grad and same_bits(out, raw_loss)
    out.backward(c.g.to(dev))
    assert all(same_bits(x.grad, y) for x, y in zip((al, pl, nl), raw_grads))
    assert_case(c, out.detach().cpu(), [x.grad.cpu() for x in (al, pl, nl)], name)
    # four-dimensional inputs as the reference passes them: [N,1,R,D] -> [n_sel,1,R]
    out4 = hdn_amd.triplet_l1(a.unsqueeze(1), p.unsqueeze(1), n.unsqueeze(1), margin=c.margin, eps=c.eps, ids=ids)
    assert tuple(out4.shape) == (c.n_sel, 1, c.R) and same_bits(out4.squeeze(1), raw_loss)


# ------------------------------------------------------------------------------------------------------------------------------ 2. requested outputs
@pytest.mark.parametrize("name", ["n01_3x3x127", "ids_0_2_of_3", "boundary_D65"])
def test_every_subset_of_requested_gradients(dev, name):
    """Every non-empty subset: the requested gradients have the bits of the all-three call; a NULL one is never written (nothing but the requested
    buffers exists to be written, and their margins stay 0xA5)."""
    import hdn_amd
    c = TC.CASES[name]
    _, full, _ = run_raw(c, dev)
    a, p, n = (t.to(dev) for t in (c.a, c.p, c.n))
    ids = None if c.ids is None else torch.tensor(c.ids, dtype=torch.long, device=dev)
    for need in itertools.product((True, False), repeat=3):
        if not any(need):
            continue
        _, grads, rep = run_raw(c, dev, off=1, need=need)
        assert rep["clean"] and rep["unchanged"]
        for w, got, want in zip(need, grads, full):
            assert (got is None) if not w else same_bits(got, want), need
        py = hdn_amd.triplet_l1_backward(a, p, n, c.g.to(dev), margin=c.margin, eps=c.eps, ids=ids, need_anchor=need[0], need_positive=need[1],
                                         need_negative=need[2])
        for w, got, want in zip(need, py, full):
            assert (got is None) if not w else same_bits(got, want), need


# ------------------------------------------------------------------------------------------------------------------------------ 3. autograd
def test_autograd_every_needs_input_grad_combination(dev):
    import hdn_amd
    c = TC.CASES["ids_0_2_of_3"]
    _, full, _ = run_raw(c, dev)
    ids = torch.tensor(c.ids, dtype=torch.long, device=dev)
    for need in itertools.product((True, False), repeat=3):
        leaves = [t.to(dev).requires_grad_(w) for t, w in zip((c.a, c.p, c.n), need)]
        out = hdn_amd.triplet_l1(*leaves, margin=c.margin, eps=c.eps, ids=ids, differentiable=True)
        assert out.requires_grad == any(need)
        if any(need):
            out.backward(c.g.to(dev))
        for w, leaf, want in zip(need, leaves, full):
            assert (leaf.grad is None) if not w else same_bits(leaf.grad, want), need


def test_autograd_noncontiguous_expanded_double_backward_and_no_grad(dev):
    import hdn_amd
    c = TC.CASES["n01_3x3x65"]
    N, R, D = c.a.shape
    _, full, _ = run_raw(c, dev)
    # positive and negative as transposed views, grad_out expanded from one row and permuted
    pl = c.p.transpose(1, 2).contiguous().to(dev).requires_grad_(True)                        # [N,D,R]
    nl = c.n.permute(2, 0, 1).contiguous().to(dev).requires_grad_(True)                       # [D,N,R]
    al = c.a.to(dev).requires_grad_(True)
    out = hdn_amd.triplet_l1(al, pl.transpose(1, 2), nl.permute(1, 2, 0), margin=c.margin, eps=c.eps, differentiable=True)
    g_t = c.g.t().contiguous().to(dev)                                                        # [R,N]
    out.backward(g_t.t())
    assert same_bits(al.grad, full[0]) and same_bits(pl.grad.transpose(1, 2), full[1]) and same_bits(nl.grad.permute(1, 2, 0), full[2])
    # an anchor expanded over the rows: its leaf gradient is the sum over the rows of the full one
    base = c.a[:, :1].contiguous().to(dev).requires_grad_(True)                               # [N,1,D]
    p, n = c.p.to(dev), c.n.to(dev)
    out = hdn_amd.triplet_l1(base.expand(N, R, D), p, n, margin=c.margin, eps=c.eps, differentiable=True)
    ones = torch.ones(1, 1, device=dev).expand(N, R)
    out.backward(ones)
    want = hdn_amd.triplet_l1_backward(base.detach().expand(N, R, D), p, n, ones, margin=c.margin, eps=c.eps, need_positive=False,
                                       need_negative=False)[0].sum(1, keepdim=True)          # small integers: the sum is exact in any order
    assert torch.equal(base.grad, want)
    # first order only
    al = c.a.to(dev).requires_grad_(True)
    (ga,) = torch.autograd.grad(hdn_amd.triplet_l1(al, p, n, differentiable=True).sum(), al, create_graph=True)
    with pytest.raises(RuntimeError):
        ga.sum().backward()
    with torch.no_grad():
        out = hdn_amd.triplet_l1(al, p, n, differentiable=True)
        assert not out.requires_grad and out.grad_fn is None
        out = hdn_amd.triplet_l1(al, p, n)
        assert not out.requires_grad
    with pytest.raises(RuntimeError, match="inference-only"):
        hdn_amd.triplet_l1(al, p, n)


def test_zero_rows_launch_nothing_and_backward_is_zeros(dev):
    import hdn_amd
    c = TC.CASES["n01_3x3x65"]
    leaves = [t.to(dev).requires_grad_(True) for t in (c.a, c.p, c.n)]
    out = hdn_amd.triplet_l1(*leaves, ids=torch.zeros(0, dtype=torch.long, device=dev), differentiable=True)
    assert tuple(out.shape) == (0, 3)
    out.sum().backward()
    assert all(tuple(t.grad.shape) == tuple(c.a.shape) and not bool(t.grad.any()) for t in leaves)
    empty = [torch.zeros(0, 3, 65, device=dev, requires_grad=True) for _ in range(3)]
    out = hdn_amd.triplet_l1(*empty, differentiable=True)
    assert tuple(out.shape) == (0, 3)
    out.sum().backward()
    assert all(tuple(t.grad.shape) == (0, 3, 65) for t in empty)


# ------------------------------------------------------------------------------------------------------------------------------ 4. poisoned rows
@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_one_poisoned_row_leaves_every_other_row_alone(dev, poison):
    c = TC.CASES["n01_3x3x127"]
    clean_loss, clean_grads, _ = run_raw(c, dev)
    row = (1, 2)
    for which in range(3):
        ins = [t.clone() for t in (c.a, c.p, c.n)]
        ins[which][row[0], row[1], 70] = poison
        loss, grads, rep = run_raw(c, dev, inputs=ins)
        assert rep["clean"] and rep["unchanged"]
        want = TC.closed(*[t.numpy() for t in ins], c.margin, c.eps)["loss"][row]           # float64: NaN, or inf, or 0 when d_an is inf
        got = float(loss[row])
        assert np.isnan(got) or got == float(want), (which, got, want)
        keep = torch.ones(3, 3, dtype=torch.bool)
        keep[row] = False
        assert torch.equal(bits(loss)[keep], bits(clean_loss)[keep])
        for g, cg in zip(grads, clean_grads):
            assert torch.equal(bits(g)[keep], bits(cg)[keep])                                 # (no assertion on the gradients of the poisoned row)


# ------------------------------------------------------------------------------------------------------------------------------ 5. ids
@pytest.mark.parametrize("name", [k for k in TC.NAMES if k.startswith("ids_")])
def test_ids_equal_the_call_on_gathered_copies_bit_for_bit(dev, name):
    c = TC.CASES[name]
    loss, grads, _ = run_raw(c, dev)
    gl, gg, _ = run_raw(c, dev, ids=None, inputs=c.gathered())
    assert same_bits(loss, gl)
    sel = torch.tensor(c.ids, dtype=torch.long)
    out = torch.ones(c.N, dtype=torch.bool)
    out[sel] = False
    for full, part in zip(grads, gg):
        assert same_bits(full[sel], part) and not bool(bits(full)[out].any())                 # zero bits outside the selection


def test_an_id_outside_the_batch_reads_and_writes_nothing(dev):
    """ids = [0, N, 1] with the three inputs as views into one allocation that has a whole sample behind them (an unguarded kernel would still stay
    inside the allocation): NaN loss rows for that id, every other row unchanged, the margins untouched, the sample behind never read into a
    result."""
    c = TC.CASES["n01_3x3x127"]
    N, R, D = c.a.shape
    from hdn_amd import _lib
    lib = _lib.load()
    whole = torch.full((3, N + 1, R, D), 7.0)
    for k, t in enumerate((c.a, c.p, c.n)):
        whole[k, :N] = t
    whole = whole.to(dev)
    before = whole.clone()
    ids = torch.tensor([0, N, 1], dtype=torch.long, device=dev)
    g = torch.ones(3, R, device=dev)
    loss_v, loss_b = GC.at_offset(3 * R, 0, dev, margin=GC.PAD, fill=GC.FILL)
    outs = [GC.at_offset(N * R * D, 0, dev, margin=GC.PAD, fill=GC.FILL) for _ in range(3)]
    _lib.launch("triplet_l1", dev, lib.hdn_triplet_l1_f32, *[_lib.ptr(whole[k]) for k in range(3)], _lib.ptr(ids), _lib.ptr(loss_v), N, R, D, 3,
                c.margin, c.eps)
    _lib.launch("triplet_l1_backward", dev, lib.hdn_triplet_l1_bwd_f32, *[_lib.ptr(whole[k]) for k in range(3)], _lib.ptr(ids), _lib.ptr(g),
                *[_lib.ptr(v) for v, _ in outs], N, R, D, 3, c.margin, c.eps)
    torch.cuda.synchronize()
    assert same_bits(whole, before)
    assert GC.untouched(loss_b.cpu(), GC.PAD, GC.PAD + 3 * R) and all(GC.untouched(b.cpu(), GC.PAD, GC.PAD + N * R * D) for _, b in outs)
    loss = loss_v.cpu().reshape(3, R)
    ref = types.SimpleNamespace(**{**c.__dict__, "ids": [0, 1], "g": torch.ones(2, R)})
    ref_loss, ref_grads, _ = run_raw(ref, dev, ids=[0, 1])
    assert bool(loss[1].isnan().all()) and same_bits(loss[[0, 2]], ref_loss)
    for (v, _), want in zip(outs, ref_grads):
        assert same_bits(v.cpu().reshape(N, R, D), want)


# ------------------------------------------------------------------------------------------------------------------------------ 6. install(train=True)
def test_the_rebound_site_gives_the_leaves_the_exact_gradient(dev):
    """Stand-ins of the two modules hold the reference's nn.TripletMarginLoss; after install(train=True) the sim_loss lines
    (model_builder_e2e_unconstrained_v2.py:438-440: loss matrix, sum / n / 127^2) run on the kernel and the leaves receive the gradient above."""
    import hdn_amd
    import hdn_amd.install as hinstall
    c = TC.CASES["ids_24_of_32"]
    t = c.truth()
    mods = {name: types.ModuleType(name) for name in hinstall.TRIPLET_SITES}
    for m in mods.values():
        m.triplet_loss = nn.TripletMarginLoss(margin=1.0, p=1, reduction="none")
    assert hinstall.TRIPLET_TRAIN_BOUND in (True, False)
    saved, hinstall.TRIPLET_TRAIN_BOUND = hinstall.TRIPLET_TRAIN_BOUND, True
    try:
        done = hinstall.install(modules=mods, train=True)
        ids = torch.tensor(c.ids, dtype=torch.long, device=dev)
        for name, m in mods.items():
            assert isinstance(m.triplet_loss, hdn_amd.TripletMarginLossL1) and (name, "triplet_loss") in done
            leaves = [x.to(dev).requires_grad_(True) for x in (c.a, c.p, c.n)]
            mat = m.triplet_loss(*[x[ids] for x in leaves])
            mat.retain_grad()
            n_pos = ids.shape[0]
            loss = torch.sum(mat) / n_pos / (127 * 127)
            loss.backward()
            err = (mat.detach().cpu().double() - t["loss"]).abs()
            assert bool((err <= t["tol"]).all())
            c2 = copy.copy(c)                                                                 # the same case with the g that autograd delivered to the rows
            c2.g = mat.grad.cpu()
            assert bool((c2.g == c2.g[0, 0]).all()) and abs(float(c2.g[0, 0]) * n_pos * 127 * 127 - 1.0) < 1e-6
            t2 = c2.truth()
            for leaf, want in zip(leaves, t2["grads"]):
                assert float(want.abs().max()) > 0
                assert torch.equal(leaf.grad.cpu()[t2["compared_full"]], want[t2["compared_full"]])
    finally:
        hinstall.uninstall()
        hinstall.TRIPLET_TRAIN_BOUND = saved
    assert all(isinstance(m.triplet_loss, nn.TripletMarginLoss) for m in mods.values())


# ------------------------------------------------------------------------------------------------------------------------------ 7. end to end
def assert_chain_bound(what, got, g64, g32):
    """Every parameter's gradient within max(4 d_ref, 1e-5) max|grad| of the float64 twin's; d_ref: the fp32 CPU twin's deviation over max|grad|.
    -> the worst d / bound."""
    assert set(got) == set(g64) == set(g32)
    worst, over = 0.0, []
    for name in sorted(got):
        assert got[name] is not None, f"{what}: {name} received no gradient"
        t = g64[name]
        scale = float(t.abs().max())
        d_ref = float((g32[name].double() - t).abs().max()) / scale
        d = float((got[name].detach().cpu().double() - t).abs().max()) / scale
        bound = max(4 * d_ref, 1e-5)
        worst = max(worst, d / bound)
        print(f"FORMS triplet {what} {name}: d = {d:.3e}, d_ref = {d_ref:.3e}, bound {bound:.3e}")
        if not d <= bound:
            over.append((name, d, d_ref))
    assert not over, (what, f"{len(over)} of {len(got)} parameters over the bound", over[:8])
    return worst


def _twin_forward(net, data, dt):
    """homo_model_builder.py:154-215 composed from stock PyTorch at dtype dt on the CPU: the nn.Sequential ShareFeature, torch's triplet loss on
    gathered copies, and the geometry restatements of tests/geometry_bwd_cases.py."""
    org, inp, h4p, pidx = data["org_imgs"].to(dt), data["input_tensors"].to(dt), data["h4p"].to(dt), data["patch_indices"]
    if_pos, if_unsup = data["if_pos"], data["if_unsup"]
    B, _, H, W = org.shape
    share = net.ShareFeature.ShareFeature
    patch_1, patch_2 = share(inp[:, :1]), share(inp[:, 1:])
    x = net.backbone(torch.cat((patch_1, patch_2), dim=1))
    x = net.fc(net.avgpool(x).view(B, -1))
    M = torch.tensor([[63.5, 0.0, 63.5], [0.0, 63.5, 63.5], [0.0, 0.0, 1.0]], dtype=dt)
    H_mat = GC.dlt_rs(h4p, x, dt).reshape(B, 3, 3)
    Hn = torch.matmul(torch.matmul(torch.inverse(M), H_mat), M)
    flat = GC.transformer_rs(org[:, :1], Hn.reshape(B, 9), dt).reshape(-1, 1)
    base = torch.arange(0, B * H * W, H * W).unsqueeze(1).expand(B, H * W).reshape(-1)
    pred_I2 = flat[pidx.reshape(-1).long() + base].reshape(B, H, W, 1).permute(0, 3, 1, 2)
    pred = share(pred_I2)
    neg_ids = if_pos.eq(0).nonzero().squeeze(1)
    pos_ids = (if_pos * if_unsup).eq(1).nonzero().squeeze(1)
    assert neg_ids.shape[0] != 0
    mat = nn.TripletMarginLoss(margin=1.0, p=1, reduction="none")(patch_2[pos_ids], pred[pos_ids], patch_1[pos_ids])
    feature_loss = torch.sum(mat) / pos_ids.shape[0] / (127 * 127)
    homo_neg_loss = torch.sum(torch.norm(x[neg_ids, :], p=2, dim=1)) / neg_ids.shape[0]
    return feature_loss, homo_neg_loss, x


def smooth_images(B, S):
    """[B,2,S,S]: each image a sum of 16 plane waves of up to half a radian per pixel, random direction, phase and amplitude, of unit variance or so.
    Band-limited, so the warp and the 3 x 3 max pooling of the trunk see no near-ties between neighbours, yet rich enough that no BatchNorm channel of
    the trunk degenerates at B = 3 (with two plane waves per image the fp32 CPU twin already leaves float64 by 2e-2 of max|grad|)."""
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    gen = torch.Generator().manual_seed(11)
    out = []
    for _ in range(2 * B):
        img = torch.zeros(S, S)
        for _ in range(16):
            fx, fy = (torch.rand(2, generator=gen) * 2 - 1) * 0.5
            phase, amp = torch.rand(1, generator=gen) * 6.28, torch.rand(1, generator=gen) + 0.5
            img += amp * torch.sin(xx * fx + yy * fy + phase)
        out.append(img / 4.0)
    return torch.stack(out).reshape(B, 2, S, S).contiguous()


def test_training_forward_against_the_float64_twin(dev):
    """HomoModelBuilder().train() with ShareFeature.hip_train, B = 3, smooth 127 x 127 images, if_pos = [1,0,1], if_unsup = [1,1,1] (pos_ids = [0,2],
    one negative sample): feature_loss, homo_neg_loss and every parameter gradient of training_forward against the same lines in float64 on the CPU,
    by the chain bound max(4 d_ref, 1e-5) max|grad| with d_ref from the fp32 CPU twin."""
    import hdn_amd
    torch.manual_seed(TC.SEED + 5)
    net = hdn_amd.HomoModelBuilder().train()
    with torch.no_grad():
        net.fc.weight.mul_(0.05)
        net.fc.bias.copy_(torch.tensor([1.5, -1.0, -2.0, 1.0, 1.0, 2.0, -1.5, -1.0]))
    B, S = 3, 127
    org = smooth_images(B, S)
    data = {"org_imgs": org, "input_tensors": org.clone(), "h4p": torch.tensor([[0.0, 0.0, 0.0, S, S, S, S, 0.0]]).repeat(B, 1),
            "patch_indices": torch.arange(S * S, dtype=torch.float32).repeat(B, 1), "if_pos": torch.tensor([1.0, 0.0, 1.0]),
            "if_unsup": torch.tensor([1.0, 1.0, 1.0])}
    ref = {}
    for dt in (torch.float64, torch.float32):
        twin = copy.deepcopy(net).to(dt).train()
        fl, hn, x = _twin_forward(twin, data, dt)
        (fl + hn).backward()
        ref[dt] = (fl.detach(), hn.detach(), {k: p.grad for k, p in twin.named_parameters()}, x.detach())
    net = net.to(dev)
    net.ShareFeature.hip_train = True
    # the trunk's convolutions are the library's: pin its choice of algorithm to the deterministic default for this comparison (left to itself it
    # picks per process, and one of eleven processes measured here chose a backward that left ShareFeature.0.weight 1.2e-3 of max|grad| from
    # float64, where every other run stayed below 1.7e-5); nothing of this package depends on the flag
    pinned, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    try:
        out = net.training_forward({k: v.to(dev) for k, v in data.items()})
        assert set(out) == {"feature_loss", "pred_I2_d", "x", "H_mat", "patch_2_res_d", "pred_I2_CnnFeature_d", "homo_neg_loss"}
        assert tuple(out["feature_loss"].shape) == (1,) and out["feature_loss"].requires_grad and out["homo_neg_loss"].requires_grad
        (out["feature_loss"].sum() + out["homo_neg_loss"]).backward()
    finally:
        torch.backends.cudnn.deterministic = pinned
    got = {k: p.grad for k, p in net.named_parameters()}
    for name, val, i in (("feature_loss", out["feature_loss"][0], 0), ("homo_neg_loss", out["homo_neg_loss"], 1)):
        t64, t32 = float(ref[torch.float64][i]), float(ref[torch.float32][i])
        d, d_ref = abs(float(val.detach()) - t64) / abs(t64), abs(t32 - t64) / abs(t64)
        print(f"FORMS triplet training_forward {name}: {float(val.detach()):.6f}, float64 {t64:.6f}, d = {d:.3e}, d_ref = {d_ref:.3e}")
        assert t64 > 0 and d <= max(4 * d_ref, 1e-5), (name, d, d_ref)
    assert float(got["fc.weight"].abs().max()) > 0                                            # the regressor hears the feature loss
    worst = assert_chain_bound("training_forward", got, ref[torch.float64][2], ref[torch.float32][2])
    print(f"FORMS triplet training_forward: worst d / bound = {worst:.3f}; max |x| of the twin {float(ref[torch.float64][3].abs().max()):.3f}")
    # eval() mode without hip_train detaches: refused
    net.eval()
    net.ShareFeature.hip_train = False
    with pytest.raises(RuntimeError, match="ShareFeature"):
        net.training_forward({k: v.to(dev) for k, v in data.items()})
