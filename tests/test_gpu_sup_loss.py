"""csrc/sup_losses.hip on the device against the float64 truth of tests/sup_loss_cases.py: every case in both input forms (each loss and each gradient
within its bound, tie cases on the documented indices, two calls bit-identical), form 0 with a mask against form 1 on the gathered inputs, the
drop-ins through autograd down to the logits, supervised_losses captured in a graph and replayed after labels and mask changed in place, and
install(train=True) on a stand-in module that holds the five names."""
import types

import pytest
import torch
import torch.nn.functional as F

import sup_loss_cases as SC

pytestmark = pytest.mark.gpu

GRADS = ("cls", "loc", "cls_lp", "loc_lp", "rows")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _args(view, dev):
    from hdn_amd import losses
    return {k: (view.t[k].to(dev) if k in view.t else None) for k in losses._NAMES}


def _run(view, dev):
    from hdn_amd import losses
    t = _args(view, dev)
    out = losses._forward(view.form, view.topk, t)
    g5 = torch.tensor(SC.UPSTREAM, dtype=torch.float32, device=dev)
    grads = losses._backward(view.form, view.topk, t, g5, (True,) * 5)
    torch.cuda.synchronize()
    return out, dict(zip(GRADS, grads))


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("name", SC.VIEW_NAMES)
def test_every_case_in_both_forms(name, dev):
    v = SC.VIEWS[name]
    out, grads = _run(v, dev)
    SC.check(out, grads, v, what="hip")
    out2, grads2 = _run(v, dev)                                             # bit-reproducible, NaN included
    assert torch.equal(_bits(out), _bits(out2))
    for k in GRADS:
        assert torch.equal(_bits(grads[k]), _bits(grads2[k])), k
    if v.case.ties:                                                         # the gradient goes to exactly the documented cells
        want = v.truth()["grads"]["cls"]
        assert torch.equal(grads["cls"].cpu() != 0, want != 0)
        _, gtop, _ = v.evaluate(variant="ties_from_top")
        assert not torch.equal(gtop["cls"] != 0, want != 0)                 # ... which the other choice would not be


@pytest.mark.parametrize("case", ["mask_all", "mask_last", "mask_last_hits_1", "full_32_mask24"])
def test_form_0_with_a_mask_equals_form_1_on_the_gathered_inputs(case, dev):
    """|form 0 - form 1| <= 2 bound_0 + bound_1: each is within its bound of its truth, and the two truths differ by the rounding of the
    probabilities to fp32, which is inside the error model of form 0's bound (rel_p >= u)."""
    v0, v1 = SC.CASES[case].views()
    o0, _ = _run(v0, dev)
    o1, _ = _run(v1, dev)
    lim = 2 * v0.truth()["loss_bounds"] + v1.truth()["loss_bounds"]
    err = (o0.cpu().double() - o1.cpu().double()).abs()
    print(f"SUP {case}: form 0 {o0.tolist()} form 1 {o1.tolist()} |diff| {err.tolist()} limit {lim.tolist()}")
    assert bool((err <= lim).all())


@pytest.mark.parametrize("case", ["n2_S5", "mask_last", "n3_S13"])
def test_drop_ins_through_autograd_reach_the_logits(case, dev):
    """The reference's lines with the drop-ins inside: gather, torch's softmax / log_softmax, the five functions, backward.  Against the truth of
    form 0: torch's softmax forward is within rel_p (which form 0's bound charges), the kernel's form 1 within form 1's smaller bound, torch's
    softmax backward inside GRAD_SLACK: twice form 0's bound."""
    import hdn_amd
    v0 = SC.CASES[case].views()[0]
    t = {k: x.to(dev) for k, x in v0.t.items()}
    leaves = {k: t[k].clone().requires_grad_(True) for k in GRADS}
    sel = v0.selected().to(dev)
    p = F.softmax(leaves["cls"][sel].permute(0, 2, 3, 1).contiguous(), dim=3)
    logp = F.log_softmax(leaves["cls_lp"][sel].permute(0, 2, 3, 1).contiguous(), dim=3)
    from hdn_amd import losses
    la = losses._apply(1, topk=v0.topk, cls=p, label_cls=t["label_cls"][sel])[0] if v0.topk != 100 else \
        hdn_amd.select_xr_focal_fuse_smooth_l1_loss_top_k(p, t["label_cls"][sel])
    out = [la, hdn_amd.select_l1_loss_c(leaves["loc"][sel], t["label_loc_c"][sel], t["label_cls"][sel]),
           hdn_amd.select_cross_entropy_loss(logp, t["label_cls_lp"][sel]),
           hdn_amd.select_l1_loss(leaves["loc_lp"][sel], t["label_loc_lp"][sel], t["label_cls_lp"][sel]),
           hdn_amd.kalyo_l1_loss(leaves["rows"], t["rows_target"])]
    assert all(o.dim() == 0 and o.requires_grad for o in out)
    sum(w * o for w, o in zip(SC.UPSTREAM, out)).backward()
    torch.cuda.synchronize()
    tr = v0.truth()
    got = torch.stack([o.detach() for o in out]).cpu().double()
    assert bool(((got - tr["losses"]).abs() <= 2 * tr["loss_bounds"]).all()), (got, tr["losses"])
    for k in GRADS:
        g = leaves[k].grad.cpu().double()
        err, b = (g - tr["grads"][k]).abs(), 2 * tr["grad_bounds"][k]
        assert bool((err <= b).all()), (k, float((err - b).max()))
        assert bool((g != 0).any())
    assert float(leaves["cls"].grad.abs().sum()) > 0 and float(leaves["cls_lp"].grad.abs().sum()) > 0


def test_supervised_losses_in_a_graph_follows_labels_and_mask_changed_in_place(dev):
    """One capture of forward and explicit backward; then every label, the mask and the maps are overwritten in place with another case's and the
    graph is replayed: the new values come out.  (The reference's path reads nonzero() on the host and cannot be captured.)"""
    import hdn_amd
    names = ("cls", "loc", "cls_lp", "loc_lp", "label_cls", "label_loc_c", "label_cls_lp", "label_loc_lp")
    a, b = SC.CASES["mask_all"].views()[0], SC.CASES["mask_last"].views()[0]
    # topk_per_sample is 100 through the public call: the truth here is evaluated at 100 as well
    va, vb = (SC.View(types.SimpleNamespace(name=v.case.name + "@100", topk=100, on_threshold=False), 0, v.t) for v in (a, b))
    st = {k: a.t[k].to(dev).clone() for k in names + ("if_unsup",)}
    g4 = torch.tensor(SC.UPSTREAM[:4], dtype=torch.float32, device=dev)

    def step():
        d = hdn_amd.supervised_losses(*(st[k] for k in names), if_unsup=st["if_unsup"])
        g = hdn_amd.supervised_losses_backward(*(st[k] for k in names), g4, if_unsup=st["if_unsup"])
        return torch.stack([d[k] for k in hdn_amd.losses.KEYS]), g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                              # warm-up outside the capture (one-time attribute calls)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grads = step()
    for view in (va, vb, va):
        for k in names + ("if_unsup",):
            st[k].copy_(view.t[k].to(dev))
        graph.replay()
        torch.cuda.synchronize()
        tr = view.truth()
        got = out.cpu().double()
        assert bool(((got - tr["losses"][:4]).abs() <= tr["loss_bounds"][:4]).all()), (view.name, got, tr["losses"])
        for k, g in zip(GRADS[:4], grads):
            err = (g.cpu().double() - tr["grads"][k]).abs()
            assert bool(((err <= tr["grad_bounds"][k]) | ~tr["compared"][k]).all()), (view.name, k)
    assert not torch.equal(va.truth()["losses"], vb.truth()["losses"])


def test_supervised_losses_dict_and_autograd(dev):
    import hdn_amd
    v = SC.CASES["full_32_mask24"].views()[0]
    t = {k: x.to(dev) for k, x in v.t.items()}
    leaves = {k: t[k].clone().requires_grad_(True) for k in GRADS[:4]}
    d = hdn_amd.supervised_losses(leaves["cls"], leaves["loc"], leaves["cls_lp"], leaves["loc_lp"], t["label_cls"], t["label_loc_c"],
                                  t["label_cls_lp"], t["label_loc_lp"], if_unsup=t["if_unsup"])
    assert tuple(d) == hdn_amd.losses.KEYS and all(x.dim() == 0 for x in d.values())
    sum(w * d[k] for w, k in zip(SC.UPSTREAM, hdn_amd.losses.KEYS)).backward()
    torch.cuda.synchronize()
    got = torch.cat([torch.stack([d[k].detach() for k in hdn_amd.losses.KEYS]).cpu(), v.truth()["losses"][4:].float()])
    SC.check(got, {k: leaves[k].grad for k in GRADS[:4]}, v, what="autograd")
    unsel = [i for i in range(32) if i % 4 == 1]
    assert all(float(leaves[k].grad[unsel].abs().sum()) == 0 for k in GRADS[:4])


def test_install_train_on_a_stand_in_module(dev, monkeypatch):
    import hdn_amd
    import hdn_amd.install as hinstall
    site = types.ModuleType(hinstall.SUP_LOSS_SITE)
    for n in hinstall.SUP_LOSS_NAMES:
        setattr(site, n, None)
    monkeypatch.setattr(hinstall, "SUP_LOSS_TRAIN_BOUND", True)
    v = SC.CASES["n5_S25"].views()[1]
    t = {k: x.to(dev) for k, x in v.t.items()}
    try:
        done = hinstall.install(modules={hinstall.SUP_LOSS_SITE: site}, train=True)
        assert all((hinstall.SUP_LOSS_SITE, n) in done for n in hinstall.SUP_LOSS_NAMES)
        out = torch.stack([site.select_xr_focal_fuse_smooth_l1_loss_top_k(t["cls"], t["label_cls"]),
                           site.select_l1_loss_c(t["loc"], t["label_loc_c"], t["label_cls"]),
                           site.select_cross_entropy_loss(t["cls_lp"], t["label_cls_lp"]),
                           site.select_l1_loss(t["loc_lp"], t["label_loc_lp"], t["label_cls_lp"]),
                           site.kalyo_l1_loss(t["rows"], t["rows_target"])])
        torch.cuda.synchronize()
    finally:
        hinstall.uninstall()
    assert all(getattr(site, n) is None for n in hinstall.SUP_LOSS_NAMES)
    SC.check(out, None, v, what="install")
