"""csrc/corner_losses.hip on the device against tests/corner_loss_cases.py: every case forward and backward within the a-priori bounds of the float64
truth (beside PyTorch-ROCm's own fp32 run of the restated lines), counts exactly, every subset of `need`, two calls bit-equal, every element written;
the exact fixtures with torch.equal; H_gt against hdn_amd.DLT_solve; samples outside the sets filled with NaN; rows independent given the counts;
autograd down to leaves against the explicit backward; total_loss of training_outputs; one graph capture of forward and backward replayed while flags
and data change in place; the refusals."""
import itertools

import numpy as np
import pytest
import torch

import corner_loss_cases as CC
from simi_geometry_cases import U, Qv

pytestmark = pytest.mark.gpu

NAMES = ("H_mat", "pred_points", "aug_sear_points", "template_poly", "x", "if_pos", "if_unsup")
NAN_BITS = 0x7FC0ABCD
E_NULL, E_SHAPE, E_LIMIT = -1, -2, -3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _t(c, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in c.arrays().items()}


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b)) if a.dtype == torch.float32 else torch.equal(a, b)


def _nan_filled(monkeypatch):
    """torch.empty inside hdn_amd.corner hands out buffers full of one NaN pattern: what comes back with it was not written"""
    from hdn_amd import corner as G
    real = G._new

    def new(*a, **k):
        out = real(*a, **k)
        if out.dtype == torch.float32:
            out.view(torch.int32).fill_(NAN_BITS)
        else:
            out.fill_(-7)
        return out
    monkeypatch.setattr(G, "_new", new)


def _written(x):
    return not bool((_bits(x) == NAN_BITS).any()) if x.dtype == torch.float32 else not bool((x == -7).any())


def _run(t, w, need=(True, True, True, True)):
    """KEYS, counts and the GRADS that are asked for, from the explicit launches; t: name -> device tensor, w: grad_out"""
    from hdn_amd import corner as G
    out, counts = G._forward(*(t[k] for k in NAMES))
    res = {k: out[i] for i, k in enumerate(CC.KEYS)}
    res["counts"] = counts
    gr = G.corner_losses_backward(t["H_mat"], t["pred_points"], t["template_poly"], t["x"], t["if_pos"], t["if_unsup"], w,
                                  aug_sear_points=t["aug_sear_points"], need=need)
    res.update({k: g for k, g in zip(CC.GRADS, gr) if g is not None})
    return res


_worst = {"kernel": 0.0, "rocm": 0.0, "rocm_no_solve": 0.0}


@pytest.mark.parametrize("name", CC.CASE_NAMES)
def test_every_case(name, dev, monkeypatch):
    c = CC.CASES[name]
    t = _t(c, dev)
    keep = {k: v.clone() for k, v in t.items()}
    _nan_filled(monkeypatch)
    w = torch.from_numpy(c.w).to(dev)
    got = _run(t, w)
    again = _run(t, w)
    got_ns = _run(t, torch.from_numpy(c.w * CC.NO_SOLVE).to(dev))
    torch.cuda.synchronize()
    for k, v in got.items():
        assert _written(v), (name, k)
        assert _same(v, again[k]), (name, k, "two calls differ")
    for k in NAMES:                                                          # the inputs are as they were, NaN flags included
        assert torch.equal(_bits(keep[k]), _bits(t[k]))
    r = max(CC.check(got, c, what="kernel"), CC.check(got_ns, c, truth="q_ns", what="kernel, no solve"))
    monkeypatch.undo()
    rocm = c.torch_run(torch.float32, dev)
    r_rocm = CC.check(rocm, c, what="PyTorch-ROCm", limit=np.inf)
    r_rocm_ns = CC.check(c.torch_run(torch.float32, dev, weights=c.w * CC.NO_SOLVE), c, truth="q_ns", what="PyTorch-ROCm",
                         keys=("cor_err", "cor_err_aug", "cor_err_sim", "cor_neg_loss") + CC.GRADS, limit=np.inf)
    assert np.array_equal(rocm["counts"], got["counts"].cpu().numpy())
    print(f"{name}: error / bound  kernel {r:.3f}  PyTorch-ROCm {r_rocm:.3f} (without the solve {r_rocm_ns:.3f})")
    _worst["kernel"], _worst["rocm"], _worst["rocm_no_solve"] = max(_worst["kernel"], r), max(_worst["rocm"], r_rocm), max(_worst["rocm_no_solve"], r_rocm_ns)


def test_worst_ratios_are_printed():
    """runs after the sweep (file order): the figures of docs/PARITY.md"""
    print("worst error / bound over the cases: kernel %(kernel).3f, PyTorch-ROCm %(rocm).3f, PyTorch-ROCm without the solve %(rocm_no_solve).3f" % _worst)
    assert _worst["kernel"] <= 1.0


@pytest.mark.parametrize("name", CC.CASE_NAMES)
def test_every_subset_of_need(name, dev, monkeypatch):
    c = CC.CASES[name]
    t = _t(c, dev)
    w = torch.from_numpy(c.w).to(dev)
    full = _run(t, w)
    _nan_filled(monkeypatch)
    for need in itertools.product((False, True), repeat=4):
        if not any(need):
            continue
        got = _run(t, w, need)
        assert [k in got for k in CC.GRADS] == list(need)
        for k in CC.GRADS:
            if k in got:
                assert _written(got[k]) and _same(got[k], full[k]), (name, need, k)
    # without aug_sear_points: slot 1 is 0, the rest is unchanged
    t2 = dict(t, aug_sear_points=None)
    got = _run(t2, w, (True, True, False, True))
    for k in got:
        if k == "cor_err_aug":
            assert float(got[k]) == 0.0
        else:
            assert _same(got[k], full[k]), (name, k)


@pytest.mark.parametrize("name", CC.EXACT_NAMES)
def test_exact_fixtures(name, dev):
    c = CC.EXACT_CASES[name]
    want = c.expected()
    got = _run(_t(c, dev), torch.from_numpy(c.w).to(dev))
    for k in CC.KEYS + ("counts", "grad_x"):
        assert torch.equal(got[k].cpu(), torch.from_numpy(np.asarray(want[k]))), (name, k, got[k], want[k])


def test_h_gt_agrees_with_dlt_solve(dev):
    """x = 0 and one selected sample: slot 3 is kalyo_l1_loss(0, delta) / 9 with delta from H_gt.  The same delta is formed here in float64 from the H
    that hdn_amd.DLT_solve returns for (template_poly, off); the two may differ by the fp32 roundings after the solve only (the Qv bound below)."""
    import hdn_amd
    c = CC.CASES["first_only_B65"]
    t = _t(c, dev)
    t["x"] = torch.zeros_like(t["x"])
    assert c.ids["sup_pos"].tolist() == [0]
    out, counts = hdn_amd.corner._forward(*(t[k] for k in NAMES))
    pp, tp = t["pred_points"][:1], t["template_poly"][:1]
    off = (pp[:, :2] / pp[:, 2:3]).permute(0, 2, 1) - tp                                   # IEEE fp32 division and subtraction, as in the kernel
    H = hdn_amd.DLT_solve(tp.reshape(1, 8), off.reshape(1, 8)).reshape(9).cpu().double().numpy()
    h = [Qv(v) for v in H]
    terms = []
    for j in range(4):
        cx, cy = CC.SQUARE[j]
        Qw = (h[6] * cx + h[7] * cy) + 1.0
        for cc in range(2):
            q = (h[3 * cc] * cx + h[3 * cc + 1] * cy) + h[3 * cc + 2]
            d = CC.QA().div(q, Qw) - CC.SQUARE[j, cc]
            terms.append(CC.QA().kalyo(d)[0])
    want = CC.QA().div(CC.QA().total(terms), 9.0)
    assert int(counts[1]) == 1 and abs(float(out[3]) - float(want.v)) <= float(want.e), (float(out[3]), float(want.v), float(want.e))
    assert float(want.e) <= 64 * U * float(want.v)                                         # a few roundings, not a tolerance


def _poison(c, t):
    """every tensor's rows of the samples that are in no set which reads them, filled with NaN"""
    ids = c.ids
    B = c.B
    member = lambda *sets: np.isin(np.arange(B), np.concatenate([ids[s] for s in sets]))
    reads = {"H_mat": member("sup_pos"), "aug_sear_points": member("sup_pos"), "pred_points": member("sup_pos", "unsup_pos"),
             "template_poly": member("sup_pos", "unsup_pos"), "x": member("sup_pos", "neg")}
    out = dict(t)
    for k, m in reads.items():
        v = t[k].clone()
        v[torch.from_numpy(~m).to(v.device)] = float("nan")
        out[k] = v
    return out, reads


@pytest.mark.parametrize("name", ("odd_flags_B33", "mix_B65", "no_sup_pos_B33", "first_only_B65"))
def test_samples_outside_the_sets_reach_nothing(name, dev):
    c = CC.CASES[name]
    t = _t(c, dev)
    w = torch.from_numpy(c.w).to(dev)
    clean = _run(t, w)
    bad, reads = _poison(c, t)
    assert any(bool(torch.isnan(bad[k]).any()) for k in reads)
    got = _run(bad, w)
    for k in got:
        assert _same(got[k], clean[k]), (name, k)                                          # NaN-free, bit for bit
        assert not bool(torch.isnan(got[k].float()).any())
    for gk, k in zip(CC.GRADS, ("H_mat", "pred_points", "aug_sear_points", "x")):
        rows = got[gk][torch.from_numpy(~reads[k]).to(dev)]
        assert bool((_bits(rows) == 0).all()), (name, gk)                                  # exactly +0


@pytest.mark.parametrize("name", ("mix_B33", "mix_B257"))
def test_rows_are_independent_given_the_counts(name, dev):
    """the same flags, the data of every other sample replaced: the rows of the samples that kept their data keep their bits"""
    c = CC.CASES[name]
    other = CC.Case(name + "_other", c.B, c.seed + 5, (c.if_pos, c.if_unsup), bounded=False)
    t, o = _t(c, dev), _t(other, dev)
    w = torch.from_numpy(c.w).to(dev)
    base = _run(t, w)
    for parity in (0, 1):
        swap = torch.arange(c.B, device=dev) % 2 == parity
        mixed = {k: torch.where(swap.reshape(-1, *([1] * (t[k].dim() - 1))), o[k], t[k]) for k in NAMES}
        got = _run(mixed, w)
        assert torch.equal(got["counts"], base["counts"])
        for k in CC.GRADS:
            assert _same(got[k][~swap], base[k][~swap]), (name, parity, k)
            assert not _same(got[k][swap], base[k][swap])


def test_autograd_down_to_leaves_agrees_with_the_explicit_backward(dev):
    import hdn_amd
    c = CC.CASES["production_B32"]
    t = _t(c, dev)
    w = torch.from_numpy(c.w).to(dev)
    want = _run(t, w)
    leaves = {k: t[k].clone().requires_grad_(True) for k in ("H_mat", "pred_points", "aug_sear_points", "x")}
    d = hdn_amd.corner_losses(leaves["H_mat"] * 1.0, leaves["pred_points"] * 1.0, t["template_poly"], leaves["x"] * 1.0, t["if_pos"], t["if_unsup"],
                              aug_sear_points=leaves["aug_sear_points"] * 1.0)
    assert set(d) == set(CC.KEYS) | {"counts"} and all(d[k].dim() == 0 for k in CC.KEYS)
    assert d["counts"].dtype == torch.int32 and not d["counts"].requires_grad
    sum(w[i] * d[k] for i, k in enumerate(CC.KEYS)).backward()
    for gk, k in zip(CC.GRADS, leaves):
        assert _same(leaves[k].grad, want[gk]), gk
    for k in CC.KEYS:
        assert _same(d[k].detach(), want[k])
    # only x needs a gradient: one launch with need = (F, F, F, T)
    x = t["x"].clone().requires_grad_(True)
    d = hdn_amd.corner_losses(t["H_mat"], t["pred_points"], t["template_poly"], x, t["if_pos"], t["if_unsup"], aug_sear_points=t["aug_sear_points"])
    (d["cor_loss"] * w[5] + d["cor_pos_loss"] * w[3] + d["cor_neg_loss"] * w[4]).backward()
    assert _same(x.grad, _run(t, w * torch.tensor([0, 0, 0, 1, 1, 1.0], device=dev))["grad_x"])


def test_total_loss_backpropagates(dev):
    import hdn_amd
    c = CC.CASES["production_B32"]
    t = _t(c, dev)
    leaves = {k: t[k].clone().requires_grad_(True) for k in ("H_mat", "pred_points", "x")}
    head = {k: torch.tensor(0.1 * (i + 1), device=dev, requires_grad=True) for i, k in enumerate(hdn_amd.losses.KEYS)}
    sim, feat = torch.tensor(0.7, device=dev, requires_grad=True), torch.tensor(0.9, device=dev, requires_grad=True)
    d = hdn_amd.corner_losses(leaves["H_mat"], leaves["pred_points"], t["template_poly"], leaves["x"], t["if_pos"], t["if_unsup"],
                              aug_sear_points=t["aug_sear_points"])
    out = hdn_amd.training_outputs(head, d, sim, feat, 1.0, 1.2)
    assert tuple(out) == hdn_amd.corner.OUTPUT_KEYS
    want_total = (1.0 * (0.3 + 0.1) + 1.2 * (0.2 + 0.4)) * 100 + 0.9 + float(d["cor_neg_loss"].detach()) + float(d["cor_err"].detach()) / 4
    assert float(out["total_loss"].detach()) == pytest.approx(want_total, rel=1e-6)
    assert float(out["sim_loss"].detach()) == pytest.approx(0.7) and _same(out["cor_loss"].detach(), d["cor_loss"].detach())
    out["total_loss"].backward()
    g = torch.tensor([0.25, 0, 0, 0, 1, 0], device=dev)
    want = _run(t, g, (True, True, False, True))
    for gk, k in (("grad_H_mat", "H_mat"), ("grad_pred_points", "pred_points"), ("grad_x", "x")):
        assert _same(leaves[k].grad, want[gk]), gk
    assert float(feat.grad) == 1.0 and sim.grad is None                     # sim_loss is reported, not part of total_loss
    assert [float(head[k].grad) for k in hdn_amd.losses.KEYS] == [pytest.approx(v) for v in (100.0, 120.0, 100.0, 120.0)]


def test_forward_and_backward_in_a_graph_follow_flags_and_data_changed_in_place(dev):
    """One capture of forward and explicit backward on one stream; then flags and data are overwritten in place with other cases' - emptying and
    refilling every set - and the graph is replayed: it gives what an eager call gives, bit for bit."""
    seq = ("mix_B33", "all_sup_pos_B33", "no_sup_pos_B33", "neg_all_unsup_B33", "odd_flags_B33", "w_B33", "mix_B33")
    st = {k: v.clone() for k, v in _t(CC.CASES[seq[0]], dev).items()}
    w = torch.from_numpy(CC.CASES[seq[0]].w).to(dev)

    def step():
        r = _run(st, w)
        return [r[k] for k in CC.KEYS + ("counts",) + CC.GRADS]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    seen = set()
    for name in seq:
        c = CC.CASES[name]
        for k, v in _t(c, dev).items():
            st[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        eager = step()
        torch.cuda.synchronize()
        for k, a, b in zip(CC.KEYS + ("counts",) + CC.GRADS, got, eager):
            assert _same(a, b), (name, k)
        CC.check(dict(zip(CC.KEYS + ("counts",), got[:7])), c, what="replay")
        seen.add(tuple(int(v > 0) for v in got[6].cpu().tolist()))
    assert len(seen) >= 4                                                   # the sets were emptied and refilled


def test_refusals(dev):
    import hdn_amd
    from hdn_amd import _lib as L
    c = CC.CASES["mix_B7"]
    t = _t(c, dev)
    args = (t["H_mat"], t["pred_points"], t["template_poly"], t["x"], t["if_pos"], t["if_unsup"])
    lib = L.load()
    out = torch.full((6,), -5.0, device=dev)
    counts = torch.full((6,), -7, dtype=torch.int32, device=dev)
    p = [L.ptr(t[k]) for k in NAMES]
    for i in (0, 1, 3, 4, 5, 6):
        q = list(p)
        q[i] = None
        assert lib.hdn_corner_losses_f32(*q, L.ptr(out), L.ptr(counts), c.B, None) == E_NULL
    assert lib.hdn_corner_losses_f32(*p, None, L.ptr(counts), c.B, None) == E_NULL
    assert lib.hdn_corner_losses_f32(*p, L.ptr(out), L.ptr(counts), 0, None) == E_SHAPE
    assert lib.hdn_corner_losses_f32(*p, L.ptr(out), L.ptr(counts), 65537, None) == E_LIMIT
    g = torch.ones(6, device=dev)
    gx = torch.full((c.B, 8), -5.0, device=dev)
    assert lib.hdn_corner_losses_bwd_f32(*p, None, None, None, None, L.ptr(gx), c.B, None) == E_NULL
    assert lib.hdn_corner_losses_bwd_f32(*p, L.ptr(g), None, None, None, None, c.B, None) == E_SHAPE
    assert lib.hdn_corner_losses_bwd_f32(*p, L.ptr(g), None, None, None, L.ptr(gx), 65537, None) == E_LIMIT
    torch.cuda.synchronize()
    assert bool((out == -5).all()) and bool((counts == -7).all()) and bool((gx == -5).all())        # nothing was launched
    with pytest.raises(ValueError):
        hdn_amd.corner_losses(*(a[:0] for a in args))                                                 # B = 0
    big = 65537
    z = lambda *s: torch.zeros(big, *s, device=dev)
    with pytest.raises(ValueError, match="HDN_E_LIMIT"):
        hdn_amd.corner_losses(z(3, 3), z(3, 4), z(4, 2), z(8), z(), z())                              # B over the limit
    with pytest.raises(L.HdnHipError):
        hdn_amd.corner_losses(args[0].cpu(), *args[1:])                                               # a CPU tensor
    with pytest.raises(ValueError, match="template_poly"):
        hdn_amd.corner_losses(args[0], args[1], args[2].clone().requires_grad_(True), *args[3:])
    with pytest.raises(ValueError):
        hdn_amd.corner_losses(args[0], args[1][:, :2], *args[2:])                                     # a wrong shape
    # the largest batch the issue names, and the limit itself: B = 4096 and 65536 run
    for B in (4096, 65536):
        flags = (torch.arange(B, device=dev) % 2).float()
        sq = torch.tensor(CC.SQUARE, dtype=torch.float32, device=dev).expand(B, 4, 2).contiguous()
        ppB = torch.cat([sq.permute(0, 2, 1) + 4.0, torch.ones(B, 1, 4, device=dev)], 1).contiguous()
        d = hdn_amd.corner_losses(torch.eye(3, device=dev).expand(B, 3, 3).contiguous(), ppB, sq, torch.zeros(B, 8, device=dev), flags,
                                  torch.zeros(B, device=dev))
        assert d["counts"].cpu().tolist() == [B, B // 2, B // 2, 0, 0, B // 2]
        assert float(d["cor_err"]) == 8.0                                                             # 32 px per sample, exact sums
        assert float(d["cor_pos_loss"]) == float(np.float32(14 * B) / np.float32(4 * B + 1))          # d = 4 everywhere: 3.5 per element
