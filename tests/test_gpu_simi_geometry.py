"""csrc/simi_geometry.hip on the device against tests/simi_geometry_cases.py: every cell as the winner at S in {1, 2, 8, 9, 13, 25}, the tie, saturated
and NaN-first families in both modes (indices equal, polar / rot / the pick's exact gradients bit for bit, the rest within the a-priori bounds, beside
PyTorch-ROCm's own fp32 run of the restated lines), batch independence and reproducibility, buffer hygiene, the stand-alone matrices, autograd through
the fused form and through the drop-ins inside the restated lines, the raises, a graph capture replayed on new inputs, and install(train=True)."""
import types

import numpy as np
import pytest
import torch

import simi_geometry_cases as SC

pytestmark = pytest.mark.gpu

HALF = SC.OUT_SZ / 2
CFG = dict(stride=SC.STRIDE, stride_lp=SC.STRIDE_LP, map_size=SC.MAP_SIZE, in_sz=SC.IN_SZ, out_sz=SC.OUT_SZ)
CFG_T = (SC.STRIDE, SC.STRIDE_LP, SC.MAP_SIZE, SC.IN_SZ, SC.OUT_SZ)
FWD = ("best_idx_lp", "scale", "rot") + SC.MATS + ("pred_points", "aug_sear_points")
UP = ("scale", "rot", "affine_m", "affine_m_lt0", "pred_points")
NAN_BITS = 0x7FC0ABCD


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _nan_filled(monkeypatch):
    """torch.empty inside hdn_amd.simi_geometry hands out buffers full of one NaN pattern: what comes back with it was not written"""
    from hdn_amd import simi_geometry as G
    real = G._new

    def new(*a, **k):
        out = real(*a, **k)
        if out.dtype == torch.float32:
            out.view(torch.int32).fill_(NAN_BITS)
        else:
            out.fill_(-7)
        return out
    monkeypatch.setattr(G, "_new", new)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b)) if a.dtype == torch.float32 else torch.equal(a, b)


def _written(x):
    return not bool((_bits(x) == NAN_BITS).any()) if x.dtype == torch.float32 else not bool((x == -7).any())


def _run(c, dev):
    """every key of Case.evaluate from the explicit launches: the two picks, the fused form, and the three backwards"""
    from hdn_amd import simi_geometry as G
    cls, loc, cls_lp, loc_lp = (_t(a, dev) for a in (c.cls, c.loc, c.cls_lp, c.loc_lp))
    tcx, tcy, poly = _t(c.temp_cx, dev), _t(c.temp_cy, dev), _t(c.search_poly, dev)
    w = {k: _t(v, dev) for k, v in c.w.items()}
    keep = [x.clone() for x in (cls, loc, cls_lp, loc_lp, tcx, tcy, poly)]
    out = {}
    out["polar"], out["best_idx"] = G._pick_forward(0, SC.STRIDE, SC.STRIDE, 0.0, 0.0, cls, loc)
    out["pick_grad_loc"] = G._pick_backward(0, SC.STRIDE, 0.0, 0.0, out["best_idx"], w["polar"], out["polar"], loc.shape)
    sr, best_lp = G._pick_forward(1, SC.STRIDE, SC.STRIDE_LP, SC.MAG, SC.ROT_UNIT, cls_lp, loc_lp)
    out["pick_grad_loc_lp"] = G._pick_backward(1, SC.STRIDE_LP, SC.MAG, SC.ROT_UNIT, best_lp, torch.stack([w["scale"], w["rot"]]), sr, loc_lp.shape)
    res = G._warps_forward(CFG_T, cls_lp, loc_lp, out["polar"], tcx, tcy, poly)
    out.update(zip(FWD, res))
    assert torch.equal(best_lp, out["best_idx_lp"]) and torch.equal(_bits(sr[0]), _bits(out["scale"])) and torch.equal(_bits(sr[1]), _bits(out["rot"]))
    out["grad_loc_lp"], out["grad_polar"] = G._warps_backward(CFG_T, res[0], res[1], res[2], out["polar"], poly, loc_lp.shape, [w[k] for k in UP])
    g_chain = (w["polar"] + out["grad_polar"]).contiguous()                 # one fp32 addition, as autograd accumulates the two uses of polar
    out["chain_grad_loc"] = G._pick_backward(0, SC.STRIDE, 0.0, 0.0, out["best_idx"], g_chain, out["polar"], loc.shape)
    torch.cuda.synchronize()
    for a, b in zip(keep, (cls, loc, cls_lp, loc_lp, tcx, tcy, poly)):      # the inputs are as they were, NaN included
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    return out


_worst = {}


@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_every_case(name, dev, monkeypatch):
    """every_cell_S*: B = S S, sample b's softmax winner is cell b and its raw winner cell n - 1 - b.  The other families as their names say."""
    c = SC.CASES[name]
    _nan_filled(monkeypatch)
    out = _run(c, dev)
    for k, v in out.items():
        assert _written(v), (name, k)
    r_hip = SC.check(out, c, what="hip")
    if c.want is not None:
        assert np.array_equal(out["best_idx"].cpu().numpy(), c.want) and np.array_equal(out["best_idx_lp"].cpu().numpy(), c.want_lp)
    monkeypatch.undo()
    out2 = _run(c, dev)                                                     # two calls are bit-equal
    for k in out:
        assert _same(out[k], out2[k]), k
    r_torch = 0.0
    if c.family != "nan_first":                                            # torch.argmax on NaN maps is not pinned; everywhere else PyTorch-ROCm is held to the same bound
        r_torch = SC.check(c.torch_run(torch.float32, dev), c, keys=SC.BOUNDED, what="PyTorch-ROCm fp32")
    _worst[name] = (r_hip, r_torch)
    print(f"SIMI {name}: worst error / bound  kernel {r_hip:.3f}  PyTorch-ROCm {r_torch:.3f}")


def test_worst_ratios():
    if len(_worst) != len(SC.CASE_NAMES):
        pytest.skip("needs the whole parametrised test above in the same run")
    print(f"SIMI worst error / bound over all cases: kernel {max(v[0] for v in _worst.values()):.3f}, PyTorch-ROCm {max(v[1] for v in _worst.values()):.3f}"
          f" ({SC.LIBM_ROUNDINGS} roundings per libm call and division, r_ref {SC.R_REF})")


@pytest.mark.parametrize("name", ["separated_B1", "separated_B2", "separated_B3", "separated_B65"])
def test_a_sample_does_not_depend_on_its_batch(name, dev):
    c = SC.CASES[name]
    whole = _run(c, dev)
    for b in sorted({0, c.B // 2, c.B - 1}):
        one = _run(c.sub(b), dev)
        for k, v in one.items():
            assert _same(v, whole[k][b:b + 1]), (name, b, k)


def test_optional_gradient_slots_and_null_upstreams(dev, monkeypatch):
    from hdn_amd import simi_geometry as G
    c = SC.CASES["separated_B3"]
    full = _run(c, dev)
    _nan_filled(monkeypatch)
    poly = _t(c.search_poly, dev)
    w = {k: _t(v, dev) for k, v in c.w.items()}
    args = (CFG_T, full["best_idx_lp"], full["scale"], full["rot"], full["polar"], poly, c.loc_lp.shape)
    for need in ((True, False), (False, True), (True, True)):               # each slot alone and both
        g = G._warps_backward(*args, [w[k] for k in UP], need)
        for got, want, asked in zip(g, (full["grad_loc_lp"], full["grad_polar"]), need):
            assert (got is None) == (not asked)
            if asked:
                assert torch.equal(_bits(got), _bits(want))
    with pytest.raises(ValueError):
        G._warps_backward(*args, [w[k] for k in UP], (False, False))
    # a NULL upstream gradient is read as zero: each upstream alone equals, bit for bit, the call with explicit zeros in the other slots
    zeros = {k: torch.zeros_like(w[k]) for k in UP}
    for k in UP:
        alone = G._warps_backward(*args, [w[q] if q == k else None for q in UP])
        same = G._warps_backward(*args, [w[q] if q == k else zeros[q] for q in UP])
        assert all(_written(x) for x in alone) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(alone, same)), k
        assert bool((alone[0] != 0).any()), k                                # every one of the five reaches loc_lp
    none = G._warps_backward(*args, [None] * 5)
    assert all(bool((x == 0).all()) for x in none)
    # the stand-alone matrices: each gradient slot alone and together
    a = SC.AFFINE_CASES["kind0_scale_h1_vector"]
    t = [_t(v, dev) for v in (a.cx, a.cy, a.nm, a.scale, a.rot, a.grad)]
    allg = G._affine_backward(0, True, SC.IN_SZ, SC.OUT_SZ, *t)
    assert all(_written(x) for x in allg)
    for i in range(3):
        need = tuple(j == i for j in range(3))
        g = G._affine_backward(0, True, SC.IN_SZ, SC.OUT_SZ, *t, need=need)
        assert [x is not None for x in g] == list(need) and torch.equal(_bits(g[i]), _bits(allg[i]))


def _affine_fn(c, cx, cy, nm, scale, rot):
    import hdn_amd
    if c.kind == 0:
        return hdn_amd.combine_affine_c0_v2(cx, cy, nm, scale, rot, c.scale_h, SC.IN_SZ, SC.OUT_SZ)
    return hdn_amd.combine_affine_lt0(cx, cy, nm, scale, rot, SC.IN_SZ, SC.OUT_SZ)


@pytest.mark.parametrize("name", SC.AFFINE_NAMES)
def test_the_two_matrices_alone(name, dev, monkeypatch):
    """both kinds, scale_h both ways, the centre as numbers and as vectors, rot in {0, +-pi/2, +-2.4} x scale in {0.2, 1, 4.8}, forward and backward
    through the drop-ins' autograd; PyTorch-ROCm's fp32 run of the restated functions beside it"""
    c = SC.AFFINE_CASES[name]
    _nan_filled(monkeypatch)
    got = c.torch_run(torch.float32, dev, fn=_affine_fn)
    assert all(_written(v) for v in got.values())
    r_hip = c.check(got, what="hip")
    monkeypatch.undo()
    again = c.torch_run(torch.float32, dev, fn=_affine_fn)
    assert all(torch.equal(_bits(got[k]), _bits(again[k])) for k in got)
    r_torch = c.check(c.torch_run(torch.float32, dev), what="PyTorch-ROCm fp32")
    print(f"SIMI affine {name}: worst error / bound  kernel {r_hip:.3f}  PyTorch-ROCm {r_torch:.3f}")
    with torch.no_grad():                                                   # the plain launch
        T = lambda a: _t(a, dev)
        cx, cy = (T(c.cx), T(c.cy)) if c.vec else (c.cx, c.cy)
        plain = _affine_fn(c, cx, cy, T(c.nm), T(c.scale), T(c.rot))
    assert not plain.requires_grad and torch.equal(_bits(plain), _bits(got["out"]))


def _package_pick(cls, loc):
    import hdn_amd
    return hdn_amd.polar_pick(cls, loc, stride=SC.STRIDE, return_index=True)


def _fused(c, dev):
    import hdn_amd

    def warps(cls_lp, loc_lp, polar):
        return hdn_amd.similarity_warps(cls_lp, loc_lp, polar, _t(c.temp_cx, dev), _t(c.temp_cy, dev), _t(c.search_poly, dev), return_index=True, **CFG)
    return c.torch_run(torch.float32, dev, pick=_package_pick, warps=warps)


def _drop_ins(c, dev):
    """the reference's lines restated, with the four drop-ins inside"""
    import hdn_amd
    picker = types.SimpleNamespace(points=torch.from_numpy(SC.analytic_points(SC.STRIDE, c.S)))
    B = c.B

    def pick(cls, loc):
        polar = hdn_amd.get_polar_from_two_para_loc(picker, cls, loc * SC.STRIDE)
        return polar, hdn_amd.polar_pick(cls, loc.detach(), return_index=True)[1]

    def warps(cls_lp, loc_lp, polar):
        scale, rot, best = hdn_amd.lp_pick(cls_lp, loc_lp, 2, SC.STRIDE, SC.STRIDE_LP, c.S, SC.MAP_SIZE, return_index=True)
        ones, zeros, zeros2 = torch.ones([B], device=dev), torch.zeros([B], device=dev), torch.zeros([B, 2], device=dev)
        tcx, tcy, poly = _t(c.temp_cx, dev), _t(c.temp_cy, dev), _t(c.search_poly, dev)
        res = {"best_idx_lp": best, "scale": scale, "rot": rot,
               "affine_m": hdn_amd.combine_affine_c0_v2(HALF, HALF, polar, scale, rot, True, SC.IN_SZ, SC.OUT_SZ),
               "affine_m_lt0": hdn_amd.combine_affine_lt0(HALF, HALF, polar, 1 / scale, -rot, SC.IN_SZ, SC.OUT_SZ),
               "affine_m_c_aug": hdn_amd.combine_affine_c0_v2(tcx, tcy, zeros2, ones, zeros, True, SC.IN_SZ, SC.OUT_SZ),
               "affine_m_lt0_aug": hdn_amd.combine_affine_lt0(tcx, tcy, zeros2, ones, zeros, SC.IN_SZ, SC.OUT_SZ)}
        hmg = torch.cat([poly.permute(0, 2, 1), torch.ones([B, 1, 4], device=dev)], 1)
        last = torch.tensor([0.0, 0.0, 1.0], device=dev).repeat([B, 1, 1])
        res["aug_sear_points"] = torch.bmm(torch.cat([res["affine_m_lt0_aug"], last], 1), hmg)
        res["pred_points"] = torch.bmm(torch.cat([res["affine_m_lt0"], last], 1), hmg)
        return res
    return c.torch_run(torch.float32, dev, pick=pick, warps=warps)


@pytest.mark.parametrize("name", ["separated_B3", "step_B32", "every_cell_S9"])
def test_autograd_through_the_fused_form_and_through_the_drop_ins(name, dev):
    """torch.autograd.grad of the weighted scalars; each against float64 autograd of the restatement (the truth of check), and the two against each other"""
    c = SC.CASES[name]
    fused, drop = _fused(c, dev), _drop_ins(c, dev)
    r_f, r_d = SC.check(fused, c, what="fused autograd"), SC.check(drop, c, what="drop-in autograd")
    t64, tr = c.torch_run(torch.float64), c.truth()
    for k in SC.BOUNDED:
        assert np.abs(t64[k].numpy() - tr["q"][k].v).max() <= 1e-12 * max(1.0, np.abs(tr["q"][k].v).max()), k   # the truth is float64 autograd
        diff = (fused[k].double() - drop[k].double()).abs().cpu().numpy()
        assert (diff <= tr["q"][k].e).all(), (name, k)
    for k in ("best_idx", "best_idx_lp"):
        assert torch.equal(fused[k].cpu().long(), drop[k].cpu().long())
    explicit = _run(c, dev)                                                 # autograd delivers what the explicit launches deliver
    for k in ("grad_loc_lp", "grad_polar", "pick_grad_loc", "pick_grad_loc_lp", "chain_grad_loc"):
        assert torch.equal(_bits(fused[k]), _bits(explicit[k])), k
    print(f"SIMI autograd {name}: worst error / bound  fused {r_f:.3f}  drop-ins {r_d:.3f}")


def test_raises(dev):
    import hdn_amd
    c = SC.CASES["separated_B3"]
    T = lambda a: _t(a, dev)
    good = dict(cls_lp=T(c.cls_lp), loc_lp=T(c.loc_lp).requires_grad_(True), polar=T(c.truth()["exact"]["polar"]), temp_cx=T(c.temp_cx),
                temp_cy=T(c.temp_cy), search_poly=T(c.search_poly))
    for k in ("cls_lp", "temp_cx", "temp_cy", "search_poly"):               # data inputs are never detached silently
        bad = dict(good)
        bad[k] = good[k].clone().requires_grad_(True)
        with pytest.raises(ValueError, match="data"):
            hdn_amd.similarity_warps(**bad)
    with pytest.raises(ValueError, match="data"):
        hdn_amd.polar_pick(T(c.cls).requires_grad_(True), T(c.loc))
    with pytest.raises(ValueError, match="data"):
        hdn_amd.lp_pick(T(c.cls_lp).requires_grad_(True), T(c.loc_lp), 2, 8, 8, c.S, 127)
    with pytest.raises(ValueError, match="data"):
        hdn_amd.combine_affine_c0_v2(T(c.temp_cx).requires_grad_(True), T(c.temp_cy), good["polar"], T(c.temp_cx), T(c.temp_cy), True, 255, 127)
    with pytest.raises(ValueError):
        hdn_amd.similarity_warps(**{**good, "polar": good["polar"][:2]})
    with pytest.raises(TypeError):
        hdn_amd.polar_pick(T(c.cls), T(c.loc).double())
    # first order only
    out = hdn_amd.similarity_warps(**good)
    g, = torch.autograd.grad(out["affine_m"].sum(), good["loc_lp"], create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    loc = T(c.loc).requires_grad_(True)
    g, = torch.autograd.grad(hdn_amd.polar_pick(T(c.cls), loc).sum(), loc, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    # under no_grad a call is the plain launch
    with torch.no_grad():
        plain = hdn_amd.similarity_warps(**good)
    assert not any(v.requires_grad for v in plain.values()) and all(torch.equal(_bits(plain[k]), _bits(out[k])) for k in plain)


def test_capture_and_replay_on_new_inputs(dev):
    """polar_pick + similarity_warps + backward captured once on one stream (no parallel branches), replayed after the inputs were overwritten in place"""
    import hdn_amd
    a, b = SC.CASES["step_B32"], SC.Case("step_B32_other", "separated", 32, 13, 601)
    T = lambda x: _t(x, dev)
    names = ("cls", "loc", "cls_lp", "loc_lp", "temp_cx", "temp_cy", "search_poly")
    buf = {k: T(getattr(a, k)) for k in names}
    w = {k: T(v) for k, v in a.w.items()}
    buf["loc"].requires_grad_(True)
    buf["loc_lp"].requires_grad_(True)

    def step():
        polar = hdn_amd.polar_pick(buf["cls"], buf["loc"], stride=SC.STRIDE)
        out = hdn_amd.similarity_warps(buf["cls_lp"], buf["loc_lp"], polar, buf["temp_cx"], buf["temp_cy"], buf["search_poly"], **CFG)
        total = (w["polar"] * polar).sum() + sum((w[k] * out[k]).sum() for k in ("affine_m", "affine_m_lt0", "pred_points"))
        g = torch.autograd.grad(total, (buf["loc"], buf["loc_lp"]))
        return [polar] + [out[k] for k in hdn_amd.simi_geometry.WARP_KEYS] + list(g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    for case in (b, a):
        with torch.no_grad():
            for k in names:
                buf[k].copy_(T(getattr(case, k)))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [x.clone() for x in held]
        eager = step()
        torch.cuda.synchronize()
        for i, (x, y) in enumerate(zip(replayed, eager)):
            assert torch.equal(_bits(x), _bits(y)), (case.name, i)
    assert not torch.equal(_bits(T(a.loc)), _bits(T(b.loc)))


def test_install_train_on_stand_ins_and_one_step(dev, monkeypatch):
    import hdn_amd
    import hdn_amd.install as hinstall
    site = types.ModuleType(hinstall.SIMI_GEOMETRY_SITE)
    lp = types.ModuleType("hdn.models.logpolar")

    def theirs(*a, **k):
        raise AssertionError("the reference's function was called")

    class Polar_Pick:
        def __init__(self, S):
            self.points = torch.from_numpy(SC.analytic_points(SC.STRIDE, S))

        get_polar_from_two_para_loc = theirs
    lp.Polar_Pick = Polar_Pick
    for n in hinstall.SIMI_GEOMETRY_NAMES:
        setattr(site, n, theirs)
    monkeypatch.setattr(hinstall, "SIMI_GEOMETRY_TRAIN_BOUND", True)
    c = SC.CASES["step_B32"]
    done = hinstall.install(modules={hinstall.SIMI_GEOMETRY_SITE: site, "hdn.models.logpolar": lp}, train=True)
    try:
        assert len([d for d in done if d[1] in hinstall.SIMI_GEOMETRY_NAMES or "get_polar" in d[1]]) == 4
        picker = Polar_Pick(c.S)

        def pick(cls, loc):
            return picker.get_polar_from_two_para_loc(cls, loc * SC.STRIDE), hdn_amd.polar_pick(cls, loc.detach(), return_index=True)[1]

        def warps(cls_lp, loc_lp, polar):
            scale, rot = site.lp_pick(cls_lp, loc_lp, 2, SC.STRIDE, SC.STRIDE_LP, c.S, SC.MAP_SIZE)
            m = site.combine_affine_c0_v2(HALF, HALF, polar, scale, rot, True, SC.IN_SZ, SC.OUT_SZ)
            m_lt0 = site.combine_affine_lt0(HALF, HALF, polar, 1 / scale, -rot, SC.IN_SZ, SC.OUT_SZ)
            poly = _t(c.search_poly, dev)
            hmg = torch.cat([poly.permute(0, 2, 1), torch.ones([c.B, 1, 4], device=dev)], 1)
            last = torch.tensor([0.0, 0.0, 1.0], device=dev).repeat([c.B, 1, 1])
            return {"scale": scale, "rot": rot, "affine_m": m, "affine_m_lt0": m_lt0, "pred_points": torch.bmm(torch.cat([m_lt0, last], 1), hmg)}
        got = c.torch_run(torch.float32, dev, pick=pick, warps=warps)
        SC.check(got, c, what="installed")
    finally:
        hinstall.uninstall()
    assert site.lp_pick is theirs and Polar_Pick.__dict__["get_polar_from_two_para_loc"] is theirs
