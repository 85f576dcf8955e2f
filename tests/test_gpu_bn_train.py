"""The training BatchNorm + ReLU on the device: hdn_bn_relu_train_fwd_f32 / _bwd_f32 against float64 in both forms, both layouts on either side, with and
without the ReLU and the running buffers; the large-mean problem; exact problems; float-aligned NCHW planes; NaN; guarded arenas; the autograd Function;
a captured graph; the rebound head branches with install.HEAD_BN_TRAIN_BOUND forced on.  Cases, builders and bounds are tests/bn_train_cases.py's, which
tests/test_bn_train_host.py holds to float64 autograd without a GPU."""
import copy
import itertools
import os
import sys
import types

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bn_train_cases as BC  # noqa: E402
import buffer_guard as BG  # noqa: E402
from hdn_amd import _lib, batchnorm_relu_train, bn_train as BT, conv_train as CT  # noqa: E402  (without the feature nothing here is collected)

pytestmark = pytest.mark.gpu

CL = torch.channels_last
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _y_flat(y, B, P, C, nchw):
    """y of a raw call as [B][C][P], whichever layout it was written in."""
    return y.reshape(B, C, P) if nchw else y.reshape(B, P, C).permute(0, 2, 1)


def run_raw(dev, prob, B, P, C, relu, y_nchw, dy_nchw, track, eps=BC.EPS, momentum=BC.MOMENTUM, need=(True, True, True)):
    """One forward and one backward through the raw wrappers on flat buffers pre-filled with NaN: y [B][C][P], dc [N][C], ..."""
    c, gamma, beta, dy, rm0, rv0 = (t.to(dev) for t in prob)
    c4 = BC.as4(c, B, P, C)
    rm, rv = (rm0.clone(), rv0.clone()) if track else (None, None)
    y = torch.full((B * P * C, ), float("nan"), device=dev)
    stats = torch.full((2 * C, ), float("nan"), device=dev)
    BT.forward(c4, gamma, beta, rm, rv, momentum, eps, relu, y_nchw, out=y, stats=stats)
    dyd = dy.contiguous() if dy_nchw else dy.permute(0, 2, 1).contiguous()
    dc, dgamma, dbeta = BT.backward(dyd, c4, gamma, beta, stats, relu, dy_nchw, need)
    return {"y": _y_flat(y, B, P, C, y_nchw), "dc": None if dc is None else dc.permute(0, 2, 3, 1).reshape(B * P, C), "dgamma": dgamma, "dbeta": dbeta,
            "mean": stats[:C], "invstd": stats[C:], "rm": rm, "rv": rv}


def check_against_float64(dev, kind, case, worst):
    B, P, C = case
    prob = BC.random_problem(*case) if kind == "a" else BC.large_mean_problem(*case)
    for relu, y_nchw, dy_nchw, track in itertools.product((0, 1), (0, 1), (0, 1), (True, False)):
        truth, ref32 = BC.references(kind, B, P, C, relu)
        got = run_raw(dev, prob, B, P, C, relu, y_nchw, dy_nchw, track)
        again = run_raw(dev, prob, B, P, C, relu, y_nchw, dy_nchw, track)
        tag = (case, relu, y_nchw, dy_nchw, track)
        for name in ("y", "dc", "dgamma", "dbeta"):
            err, lim = BC.bound(got[name].cpu(), truth[name], ref32[name])
            worst[name] = max(worst.get(name, 0.0), err / lim)
            assert err <= lim, (tag, name, err, lim)
        std = 1.0 / truth["invstd"]
        for name, rel in (("invstd", truth["invstd"].abs()), ("mean", torch.maximum(truth["mean"].abs(), std))) + \
                ((("rv", truth["rv"].abs()), ("rm", torch.maximum(truth["mean"].abs(), std))) if track else ()):
            err = (got[name].cpu().double() - truth[name].float().double()).abs()
            worst[name] = max(worst.get(name, 0.0), float((err / (ULP * rel)).max()))
            assert bool((err <= ULP * rel).all()), (tag, name, float((err / rel).max()))
        for name, t in got.items():
            assert (t is None) == (again[name] is None) and (t is None or torch.equal(t, again[name])), (tag, name)      # two calls: the same bits


# ------------------------------------------------------------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("case", BC.CASES)
def test_random_problems_against_float64(dev, case):
    worst = {}
    check_against_float64(dev, "a", case, worst)
    form = _lib.load().hdn_bn_relu_train_form(*case)
    print(f"FORMS bn_relu_train {case} form {form}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------------------------------- 2. the large mean
@pytest.mark.parametrize("case", BC.LARGE_MEAN_CASES)
def test_a_mean_of_a_thousand_standard_deviations(dev, case):
    worst = {}
    check_against_float64(dev, "c", case, worst)
    print(f"FORMS bn_relu_train large mean {case}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ----------------------------------------------------------------------------------------------------------------------------------- 3. exact
@pytest.mark.parametrize("case", BC.EXACT_CASES)
def test_exact_problems_are_exact(dev, case):
    B, P, C = case
    prob, expect = BC.exact_problem(*case)
    for relu, y_nchw, dy_nchw in itertools.product((0, 1), (0, 1), (0, 1)):
        got = run_raw(dev, prob, B, P, C, relu, y_nchw, dy_nchw, True, eps=BC.EXACT_EPS, momentum=BC.EXACT_MOMENTUM)
        for name in ("y", "dc", "dgamma", "dbeta", "rm", "mean"):
            d = BG.first_difference(got[name].cpu(), expect[relu][name].float())
            assert d is None, (case, relu, y_nchw, dy_nchw, name, d)


# ------------------------------------------------------------------------------------------------------- 4. float alignment of the NCHW side
@pytest.mark.parametrize("case", [(3, 25, 32), (1, 169, 64)])
def test_nchw_planes_at_float_offsets(dev, case):
    B, P, C = case
    prob = BC.random_problem(*case)
    c, gamma, beta, dy, rm0, rv0 = (t.to(dev) for t in prob)
    c4, n = BC.as4(c, B, P, C), B * P * C
    want = run_raw(dev, prob, B, P, C, 1, 1, 1, False)        # 16-byte aligned buffers; test 1 holds it to float64
    for off in range(4):
        ybuf = torch.full((n + 8, ), float("nan"), device=dev)
        dybuf = torch.full((n + 8, ), float("nan"), device=dev)
        assert ybuf.data_ptr() % 16 == 0 and dybuf.data_ptr() % 16 == 0
        y, dyd = ybuf[off:off + n], dybuf[off:off + n]
        dyd.copy_(dy.reshape(-1))
        stats = torch.empty(2 * C, device=dev)
        BT.forward(c4, gamma, beta, None, None, BC.MOMENTUM, BC.EPS, True, True, out=y, stats=stats)
        dc, dgamma, dbeta = BT.backward(dyd, c4, gamma, beta, stats, True, True)
        assert torch.equal(y.view(B, C, P), want["y"]), off
        assert torch.equal(dc.permute(0, 2, 3, 1).reshape(B * P, C), want["dc"]), off
        assert torch.equal(dgamma, want["dgamma"]) and torch.equal(dbeta, want["dbeta"]), off
        assert bool(torch.isnan(ybuf[:off]).all()) and bool(torch.isnan(ybuf[off + n:]).all()), off


# ------------------------------------------------------------------------------------------------------------------------------------- 5. NaN
def test_a_nan_stays_in_its_channel(dev):
    B, P, C = 2, 25, 256
    prob = BC.random_problem(B, P, C)
    clean = run_raw(dev, prob, B, P, C, 1, 1, 1, True)
    c = prob[0].clone()
    c[17, 77] = float("nan")
    got = run_raw(dev, (c, ) + prob[1:], B, P, C, 1, 1, 1, True)
    assert bool(torch.isnan(got["y"][:, 77]).all())
    keep = torch.arange(C, device=dev) != 77
    assert torch.equal(got["y"][:, keep], clean["y"][:, keep])
    for name in ("mean", "invstd", "rm", "rv"):
        assert torch.equal(got[name][keep], clean[name][keep]), name
    assert bool(torch.isnan(got["mean"][77]))


# ----------------------------------------------------------------------------------------------------------------------- 6. buffer discipline
@pytest.mark.parametrize("case", BC.EXACT_CASES)
def test_both_entry_points_stay_inside_their_buffers(dev, case):
    B, P, C = case
    lib = _lib.load()
    prob, expect = BC.exact_problem(*case)
    c, gamma, beta, dy, rm0, rv0 = prob
    nws = int(lib.hdn_bn_relu_train_workspace_bytes(B, P, C))
    assert (nws == 0) == (lib.hdn_bn_relu_train_form(B, P, C) == 0)
    stats = torch.cat([expect[1]["mean"], expect[1]["invstd"]]).float()           # what the forward is held to below; the same for either relu
    for relu, nchw in itertools.product((0, 1), (0, 1)):
        track = relu == nchw                                                      # running buffers given / NULL
        offs = BG.offsets16(8, start=2 * relu + nchw)
        g = BG.Guard(dev)
        g.input("c", c, offs[0]); g.input("gamma", gamma, offs[1]); g.input("beta", beta, offs[2])
        g.output("y", (B * P * C, ), offs[3]); g.output("stats", (2 * C, ), offs[4]); g.workspace("ws", nws, offs[7])
        if track:
            g.inout("rm", rm0, offs[5]); g.inout("rv", rv0, offs[6])
        run = lambda g: _lib.launch("fwd", dev, lib.hdn_bn_relu_train_fwd_f32, g.ptr("c"), g.ptr("gamma"), g.ptr("beta"), g.ptr("y"), g.ptr("stats"),
                                    g.ptr("rm") if track else None, g.ptr("rv") if track else None, BC.EXACT_MOMENTUM, BC.EXACT_EPS, g.ptr("ws"),
                                    g.nbytes("ws"), B, P, C, relu, nchw)
        rc = g.run(run)
        torch.cuda.synchronize()
        assert rc is None and g.verdict() == [], (case, relu, nchw, g.verdict())
        assert torch.equal(_y_flat(g.result("y"), B, P, C, nchw).cpu(), expect[relu]["y"].float()), (case, relu, nchw)
        assert torch.equal(g.result("stats").cpu(), stats), (case, relu, nchw)
        assert not track or torch.equal(g.result("rm").cpu(), expect[relu]["rm"].float())

        # the backward with every set of outputs an operator asks for; without dc the apply pass (form 1: its launch) is skipped
        for outs in (("dc", "dgamma", "dbeta"), ("dgamma", "dbeta"), ("dc", )):
            g = BG.Guard(dev)
            g.input("dy", dy if nchw else dy.permute(0, 2, 1).contiguous(), offs[0]); g.input("c", c, offs[1]); g.input("gamma", gamma, offs[2])
            g.input("beta", beta, offs[3]); g.input("stats", stats, offs[4]); g.workspace("ws", nws, offs[0])
            for k, name in enumerate(outs):
                g.output(name, (B * P, C) if name == "dc" else (C, ), offs[5 + k])
            ptr = lambda g, name: g.ptr(name) if name in outs else None
            rc = g.run(lambda g: _lib.launch("bwd", dev, lib.hdn_bn_relu_train_bwd_f32, g.ptr("dy"), g.ptr("c"), g.ptr("gamma"), g.ptr("beta"),
                                             g.ptr("stats"), ptr(g, "dc"), ptr(g, "dgamma"), ptr(g, "dbeta"), g.ptr("ws"), g.nbytes("ws"), B, P, C,
                                             relu, nchw))
            torch.cuda.synchronize()
            assert rc is None and g.verdict() == [], (case, relu, nchw, outs, g.verdict())
            for name in outs:
                assert torch.equal(g.result(name).cpu(), expect[relu][name].float()), (case, relu, nchw, outs, name)


# ---------------------------------------------------------------------------------------------------------------------------- 7. the operator
@pytest.mark.parametrize("case", [(3, 25, 32), (BC.THRESHOLD_CASES[1][0], 25, 256)])
def test_the_operator_against_the_float64_twin(dev, case):
    B, P, C = case
    prob = BC.random_problem(*case)
    c, gamma, beta, dy, rm0, rv0 = (t.to(dev) for t in prob)
    truth, ref32 = BC.references("a", B, P, C, 1)
    shape = BC.shape4(B, P, C)
    for needs in itertools.product((True, False), repeat=3):
        for layout in ("cl", "nchw"):
            c4 = BC.as4(c, B, P, C)
            cd = (c4.clone(memory_format=torch.preserve_format) if layout == "cl" else c4.contiguous()).requires_grad_(needs[0])
            gd, bd = gamma.clone().requires_grad_(needs[1]), beta.clone().requires_grad_(needs[2])
            rm, rv = rm0.clone(), rv0.clone()
            before = dict(BT.launches)
            y = batchnorm_relu_train(cd, gd, bd, rm, rv, BC.MOMENTUM, BC.EPS)
            assert y.is_contiguous() and tuple(y.shape) == shape and y.requires_grad == any(needs)
            err, lim = BC.bound(y.detach().reshape(B, C, P).cpu(), truth["y"], ref32["y"])
            assert err <= lim
            if any(needs):
                y.backward(dy.view(shape))
            made = {k: BT.launches[k] - before[k] for k in before}
            assert made == {"forward": 1, "backward": int(any(needs))}, (needs, made)
            for t, need, name in ((cd, needs[0], "dc"), (gd, needs[1], "dgamma"), (bd, needs[2], "dbeta")):
                assert (t.grad is None) == (not need), (needs, name)
                if need:
                    got = t.grad.permute(0, 2, 3, 1).reshape(B * P, C) if name == "dc" else t.grad
                    err, lim = BC.bound(got.cpu(), truth[name], ref32[name])
                    assert err <= lim, (needs, layout, name, err, lim)
    # out_nchw=False, relu=False, no running buffers
    t0, r0 = BC.references("a", B, P, C, 0)
    y = batchnorm_relu_train(BC.as4(c, B, P, C), gamma, beta, relu=False, out_nchw=False)
    assert y.is_contiguous(memory_format=CL) or P == 1
    err, lim = BC.bound(y.permute(0, 2, 3, 1).reshape(B, P, C).permute(0, 2, 1).cpu(), t0["y"], r0["y"])
    assert err <= lim
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        batchnorm_relu_train(torch.zeros(1, 32, 1, 1, device=dev), gamma[:32], beta[:32])
    assert BT.qualifies(nn.BatchNorm2d(64).to(dev)) and BT.qualifies(nn.BatchNorm2d(64).to(dev), torch.zeros(2, 64, 3, 3, device=dev))
    assert not BT.qualifies(nn.BatchNorm2d(64).to(dev), torch.zeros(2, 32, 3, 3, device=dev)) and not BT.qualifies(nn.BatchNorm2d(64))


# ------------------------------------------------------------------------------------------------------------------------------------ 8. graph
def test_forward_backward_replay_sees_in_place_changes_and_advances_the_buffers(dev):
    B, P, C = 2, 25, 256
    prob = BC.random_problem(B, P, C)
    c, gamma, beta, dy, rm0, rv0 = (t.to(dev) for t in prob)
    shape = BC.shape4(B, P, C)
    cs = BC.as4(c, B, P, C).clone(memory_format=torch.preserve_format).requires_grad_(True)
    gs, bs = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv, dys = rm0.clone(), rv0.clone(), dy.view(shape).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            cs.grad = gs.grad = bs.grad = None
            batchnorm_relu_train(cs, gs, bs, rm, rv, BC.MOMENTUM, BC.EPS).backward(dys)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    cs.grad = gs.grad = bs.grad = None
    rm.copy_(rm0), rv.copy_(rv0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="global"):
        y = batchnorm_relu_train(cs, gs, bs, rm, rv, BC.MOMENTUM, BC.EPS)
        y.backward(dys)
    erm, erv = rm0.clone(), rv0.clone()
    g = torch.Generator().manual_seed(12)
    for k in range(3):
        with torch.no_grad():
            cs.add_(BC.as4(torch.randn(B * P, C, generator=g).to(dev), B, P, C) * 0.05)
            gs.mul_(1.25 if k else 0.5)
        graph.replay()
        torch.cuda.synchronize()
        ce, ge, be = (t.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) for t in (cs, gs, bs))
        ye = batchnorm_relu_train(ce, ge, be, erm, erv, BC.MOMENTUM, BC.EPS)
        ye.backward(dys)
        assert torch.equal(y, ye) and torch.equal(cs.grad, ce.grad) and torch.equal(gs.grad, ge.grad) and torch.equal(bs.grad, be.grad), k
        assert torch.equal(rm, erm) and torch.equal(rv, erv), k                     # advanced on every replay, as the eager calls advance theirs


# ------------------------------------------------------------------------------------------------------------------------------ 9. bound heads
def _stock_forward(self, kernel, search):
    kernel = self.conv_kernel(kernel)
    search = self.conv_search(search)
    feature = _XCORR[self.xcorr_name](search, kernel)
    return self.head(feature)


class DepthwiseXCorr(nn.Module):
    """A stand-in with the attribute layout of the reference's DepthwiseXCorr / DepthwiseXCorrCirc (conv_kernel, conv_search, head)."""

    def __init__(self, in_channels, hidden, out_channels, xcorr_name="xcorr_depthwise"):
        super().__init__()
        branch = lambda: nn.Sequential(nn.Conv2d(in_channels, hidden, kernel_size=3, bias=False), nn.BatchNorm2d(hidden), nn.ReLU(inplace=True))
        self.conv_kernel, self.conv_search = branch(), branch()
        self.head = nn.Sequential(nn.Conv2d(hidden, hidden, kernel_size=1, bias=False), nn.BatchNorm2d(hidden), nn.ReLU(inplace=True),
                                  nn.Conv2d(hidden, out_channels, kernel_size=1))
        self.xcorr_name = xcorr_name

    def forward(self, kernel, search):
        return _stock_forward(self, kernel, search)


class DepthwiseXCorrCirc(DepthwiseXCorr):
    def __init__(self, in_channels, hidden, out_channels):
        super().__init__(in_channels, hidden, out_channels, "xcorr_depthwise_circular")

    def forward(self, kernel, search):          # its own forward, as the reference's class has
        return _stock_forward(self, kernel, search)


from oracle import hdn_oracle as O  # noqa: E402

_XCORR = {"xcorr_depthwise": O.xcorr_depthwise, "xcorr_depthwise_circular": O.xcorr_depthwise_circular}
_seen = []          # what reached the correlation of the bound forward: (search, kernel) per call
_bound_xcorr = {}   # xcorr name -> the correlation install() bound at the stand-in modules (hdn_amd.xcorr's)


def _spy(fn):
    def xcorr(search, kernel):
        _seen.append((search, kernel))
        return fn(search, kernel)
    return xcorr


def _standin_modules():
    ban = types.SimpleNamespace(DepthwiseXCorr=DepthwiseXCorr, xcorr_depthwise=O.xcorr_depthwise)
    ban_lp = types.SimpleNamespace(DepthwiseXCorrCirc=DepthwiseXCorrCirc, xcorr_depthwise_circular=O.xcorr_depthwise_circular)
    return {"hdn.models.head.ban": ban, "hdn.models.head.ban_lp": ban_lp}


@pytest.fixture
def bound_heads(monkeypatch):
    import hdn_amd.install as hi
    monkeypatch.setattr(hi, "HEAD_CONV_TRAIN_BOUND", True)
    monkeypatch.setattr(hi, "HEAD_BN_TRAIN_BOUND", True)
    # the 1x1 tail's convolutions are the library's, which picks an algorithm per process and call: pinned, as tests/test_gpu_train_step_graph.py and
    # tests/test_gpu_simi_training_forward.py pin theirs, so that two runs of one path can be held to each other bit for bit
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    orig = {c: c.__dict__["forward"] for c in (DepthwiseXCorr, DepthwiseXCorrCirc)}
    mods = _standin_modules()
    hi.install(train=True, modules=mods)
    for mod, name in ((mods["hdn.models.head.ban"], "xcorr_depthwise"), (mods["hdn.models.head.ban_lp"], "xcorr_depthwise_circular")):
        _bound_xcorr[name] = getattr(mod, name)                  # install() bound hdn_amd.xcorr's correlation there
        setattr(mod, name, _spy(_bound_xcorr[name]))             # (the dispatcher resolves the attribute at every call)
    yield orig
    hi.uninstall()
    assert all(c.__dict__["forward"] is f for c, f in orig.items())                 # uninstall() restores everything


def _run(mod, z, x, fwd=None):
    mod.train()
    for p in mod.parameters():
        p.grad = None
    out = fwd(mod, z, x) if fwd else mod(z, x)
    loss = (out * out).mean()
    loss.backward()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in mod.named_parameters()}


def test_a_batchnorm_frozen_by_its_own_eval_keeps_the_module(dev, bound_heads):
    torch.manual_seed(9)
    m = DepthwiseXCorr(32, 32, 4).to(dev).train()
    m.conv_kernel[1].eval()                                   # frozen inside a .train() parent: running statistics are used and left alone
    with torch.no_grad():
        m.conv_kernel[1].running_mean.normal_()
        m.conv_kernel[1].running_var.uniform_(0.5, 1.5)
    stock = copy.deepcopy(m)
    frozen = {n: b.clone() for n, b in m.conv_kernel[1].named_buffers()}
    z, x = torch.randn(3, 32, 7, 7, device=dev).clamp_min(0).contiguous(memory_format=CL), torch.randn(3, 32, 15, 15, device=dev).clamp_min(0).contiguous(memory_format=CL)
    before = dict(BT.launches)
    with torch.device(dev):
        out = m(z, x)
        want = bound_heads[DepthwiseXCorr](stock, z, x)
    assert {k: BT.launches[k] - before[k] for k in before} == {"forward": 1, "backward": 0}      # conv_search's only
    assert all(torch.equal(b, frozen[n]) for n, b in m.conv_kernel[1].named_buffers())
    assert int(m.conv_search[1].num_batches_tracked) == 1
    assert torch.allclose(out, want, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("klass,C,sk,ss", [(DepthwiseXCorr, 32, 7, 15), (DepthwiseXCorrCirc, 64, 9, 9)])
def test_bound_head_branches_with_the_fused_batchnorm(dev, bound_heads, monkeypatch, klass, C, sk, ss):
    import hdn_amd.install as hi
    torch.manual_seed(C)
    B = 3
    m = klass(C, C, 4)
    twin64, twin32, stock = copy.deepcopy(m).double(), copy.deepcopy(m), copy.deepcopy(m).to(dev)
    off, today_m = copy.deepcopy(m).to(dev), copy.deepcopy(m).to(dev)
    m = m.to(dev)
    zf, xf = torch.randn(B, C, sk, sk).clamp_min(0), torch.randn(B, C, ss, ss).clamp_min(0)
    zd, xd = zf.to(dev).contiguous(memory_format=CL), xf.to(dev).contiguous(memory_format=CL)
    orig = bound_heads

    # what reaches _Conv3x3Valid.backward is already channels-last: _cl returns its argument
    real_cl, handed = CT._cl, []

    def spy_cl(t):
        out = real_cl(t)
        handed.append(out is t)
        return out
    monkeypatch.setattr(CT, "_cl", spy_cl)
    del _seen[:]
    before, cbefore = dict(BT.launches), dict(CT.launches)
    with torch.device(dev):
        loss, grads = _run(m, zd, xd)
    made = {k: BT.launches[k] - before[k] for k in before}
    assert made == {"forward": 2, "backward": 2}, made
    assert CT.launches["forward"] - cbefore["forward"] == 2 and CT.launches["wgrad"] - cbefore["wgrad"] == 2
    assert len(_seen) == 1 and all(t.is_contiguous() for t in _seen[0])             # the correlation gets contiguous NCHW maps: no copy in front
    assert handed and all(handed), handed                                           # forward inputs and both backward gradients: no layout copy
    monkeypatch.setattr(CT, "_cl", real_cl)

    l64, g64 = _run(twin64, zf.double(), xf.double(), orig[klass])
    l32, g32 = _run(twin32, zf, xf, orig[klass])
    e_ref, scale = abs(float(l32) - float(l64)), abs(float(l64))
    print(f"FORMS bn_relu_train module {klass.__name__} loss: err {abs(float(loss) - float(l64)):.3e}, bound {4 * e_ref + 1e-5 * scale:.3e}")
    assert abs(float(loss) - float(l64)) <= 4 * e_ref + 1e-5 * scale
    for n in g64:
        err = float((grads[n].cpu().double() - g64[n]).abs().max())
        e_ref, scale = float((g32[n].double() - g64[n]).abs().max()), float(g64[n].abs().max())
        print(f"FORMS bn_relu_train module {klass.__name__} {n}: err {err:.3e}, e_ref {e_ref:.3e}, scale {scale:.3e}, "
              f"err/bound {err / (4 * e_ref + 1e-5 * scale):.3f}")
        assert err <= 4 * e_ref + 1e-5 * scale, n
    with torch.device(dev):              # (the oracle's circular pad builds its index vectors on the default device)
        _run(stock, zd, xd, orig[klass])
    for (n, b), (_, bs) in zip(m.named_buffers(), stock.named_buffers()):
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(bs) == 1, n
        else:
            assert torch.allclose(b, bs, rtol=1e-5, atol=1e-6), n

    # HEAD_BN_TRAIN_BOUND off: no BatchNorm launch, today's path bit for bit (the convolution on HIP, the sequential's own BatchNorm and ReLU)
    monkeypatch.setattr(hi, "HEAD_BN_TRAIN_BOUND", False)
    before = dict(BT.launches)

    def today(self, kernel, search):
        k = self.conv_kernel[2](self.conv_kernel[1](CT.conv3x3_valid(kernel, self.conv_kernel[0].weight)))
        s = self.conv_search[2](self.conv_search[1](CT.conv3x3_valid(search, self.conv_search[0].weight)))
        return self.head(_bound_xcorr[self.xcorr_name](s, k))
    with torch.device(dev):
        l_off, g_off = _run(off, zd, xd)
        l_ref, g_ref = _run(today_m, zd, xd, today)
    assert BT.launches == before
    assert torch.equal(l_off, l_ref)
    assert all(torch.equal(a, b) for a, b in zip(off.buffers(), today_m.buffers()))
    for n in g_ref:
        d = BG.first_difference(g_off[n], g_ref[n])
        assert d is None, (n, d)
    monkeypatch.setattr(hi, "HEAD_BN_TRAIN_BOUND", True)

    # .eval(): the class's own forward, no launch
    before, cbefore = dict(BT.launches), dict(CT.launches)
    m.eval()
    with torch.no_grad(), torch.device(dev):
        a, b = m(zd, xd), orig[klass](m, zd, xd)
    assert torch.equal(a, b) and BT.launches == before and CT.launches == cbefore
