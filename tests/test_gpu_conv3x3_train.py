"""The heads' 3x3 convolutions in training on the device: hdn_pack_conv3x3d_dev_f32 against the host packer, hdn_grad_scale_f32,
hdn_conv3x3v_dgrad_f32 and hdn_conv3x3v_wgrad_f32 exactly (integer data), by position (one nonzero element), against float64 in every launch form,
under power-of-two scalings of the gradient, through autograd (hdn_amd.conv3x3_valid), through the rebound head branches
(install(train=True) with HEAD_CONV_TRAIN_BOUND forced on) and replayed from a hipGraph, alone and inside a whole GatedAMSGrad iteration.
Truths, cases and the checks are tests/conv3x3_train_cases.py's, which tests/test_conv3x3_train_host.py holds to float64 autograd without a GPU."""
import copy
import functools
import os
import sys
import types

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv3x3_train_cases as TC  # noqa: E402
from hdn_amd import conv3x3_valid, conv_train as CT  # noqa: E402  (without the feature nothing here is collected)

pytestmark = pytest.mark.gpu

CL = torch.channels_last


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _cl(t, dev):
    return t.float().to(dev).contiguous(memory_format=CL)


def direct(dev, x, w, dy, need=("gx", "gw")):
    """(gx, gw) through the entry points, outputs pre-filled with NaN."""
    xd, wd, dyd = _cl(x, dev), w.float().to(dev).contiguous(), _cl(dy, dev)
    B, CI, S, _ = x.shape
    e = CT.grad_scale(dyd)
    gx = gw = None
    if "gx" in need:
        gx = torch.full((B, CI, S, S), float("nan"), device=dev).contiguous(memory_format=CL)
        CT.dgrad(dyd, wd, e, S, out=gx)
    if "gw" in need:
        gw = torch.full(tuple(w.shape), float("nan"), device=dev)
        CT.wgrad(xd, dyd, e, out=gw)
    return gx, gw


@functools.lru_cache(maxsize=None)
def reference(case):
    x, w, dy = TC.random_problem(*case)
    return (x, w, dy) + TC.reference_backward(x, w, dy)


# ------------------------------------------------------------------------------------------------------------------------------ 1. the packer
@pytest.mark.parametrize("CO,CI", TC.PACK_CASES)
def test_device_packer_writes_the_host_packers_bytes(dev, CO, CI):
    from hdn_amd import _lib
    from hdn_amd.ops import pack_conv3x3d
    lib = _lib.load()
    w = torch.randn(CO, CI, 3, 3, generator=torch.Generator().manual_seed(CO + CI)) * 3.0
    w[0, 0, 0, 0], w[1, 2, 1, 1], w[CO - 1, CI - 1, 2, 2] = 1e-7, -6.0e4, 3.1e-5       # subnormal pieces, the top of the range
    n = lib.hdn_pack_conv3x3d_bytes(CO, CI)
    wd = w.to(dev)
    for mode, src in ((0, w), (1, TC.w_dgrad(w))):
        want = pack_conv3x3d(src).view(torch.uint8)
        assert want.numel() == n
        buf = torch.full((n + 128, ), 0xAB, dtype=torch.uint8, device=dev)
        CT.pack_dev(wd, mode, out=buf[64:64 + n])
        got = buf.cpu()
        assert torch.equal(got[64:64 + n], want), (mode, int((got[64:64 + n] != want).sum()))
        assert bool((got[:64] == 0xAB).all()) and bool((got[64 + n:] == 0xAB).all())
    CT.bad_weight_count(dev)
    wb = wd.clone()
    wb[3, 5, 0, 1], wb[7, 1, 2, 2], wb[2, 2, 2, 0] = float("inf"), float("nan"), 65504.0
    for mode in (0, 1):
        CT.pack_dev(wb, mode)
        assert CT.bad_weight_count(dev) == 3, mode
    CT.pack_dev(wd, 0)
    assert CT.bad_weight_count(dev) == 0


def test_grad_scale_is_the_exponent_rule(dev):
    g = torch.Generator().manual_seed(5)
    for n, mag in ((1, 3.0), (5, 1e-7), (4099, 1e-30), (70001, 1e20), (1 << 20, 2.5e-6)):
        v = (torch.randn(n, generator=g) * mag).float()
        v[n // 2] = mag * 7
        assert int(CT.grad_scale(v.to(dev)).item()) == TC.grad_exponent(v), (n, mag)
    for special in (0.0, float("inf"), float("nan")):
        v = torch.zeros(1000)
        v[777] = special
        assert int(CT.grad_scale(v.to(dev)).item()) == 0


# ------------------------------------------------------------------------------------------------------------------------------------ 2. exact
@pytest.mark.parametrize("case", TC.EXACT_CASES)
def test_integer_problems_are_exact(dev, case):
    x, w, dy, y, gx, gw = TC.integer_problem(*case)
    assert TC.integer_sum_limit(*case) < 2 ** 24
    got_y = CT.forward(_cl(x, dev), w.float().to(dev))
    assert torch.equal(got_y.cpu().double(), y.double()), case
    got_gx, got_gw = direct(dev, x, w, dy)
    for name, got, want in (("gx", got_gx, gx), ("gw", got_gw, gw)):
        got = got.cpu().double()
        if not torch.equal(got, want.double()):
            bad = (got != want.double()).nonzero()
            raise AssertionError(f"{case} {name}: {bad.shape[0]} of {got.numel()} differ; first at {bad[0].tolist()}: got {float(got[tuple(bad[0])])!r}, "
                                 f"want {float(want[tuple(bad[0])])!r}")


# -------------------------------------------------------------------------------------------------------------------------------- 3. positions
def test_one_nonzero_element_reaches_only_its_window(dev):
    B, S, CI, CO = 3, 9, 64, 32
    So = S - 2
    g = torch.Generator().manual_seed(3)
    w = torch.randint(1, 6, (CO, CI, 3, 3), generator=g).float()
    x = torch.randint(1, 5, (B, CI, S, S), generator=g).float()
    for (b0, c0, y0, x0) in ((1, 17, 0, 0), (2, 5, 0, 3), (0, 31, 6, 6), (1, 9, 3, 4), (0, 1, 6, 2)):       # corners, edges, interior of dy
        dy = torch.zeros(B, CO, So, So)
        dy[b0, c0, y0, x0] = 2.0
        gx, gw = direct(dev, x, w, dy)
        gx, gw = gx.cpu(), gw.cpu()
        want = torch.zeros(B, CI, S, S)
        want[b0, :, y0:y0 + 3, x0:x0 + 3] = 2.0 * w[c0]
        assert torch.equal(gx, want), (b0, c0, y0, x0)
        assert int((gx != 0).any(1).sum()) == 9
        want_w = torch.zeros(CO, CI, 3, 3)
        want_w[c0] = 2.0 * x[b0, :, y0:y0 + 3, x0:x0 + 3]
        assert torch.equal(gw, want_w), (b0, c0, y0, x0)
    dy = torch.randint(1, 4, (B, CO, So, So), generator=g).float()
    for (b0, c0, y0, x0) in ((1, 37, 4, 4), (2, 5, 0, 0), (0, 63, 8, 3), (1, 9, 3, 8), (0, 1, 8, 8)):       # ... and one nonzero x pixel
        xz = torch.zeros(B, CI, S, S)
        xz[b0, c0, y0, x0] = 3.0
        _, gw = direct(dev, xz, w, dy, need=("gw", ))
        want_w = torch.zeros(CO, CI, 3, 3)
        for ky in range(3):
            for kx in range(3):
                if 0 <= y0 - ky < So and 0 <= x0 - kx < So:
                    want_w[:, c0, ky, kx] = 3.0 * dy[b0, :, y0 - ky, x0 - kx]
        assert torch.equal(gw.cpu(), want_w), (b0, c0, y0, x0)


# ------------------------------------------------------------------------------------------------------------------ 4. random data, every form
def test_cases_cover_every_form():
    from hdn_amd import _lib
    lib = _lib.load()
    for name, cases in TC.DGRAD_CASES.items():
        for c in cases:
            assert TC.dgrad_form_name(lib.hdn_conv3x3v_dgrad_form(*c)) == name, (c, name)
    for name, cases in TC.WGRAD_CASES.items():
        for c in cases:
            assert TC.wgrad_form_name(lib.hdn_conv3x3v_wgrad_form(*c)) == name, (c, name)
    assert set(TC.DGRAD_CASES) == {"A", "A split", "B", "B split", "C"}
    assert set(TC.WGRAD_CASES) == {"W1", "W2", "W4", "W1 split", "W2 split", "W4 split"}
    for c in ((2, 7, 256, 256), (2, 31, 256, 256), (2, 15, 256, 256)):
        assert c in TC.RANDOM_CASES


@pytest.mark.parametrize("case", TC.RANDOM_CASES)
def test_gradients_vs_float64(dev, case):
    from hdn_amd import _lib
    lib = _lib.load()
    x, w, dy, gx64, gw64, gx32, gw32 = reference(case)
    gx, gw = direct(dev, x, w, dy)
    gx2, gw2 = direct(dev, x, w, dy)
    assert torch.equal(gx, gx2) and torch.equal(gw, gw2), case
    fd, fw = TC.dgrad_form_name(lib.hdn_conv3x3v_dgrad_form(*case)), TC.wgrad_form_name(lib.hdn_conv3x3v_wgrad_form(*case))
    ok_x, rx = TC.bound_check(f"{case} gx [{fd}]", gx, gx64, gx32, (1, 2, 3))
    ok_w, rw = TC.bound_check(f"{case} gw [{fw}]", gw, gw64, gw32, (1, 2, 3))
    assert ok_x and ok_w, (case, rx, rw)


# ------------------------------------------------------------------------------------------------------------------------------------ 5. scale
def test_power_of_two_scalings_of_the_gradient(dev):
    case = (3, 9, 64, 64)
    x, w, dy = TC.random_problem(*case, dy_scale=1.0)
    gx, gw = direct(dev, x, w, dy)
    for k in (-60, -20, 30):
        sx, sw = direct(dev, x, w, dy * 2.0 ** k)
        assert torch.equal(sx, gx * 2.0 ** k) and torch.equal(sw, gw * 2.0 ** k), k
    zx, zw = direct(dev, x, w, torch.zeros_like(dy))
    assert not bool(zx.any()) and not bool(zw.any())
    bad = dy.clone()
    bad[1, 5, 2, 3] = float("nan")
    nx, nw = direct(dev, x, w, bad)
    assert not bool(torch.isfinite(nx[1, :, 2:5, 3:6]).any()) and not bool(torch.isfinite(nw[5]).any())
    bad[1, 5, 2, 3] = float("inf")
    nx, nw = direct(dev, x, w, bad)
    assert not bool(torch.isfinite(nx[1, :, 2:5, 3:6]).any()) and not bool(torch.isfinite(nw[5]).any())


# --------------------------------------------------------------------------------------------------------------------------------- 6. autograd
def test_autograd_function(dev):
    case = (3, 9, 64, 64)
    x, w, dy = TC.random_problem(*case)
    gx, gw = direct(dev, x, w, dy)
    want_y = CT.forward(_cl(x, dev), w.to(dev))
    for needs in ((True, True), (True, False), (False, True)):
        for layout in ("cl", "nchw"):
            xd = (_cl(x, dev) if layout == "cl" else x.to(dev).contiguous()).requires_grad_(needs[0])
            wd = w.to(dev).requires_grad_(needs[1])
            y = conv3x3_valid(xd, wd)
            assert y.is_contiguous(memory_format=CL) and torch.equal(y, want_y)
            before = dict(CT.launches)
            y.backward(_cl(dy, dev))
            made = {k: CT.launches[k] - before[k] for k in before}
            assert made["dgrad"] == int(needs[0]) and made["wgrad"] == int(needs[1]) and made["scale"] == 1 and made["pack"] == int(needs[0]), (needs, made)
            assert (xd.grad is None) == (not needs[0]) and (wd.grad is None) == (not needs[1])
            if needs[0]:
                assert torch.equal(xd.grad, gx), (needs, layout)
            if needs[1]:
                assert torch.equal(wd.grad, gw), (needs, layout)
    with pytest.raises(Exception):
        conv3x3_valid(x, w)                                   # host tensors: no CPU fallback


# ----------------------------------------------------------------------------------------------------------------------------------- 7. module
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


def _standin_modules():
    ban = types.SimpleNamespace(DepthwiseXCorr=DepthwiseXCorr, xcorr_depthwise=O.xcorr_depthwise)
    ban_lp = types.SimpleNamespace(DepthwiseXCorrCirc=DepthwiseXCorrCirc, xcorr_depthwise_circular=O.xcorr_depthwise_circular)
    return {"hdn.models.head.ban": ban, "hdn.models.head.ban_lp": ban_lp}


@pytest.fixture
def bound_heads(monkeypatch):
    import hdn_amd.install as hi
    monkeypatch.setattr(hi, "HEAD_CONV_TRAIN_BOUND", True)
    orig = {c: c.__dict__["forward"] for c in (DepthwiseXCorr, DepthwiseXCorrCirc)}
    done = hi.install(train=True, modules=_standin_modules())
    assert ("hdn.models.head.ban", "DepthwiseXCorr.forward") in done and ("hdn.models.head.ban_lp", "DepthwiseXCorrCirc.forward") in done
    yield orig
    hi.uninstall()
    assert all(c.__dict__["forward"] is f for c, f in orig.items())


@pytest.mark.parametrize("klass,C,sk,ss", [(DepthwiseXCorr, 32, 7, 15), (DepthwiseXCorrCirc, 64, 9, 9)])
def test_bound_head_branch_against_float64_twin(dev, bound_heads, klass, C, sk, ss):
    torch.manual_seed(C)
    B = 3
    m = klass(C, C, 4)
    twin64, twin32, stock = copy.deepcopy(m).double(), copy.deepcopy(m), copy.deepcopy(m).to(dev)
    m = m.to(dev)
    zf, xf = torch.randn(B, C, sk, sk).clamp_min(0), torch.randn(B, C, ss, ss).clamp_min(0)
    before = dict(CT.launches)

    def run(mod, z, x, fwd=None):
        mod.train()
        out = (fwd(mod, z, x) if fwd else mod(z, x))
        loss = (out * out).mean()
        loss.backward()
        return loss.detach(), {n: p.grad.detach() for n, p in mod.named_parameters()}

    loss, grads = run(m, _cl(zf, dev), _cl(xf, dev))
    made = {k: CT.launches[k] - before[k] for k in before}
    assert made["forward"] == 2 and made["wgrad"] == 2 and made["dgrad"] == 0, made            # the inputs need no gradient: no dgrad is launched
    orig = bound_heads
    l64, g64 = run(twin64, zf.double(), xf.double(), orig[klass])
    l32, g32 = run(twin32, zf, xf, orig[klass])
    e_ref, scale = abs(float(l32) - float(l64)), abs(float(l64))
    print(f"FORMS conv3x3 train module {klass.__name__} loss: err {abs(float(loss) - float(l64)):.3e}, bound {4 * e_ref + 1e-5 * scale:.3e}")
    assert abs(float(loss) - float(l64)) <= 4 * e_ref + 1e-5 * scale
    for n in g64:
        err = float((grads[n].cpu().double() - g64[n]).abs().max())
        e_ref, scale = float((g32[n].double() - g64[n]).abs().max()), float(g64[n].abs().max())
        print(f"FORMS conv3x3 train module {klass.__name__} {n}: err {err:.3e}, e_ref {e_ref:.3e}, scale {scale:.3e}, err/bound {err / (4 * e_ref + 1e-5 * scale):.3f}")
        assert err <= 4 * e_ref + 1e-5 * scale, n
    # running statistics: the BatchNorm modules ran as modules, as in the stock forward
    with torch.device(dev):              # (the oracle's circular pad builds its index vectors on the default device)
        run(stock, _cl(zf, dev), _cl(xf, dev), orig[klass])
    for (n, b), (_, bs) in zip(m.named_buffers(), stock.named_buffers()):
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(bs) == 1, n
        else:
            assert torch.allclose(b, bs, rtol=1e-5, atol=1e-6), n
    # .eval(): the class's own forward, no HIP convolution
    before = dict(CT.launches)
    m.eval()
    stock.eval()
    with torch.no_grad(), torch.device(dev):
        a, b = m(_cl(zf, dev), _cl(xf, dev)), orig[klass](m, _cl(zf, dev), _cl(xf, dev))
    assert torch.equal(a, b) and CT.launches == before


def test_uninstall_restores_the_forwards(dev, monkeypatch):
    import hdn_amd.install as hi
    orig = {c: c.__dict__["forward"] for c in (DepthwiseXCorr, DepthwiseXCorrCirc)}
    hi.install(train=True, modules=_standin_modules())                      # the flag as shipped or off: bound only while HEAD_CONV_TRAIN_BOUND
    bound = any(c.__dict__["forward"] is not f for c, f in orig.items())
    assert bound == hi.HEAD_CONV_TRAIN_BOUND
    hi.uninstall()
    assert all(c.__dict__["forward"] is f for c, f in orig.items())
    monkeypatch.setattr(hi, "HEAD_CONV_TRAIN_BOUND", True)
    hi.install(train=False, modules=_standin_modules())
    assert all(c.__dict__["forward"] is f for c, f in orig.items())         # train=False never binds it
    hi.uninstall()


# ------------------------------------------------------------------------------------------------------------------------------------ 8. graph
def test_forward_backward_replay_sees_an_in_place_weight_change(dev):
    case = (3, 9, 64, 64)
    x, w, dy = TC.random_problem(*case)
    xs, dys = _cl(x, dev).requires_grad_(True), _cl(dy, dev)
    ws = w.to(dev).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            xs.grad = ws.grad = None
            conv3x3_valid(xs, ws).backward(dys)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    xs.grad = ws.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="global"):
        y = conv3x3_valid(xs, ws)
        y.backward(dys)
    g = torch.Generator().manual_seed(11)
    for k in range(2):
        with torch.no_grad():
            ws.add_(torch.randn(ws.shape, generator=g).to(dev) * 0.05)        # in place: what a replayed optimizer step does
            dys.mul_(0.5 if k else 3.0)
        graph.replay()
        torch.cuda.synchronize()
        xe, we = xs.detach().clone().requires_grad_(True), ws.detach().clone().requires_grad_(True)
        ye = conv3x3_valid(xe, we)
        ye.backward(dys)
        assert torch.equal(y, ye) and torch.equal(xs.grad, xe.grad) and torch.equal(ws.grad, we.grad), k


class _Heads(nn.Module):
    def __init__(self):
        super().__init__()
        self.a, self.b = DepthwiseXCorr(32, 32, 2), DepthwiseXCorrCirc(32, 32, 4)

    def forward(self, z, x, zl, xl):
        return (self.a(z, x) ** 2).mean() + (self.b(zl, xl) ** 2).mean()


def test_a_whole_iteration_with_bound_heads_replays_as_one_graph(dev, bound_heads):
    from hdn_amd import GatedAMSGrad
    torch.manual_seed(4)
    proto = _Heads()
    models = {k: copy.deepcopy(proto).to(dev).train() for k in ("graph", "eager")}
    opts = {k: GatedAMSGrad(list(m.parameters()), lr=1e-3, max_norm=10.0) for k, m in models.items()}
    g = torch.Generator().manual_seed(9)
    batch = lambda: [_cl(torch.randn(2, 32, s, s, generator=g).clamp_min(0), dev) for s in (7, 15, 9, 9)]
    static = batch()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = copy.deepcopy(models["graph"])
        for _ in range(2):
            warm.zero_grad(set_to_none=True)
            warm(*static).backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    models["graph"].zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="global"):
        loss = models["graph"](*static)
        loss.backward()
        opts["graph"].step(loss)
    for k in range(3):
        for s, n in zip(static, batch()):
            s.copy_(n)
        graph.replay()
        torch.cuda.synchronize()
        models["eager"].zero_grad(set_to_none=True)
        le = models["eager"](*static)
        le.backward()
        opts["eager"].step(le)
        torch.cuda.synchronize()
        assert int(opts["graph"].report.status) == int(opts["eager"].report.status) == 0
        for (n, p), (_, q) in zip(models["graph"].named_parameters(), models["eager"].named_parameters()):
            assert torch.equal(p, q), (k, n)
        for (n, p), (_, q) in zip(models["graph"].named_buffers(), models["eager"].named_buffers()):
            assert torch.equal(p, q), (k, n)
