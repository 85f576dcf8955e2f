"""GPU tests of the ResNet-50 (Bottleneck) homography trunk: hdn_conv1x1_f32 against float64 at every shape of the trunk, its argument
errors, the folded HIP trunk against the reference's output (tests/golden/trunk_resnet50.npz) and a float64 forward, the regressor head
through HomoModelBuilder(backbone="resnet50"), and a captured replay."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

pytestmark = pytest.mark.gpu

# CI -> CO @ input side, stride: every 1x1 convolution of the ResNet-50 trunk at 127-px crops
SHAPES = [(64, 64, 32, 1), (64, 256, 32, 1), (256, 64, 32, 1),
          (256, 128, 32, 1), (128, 512, 16, 1), (512, 128, 16, 1), (256, 512, 32, 2),
          (512, 256, 16, 1), (256, 1024, 8, 1), (1024, 256, 8, 1), (512, 1024, 16, 2),
          (1024, 512, 8, 1), (512, 2048, 4, 1), (2048, 512, 4, 1), (1024, 2048, 8, 2)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def seeded_resnet50():
    import make_golden as mg
    from hdn_amd.trunk import resnet50_homo
    return mg.seeded_trunk_state_(resnet50_homo().eval())


@pytest.mark.parametrize("CI,CO,S,stride", SHAPES)
@pytest.mark.parametrize("B", [1, 2, 64])
def test_conv1x1_vs_float64(dev, CI, CO, S, stride, B):
    """hdn_conv1x1_f32 (split-fp16 implicit GEMM, bias / residual / ReLU fused) against a float64 convolution, within 4x the error of PyTorch's
    own fp32 convolution + 1e-5 of the output scale (the bound of test_conv3x3_matrix_core_vs_float64); with and without residual and ReLU,
    act_domain 0 and 1; deterministic."""
    from hdn_amd.trunk import ACT_SCALE_LOG2, conv1x1, pack_conv1x1
    g = torch.Generator().manual_seed(CI + 3 * CO + S + B)
    So = (S - 1) // stride + 1
    w = torch.randn(CO, CI, 1, 1, generator=g) * (2.0 / CI) ** 0.5
    b = torch.randn(CO, generator=g) * 0.1
    x = torch.randn(B, CI, S, S, generator=g).clamp_min_(0)
    r = torch.randn(B, CO, So, So, generator=g)
    cl = torch.channels_last
    wp, bd = pack_conv1x1(w).to(dev), b.to(dev)
    xd, rd = x.to(dev).contiguous(memory_format=cl), r.to(dev).contiguous(memory_format=cl)
    y = conv1x1(xd, wp, bd, rd, stride=stride, relu=True)
    y0 = conv1x1(xd, wp, bd, stride=stride, relu=False)
    assert torch.equal(y, conv1x1(xd, wp, bd, rd, stride=stride, relu=True))          # deterministic
    assert y.is_contiguous(memory_format=cl) and tuple(y.shape) == (B, CO, So, So)
    sc = 2.0 ** -ACT_SCALE_LOG2
    yd = conv1x1((xd * sc).contiguous(memory_format=cl), wp, bd * sc, (rd * sc).contiguous(memory_format=cl), stride=stride, relu=True,
                 act_domain=1) * 2.0 ** ACT_SCALE_LOG2
    nb = min(B, 3)                                      # the float64 truth on the first and last images only
    for sl in (slice(0, nb), slice(B - nb, B)):
        conv = F.conv2d(x[sl].double(), w.double(), b.double(), stride=stride)
        t, t0 = torch.relu(conv + r[sl].double()), conv
        e_ref = float((torch.relu(F.conv2d(x[sl], w, b, stride=stride) + r[sl]).double() - t).abs().max())
        e_ref0 = float((F.conv2d(x[sl], w, b, stride=stride).double() - t0).abs().max())
        for got, truth, er in ((y, t, e_ref), (yd, t, e_ref), (y0, t0, e_ref0)):
            scale = float(truth.abs().max())
            e = float((got[sl].cpu().double() - truth).abs().max())
            assert e <= 4 * er + 1e-5 * scale, (e, er, scale)


def test_conv1x1_argument_errors(dev):
    """NULL, aliasing and shapes are refused before any launch; with the range guard on, |x| >= 1.67e7 gives HDN_E_LIMIT."""
    from hdn_amd import _lib
    from hdn_amd.trunk import conv1x1, pack_conv1x1
    lib = _lib.load()
    cl = torch.channels_last
    x = torch.rand(2, 64, 32, 32, device=dev).contiguous(memory_format=cl)
    wp = pack_conv1x1(torch.randn(256, 64, 1, 1) * 0.1).to(dev)
    b = torch.zeros(256, device=dev)
    out = torch.empty(2, 256, 32, 32, device=dev).contiguous(memory_format=cl)
    p = _lib.ptr
    s = _lib.stream_ptr(dev)
    f = lib.hdn_conv1x1_f32
    assert f(None, p(wp), p(b), None, p(out), 2, 32, 64, 256, 1, 1, 0, s) == -1
    assert f(p(x), p(wp), p(b), None, p(x), 2, 32, 64, 256, 1, 1, 0, s) == -4
    assert f(p(x), p(wp), p(b), p(out), p(out), 2, 32, 64, 256, 1, 1, 0, s) == -4
    assert f(p(x), p(wp), p(b), None, p(out), 2, 32, 48, 256, 1, 1, 0, s) == -2
    assert f(p(x), p(wp), p(b), None, p(out), 2, 32, 64, 256, 3, 1, 0, s) == -2
    with pytest.raises(ValueError):
        conv1x1(x.contiguous(), wp, b)                                  # NCHW input
    with pytest.raises(ValueError):
        conv1x1(x, wp[:-8], b)
    prev = lib.hdn_set_check_range(1)
    try:
        big = x.clone()
        big[1, 3, 4, 5] = 2e7
        assert f(p(big), p(wp), p(b), None, p(out), 2, 32, 64, 256, 1, 1, 0, s) == -3
        with pytest.raises(ValueError):
            conv1x1(big, wp, b)
        assert f(p(x), p(wp), p(b), None, p(out), 2, 32, 64, 256, 1, 1, 0, s) == 0
    finally:
        lib.hdn_set_check_range(prev)
    torch.cuda.synchronize()


def _fold_hip(m, dev):
    from hdn_amd.trunk import fold_for_inference
    return fold_for_inference(m.to(dev), channels_last=True, fused_stem=True, fused_epilogue=True)


def test_folded_resnet50_trunk_vs_reference_output(dev, monkeypatch):
    """The folded HIP trunk (fused stem, fused Bottlenecks, channels-last) on the fixture's input against the reference's output; at B = 64 against
    a float64 forward.  No 1x1 nn.Conv2d is left and hdn_conv1x1_f32 runs every 1x1 convolution; the ResNet-34 fold has no Bottleneck pieces."""
    from hdn_amd import trunk as T
    gold = load_golden("trunk_resnet50")
    m = seeded_resnet50()
    fast = _fold_hip(m, dev)
    assert not any(isinstance(mod, nn.Conv2d) and mod.kernel_size == (1, 1) for mod in fast.modules())
    assert sum(isinstance(mod, T.FusedBottleneck) for mod in fast.modules()) == 16 and fast.act_domain == 1
    calls = []
    real = T.conv1x1
    monkeypatch.setattr(T, "conv1x1", lambda *a, **k: calls.append(tuple(a[0].shape)) or real(*a, **k))
    with torch.no_grad():
        got = fast(torch.from_numpy(gold["x"]).to(dev))
    monkeypatch.setattr(T, "conv1x1", real)
    assert len(calls) == 2 * 16 + 4, len(calls)
    ref = torch.from_numpy(gold["out"])
    assert got.shape == ref.shape == (2, 2048, 4, 4)
    err = float((got.cpu() - ref).abs().max())
    assert err <= 1e-4 * float(ref.abs().max()), err
    # B = 64, seeded inputs, against float64 on the first and last images
    g = np.random.default_rng(64)
    x = torch.from_numpy(g.standard_normal((64, 2, 127, 127)).astype(np.float32))
    with torch.no_grad():
        y = fast(x.to(dev)).cpu()
        m64 = seeded_resnet50().double()
        for sl in (slice(0, 2), slice(62, 64)):
            t = m64(x[sl].double())
            e = float((y[sl].double() - t).abs().max())
            assert e <= 1e-4 * float(t.abs().max()), e
    # the ResNet-34 fold beside it: BasicBlocks only
    f34 = _fold_hip(T.resnet34_homo().eval(), dev)
    assert not any(isinstance(mod, T.FusedBottleneck) for mod in f34.modules())
    assert sum(isinstance(mod, T.FusedBasicBlock) for mod in f34.modules()) == 16


@pytest.mark.parametrize("B", [1, 2, 64])
def test_homo_model_builder_resnet50_head(dev, B):
    """HomoModelBuilder(backbone="resnet50").optimize_for_inference() on the GPU: the corner offsets of track_proj's regressor against the same
    model's unoptimised trunk + avgpool + fc on the CPU (1e-4 abs, the north-star bound)."""
    import make_golden as mg
    import hdn_amd
    from hdn_amd.homo_model import homo_stages
    torch.manual_seed(0)
    net = hdn_amd.HomoModelBuilder(backbone="resnet50").eval()
    mg.seeded_trunk_state_(net.backbone, 640)
    net.fc.weight.data.mul_(0.01)
    cpu_backbone = seeded_resnet50()
    cpu_backbone.load_state_dict(net.backbone.state_dict())
    fc = nn.Linear(2048, 8)
    fc.load_state_dict(net.fc.state_dict())
    net = net.to(dev).optimize_for_inference(channels_last=True)
    g = np.random.default_rng(100 + B)
    imgs = torch.from_numpy(g.standard_normal((B, 2, 127, 127)).astype(np.float32)).to(dev)
    h4p = torch.tensor([[0, 0, 0, 127, 127, 127, 127, 0]], dtype=torch.float32).repeat(B, 1).to(dev)
    pidx = torch.arange(127 * 127, dtype=torch.float32).repeat(B, 1).to(dev)
    data = {"org_imgs": imgs, "input_tensors": imgs.clone(), "h4p": h4p, "patch_indices": pidx}
    st = homo_stages(net, data)
    H, _, _ = net.track_proj(data)
    assert torch.isfinite(H).all()
    feats = torch.cat((st["patch_1"], st["patch_2"]), dim=1).cpu()
    with torch.no_grad():
        ref = fc(cpu_backbone(feats).mean((2, 3)))
    err = float((st["x"].cpu() - ref).abs().max())
    assert err <= 1e-4, err


def test_resnet50_trunk_capture_replay(dev):
    """The folded ResNet-50 trunk at B = 1 captured with torch.cuda.graph and replayed: bit for bit the eager result.  MIOpen, which runs the three
    stride-2 3x3 convolutions, is asked for its deterministic solvers (its default ones at B = 1 differ between two eager calls by ~1 ulp);
    every HIP kernel of the trunk is deterministic as it stands."""
    fast = _fold_hip(seeded_resnet50(), dev)
    x = torch.randn(1, 2, 127, 127, device=dev)
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        _capture_and_compare(fast, x)
    finally:
        torch.backends.cudnn.deterministic = prev


def _capture_and_compare(fast, x):
    with torch.no_grad():
        side = torch.cuda.Stream()          # warm-up off the capture stream (MIOpen settles its choice for the three stride-2 3x3 convolutions)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fast(x)
            fast(x)
        torch.cuda.current_stream().wait_stream(side)
        y = fast(x)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            yg = fast(x)
        gr.replay()
        torch.cuda.synchronize()
    assert torch.equal(yg, y), float((yg - y).abs().max())
