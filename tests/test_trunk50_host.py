"""CPU tests of the ResNet-50 (Bottleneck) homography trunk: the architecture against the reference's (tests/golden/trunk_resnet50.npz,
tests/golden/make_golden_trunk50.py), HomoModelBuilder(backbone="resnet50"), the CPU fold, the refusal of unknown block layouts and
hdn_pack_conv1x1_f32 (host code).  No kernel is launched here."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def seeded_resnet50():
    import make_golden as mg
    from hdn_amd.trunk import resnet50_homo
    return mg.seeded_trunk_state_(resnet50_homo().eval())


def test_resnet50_state_dict_is_the_references():
    from hdn_amd.trunk import resnet50_homo
    gold = load_golden("trunk_resnet50")
    sd = resnet50_homo().state_dict()
    assert list(sd.keys()) == gold["keys"].tolist()
    assert [str(tuple(v.shape)) for v in sd.values()] == gold["shapes"].tolist()
    assert len(sd) == 318


def test_resnet50_matches_reference_output_on_cpu():
    gold = load_golden("trunk_resnet50")
    m = seeded_resnet50()
    psum = sum(float(v.double().sum()) for v in m.state_dict().values() if v.dtype == torch.float32)
    assert abs(psum - float(gold["param_sum"])) <= 1e-12 * abs(float(gold["param_sum"])), psum
    with torch.no_grad():
        got = m(torch.from_numpy(gold["x"]))
    ref = torch.from_numpy(gold["out"])
    assert got.shape == ref.shape == (2, 2048, 4, 4)
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max()), float((got - ref).abs().max())


def test_homo_model_builder_resnet50_has_the_reference_layout():
    import hdn_amd
    gold = load_golden("trunk_resnet50")
    m = hdn_amd.HomoModelBuilder(backbone="resnet50")
    keys = [k[len("backbone."):] for k in m.state_dict() if k.startswith("backbone.")]
    assert keys == gold["keys"].tolist()
    assert isinstance(m.fc, nn.Linear) and (m.fc.in_features, m.fc.out_features) == (2048, 8)
    m34 = hdn_amd.HomoModelBuilder()
    assert (m34.fc.in_features, m34.fc.out_features) == (512, 8)
    with pytest.raises(ValueError):
        hdn_amd.HomoModelBuilder(backbone="resnet18")


def test_fold_of_the_bottleneck_trunk_on_cpu_equals_the_unfolded_net():
    from hdn_amd.trunk import fold_for_inference
    m = seeded_resnet50()
    g = np.random.default_rng(5)
    x = torch.from_numpy(g.standard_normal((2, 2, 127, 127)).astype(np.float32))
    folded = fold_for_inference(m, channels_last=False, fused_stem=False, fused_epilogue=False)
    assert not any(isinstance(mod, nn.BatchNorm2d) for mod in folded.modules())
    with torch.no_grad():
        ref, got = m(x), folded(x)
        t = m.double()(x.double())
    assert got.shape == (2, 2048, 4, 4)
    # both are fp32 evaluations of the same real-number function: each within a few ulps of the float64 forward, hence of each other
    scale = float(t.abs().max())
    assert float((got.double() - t).abs().max()) <= 1e-5 * scale
    assert float((got - ref).abs().max()) <= 1e-5 * scale


class _OddBlock(nn.Module):
    """A block with a layout the fold does not know (a 5x5 convolution)."""

    def __init__(self, c):
        super().__init__()
        self.conv1 = nn.Conv2d(c, c, 5, 1, 2, bias=False)
        self.bn1 = nn.BatchNorm2d(c)

    def forward(self, x):
        return torch.relu(self.bn1(self.conv1(x)))


def test_fold_and_optimize_trunk_refuse_an_unknown_block_layout():
    from hdn_amd.homo_model import optimize_trunk
    from hdn_amd.trunk import block_kind, fold_for_inference, resnet34_homo, resnet50_homo
    net = resnet50_homo().eval()
    net.layer3[2] = _OddBlock(1024)
    with pytest.raises(ValueError):
        fold_for_inference(net, channels_last=False)
    holder = nn.Module()
    holder.backbone = net
    with pytest.raises(ValueError):
        optimize_trunk(holder, channels_last=False, fused_stem=False, fused_epilogue=False)
    # a Bottleneck whose conv3 went missing is no BasicBlock either
    b = resnet50_homo().layer1[1]
    del b.conv3
    with pytest.raises(ValueError):
        block_kind(b)
    assert block_kind(resnet34_homo().layer2[0]) == "basic" and block_kind(resnet50_homo().layer2[0]) == "bottleneck"


def _split_pack_conv1x1(w):
    """An independent statement of hdn_pack_conv1x1_f32's layout: [CO/32][CI/32][k step t][piece][k half g][32 n][8 e] with
    ci = 32 chunk + 16 g + 8 t + e, pieces p0 = fp16(w), p1 = fp16((w - p0) 2^11)."""
    CO, CI = w.shape[0], w.shape[1]
    w = w.reshape(CO, CI).float()
    p0 = w.half()
    p1 = ((w - p0.float()) * 2048.0).half()
    pieces = torch.stack((p0, p1))                                         # [piece][CO][CI]
    v = pieces.reshape(2, CO // 32, 32, CI // 32, 2, 2, 8)                 # [piece][nt][n][chunk][g][t][e]
    return v.permute(1, 3, 5, 0, 4, 2, 6).contiguous().view(torch.int16).reshape(-1)


def test_pack_conv1x1_matches_an_independent_layout_bit_for_bit():
    from hdn_amd import _lib, trunk as T
    g = torch.Generator().manual_seed(11)
    for CO, CI in ((64, 64), (256, 64), (64, 256), (128, 256), (512, 128), (2048, 512), (512, 2048), (32, 96)):
        w = torch.randn(CO, CI, 1, 1, generator=g) * 0.1
        assert torch.equal(T.pack_conv1x1(w), _split_pack_conv1x1(w)), (CO, CI)
    w = torch.zeros(64, 64, 1, 1)
    w.view(-1)[:6] = torch.tensor([65503.9, -65000.0, 1.0009765625, 6.1e-5, 5.9e-8, -0.0])
    assert torch.equal(T.pack_conv1x1(w), _split_pack_conv1x1(w))
    lib = _lib.load()
    assert lib.hdn_pack_conv1x1_bytes(256, 64) == 2 * 2 * 256 * 64
    for CO, CI in ((100, 64), (64, 48), (0, 64), (64, -32)):
        assert lib.hdn_pack_conv1x1_bytes(CO, CI) < 0
    with pytest.raises(ValueError):
        T.pack_conv1x1(torch.randn(96, 48, 1, 1))
    with pytest.raises(ValueError):
        T.pack_conv1x1(torch.randn(64, 64, 3, 3))
    # the range check of the weights
    for bad in (65504.0, float("nan"), -float("inf")):
        w = torch.randn(64, 64, 1, 1, generator=g) * 0.1
        w[5, 6] = bad
        with pytest.raises(ValueError, match="fp16 range"):
            T.pack_conv1x1(w)
    # the C entry point itself: NULL, a wrong byte count, HDN_E_LIMIT
    w = torch.randn(64, 64, generator=g)
    buf = torch.empty(64 * 64 * 2, dtype=torch.int16)
    assert lib.hdn_pack_conv1x1_f32(None, 64, 64, buf.data_ptr(), 64 * 64 * 4) == -1
    assert lib.hdn_pack_conv1x1_f32(w.data_ptr(), 64, 64, buf.data_ptr(), 64 * 64 * 4 - 2) == -2
    w[0, 0] = 1e6
    assert lib.hdn_pack_conv1x1_f32(w.data_ptr(), 64, 64, buf.data_ptr(), 64 * 64 * 4) == -3


def test_conv1x1_argument_errors_need_no_gpu():
    """hdn_conv1x1_f32 validates before any launch: NULL, shape, alias, alignment."""
    import ctypes
    from hdn_amd import _lib
    lib = _lib.load()
    a, w, b, o = (ctypes.c_void_p(v) for v in (1 << 20, 2 << 20, 3 << 20, 4 << 20))
    f = lib.hdn_conv1x1_f32
    assert f(None, w, b, None, o, 2, 32, 64, 256, 1, 1, 0, None) == -1
    assert f(a, None, b, None, o, 2, 32, 64, 256, 1, 1, 0, None) == -1
    assert f(a, w, None, None, o, 2, 32, 64, 256, 1, 1, 0, None) == -1
    assert f(a, w, b, None, None, 2, 32, 64, 256, 1, 1, 0, None) == -1
    for args in ((0, 32, 64, 256, 1, 1, 0), (2, 32, 48, 256, 1, 1, 0), (2, 32, 64, 100, 1, 1, 0), (2, 32, 64, 256, 3, 1, 0),
                 (2, 32, 64, 256, 1, 2, 0), (2, 32, 64, 256, 1, 1, 2), (2, 0, 64, 256, 1, 1, 0)):
        assert f(a, w, b, None, o, *args, None) == -2, args
    assert f(a, w, b, None, a, 2, 32, 64, 256, 1, 1, 0, None) == -4                                  # out == x
    assert f(a, w, b, None, ctypes.c_void_p((1 << 20) + 4096), 2, 32, 64, 256, 1, 1, 0, None) == -4  # out overlaps x
    assert f(a, w, b, o, o, 2, 32, 64, 256, 1, 1, 0, None) == -4                                     # out == residual
    assert f(ctypes.c_void_p((1 << 20) + 4), w, b, None, o, 1, 4, 64, 64, 1, 1, 0, None) == -3       # misaligned x
    assert f(a, w, b, None, o, 1 << 14, 128, 64, 64, 1, 1, 0, None) == -3                            # > 2^31 - 1 elements
