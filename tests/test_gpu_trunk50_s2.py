"""GPU tests of hdn_conv3x3s2_f32 (the stride-2 3x3 convolution of a Bottleneck) and of the ResNet-50 trunk that no longer calls MIOpen: the kernel
against float64 at its three shapes, a border pattern, its argument errors, the folded trunk with torch's conv2d disabled, and a capture without
preparation."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

pytestmark = pytest.mark.gpu

SHAPES = [(16, 128), (8, 256), (4, 512)]          # (output side S, channels C): conv2 of the first block of layer2 / 3 / 4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def seeded_resnet50():
    import make_golden as mg
    from hdn_amd.trunk import resnet50_homo
    return mg.seeded_trunk_state_(resnet50_homo().eval())


@pytest.mark.parametrize("S,C", SHAPES)
@pytest.mark.parametrize("B", [1, 2, 64])
def test_conv3x3s2_vs_float64(dev, S, C, B):
    """hdn_conv3x3s2_f32 against a float64 convolution within 4x the error of PyTorch's own CPU fp32 convolution + 1e-5 of the output scale (the bound
    of test_conv1x1_vs_float64 / test_conv3x3_matrix_core_vs_float64), act_domain 0 and 1; deterministic; channels-last [B, C, S, S]."""
    from hdn_amd.trunk import ACT_SCALE_LOG2, conv3x3s2, pack_conv3x3s2
    g = torch.Generator().manual_seed(S + 3 * C + B)
    w = torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(C, generator=g) * 0.1
    x = torch.randn(B, C, 2 * S, 2 * S, generator=g).clamp_min_(0)
    cl = torch.channels_last
    wp, bd = pack_conv3x3s2(w).to(dev), b.to(dev)
    xd = x.to(dev).contiguous(memory_format=cl)
    y = conv3x3s2(xd, wp, bd)
    assert torch.equal(y, conv3x3s2(xd, wp, bd))                                 # deterministic
    assert y.is_contiguous(memory_format=cl) and tuple(y.shape) == (B, C, S, S)
    sc = 2.0 ** -ACT_SCALE_LOG2
    yd = conv3x3s2((xd * sc).contiguous(memory_format=cl), wp, bd * sc, act_domain=1) * 2.0 ** ACT_SCALE_LOG2
    nb = min(B, 3)                                      # the float64 truth on the first and last images only
    for sl in (slice(0, nb), slice(B - nb, B)):
        t = torch.relu(F.conv2d(x[sl].double(), w.double(), b.double(), stride=2, padding=1))
        e_ref = float((torch.relu(F.conv2d(x[sl], w, b, stride=2, padding=1)).double() - t).abs().max())
        scale = float(t.abs().max())
        for name, got in (("domain 0", y), ("domain 1", yd)):
            e = float((got[sl].cpu().double() - t).abs().max())
            print(f"conv3x3s2 S={S} C={C} B={B} {name} images {sl.start}:{sl.stop}: err {e:.3e}, fp32 reference err {e_ref:.3e}, scale {scale:.3f}")
            assert e <= 4 * e_ref + 1e-5 * scale, (name, e, e_ref, scale)


@pytest.mark.parametrize("S,C", SHAPES)
@pytest.mark.parametrize("B", [1, 5])
def test_conv3x3s2_border_pattern(dev, S, C, B):
    """x = 1, w = 1 / (9 C), bias 0: interior outputs 1, the top row and the left column 6/9, the corner 4/9 (stride 2 on an even side with padding 1
    touches padding at the top and the left only) - an off-by-one in the padding or the stride phase shows here at 1e-6."""
    from hdn_amd.trunk import conv3x3s2, pack_conv3x3s2
    w = torch.full((C, C, 3, 3), 1.0 / (9 * C))
    x = torch.ones(B, C, 2 * S, 2 * S)
    expect = torch.ones(S, S, dtype=torch.float64)
    expect[0, :] = expect[:, 0] = 6.0 / 9.0
    expect[0, 0] = 4.0 / 9.0
    ref = F.conv2d(x[:1].double(), w.double(), None, stride=2, padding=1)          # the pattern itself, checked on the CPU
    assert float((ref - expect).abs().max()) <= 1e-7                               # (1 / (9 C) is rounded to fp32 once: 6e-8 relative)
    y = conv3x3s2(x.to(dev).contiguous(memory_format=torch.channels_last), pack_conv3x3s2(w).to(dev), torch.zeros(C, device=dev)).cpu().double()
    assert float((y - expect).abs().max()) <= 1e-6, float((y - expect).abs().max())


def test_conv3x3s2_argument_errors(dev):
    """NULL, aliasing, shapes, limits and the workspace are refused before any launch; with the range guard on, |x| >= 1.67e7 gives HDN_E_LIMIT."""
    import ctypes
    from hdn_amd import _lib
    from hdn_amd.trunk import conv3x3s2, pack_conv3x3s2
    lib = _lib.load()
    cl = torch.channels_last
    B, S, C = 2, 16, 128
    # x and out are cut from ONE allocation, 256 bytes apart: wherever the caching allocator puts things after the tests that ran before this one,
    # `x + 1 float` below overlaps nothing (with two allocations `out` can lie right behind `x`, and the entry point then rightly answers HDN_E_ALIAS
    # before it looks at the alignment)
    n_x, n_out, gap = B * C * 4 * S * S, B * C * S * S, 64
    arena = torch.empty(n_x + gap + n_out, device=dev)
    x = arena[:n_x].view(B, 2 * S, 2 * S, C).permute(0, 3, 1, 2).copy_(torch.rand(B, C, 2 * S, 2 * S, device=dev))
    out = arena[n_x + gap:].view(B, S, S, C).permute(0, 3, 1, 2)
    assert x.is_contiguous(memory_format=cl) and out.is_contiguous(memory_format=cl) and out.data_ptr() - x.data_ptr() == (n_x + gap) * 4
    wp = pack_conv3x3s2(torch.randn(C, C, 3, 3) * 0.03).to(dev)
    b = torch.zeros(C, device=dev)
    nws = lib.hdn_conv3x3s2_workspace_bytes(B, S, C)
    assert nws > 0
    ws = torch.empty(nws // 4, device=dev)
    p, s, f = _lib.ptr, _lib.stream_ptr(dev), lib.hdn_conv3x3s2_f32
    assert f(None, p(wp), p(b), p(out), p(ws), nws, B, S, C, 0, s) == -1
    assert f(p(x), p(wp), p(b), p(out), None, 0, B, S, C, 0, s) == -1
    assert f(p(x), p(wp), p(b), p(x), p(ws), nws, B, S, C, 0, s) == -4
    assert f(p(x), p(wp), p(b), p(out), p(ws), nws, 0, S, C, 0, s) == -2
    assert f(p(x), p(wp), p(b), p(out), p(ws), nws, B, S, C, 2, s) == -2
    assert f(p(x), p(wp), p(b), p(out), p(ws), nws, B, 16, 256, 0, s) == -3
    assert f(ctypes.c_void_p(x.data_ptr() + 4), p(wp), p(b), p(out), p(ws), nws, B, S, C, 0, s) == -3      # x + 1 float: misaligned
    assert f(p(x), p(wp), p(b), p(out), p(ws), nws - 4, B, S, C, 0, s) == -3
    with pytest.raises(ValueError):
        conv3x3s2(x.contiguous(), wp, b)                                  # NCHW input
    with pytest.raises(ValueError):
        conv3x3s2(x, wp[:-8], b)
    prev = lib.hdn_set_check_range(1)
    try:
        big = x.clone()
        big[1, 3, 4, 5] = 2e7
        assert f(p(big), p(wp), p(b), p(out), p(ws), nws, B, S, C, 0, s) == -3
        with pytest.raises(ValueError):
            conv3x3s2(big, wp, b)
        assert f(p(x), p(wp), p(b), p(out), p(ws), nws, B, S, C, 0, s) == 0
    finally:
        lib.hdn_set_check_range(prev)
    torch.cuda.synchronize()


def _fold_hip(m, dev):
    from hdn_amd.trunk import fold_for_inference
    return fold_for_inference(m.to(dev), channels_last=True, fused_stem=True, fused_epilogue=True)


def test_folded_resnet50_trunk_makes_no_conv2d_call(dev, monkeypatch):
    """The folded HIP ResNet-50 trunk with torch.nn.functional.conv2d raising: B = 1, 2 and 64 still run; the output against the reference's
    (tests/golden/trunk_resnet50.npz) and, at B = 64, against a float64 forward, both within 1e-4 of max|ref|."""
    from hdn_amd import trunk as T
    gold = load_golden("trunk_resnet50")
    fast = _fold_hip(seeded_resnet50(), dev)
    assert sum(m.p2s2 is not None for m in fast.modules() if isinstance(m, T.FusedBottleneck)) == 3

    def no_conv2d(*a, **k):
        raise AssertionError("F.conv2d called by the folded ResNet-50 trunk")

    monkeypatch.setattr(torch.nn.functional, "conv2d", no_conv2d)
    g = np.random.default_rng(64)
    x64 = torch.from_numpy(g.standard_normal((64, 2, 127, 127)).astype(np.float32))
    with torch.no_grad():
        y1 = fast(x64[:1].to(dev)).cpu()
        got = fast(torch.from_numpy(gold["x"]).to(dev)).cpu()                  # B = 2
        y64 = fast(x64.to(dev)).cpu()
    monkeypatch.undo()
    ref = torch.from_numpy(gold["out"])
    err = float((got - ref).abs().max())
    print(f"folded ResNet-50 trunk vs golden: {err:.3e} (bound {1e-4 * float(ref.abs().max()):.3e})")
    assert got.shape == ref.shape and err <= 1e-4 * float(ref.abs().max()), err
    with torch.no_grad():
        m64 = seeded_resnet50().double()
        for sl in (slice(0, 2), slice(62, 64)):
            t = m64(x64[sl].double())
            e = float((y64[sl].double() - t).abs().max())
            print(f"folded ResNet-50 trunk B=64 images {sl.start}:{sl.stop} vs float64: {e:.3e} (bound {1e-4 * float(t.abs().max()):.3e})")
            assert e <= 1e-4 * float(t.abs().max()), e
        t1 = m64(x64[:1].double())
        assert float((y1.double() - t1).abs().max()) <= 1e-4 * float(t1.abs().max())


def test_resnet50_trunk_captures_without_preparation(dev):
    """cudnn.deterministic / benchmark left off, one eager call, then a torch.cuda.graph capture on the current stream with no side-stream warm-up:
    the replay is bit for bit the eager result, and so are two further eager calls."""
    assert torch.backends.cudnn.deterministic is False and torch.backends.cudnn.benchmark is False
    fast = _fold_hip(seeded_resnet50(), dev)
    x = torch.randn(1, 2, 127, 127, device=dev)
    st = torch.cuda.Stream()                      # (a capture cannot run on the legacy default stream: eager call and capture share this one)
    st.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(st):
        y = fast(x)                               # loads the code objects
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            yg = fast(x)
        gr.replay()
        st.synchronize()
        assert torch.equal(yg, y), float((yg - y).abs().max())
        a, b = fast(x), fast(x)
        assert torch.equal(a, b) and torch.equal(a, y)
    torch.cuda.synchronize()
