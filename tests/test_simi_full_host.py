"""CPU tests of level 2 of the HIP similarity backbone (tests/test_gpu_conv3x3v.py, tests/test_gpu_simi_stem.py and tests/test_gpu_backbone_hip_full.py
run it on the device): the new exports, the error codes that return before any launch, hdn_pack_simi_stem_f32 decoded from its documented layout,
hdn_conv3x3v_form / _workspace_bytes over the GPU case list, hip_plan / the level switch of hdn_amd.backbone, and the integer expectations of the GPU
exact tests against float64 F.conv2d / F.max_pool2d.  No kernel is launched here."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import simi_full_cases as SC  # noqa: E402

E_NULL, E_SHAPE, E_LIMIT = -1, -2, -3


def _lib():
    from hdn_amd import _lib as L
    return L.load()


def test_new_symbols_are_exported_and_the_abi_is_still_10():
    lib = _lib()
    for name in ("hdn_conv3x3v_f32", "hdn_conv3x3v_form", "hdn_conv3x3v_workspace_bytes", "hdn_simi_stem_f32", "hdn_pack_simi_stem_f32",
                 "hdn_pack_simi_stem_bytes"):
        assert getattr(lib, name) is not None, name
    assert lib.hdn_abi_version() == 10
    assert lib.hdn_pack_simi_stem_bytes() == 11 * 2 * 2 * 64 * 8 * 2


def test_conv3x3v_refuses_bad_arguments_before_any_launch():
    """NULL pointers, S = 2, stride 3 / 0, CI = 48, CO = 80, B = 0, relu / act_domain outside {0, 1}: HDN_E_NULL / HDN_E_SHAPE; 2^31 elements, a misaligned
    pointer: HDN_E_LIMIT; a K-split form without its workspace: HDN_E_NULL.  The two queries answer like the entry point.  (The pointers are made-up
    addresses: every case returns before anything is launched or read.)"""
    lib = _lib()
    f, wsb, run = lib.hdn_conv3x3v_form, lib.hdn_conv3x3v_workspace_bytes, lib.hdn_conv3x3v_f32
    x, w, o = (ctypes.c_void_p(v << 34) for v in (1, 2, 4))
    good = (2, 5, 32, 96, 2)
    assert run(None, w, None, o, None, 0, *good, 1, 0, None) == E_NULL
    assert run(x, None, None, o, None, 0, *good, 1, 0, None) == E_NULL
    assert run(x, w, None, None, None, 0, *good, 1, 0, None) == E_NULL
    assert wsb(*good) > 0 and run(x, w, None, o, None, 0, *good, 1, 0, None) == E_NULL               # split form, no workspace
    bad = [((1, 2, 64, 64, 1), E_SHAPE), ((1, 7, 64, 64, 3), E_SHAPE), ((1, 7, 64, 64, 0), E_SHAPE), ((1, 7, 48, 64, 2), E_SHAPE),
           ((1, 7, 64, 80, 2), E_SHAPE), ((0, 7, 64, 64, 2), E_SHAPE), ((1, 7, 0, 64, 1), E_SHAPE),
           ((1 << 14, 32, 256, 64, 1), E_LIMIT), ((1 << 12, 34, 32, 1024, 1), E_LIMIT)]
    for args, want in bad:
        assert f(*args) == want and wsb(*args) == want, args
        assert run(x, w, None, o, None, 0, *args, 1, 0, None) == want, args
    assert run(x, w, None, o, None, 0, *good, 2, 0, None) == E_SHAPE and run(x, w, None, o, None, 0, *good, 1, 2, None) == E_SHAPE
    assert run(ctypes.c_void_p((1 << 34) + 4), w, None, o, None, 0, *good, 1, 0, None) == E_LIMIT
    assert run(x, w, None, o, ctypes.c_void_p(8 << 34), wsb(*good) - 4, *good, 1, 0, None) == E_LIMIT
    assert run(x, w, None, x, ctypes.c_void_p(8 << 34), wsb(*good), *good, 1, 0, None) == -4          # out == x: HDN_E_ALIAS


def test_simi_stem_refuses_bad_arguments_before_any_launch():
    """NULL (the bias included), S = 6, B = 0, act_domain 1: HDN_E_NULL / HDN_E_SHAPE; the documented limit + 1 and a misaligned stream: HDN_E_LIMIT."""
    from hdn_amd import trunk as T
    lib = _lib()
    run = lib.hdn_simi_stem_f32
    x, w, b, o = (ctypes.c_void_p(v << 34) for v in (1, 2, 3, 4))
    assert T.SIMI_STEM_MAX_SIDE == SC.STEM_MAX_SIDE >= 255
    for args in ((None, w, b, o), (x, None, b, o), (x, w, None, o), (x, w, b, None)):
        assert run(*args, 1, 127, 0, None) == E_NULL
    assert run(x, w, b, o, 1, 6, 0, None) == E_SHAPE
    assert run(x, w, b, o, 0, 127, 0, None) == E_SHAPE
    assert run(x, w, b, o, 1, 127, 1, None) == E_SHAPE
    assert run(x, w, b, o, 1, SC.STEM_MAX_SIDE + 1, 0, None) == E_LIMIT
    assert run(x, ctypes.c_void_p((2 << 34) + 8), b, o, 1, 127, 0, None) == E_LIMIT
    assert run(x, w, b, x, 1, 127, 0, None) == -4
    with pytest.raises(ValueError):
        T.pack_simi_stem(torch.zeros(64, 2, 7, 7))
    w7 = torch.zeros(64, 3, 7, 7)
    w7[5, 1, 2, 3] = 7e4
    with pytest.raises(ValueError, match="fp16 range"):
        T.pack_simi_stem(w7)
    n = lib.hdn_pack_simi_stem_bytes()
    out = torch.full((n // 2 + 8,), 77, dtype=torch.int16)
    assert lib.hdn_pack_simi_stem_f32(w7.data_ptr(), out.data_ptr(), n - 2) == E_SHAPE and bool((out == 77).all())
    assert lib.hdn_pack_simi_stem_f32(None, out.data_ptr(), n) == E_NULL


def _stem_weights(kind):
    if kind == "random":
        w = torch.randn(64, 3, 7, 7, generator=torch.Generator().manual_seed(11)) * (2.0 / 147) ** 0.5
        w.view(-1)[::7] *= 2.0 ** -12
        return w
    # every element distinct, with a second piece that is not zero: a permuted position cannot go unseen
    return (torch.arange(64 * 147, dtype=torch.float32).view(64, 3, 7, 7) + 1) * (1.0 + 2.0 ** -13) * 2.0 ** -10


@pytest.mark.parametrize("kind", ["random", "distinct"])
def test_pack_simi_stem_stream_decoded_by_its_documented_layout(kind):
    """include/hdn_hip.h / csrc/simi_stem.hip: [11 k steps][2 n tiles][2 pieces][k half g][32 n][8] fp16, element j of lane (g, n) of k step s = piece of
    w[32 tile + n][ci][ky][kx = j] with ci 7 + ky = 2 s + g; exactly zero at j = 7 and at 2 s + g = 21.  Indexed so with numpy, piece 0 is fp16(w) and
    piece 1 is fp16((w - piece 0) 2^11) bit for bit, and p0 + 2^-11 p1 gives w back to 2^-21 relative where |w| >= 2^-14 (2^-36 absolute below)."""
    from hdn_amd import trunk as T
    w = _stem_weights(kind)
    if kind == "distinct":
        assert w.unique().numel() == w.numel()
    stream = T.pack_simi_stem(w).numpy().view(np.float16)
    assert stream.size == 11 * 2 * 2 * 2 * 32 * 8
    p = stream.reshape(11, 2, 2, 2, 32, 8)                                     # (step, tile, piece, g, n, j)
    p = p.transpose(1, 4, 0, 3, 5, 2).reshape(64, 22, 8, 2)                    # (tile, n | step, g | j | piece) = (co, r, j, piece)
    assert not p[:, 21].view(np.int16).any() and not p[:, :, 7].view(np.int16).any()          # the padding: +0.0 in both pieces
    p = torch.from_numpy(p[:, :21, :7].copy()).reshape(64, 3, 7, 7, 2)         # r = ci 7 + ky, j = kx
    p0 = w.half()
    p1 = ((w - p0.float()) * 2048.0).half()
    for name, got, want in (("piece 0", p[..., 0], p0), ("piece 1", p[..., 1], p1)):
        bad = (got.contiguous().view(torch.int16) != want.view(torch.int16)).nonzero()
        if bad.shape[0]:
            raise AssertionError(f"{name}: {bad.shape[0]} of {want.numel()} elements are not where the layout says; first (co, ci, ky, kx) = {bad[0].tolist()}")
    back = p[..., 0].double() + p[..., 1].double() * 2.0 ** -11
    err, mag = (back - w.double()).abs(), w.double().abs()
    normal = mag >= 2.0 ** -14
    assert bool((err[normal] <= 2.0 ** -21 * mag[normal]).all()), float((err[normal] / mag[normal]).max())
    if kind == "random":
        assert (~normal).any() and float(err[~normal].max()) <= 2.0 ** -36


def test_conv3x3v_queries_over_the_gpu_case_list():
    """Every case has the form the list files it under (all five are reached), Z <= 16, and the workspace is Z M CO 4 bytes with M = B So^2 and So from
    the entry point's own rule, or 0 where K is not split."""
    lib = _lib()
    assert set(SC.V_CASES) == {"A", "A split", "B", "B split", "C"} and set(SC.V_EXACT) <= set(SC.V_ALL)
    for name, cases in SC.V_CASES.items():
        for (B, S, CI, CO, st) in cases:
            fm, nb = lib.hdn_conv3x3v_form(B, S, CI, CO, st), lib.hdn_conv3x3v_workspace_bytes(B, S, CI, CO, st)
            assert SC.v_form_name(fm) == name, ((B, S, CI, CO, st), SC.v_form_name(fm), name)
            Z, So = fm >> 16, SC.v_out_side(S, st)
            assert 1 <= Z <= 16 and nb == (Z * B * So * So * CO * 4 if Z > 1 else 0), ((B, S, CI, CO, st), fm, nb)
    assert SC.v_out_side(8, 2) == 3 and SC.v_out_side(3, 2) == 1 and SC.v_out_side(7, 1) == 5
    # the same M gives the same schedule as the dilated kernel (one dispatch rule): 31 x 31 valid from 63 / stride 2 against 31 x 31 padded
    assert lib.hdn_conv3x3v_form(1, 63, 256, 512, 2) == lib.hdn_conv3x3d_form(1, 31, 256, 512, 1)


def _standin_model():
    import production_standin as PS
    torch.manual_seed(2)
    return PS, types.SimpleNamespace(backbone=PS.AtrousResNet50().eval(), neck=PS.Necks(True).eval(), neck_lp=PS.Necks(False).eval())


def test_hip_plan_level_2_leaves_nothing_to_the_library():
    from torch import nn
    from hdn_amd import backbone as BB
    PS, model = _standin_model()
    net = model.backbone
    p1, p2 = BB.hip_plan(net), BB.hip_plan(net, level=2)
    assert p1 == BB.hip_plan(net, level=1) and "stem" not in p1
    assert {k for k, v in p1.items() if v == "miopen"} == {"layer2.0.conv2", "layer2.0.downsample"}          # level 1 as it was
    assert "miopen" not in p2.values()
    assert p2["layer2.0.conv2"] == p2["layer2.0.downsample"] == "conv3x3v" and p2["stem"] == "simi_stem"
    assert set(p2) == set(p1) | {"stem"} and all(p2[k] == v for k, v in p1.items() if v != "miopen")
    conv = nn.Conv2d(128, 128, 3, stride=2)
    assert BB.hip_conv_kind(conv) == BB.hip_conv_kind(conv, level=1) == "miopen" and BB.hip_conv_kind(conv, level=2) == "conv3x3v"
    assert BB.hip_conv_kind(nn.Conv2d(128, 128, 3, stride=1), level=2) == "conv3x3v"
    assert BB.hip_conv_kind(nn.Conv2d(128, 128, 3, stride=3), level=2) == "miopen"
    assert BB.hip_conv_kind(nn.Conv2d(48, 128, 3, stride=2), level=2) == "miopen"
    assert BB.hip_conv_kind(nn.Conv2d(128, 128, 3, stride=2, dilation=2), level=2) == "miopen"
    assert BB.hip_conv_kind(nn.Conv2d(128, 128, 3, stride=2, padding=1), level=2) == "miopen"
    net.used_layers = [0, 2]
    assert BB.hip_plan(net, level=2)["stem"] == "miopen"
    net.used_layers = [2, 3, 4]
    net.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
    assert BB.hip_plan(net, level=2)["stem"] == "miopen"
    net.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=0, bias=False)
    net.maxpool = nn.MaxPool2d(3, 2, 1, ceil_mode=True)
    assert BB.hip_plan(net, level=2)["stem"] == "miopen"
    net.maxpool = nn.MaxPool2d(3, 2, 1)
    assert BB.hip_plan(net, level=2)["stem"] == "simi_stem"


def test_the_level_switch(monkeypatch):
    """HDN_HIP_BACKBONE=2 or hip=2 builds level 2 (HipAtrousResNetFull: layer2.0's conv2 / skip on "conv3x3v", the packed stem a non-persistent buffer);
    "1" / True builds exactly level 1; state_dict keys and the class name never change; restore undoes it."""
    from hdn_amd import backbone as BB
    PS, model = _standin_model()
    keys = [list(m.state_dict().keys()) for m in (model.backbone, model.neck, model.neck_lp)]
    for env, want in ((None, 0), ("", 0), ("0", 0), ("1", 1), ("2", 2), ("yes", 1)):
        if env is None:
            monkeypatch.delenv("HDN_HIP_BACKBONE", raising=False)
        else:
            monkeypatch.setenv("HDN_HIP_BACKBONE", env)
        assert BB.hip_level() == want and BB.hip_enabled() == (want > 0)
    for env, hip, level in (("2", None, 2), (None, 2, 2), ("1", None, 1), (None, True, 1), ("2", True, 1), ("2", False, 0), ("1", 2, 2), (None, None, 0)):
        if env is None:
            monkeypatch.delenv("HDN_HIP_BACKBONE", raising=False)
        else:
            monkeypatch.setenv("HDN_HIP_BACKBONE", env)
        assert BB.optimize_similarity_model(model, strict=True, hip=hip) == ["backbone", "neck", "neck_lp"]
        fb = vars(model.backbone)["_hdn_fused"]
        assert type(fb) is (BB.FusedAtrousResNet, BB.HipAtrousResNet, BB.HipAtrousResNetFull)[level]
        if level:
            assert {type(b) for layer in fb.layers for b in layer} == {BB.HipBottleneck}
            b = fb.layers[1][0]
            assert (b.c1.kind, b.c3.kind) == ("conv1x1", "conv1x1")
        if level == 2:
            assert (b.c2.kind, b.cd.kind) == ("conv3x3v", "conv3x3v") and b.c2.weight is None and b.cd.weight is None
            assert b.c2.packed.dtype == torch.int16 and b.c2.packed.numel() == 2 * 9 * 128 * 128 and b.cd.packed.numel() == 2 * 9 * 256 * 512
            assert torch.equal(b.b3, b.c3.bias + b.cd.bias)                              # the skip's shift rides in the last bias
            assert fb.fused_stem and fb.stem_packed.dtype == torch.int16 and fb.stem_packed.numel() == 11 * 2 * 2 * 64 * 8
            assert "stem_packed" in dict(fb.named_buffers()) and not any("packed" in k for k in fb.state_dict())
            assert not any(m.kind == "miopen" for m in fb.modules() if isinstance(m, BB._HipConv))
        elif level == 1:
            assert (b.c2.kind, b.cd.kind) == ("miopen", "miopen") and b.c2.packed is None and b.c2.weight is not None
            assert not hasattr(fb, "stem_packed")
        assert [list(m.state_dict().keys()) for m in (model.backbone, model.neck, model.neck_lp)] == keys
        assert type(model.backbone).__name__ == "AtrousResNet50"
    BB.restore_similarity_model(model)
    assert type(model.backbone) is PS.AtrousResNet50 and "_hdn_fused" not in vars(model.backbone) and "_hdn_fused" not in vars(model.neck)
    # a network the fused stem does not serve keeps the level-1 stem at level 2
    model.backbone.used_layers = [0, 2]
    BB.optimize_similarity_model(model, strict=True, hip=2)
    fb = vars(model.backbone)["_hdn_fused"]
    assert type(fb) is BB.HipAtrousResNetFull and not fb.fused_stem and fb.stem_packed is None
    BB.restore_similarity_model(model)


def _same(want_int, ref64):
    assert want_int.dtype == torch.int64 and ref64.dtype == torch.float64 and tuple(want_int.shape) == tuple(ref64.shape)
    assert int(want_int.abs().max()) < 1 << 24 and bool(want_int.ne(0).any())
    assert torch.equal(want_int.double(), ref64), (want_int.double() != ref64).nonzero()[0].tolist()


@pytest.mark.parametrize("B,S,CI,CO,st", SC.V_EXACT)
def test_conv3x3v_integer_expectation_equals_float64_conv2d(B, S, CI, CO, st):
    x, w, b, want = SC.v_integer_problem(B, S, CI, CO, st)
    assert int(x.abs().max()) <= 4 and int(w.abs().max()) <= 2
    _same(want, F.conv2d(x.double(), w.double(), b.double(), stride=st, padding=0))


@pytest.mark.parametrize("S", [11, 13, 68, 69])
def test_stem_integer_expectation_equals_float64_conv_and_pool(S):
    """(the expectation's code does not depend on S beyond the sides; the larger tiling sizes are built by the same lines)"""
    x, w, b, want = SC.stem_integer_problem(2, S)
    assert int(x.min()) >= 0 and int(x.max()) <= 255 and set(w.unique().tolist()) == {-1, 0, 1}
    assert w.flatten(1).unique(dim=0).shape[0] == 64                                    # no two channels alike
    assert len({tuple(w[:, c, y, xx].tolist()) for c in range(3) for y in range(7) for xx in range(7)}) == 147      # no two taps alike
    Sc, Sp = SC.stem_sides(S)
    assert tuple(want.shape) == (2, 64, Sp, Sp)
    _same(want, F.max_pool2d(torch.relu(F.conv2d(x.double(), w.double(), b.double(), stride=2)), 3, 2, 1))


def test_stem_tap_expectation_equals_float64_conv_and_pool():
    x, ws, wants = SC.stem_tap_problem(13)
    assert sum(int(w.sum()) for w in ws) == 147 and x.unique().numel() == x.numel()
    for w, want in zip(ws, wants):
        _same(want, F.max_pool2d(torch.relu(F.conv2d(x.double(), w.double(), None, stride=2)), 3, 2, 1))


@pytest.mark.parametrize("S,y0,x0", [(13, 0, 0), (13, 12, 5), (13, 6, 6), (27, 13, 26), (27, 9, 14)])
def test_stem_reached_set_equals_float64_conv_and_pool(S, y0, x0):
    x = torch.zeros(1, 3, S, S, dtype=torch.float64)
    x[0, 1, y0, x0] = 200.0
    ref = F.max_pool2d(torch.relu(F.conv2d(x, torch.ones(64, 3, 7, 7, dtype=torch.float64), None, stride=2)), 3, 2, 1)
    assert torch.equal(ref[0, 0] != 0, SC.stem_reached(S, y0, x0))


def test_stem_sides_are_the_modules_own():
    for S in SC.STEM_SIZES:
        y = F.max_pool2d(F.conv2d(torch.zeros(1, 3, S, S), torch.zeros(1, 3, 7, 7), stride=2), 3, 2, 1)
        Sc, Sp = SC.stem_sides(S)
        assert y.shape[-1] == Sp and (S - 7) // 2 + 1 == Sc
    assert [SC.stem_sides(S)[0] for S in SC.STEM_TILING_SIZES] == [31, 32, 63, 64, 95, 96]
    assert SC.stem_sides(127) == (61, 31) and SC.stem_sides(255) == (125, 63) and SC.stem_sides(11) == (3, 2) and SC.stem_sides(13) == (4, 2)
