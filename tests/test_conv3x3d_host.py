"""CPU tests of the dilated 3x3 matrix-core convolution's host side (tests/test_gpu_conv3x3d.py and tests/test_gpu_backbone_hip.py run it): the
hdn_pack_conv3x3d_f32 stream decoded from its documented layout, hdn_conv3x3d_form / hdn_conv3x3d_workspace_bytes at hand-computed cases and on bad
arguments, and which convolutions of the reference-layout ResNet-50 hdn_amd.backbone hands to which kernel.  No kernel is launched here."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

E_NULL, E_SHAPE, E_LIMIT = -1, -2, -3


def form(MT, NT, WM, WN, Z):
    """The value hdn_conv3x3d_form gives for Cfg<MT, NT, WM, WN> with Z slices of K (include/hdn_hip.h)."""
    return MT | NT << 4 | WM << 8 | WN << 12 | Z << 16


@pytest.mark.parametrize("CO,CI", [(32, 32), (96, 64), (64, 160)])
def test_pack_conv3x3d_stream_decoded_by_its_documented_layout(CO, CI):
    """include/hdn_hip.h / csrc/pack.hip: [CO/32 n tiles][9 taps][CI/32 chunks][2 k steps t][piece][k half g][32 n][8] fp16, element e of lane (g, n) =
    piece of w[32 tile + n][32 chunk + 16 g + 8 t + e][tap = 3 ky + kx].  Indexed so with numpy, piece 0 is fp16(w) and piece 1 is
    fp16((w - piece 0) 2^11) bit for bit at every (co, ci, tap), and p0 + 2^-11 p1 gives w back to 2^-21 relative where |w| >= 2^-14 (both pieces
    normal fp16 numbers) and to 2^-36 absolute below that (the bound and its reasoning: tests/test_trunk50_forms_host.py).  The weights are He-scaled
    with every 7th one shrunk by 2^-12, so that both classes have members at every shape."""
    from hdn_amd import trunk as T
    w = torch.randn(CO, CI, 3, 3, generator=torch.Generator().manual_seed(CO + CI)) * (2.0 / (9 * CI)) ** 0.5
    w.view(-1)[::7] *= 2.0 ** -12
    stream = T.pack_conv3x3d(w).numpy().view(np.float16)
    assert stream.size == 2 * 9 * CO * CI
    p = stream.reshape(CO // 32, 9, CI // 32, 2, 2, 2, 32, 8)                  # (nt, tap, chunk, t, piece, g, n, e)
    p = p.transpose(0, 6, 2, 5, 3, 7, 1, 4).reshape(CO, CI, 9, 2)             # (nt, n | chunk, g, t, e | tap | piece) = (co, ci, tap, piece)
    w9 = w.reshape(CO, CI, 9)
    p0 = w9.half()
    p1 = ((w9 - p0.float()) * 2048.0).half()
    got0, got1 = torch.from_numpy(p[..., 0].copy()), torch.from_numpy(p[..., 1].copy())
    for name, got, want in (("piece 0", got0, p0), ("piece 1", got1, p1)):
        bad = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
        if bad.shape[0]:
            raise AssertionError(f"{name}: {bad.shape[0]} of {got.numel()} elements are not where the layout says; first (co, ci, tap) = {bad[0].tolist()}")
    back = got0.double() + got1.double() * 2.0 ** -11
    err, mag = (back - w9.double()).abs(), w9.double().abs()
    normal = mag >= 2.0 ** -14
    assert normal.any() and (~normal).any()
    assert bool((err[normal] <= 2.0 ** -21 * mag[normal]).all()), float((err[normal] / mag[normal]).max())
    assert float(err[~normal].max()) <= 2.0 ** -36, float(err[~normal].max())


def test_pack_conv3x3d_refuses_what_it_cannot_hold():
    """|w| >= 65,504 or NaN: HDN_E_LIMIT (ValueError from the wrapper); an out_bytes that is not hdn_pack_conv3x3d_bytes, channel counts that are no
    multiples of 32, NULL pointers: refused, nothing written."""
    import ctypes
    from hdn_amd import _lib, trunk as T
    lib = _lib.load()
    w = torch.zeros(32, 64, 3, 3)
    n = lib.hdn_pack_conv3x3d_bytes(32, 64)
    assert n == 2 * 2 * 9 * 32 * 64
    for bad in (65504.0, -7e4, float("nan"), float("inf")):
        w2 = w.clone()
        w2[3, 5, 1, 2] = bad
        with pytest.raises(ValueError, match="fp16 range"):
            T.pack_conv3x3d(w2)
        out = torch.zeros(n // 2, dtype=torch.int16)
        assert lib.hdn_pack_conv3x3d_f32(w2.data_ptr(), 32, 64, out.data_ptr(), n) == E_LIMIT
    assert T.pack_conv3x3d(w.fill_(65503.0)).numel() == n // 2
    out = torch.full((n // 2 + 8,), 77, dtype=torch.int16)
    for nb in (n - 2, n + 2, 0, n // 2):
        assert lib.hdn_pack_conv3x3d_f32(w.data_ptr(), 32, 64, out.data_ptr(), nb) == E_SHAPE
    assert bool((out == 77).all())
    assert lib.hdn_pack_conv3x3d_bytes(48, 64) == E_SHAPE and lib.hdn_pack_conv3x3d_bytes(32, 0) == E_SHAPE
    assert lib.hdn_pack_conv3x3d_f32(None, 32, 64, out.data_ptr(), n) == E_NULL
    assert lib.hdn_pack_conv3x3d_f32(w.data_ptr(), 32, 64, None, n) == E_NULL
    with pytest.raises(ValueError):
        T.pack_conv3x3d(torch.zeros(32, 32, 1, 1))


def test_conv3x3d_form_hand_computed():
    """hdn_conv3x3d_form against the rule at the top of csrc/conv3x3d.hip, worked out by hand (FILL = 256 workgroups, tm = ceil(M / 128), K steps =
    9 CI / 32): CO % 64 -> A <1,1,4,1>, tm CO / 32 workgroups; CO % 128 == 0 and tm CO / 128 >= FILL -> C <2,2,2,2>, never split; else B <1,2,4,1>,
    tm CO / 64 workgroups.  A / B below FILL: Z' = min(ceil(FILL / workgroups), 16, steps / 4) slices wanted, ceil(steps / Z') steps per slice,
    Z = ceil(steps / that)."""
    from hdn_amd import _lib
    f = _lib.load().hdn_conv3x3d_form
    # (B, S, CI, CO, d)
    assert f(2, 5, 32, 96, 2) == form(1, 1, 4, 1, 2)              # A: 3 workgroups, 9 steps: 2 slices wanted, 5 steps each -> Z = 2
    assert f(3, 63, 32, 96, 1) == form(1, 1, 4, 1, 1)             # A: M = 11,907, 94 x 3 = 282 workgroups
    assert f(1, 31, 256, 256, 2) == form(1, 2, 4, 1, 8)           # B: the layer-3 shape at B = 1: 8 x 4 = 32 workgroups, 72 steps, 8 slices of 9
    assert f(1, 31, 1024, 2048, 2) == form(1, 2, 4, 1, 1)         # B: the layer-4 skip at B = 1: 8 x 32 = 256 workgroups (C would have 128)
    assert f(16, 31, 1024, 2048, 2) == form(2, 2, 2, 2, 1)        # C at B = 16: 121 x 16 workgroups
    assert f(1, 63, 32, 512, 1) == form(1, 2, 4, 1, 1)            # B unsplit: 32 x 8 = 256 (C: 128)
    assert f(3, 63, 32, 512, 1) == form(2, 2, 2, 2, 1)            # C: 94 x 4 = 376
    assert f(1, 5, 1024, 128, 2) == form(1, 2, 4, 1, 16)          # B: 2 workgroups, 288 steps: 16 slices of 18
    assert f(1, 5, 64, 2048, 1) == form(1, 2, 4, 1, 4)            # B: 32 workgroups, 18 steps: 8 wanted, at most 18 / 4 = 4: 5 steps each -> Z = 4
    assert f(1, 3, 64, 64, 4) == form(1, 2, 4, 1, 4)              # B: 1 workgroup, 18 steps: 4 slices wanted, 5 steps each -> Z = 4


def test_conv3x3d_queries_agree_and_refuse_bad_shapes():
    """hdn_conv3x3d_form and hdn_conv3x3d_workspace_bytes validate alike (dilation 3, CI = 48, ... -> HDN_E_SHAPE; 2^31 elements -> HDN_E_LIMIT), the
    entry point answers the same for those arguments, and the workspace is Z M CO 4 bytes exactly where the form has Z > 1 slices, else 0."""
    import ctypes
    from hdn_amd import _lib
    lib = _lib.load()
    f, wsb = lib.hdn_conv3x3d_form, lib.hdn_conv3x3d_workspace_bytes
    x, w, o = (ctypes.c_void_p(v << 34) for v in (1, 2, 4))
    bad = [((1, 7, 64, 64, 3), E_SHAPE), ((1, 7, 48, 64, 1), E_SHAPE), ((1, 7, 64, 80, 1), E_SHAPE), ((0, 7, 64, 64, 1), E_SHAPE),
           ((1, 0, 64, 64, 1), E_SHAPE), ((1, 7, 64, 64, 0), E_SHAPE), ((1, 7, 64, 64, 8), E_SHAPE), ((1, 7, 0, 64, 1), E_SHAPE),
           ((1 << 14, 32, 256, 64, 1), E_LIMIT), ((1 << 12, 32, 32, 1024, 1), E_LIMIT)]
    for args, want in bad:
        assert f(*args) == want and wsb(*args) == want, args
        B, S, CI, CO, d = args
        assert lib.hdn_conv3x3d_f32(x, w, None, o, None, 0, B, S, CI, CO, d, 1, 0, None) == want, args
    split = unsplit = 0
    for B in (1, 2, 3, 16):
        for S in (1, 2, 5, 15, 31, 63):
            for CI, CO in ((32, 32), (32, 96), (64, 64), (256, 256), (512, 1024), (1024, 2048), (64, 2048), (1024, 128)):
                for d in (1, 2, 4):
                    fm, nb = f(B, S, CI, CO, d), wsb(B, S, CI, CO, d)
                    assert fm > 0 and nb >= 0
                    Z = fm >> 16
                    assert 1 <= Z <= 16
                    assert nb == (Z * B * S * S * CO * 4 if Z > 1 else 0), (B, S, CI, CO, d, fm, nb)
                    split += Z > 1
                    unsplit += Z == 1
    assert split and unsplit
    assert lib.hdn_abi_version() == 10


def _standin_model():
    import production_standin as PS
    torch.manual_seed(2)
    return PS, types.SimpleNamespace(backbone=PS.AtrousResNet50().eval(), neck=PS.Necks(True).eval(), neck_lp=PS.Necks(False).eval())


def test_hip_plan_of_the_reference_layout():
    """hdn_amd.backbone.hip_plan on tests/production_standin.AtrousResNet50 (the reference's layout): a 3x3 convolution gets hdn_conv3x3d_f32 exactly where
    it is stride 1 with padding == dilation, every 1x1 gets hdn_conv1x1_f32, and what is left for MIOpen is layer2's first block: its stride-2,
    padding-0 conv2 and its strided 3x3 skip."""
    from torch import nn
    from hdn_amd import backbone as BB
    PS, model = _standin_model()
    net = model.backbone
    plan = BB.hip_plan(net)
    n3 = 0
    for lname in ("layer1", "layer2", "layer3", "layer4"):
        for i, blk in enumerate(getattr(net, lname)):
            convs = {"conv1": blk.conv1, "conv2": blk.conv2, "conv3": blk.conv3}
            if blk.downsample is not None:
                convs["downsample"] = blk.downsample[0]
            for cn, c in convs.items():
                key = f"{lname}.{i}.{cn}"
                if c.kernel_size == (3, 3):
                    want = "conv3x3d" if (c.stride == (1, 1) and c.padding == c.dilation) else "miopen"
                    n3 += want == "conv3x3d"
                else:
                    assert c.kernel_size == (1, 1)
                    want = "conv1x1"
                assert plan.pop(key) == want, key
    assert not plan
    assert n3 == 15 + 2                                               # every conv2 but layer2.0's, and the 3x3 skips of layer3 / layer4
    assert {k for k, v in BB.hip_plan(net).items() if v == "miopen"} == {"layer2.0.conv2", "layer2.0.downsample"}
    assert BB.hip_conv_kind(nn.Conv2d(64, 64, 3, padding=3, dilation=3)) == "miopen"           # dilation 3
    assert BB.hip_conv_kind(nn.Conv2d(48, 64, 3, padding=1)) == "miopen"                       # CI = 48
    assert BB.hip_conv_kind(nn.Conv2d(64, 64, 3, padding=2, dilation=1)) == "miopen"           # padding != dilation
    assert BB.hip_conv_kind(nn.Conv2d(64, 64, 3, padding=1, groups=2)) == "miopen"


def test_switch_is_off_by_default_and_builds_todays_classes(monkeypatch):
    """optimize_similarity_model with hip off (the default, also through HDN_HIP_BACKBONE unset / 0) builds FusedAtrousResNet / FusedBottleneck /
    _FoldedConv as before; hip=True, or HDN_HIP_BACKBONE=1 with hip=None, builds HipAtrousResNet / HipBottleneck / _HipConv with the packed streams as
    non-persistent buffers; state_dict keys and the class name never change, a CPU input still takes the class's own forward, restore undoes it."""
    from hdn_amd import backbone as BB
    PS, model = _standin_model()
    keys = [list(m.state_dict().keys()) for m in (model.backbone, model.neck, model.neck_lp)]
    monkeypatch.delenv("HDN_HIP_BACKBONE", raising=False)
    assert not BB.hip_enabled()

    def kinds():
        fb, fn = vars(model.backbone)["_hdn_fused"], vars(model.neck)["_hdn_fused"]
        return type(fb), {type(b) for layer in fb.layers for b in layer}, {type(m) for m in fn.modules() if isinstance(m, (BB._FoldedConv, BB._HipConv))}

    for env, hip, want_hip in ((None, None, False), ("0", None, False), (None, False, False), ("1", False, False), ("1", None, True), (None, True, True)):
        if env is None:
            monkeypatch.delenv("HDN_HIP_BACKBONE", raising=False)
        else:
            monkeypatch.setenv("HDN_HIP_BACKBONE", env)
        assert BB.optimize_similarity_model(model, strict=True, hip=hip) == ["backbone", "neck", "neck_lp"]
        top, blocks, necks = kinds()
        if want_hip:
            assert top is BB.HipAtrousResNet and blocks == {BB.HipBottleneck} and necks == {BB._HipConv}
            fb = vars(model.backbone)["_hdn_fused"]
            b = fb.layers[2][0]
            assert (b.c1.kind, b.c2.kind, b.c3.kind, b.cd.kind) == ("conv1x1", "conv3x3d", "conv1x1", "conv3x3d")
            assert b.c2.packed.dtype == torch.int16 and b.c2.packed.numel() == 2 * 9 * 256 * 256 and b.c2.weight is None
            b = fb.layers[1][0]
            assert (b.c2.kind, b.cd.kind) == ("miopen", "miopen") and b.c2.packed is None and b.c2.weight is not None
            assert not any("packed" in k for k in fb.state_dict())
        else:
            assert top is BB.FusedAtrousResNet and blocks == {BB.FusedBottleneck} and necks == {BB._FoldedConv}
        assert [list(m.state_dict().keys()) for m in (model.backbone, model.neck, model.neck_lp)] == keys
        assert type(model.backbone).__name__ == "AtrousResNet50"
        assert not BB._use_fused(model.backbone, torch.zeros(1, 3, 31, 31))             # a CPU tensor: the class's own forward
    BB.restore_similarity_model(model)
    assert type(model.backbone) is PS.AtrousResNet50 and "_hdn_fused" not in vars(model.backbone) and "_hdn_fused" not in vars(model.neck)
