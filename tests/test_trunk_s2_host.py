"""CPU tests of the stride-2 Bottleneck convolution's host side and of the trunk attachment: hdn_pack_conv3x3s2_f32 (host code), the activation-scale
guard (hdn_act_scale_log2 against hdn_amd.trunk.ACT_SCALE_LOG2), optimize_trunk's load_state_dict hook, the `hip_trunk` / `trunk` keywords of the
trackers and of install().  No kernel is launched here."""
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

E_NULL, E_SHAPE, E_LIMIT = -1, -2, -3


def test_pack_conv3x3s2_surface():
    from hdn_amd import _lib, trunk as T
    lib = _lib.load()
    for C in (128, 256, 512):
        assert lib.hdn_pack_conv3x3s2_bytes(C) == 2 * 2 * 9 * C * C
    for C in (64, 96, 1024, 0, -128):
        assert lib.hdn_pack_conv3x3s2_bytes(C) < 0
    g = torch.Generator().manual_seed(3)
    for C in (128, 256, 512):
        n = lib.hdn_pack_conv3x3s2_bytes(C)
        w = torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
        a, b = torch.zeros(n // 2, dtype=torch.int16), torch.ones(n // 2, dtype=torch.int16)
        assert lib.hdn_pack_conv3x3s2_f32(w.data_ptr(), C, a.data_ptr(), n) == 0
        assert lib.hdn_pack_conv3x3s2_f32(w.data_ptr(), C, b.data_ptr(), n) == 0
        assert torch.equal(a, b)                                            # two packs of the same weights: the same bytes, every byte written
        assert torch.equal(T.pack_conv3x3s2(w), a)
        assert lib.hdn_pack_conv3x3s2_f32(w.data_ptr(), C, a.data_ptr(), n - 16) != 0
        assert lib.hdn_pack_conv3x3s2_f32(None, C, a.data_ptr(), n) == E_NULL
        for bad in (7e4, float("nan")):
            w2 = w.clone()
            w2[C - 1, 5, 1, 2] = bad
            assert lib.hdn_pack_conv3x3s2_f32(w2.data_ptr(), C, b.data_ptr(), n) == E_LIMIT
            with pytest.raises(ValueError, match="fp16 range"):
                T.pack_conv3x3s2(w2)
    # no weight is dropped: one changed element in each of the nine taps changes the stream, each at a place of its own
    C = 128
    w = torch.randn(C, C, 3, 3, generator=g) * 0.05
    base = T.pack_conv3x3s2(w)
    seen = set()
    for tap in range(9):
        w2 = w.clone()
        co, ci = 7 * tap + 3, 11 * tap + 5
        w2[co, ci, tap // 3, tap % 3] += 0.25
        p = T.pack_conv3x3s2(w2)
        diff = (p != base).nonzero().flatten().tolist()
        assert 1 <= len(diff) <= 2, (tap, diff)
        assert not seen & set(diff)
        seen |= set(diff)
    with pytest.raises(ValueError):
        T.pack_conv3x3s2(torch.randn(64, 64, 3, 3))
    with pytest.raises(ValueError):
        T.pack_conv3x3s2(torch.randn(128, 128, 1, 1))


def test_pack_conv3x3s2_holds_every_weight_once():
    """The stream is a permutation of the (weight, piece) pairs: sorted first pieces equal the sorted fp16 roundings of the weights."""
    from hdn_amd import trunk as T
    C = 128
    w = torch.randn(C, C, 3, 3, generator=torch.Generator().manual_seed(8)) * 0.05
    p = T.pack_conv3x3s2(w).view(torch.float16).reshape(-1, 2, 64 * 8)            # [..][piece][lane x 8]
    p0 = w.half()
    p1 = ((w - p0.float()) * 2048.0).half()
    assert torch.equal(p[:, 0].reshape(-1).float().sort().values, p0.reshape(-1).float().sort().values)
    assert torch.equal(p[:, 1].reshape(-1).float().sort().values, p1.reshape(-1).float().sort().values)


def test_conv3x3s2_argument_errors_need_no_gpu():
    """hdn_conv3x3s2_f32 validates before any launch: NULL, shape, limit, alias, alignment, workspace."""
    import ctypes
    from hdn_amd import _lib
    lib = _lib.load()
    x, w, b, o, ws = (ctypes.c_void_p(v << 24) for v in (1, 2, 3, 4, 5))
    f = lib.hdn_conv3x3s2_f32
    big = 1 << 30
    assert f(None, w, b, o, ws, big, 2, 16, 128, 0, None) == E_NULL
    assert f(x, None, b, o, ws, big, 2, 16, 128, 0, None) == E_NULL
    assert f(x, w, None, o, ws, big, 2, 16, 128, 0, None) == E_NULL
    assert f(x, w, b, None, ws, big, 2, 16, 128, 0, None) == E_NULL
    assert f(x, w, b, o, ws, big, 0, 16, 128, 0, None) == E_SHAPE
    assert f(x, w, b, o, ws, big, 2, 16, 128, 2, None) == E_SHAPE
    for S, C in ((16, 256), (8, 128), (4, 256), (32, 64), (16, 64)):
        assert f(x, w, b, o, ws, big, 2, S, C, 0, None) == E_LIMIT, (S, C)
        assert lib.hdn_conv3x3s2_workspace_bytes(2, S, C) == E_LIMIT
    assert f(x, w, b, x, ws, big, 2, 16, 128, 0, None) == -4                                        # out == x
    assert f(x, w, b, ctypes.c_void_p((1 << 24) + 4096), ws, big, 2, 16, 128, 0, None) == -4        # out inside x
    assert f(ctypes.c_void_p((1 << 24) + 4), w, b, o, ws, big, 2, 16, 128, 0, None) == E_LIMIT      # misaligned x
    assert f(x, w, b, o, ws, big, 1 << 14, 16, 128, 0, None) == E_LIMIT                             # > 2^31 - 1 input elements
    # the tracker's B = 1 splits K over workgroups: a workspace is needed, and checked
    for S, C in ((16, 128), (8, 256), (4, 512)):
        need = lib.hdn_conv3x3s2_workspace_bytes(1, S, C)
        assert need > 0 and need % (S * S * C * 4) == 0
        assert f(x, w, b, o, None, 0, 1, S, C, 0, None) == E_NULL
        assert f(x, w, b, o, ws, need - 4, 1, S, C, 0, None) == E_LIMIT
    assert lib.hdn_conv3x3s2_workspace_bytes(0, 16, 128) == E_SHAPE
    assert lib.hdn_abi_version() == 10


def test_act_scale_constant_is_checked(monkeypatch):
    from hdn_amd import _lib, trunk as T
    lib = _lib.load()
    assert lib.hdn_act_scale_log2() == T.ACT_SCALE_LOG2 == 8
    monkeypatch.setattr(T, "_scale_checked", False)
    T.check_act_scale()
    assert T._scale_checked
    # a library built with another scale: folding into the scaled domain must refuse
    monkeypatch.setattr(T, "_scale_checked", False)
    monkeypatch.setattr(lib, "hdn_act_scale_log2", lambda: 0, raising=False)
    with pytest.raises(RuntimeError, match="HDN_ACT_SCALE_LOG2"):
        T.check_act_scale()
    # ... through fold_for_inference itself: the scaled domain is checked before any fused (GPU) module is built
    net = T.resnet34_homo().eval()
    with pytest.raises(RuntimeError, match="HDN_ACT_SCALE_LOG2"):
        T.fold_for_inference(net, channels_last=True, fused_stem=True, fused_epilogue=True)
    assert not T._scale_checked


def _seeded_builder(backbone, tag):
    import make_golden as mg
    import hdn_amd
    torch.manual_seed(tag)
    net = hdn_amd.HomoModelBuilder(backbone=backbone).eval()
    mg.seeded_trunk_state_(net.backbone, tag)
    net.fc.weight.data.mul_(0.05)
    return net


@pytest.mark.parametrize("backbone", ["resnet34", "resnet50"])
def test_optimize_trunk_refolds_after_load_state_dict(backbone):
    from hdn_amd.homo_model import _regress, optimize_trunk
    net, other = _seeded_builder(backbone, 620), _seeded_builder(backbone, 777)
    feats = torch.from_numpy(np.random.default_rng(4).standard_normal((2, 2, 127, 127)).astype(np.float32))
    plain = lambda m: m.fc(m.avgpool(m.backbone(feats)).flatten(1))
    hooks0 = len(net._load_state_dict_post_hooks)
    optimize_trunk(net, fused_stem=False, fused_epilogue=False)
    optimize_trunk(net, fused_stem=False, fused_epilogue=False)                 # twice: still one hook
    assert len(net._load_state_dict_post_hooks) == hooks0 + 1
    fast = net._hdn_fast_trunk
    assert fast is not None and not any(isinstance(m, nn.BatchNorm2d) for m in fast.modules())
    with torch.no_grad():
        old = plain(net)
        assert float((_regress(net, feats) - old).abs().max()) <= 1e-5 * float(old.abs().max())
        net.load_state_dict(other.state_dict())
        new = plain(other)
        got = _regress(net, feats)
    scale = float(new.abs().max())
    assert float((got - new).abs().max()) <= 1e-5 * scale, float((got - new).abs().max())
    assert float((got - old).abs().max()) > 1e-2 * scale                       # ... and not the old snapshot's answer
    assert net._hdn_fast_trunk is fast                                         # re-folded into the existing tensors
    assert list(net.state_dict().keys()) == list(other.state_dict().keys())    # the folded copy is no registered sub-module
    optimize_trunk(net, enable=False)
    assert len(net._load_state_dict_post_hooks) == hooks0 and net._hdn_fast_trunk is None
    optimize_trunk(net, enable=False)                                          # idempotent
    assert len(net._load_state_dict_post_hooks) == hooks0


def test_tracker_constructors_take_hip_trunk(monkeypatch):
    from hdn_amd.batched_tracker import BatchedDeviceTracker
    from hdn_amd.tracker import DeviceTrackerHomo, hip_trunk_enabled
    for cls in (DeviceTrackerHomo, BatchedDeviceTracker):
        p = inspect.signature(cls.__init__).parameters
        assert "hip_trunk" in p and p["hip_trunk"].default is None
    monkeypatch.delenv("HDN_HIP_TRUNK", raising=False)
    assert hip_trunk_enabled() is False                                        # the default of this release
    monkeypatch.setenv("HDN_HIP_TRUNK", "1")
    assert hip_trunk_enabled() is True
    monkeypatch.setenv("HDN_HIP_TRUNK", "0")
    assert hip_trunk_enabled() is False


def test_install_trunk_keyword_and_uninstall_restore_the_class():
    import hdn_amd.install as hinstall
    assert "trunk" in inspect.signature(hinstall.install).parameters
    sentinel = object()
    name = "hdn.models.model_builder_e2e_unconstrained_v2"
    mod = types.ModuleType(name)

    class ModelBuilder:
        def track_proj(self, data, tmp_mask):
            return sentinel

    mod.ModelBuilder = ModelBuilder
    before = dict(vars(ModelBuilder))
    done = hinstall.install(modules={name: mod}, trunk=True)
    assert (name, "ModelBuilder.track_proj") in done
    assert ModelBuilder.__dict__["track_proj"] is hinstall._track_proj_trunk_method
    # a CPU hm_net is left alone by the attaching method (nothing to launch here)
    net = _seeded_builder("resnet34", 5)
    assert hinstall._maybe_attach_trunk(net) is False and getattr(net, "_hdn_fast_trunk", None) is None
    hinstall.uninstall()
    assert dict(vars(ModelBuilder)) == before and ModelBuilder().track_proj(None, None) is sentinel
    hinstall.install(modules={name: mod})
    assert ModelBuilder.__dict__["track_proj"] is hinstall._track_proj_method   # the default: no attachment
    hinstall.uninstall()
    assert dict(vars(ModelBuilder)) == before and hinstall.uninstall() == 0
