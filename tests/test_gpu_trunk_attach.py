"""GPU tests of the HIP homography trunk behind the reference's objects: DeviceTrackerHomo(model, hip_trunk=True) and install(trunk=True) attach the
folded trunk to model.hm_net for both trunks the reference can build (cfg.BACKBONE_HOMO.TYPE resnet34 / resnet50), the tracker loop keeps the
bounds of test_sequence_stream_device_loop_vs_cpu_restatement, a reload of the weights is seen, uninstall() detaches."""
import copy
import os
import sys
import time
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _seeded_hm_net(backbone, tag=620):
    """hdn_amd.HomoModelBuilder with seeded weights (activations O(1) through all 16 blocks) and test_gpu_parity._seeded_net's regressor."""
    import make_golden as mg
    import hdn_amd
    torch.manual_seed(123)
    net = hdn_amd.HomoModelBuilder(backbone=backbone).eval()
    mg.seeded_trunk_state_(net.backbone, tag)
    net.fc.weight.data.mul_(0.01)
    net.fc.bias.data.copy_(torch.tensor([3.0, -2.0, 1.5, 4.0, -3.5, 2.5, 0.5, -1.0]))
    return net


def _pair(dev, backbone):
    """(CPU restatement of the loop, the seeded stand-in for the reference's ModelBuilder on the GPU, its TrackerConfig), as
    tests/test_gpu_tracker.py:_similarity_pair builds them."""
    import standin_model as SM
    from hdn_amd.similarity import TrackerConfig
    from oracle.tracker_oracle import HomoTrackerOracle, SimilarityOracle
    net = _seeded_hm_net(backbone)
    net_cpu = copy.deepcopy(net)
    twin = SM.StandInSiamese(net).eval()
    cpu = SM.StandInSiameseCPU(twin)
    sd = {k: v.clone() for k, v in net_cpu.ShareFeature.state_dict().items()}
    ref = HomoTrackerOracle(sd, lambda f: net_cpu.fc(net_cpu.avgpool(net_cpu.backbone(f)).flatten(1)), similarity=SimilarityOracle(cpu))
    twin = twin.to(dev)
    return ref, twin, TrackerConfig(cls_out_channels=twin.cls_out)


@pytest.mark.parametrize("backbone", ["resnet34", "resnet50"])
def test_device_tracker_hip_trunk_sequence_vs_cpu_loop(dev, backbone, monkeypatch):
    """DeviceTrackerHomo(model, hip_trunk=True), one hipGraph per frame, over the synthetic sequence of
    test_sequence_stream_device_loop_vs_cpu_restatement against the CPU loop, under that test's bounds: first frame <= 2e-4 px, first five
    <= 5e-4, all <= 5e-3."""
    from synth_sequence import make_sequence, success_4pts_error
    from hdn_amd import trunk as T
    from hdn_amd.tracker import DeviceTrackerHomo
    monkeypatch.delenv("HDN_HIP_TRUNK", raising=False)
    frames, corners, init = make_sequence(n_frames=16, frame_hw=(360, 640), target_wh=(150, 100), seed=7)
    ref, twin, cfg = _pair(dev, backbone)
    plain = DeviceTrackerHomo(twin, cfg=cfg, graph=True, fold_backbone=False)                       # the default: nothing attached
    assert plain.hip_trunk is False and getattr(twin.hm_net, "_hdn_fast_trunk", None) is None
    assert DeviceTrackerHomo(twin, cfg=cfg, fold_backbone=False, hip_trunk=False).hip_trunk is False
    assert getattr(twin.hm_net, "_hdn_fast_trunk", None) is None
    # the unattached loop first (its per-frame time is the yardstick), then the attached one
    times = {}
    plain.init(frames[0], init["bbox"], init["poly"], init["gt_points"], init["first_point"])
    for t in range(1, 4):
        plain.track_new(t, frames[t])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(4, len(frames)):
        plain.track_new(t, frames[t])
    times["plain"] = (time.perf_counter() - t0) / (len(frames) - 4)
    trk = DeviceTrackerHomo(twin, cfg=cfg, graph=True, fold_backbone=False, hip_trunk=True)
    fast = twin.hm_net._hdn_fast_trunk
    kind = T.FusedBasicBlock if backbone == "resnet34" else T.FusedBottleneck
    assert trk.hip_trunk is True and fast is not None and fast.act_domain == 1
    assert all(isinstance(b, kind) for name in ("layer1", "layer2", "layer3", "layer4") for b in getattr(fast, name))
    ref.init(frames[0], init["bbox"], init["poly"], init["gt_points"], init["first_point"])
    trk.init(frames[0], init["bbox"], init["poly"], init["gt_points"], init["first_point"])
    errs, dt = [], 0.0
    for t in range(1, len(frames)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a = trk.track_new(t, frames[t])
        if t >= 4:
            dt += time.perf_counter() - t0
        b = ref.track_new(t, frames[t])
        errs.append(success_4pts_error(a["points"], b["points"]))
    times["hip_trunk"] = dt / (len(frames) - 4)
    assert trk._graph is not None
    print(f"{backbone}: DeviceTrackerHomo(hip_trunk=True) corner errors vs CPU loop (px):", " ".join(f"{e:.1e}" for e in errs))
    print(f"{backbone}: per-frame time, graph on: plain {1e3 * times['plain']:.3f} ms, hip_trunk {1e3 * times['hip_trunk']:.3f} ms")
    from hdn_amd.homo_model import optimize_trunk
    optimize_trunk(twin.hm_net, enable=False)
    assert errs[0] <= 2e-4, errs
    assert max(errs[:5]) <= 5e-4 and max(errs) <= 5e-3, errs


def _data(dev, B=1, seed=3):
    g = np.random.default_rng(seed)
    imgs = torch.from_numpy(g.standard_normal((B, 2, 127, 127)).astype(np.float32)).to(dev)
    h4p = torch.tensor([[0, 0, 0, 127, 127, 127, 127, 0]], dtype=torch.float32).repeat(B, 1).to(dev)
    pidx = torch.arange(127 * 127, dtype=torch.float32).repeat(B, 1).to(dev)
    return {"org_imgs": imgs, "input_tensors": imgs.clone(), "h4p": h4p, "patch_indices": pidx}


@pytest.mark.parametrize("backbone", ["resnet34", "resnet50"])
def test_install_trunk_attaches_at_first_track_proj_and_follows_a_reload(dev, backbone):
    """install(trunk=True) without the device tracker: the first model.track_proj(data, None) attaches the folded HIP trunk to model.hm_net, the
    offsets stay within 1e-4 abs of the unattached call; after hm_net.load_state_dict they follow the new weights; uninstall() detaches."""
    import hdn_amd.install as hinstall
    from hdn_amd.homo_model import homo_stages
    name = "hdn.models.model_builder_e2e_unconstrained_v2"
    mod = types.ModuleType(name)

    class ModelBuilder(torch.nn.Module):
        def __init__(self, hm_net):
            super().__init__()
            self.hm_net = hm_net

        def track_proj(self, data, tmp_mask):
            raise AssertionError("not rebound")

    mod.ModelBuilder = ModelBuilder
    model = ModelBuilder(_seeded_hm_net(backbone)).to(dev).eval()
    net, data = model.hm_net, _data(dev)
    hinstall.install(modules={name: mod})
    try:
        H0, _, _ = model.track_proj(data, None)
        assert getattr(net, "_hdn_fast_trunk", None) is None                 # the default install attaches nothing
        x0 = homo_stages(net, data)["x"].clone()
    finally:
        hinstall.uninstall()
    hinstall.install(modules={name: mod}, trunk=True)
    try:
        H1, _, _ = model.track_proj(data, None)
        assert net._hdn_fast_trunk is not None and len(net._load_state_dict_post_hooks) == 1
        st = homo_stages(net, data)
        e = float((st["x"] - x0).abs().max())
        print(f"{backbone}: offsets attached vs unattached: {e:.3e}")
        assert e <= 1e-4 and torch.isfinite(H1).all()
        # new weights: the next call follows them
        other = _seeded_hm_net(backbone, tag=777)
        other.fc.bias.data.mul_(0.5)
        net.load_state_dict(other.state_dict())
        st = homo_stages(net, data)
        feats = torch.cat((st["patch_1"], st["patch_2"]), dim=1).cpu()
        with torch.no_grad():
            ref = other.fc(other.avgpool(other.backbone(feats)).flatten(1))
        e = float((st["x"].cpu() - ref).abs().max())
        print(f"{backbone}: offsets after load_state_dict vs the new weights' unoptimised result: {e:.3e}")
        assert e <= 1e-4 and float((st["x"] - x0).abs().max()) > 1e-2
    finally:
        hinstall.uninstall()
    assert net._hdn_fast_trunk is None and len(net._load_state_dict_post_hooks) == 0
    assert "track_proj" in vars(ModelBuilder) and vars(ModelBuilder)["track_proj"].__name__ == "track_proj"
