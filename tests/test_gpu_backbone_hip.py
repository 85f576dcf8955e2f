"""The opt-in HIP form of the similarity backbone (hdn_amd.backbone.optimize_similarity_model(model, hip=True) / HDN_HIP_BACKBONE=1): the production
stand-in's ResNet-50 and necks on hdn_conv1x1_f32 / hdn_conv3x3d_f32 against the modules' own forward, proof that the kernels run (F.conv2d call
count), reload under a captured hipGraph, and DeviceTrackerHomo with the variable set."""
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _model(dev):
    """test_backbone_folding_on_the_device's model: the stand-in, its seeds, perturbed BatchNorm statistics."""
    import production_standin as PS
    torch.manual_seed(2)
    model = types.SimpleNamespace(backbone=PS.AtrousResNet50(), neck=PS.Necks(True), neck_lp=PS.Necks(False))
    for i, part in enumerate((model.backbone, model.neck, model.neck_lp)):
        PS._seed(part, 40 + i)
        for m in part.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.1, 0.1); m.running_var.uniform_(0.8, 1.3); m.bias.data.uniform_(-0.1, 0.1)
        part.to(dev).eval()
    return PS, model


def _all(model, x):
    f = model.backbone(x)
    return list(f) + list(model.neck(f)) + list(model.neck_lp(f))


def _close(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape
        err, lim = float((g - w).abs().max()), 1e-4 * float(w.abs().max())
        assert err <= lim, (err, lim)


def test_hip_backbone_and_necks_on_the_device(dev, monkeypatch):
    """Every feature level and both necks' outputs within 1e-4 max|want| of the modules' own forward at 127- and 255-px crops, B = 1 and B = 3;
    state_dict keys unchanged; the necks return NCHW-contiguous tensors; two forwards bit-equal, the second given the first's results of its three F.conv2d calls (the library picks a
    convolution's solver per call — a heuristic before it has searched that shape, the search's winner after — so its bits may change between calls, in
    the folded form as well; every launch of the project's own must repeat bit for bit); F.conv2d is called exactly three times per forward
    (the 7x7 stem, layer2.0's stride-2 conv2 and its strided 3x3 skip: everything else is hdn_conv1x1_f32 / hdn_conv3x3d_f32); training mode takes the
    class's forward; restore_similarity_model restores the class."""
    import torch.nn.functional as F
    from hdn_amd import backbone as BB
    PS, model = _model(dev)
    keys = [list(m.state_dict().keys()) for m in (model.backbone, model.neck, model.neck_lp)]
    xs = [torch.randn(b, 3, s, s, device=dev) * 60 + 110 for s in (127, 255) for b in (1, 3)]
    with torch.no_grad():
        ref = [_all(model, x) for x in xs]
        assert BB.optimize_similarity_model(model, strict=True, hip=True) == ["backbone", "neck", "neck_lp"]
        assert isinstance(vars(model.backbone)["_hdn_fused"], BB.HipAtrousResNet)
        assert [list(m.state_dict().keys()) for m in (model.backbone, model.neck, model.neck_lp)] == keys
        assert type(model.backbone).__name__ == "AtrousResNet50"
        real = F.conv2d
        for x, want in zip(xs, ref):
            kept = []
            monkeypatch.setattr(F, "conv2d", lambda *a, **k: (kept.append(real(*a, **k)), kept[-1].clone())[1])
            got = _all(model, x)
            _close(got, want)
            assert all(g.is_contiguous() for g in got[3:])                       # the necks' outputs, cropped or not
            replay = iter(kept)
            monkeypatch.setattr(F, "conv2d", lambda *a, **k: next(replay).clone())
            again = _all(model, x)
            monkeypatch.setattr(F, "conv2d", real)
            assert len(kept) == 3 and next(replay, None) is None
            assert all(torch.equal(a, b) for a, b in zip(got, again))
        calls = []
        monkeypatch.setattr(F, "conv2d", lambda *a, **k: (calls.append(tuple(a[1].shape)), real(*a, **k))[1])
        _all(model, xs[0])
        monkeypatch.setattr(F, "conv2d", real)
        assert sorted(calls) == sorted([(64, 3, 7, 7), (128, 128, 3, 3), (512, 256, 3, 3)]), calls
        model.backbone.train()
        assert not BB._use_fused(model.backbone, xs[0])
        model.backbone.eval()
        BB.restore_similarity_model(model)
        assert "_hdn_fused" not in vars(model.backbone) and type(model.backbone) is PS.AtrousResNet50 and type(model.neck) is PS.Necks
        _close(_all(model, xs[0]), ref[0])


def test_hip_backbone_reload_under_a_captured_graph(dev):
    """A hip forward captured in a torch.cuda.graph replays; after load_state_dict with perturbed weights the SAME graph gives the unoptimised module's
    result on the new weights (1e-4 max|want|): the hook re-folds and re-packs into the same storage (buffer pointers unchanged)."""
    from hdn_amd import backbone as BB
    PS, model = _model(dev)
    x = torch.randn(1, 3, 127, 127, device=dev) * 60 + 110
    with torch.no_grad():
        want0 = _all(model, x)
        BB.optimize_similarity_model(model, strict=True, hip=True)
        parts = (model.backbone, model.neck, model.neck_lp)
        ptrs = [[(n, b.data_ptr()) for n, b in vars(p)["_hdn_fused"].named_buffers()] for p in parts]
        assert any("packed" in n for n, _ in ptrs[0]) and any("packed" in n for n, _ in ptrs[1])
        static = x.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                _all(model, static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = _all(model, static)
        graph.replay()
        torch.cuda.synchronize()
        _close([o.clone() for o in outs], want0)
        g = torch.Generator().manual_seed(9)
        plain = []
        for p in parts:
            sd = {k: (v * (1 + 0.05 * torch.randn(v.shape, generator=g).to(v.device)) if v.dtype.is_floating_point and "running_var" not in k else v.clone())
                  for k, v in p.state_dict().items()}
            p.load_state_dict(sd)
            q = type(p).__mro__[1](*(() if p is model.backbone else (p is model.neck,))).to(dev).eval()      # the unoptimised class, new weights
            q.load_state_dict(sd)
            plain.append(q)
        want1 = _all(types.SimpleNamespace(backbone=plain[0], neck=plain[1], neck_lp=plain[2]), x)
        assert float((want1[2] - want0[2]).abs().max()) > 1e-3 * float(want0[2].abs().max())       # the new weights do change the result
        graph.replay()
        torch.cuda.synchronize()
        _close([o.clone() for o in outs], want1)
        assert [[(n, b.data_ptr()) for n, b in vars(p)["_hdn_fused"].named_buffers()] for p in parts] == ptrs
        BB.restore_similarity_model(model)


def test_device_tracker_homo_with_the_hip_backbone(dev, monkeypatch):
    """DeviceTrackerHomo around the production stand-in with HDN_HIP_BACKBONE=1 (the tracker calls optimize_similarity_model itself: it follows the
    variable) against the CPU loop, the sequence and bounds of test_device_tracker_homo_runs_production_shaped_model: first frame 1e-3 px, any of the
    first 6 frames 0.1 px."""
    from synth_sequence import make_sequence, success_4pts_error
    from test_gpu_tracker import _production_pair
    from hdn_amd import backbone as BB
    from hdn_amd.tracker import DeviceTrackerHomo
    frames, corners, init = make_sequence(n_frames=13, frame_hw=(720, 1280), target_wh=(300, 200), seed=20260928)
    frames = frames[:7]
    ref, model = _production_pair(dev, frames, init)
    monkeypatch.setenv("HDN_HIP_BACKBONE", "1")
    trk = DeviceTrackerHomo(model)
    assert trk.folded == ["backbone", "neck", "neck_lp"] and isinstance(vars(model.backbone)["_hdn_fused"], BB.HipAtrousResNet)
    ref.init(frames[0], init["bbox"], init["poly"], init["gt_points"], init["first_point"])
    trk.init(frames[0], init["bbox"], init["poly"], init["gt_points"], init["first_point"])
    errs = []
    for t in range(1, len(frames)):
        a, b = trk.track_new(t, frames[t]), ref.track_new(t, frames[t])
        errs.append(success_4pts_error(a["points"], b["points"]))
    print("DeviceTrackerHomo with HDN_HIP_BACKBONE=1, corner error vs CPU loop (px):", " ".join(f"{e:.1e}" for e in errs))
    assert errs[0] <= 1e-3, errs
    assert max(errs) <= 0.1, errs
    BB.restore_similarity_model(model)
