"""Level 2 of the HIP form of the similarity backbone (hdn_amd.backbone.optimize_similarity_model(model, hip=2) / HDN_HIP_BACKBONE=2): the production
stand-in's ResNet-50 and necks with NO library convolution left — hdn_simi_stem_f32, hdn_conv1x1_f32, hdn_conv3x3d_f32, hdn_conv3x3v_f32 — against the
modules' own forward; proof that no F.conv2d is called; two forwards bit-equal with nothing replayed; reload under a captured hipGraph; and
DeviceTrackerHomo with the variable set.  The structure and the model are tests/test_gpu_backbone_hip.py's."""
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
    """test_gpu_backbone_hip's model: the stand-in, its seeds, perturbed BatchNorm statistics."""
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


def _no_library_convolution(*a, **k):
    raise AssertionError("F.conv2d was called: a convolution of the level-2 HIP backbone went to the library")


def test_hip_full_backbone_and_necks_on_the_device(dev, monkeypatch):
    """Every feature level and both necks' outputs within 1e-4 max|want| of the modules' own forward at 127- and 255-px crops, B = 1 and B = 3; state_dict
    keys unchanged; the necks return NCHW-contiguous tensors; with F.conv2d replaced by a function that raises the forward completes (zero library
    convolutions); two forwards of the same input are torch.equal on every output, nothing replayed; training mode takes the class's forward;
    restore_similarity_model restores the class."""
    import torch.nn.functional as F
    from hdn_amd import backbone as BB
    PS, model = _model(dev)
    keys = [list(m.state_dict().keys()) for m in (model.backbone, model.neck, model.neck_lp)]
    xs = [torch.randn(b, 3, s, s, device=dev) * 60 + 110 for s in (127, 255) for b in (1, 3)]
    with torch.no_grad():
        ref = [_all(model, x) for x in xs]
        assert BB.optimize_similarity_model(model, strict=True, hip=2) == ["backbone", "neck", "neck_lp"]
        fb = vars(model.backbone)["_hdn_fused"]
        assert type(fb) is BB.HipAtrousResNetFull and fb.fused_stem
        assert not any(m.kind == "miopen" for m in fb.modules() if isinstance(m, BB._HipConv))
        assert [list(m.state_dict().keys()) for m in (model.backbone, model.neck, model.neck_lp)] == keys
        assert type(model.backbone).__name__ == "AtrousResNet50"
        real = F.conv2d
        monkeypatch.setattr(F, "conv2d", _no_library_convolution)
        try:
            for x, want in zip(xs, ref):
                got = _all(model, x)
                again = _all(model, x)
                _close(got, want)
                assert all(g.is_contiguous() for g in got[3:])                       # the necks' outputs, cropped or not
                assert all(torch.equal(a, b) for a, b in zip(got, again))            # reproducible: no library result is replayed
        finally:
            monkeypatch.setattr(F, "conv2d", real)
        model.backbone.train()
        assert not BB._use_fused(model.backbone, xs[0])
        model.backbone.eval()
        BB.restore_similarity_model(model)
        assert "_hdn_fused" not in vars(model.backbone) and type(model.backbone) is PS.AtrousResNet50 and type(model.neck) is PS.Necks
        _close(_all(model, xs[0]), ref[0])


def test_hip_full_backbone_reload_under_a_captured_graph(dev):
    """A level-2 forward captured in a torch.cuda.graph replays; after load_state_dict with perturbed weights the SAME graph gives the unoptimised module's
    result on the new weights (1e-4 max|want|): the hook re-folds and re-packs into the same storage (buffer pointers unchanged, the packed stem among
    them)."""
    from hdn_amd import backbone as BB
    PS, model = _model(dev)
    x = torch.randn(1, 3, 127, 127, device=dev) * 60 + 110
    with torch.no_grad():
        want0 = _all(model, x)
        BB.optimize_similarity_model(model, strict=True, hip=2)
        parts = (model.backbone, model.neck, model.neck_lp)
        ptrs = [[(n, b.data_ptr()) for n, b in vars(p)["_hdn_fused"].named_buffers()] for p in parts]
        assert any(n == "stem_packed" for n, _ in ptrs[0]) and any("layers.1.0.c2.packed" in n for n, _ in ptrs[0]) and any("packed" in n for n, _ in ptrs[1])
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


def test_device_tracker_homo_with_the_full_hip_backbone(dev, monkeypatch):
    """DeviceTrackerHomo around the production stand-in with HDN_HIP_BACKBONE=2 (the tracker calls optimize_similarity_model itself: it follows the
    variable) against the CPU loop, the sequence and bounds of the level-1 test: first frame 1e-3 px, any of the first 6 frames 0.1 px."""
    from synth_sequence import make_sequence, success_4pts_error
    from test_gpu_tracker import _production_pair
    from hdn_amd import backbone as BB
    from hdn_amd.tracker import DeviceTrackerHomo
    frames, corners, init = make_sequence(n_frames=13, frame_hw=(720, 1280), target_wh=(300, 200), seed=20260928)
    frames = frames[:7]
    ref, model = _production_pair(dev, frames, init)
    monkeypatch.setenv("HDN_HIP_BACKBONE", "2")
    trk = DeviceTrackerHomo(model)
    assert trk.folded == ["backbone", "neck", "neck_lp"] and type(vars(model.backbone)["_hdn_fused"]) is BB.HipAtrousResNetFull
    assert vars(model.backbone)["_hdn_fused"].fused_stem
    ref.init(frames[0], init["bbox"], init["poly"], init["gt_points"], init["first_point"])
    trk.init(frames[0], init["bbox"], init["poly"], init["gt_points"], init["first_point"])
    errs = []
    for t in range(1, len(frames)):
        a, b = trk.track_new(t, frames[t]), ref.track_new(t, frames[t])
        errs.append(success_4pts_error(a["points"], b["points"]))
    print("DeviceTrackerHomo with HDN_HIP_BACKBONE=2, corner error vs CPU loop (px):", " ".join(f"{e:.1e}" for e in errs))
    assert errs[0] <= 1e-3, errs
    assert max(errs) <= 0.1, errs
    BB.restore_similarity_model(model)
