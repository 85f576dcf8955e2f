"""CPU tests of hdn_amd._loop, the host-side code the four tracker modules share: the environment switches, MIOpen find mode, the look-up of the
reference's configuration, frame_capacity, what the frame uploaders refuse before the first CUDA call, the result builders, and the geometry /
const-row functions of hdn_amd.tracker against the arithmetic HomoTracker.init used to spell out, and the class structure of the trackers (one
frame body per kind, find mode entered by the base classes).  No kernel is launched here."""
import sys
import types

import numpy as np
import pytest
import torch

from hdn_amd import _loop as LP


@pytest.mark.parametrize("value,want1,want0", [(None, True, False), ("", False, False), ("0", False, False), ("1", True, True)])
def test_env_flag(monkeypatch, value, want1, want0):
    if value is None:
        monkeypatch.delenv("HDN_LOOP_TEST_FLAG", raising=False)
    else:
        monkeypatch.setenv("HDN_LOOP_TEST_FLAG", value)
    assert LP.env_flag("HDN_LOOP_TEST_FLAG") is want1 and LP.env_flag("HDN_LOOP_TEST_FLAG", "1") is want1
    assert LP.env_flag("HDN_LOOP_TEST_FLAG", "0") is want0


def test_hip_trunk_switch_defaults_to_off(monkeypatch):
    from hdn_amd.tracker import hip_trunk_enabled
    monkeypatch.delenv("HDN_HIP_TRUNK", raising=False)
    assert hip_trunk_enabled() is False
    monkeypatch.setenv("HDN_HIP_TRUNK", "1")
    assert hip_trunk_enabled() is True


def test_find_mode_touches_benchmark_only_and_puts_it_back(monkeypatch):
    cudnn = torch.backends.cudnn
    monkeypatch.setattr(cudnn, "deterministic", True)       # (not torch's defaults: cudnn.flags() would reset both)
    monkeypatch.setattr(cudnn, "allow_tf32", False)
    for before in (False, True):
        monkeypatch.setattr(cudnn, "benchmark", before)
        with LP.find_mode(True):
            assert cudnn.benchmark is True and cudnn.deterministic is True and cudnn.allow_tf32 is False
        assert cudnn.benchmark is before
        with pytest.raises(KeyError):
            with LP.find_mode(True):
                raise KeyError("the body raises")
        assert cudnn.benchmark is before and cudnn.deterministic is True and cudnn.allow_tf32 is False
        with LP.find_mode(False):
            assert cudnn.benchmark is before
        assert cudnn.benchmark is before


def test_reference_config_without_and_with_the_reference(monkeypatch):
    from hdn_amd.similarity import TrackerConfig
    for name in ("hdn", "hdn.core", "hdn.core.config"):
        monkeypatch.setitem(sys.modules, name, None)        # (import hdn... raises ImportError)
    cfg, ref = LP.reference_config()
    assert cfg == TrackerConfig() and ref is None
    NS = types.SimpleNamespace
    node = NS(TRACK=NS(EXEMPLAR_SIZE=127, INSTANCE_SIZE=303, BASE_SIZE=8, CONTEXT_AMOUNT=0.5, WINDOW_INFLUENCE=0.4),      # no SCALE_SCORE_THRESH
              POINT=NS(STRIDE=8, STRIDE_LP=8), TRAIN=NS(OUTPUT_SIZE_LP=13), BAN=NS(KWARGS=NS(cls_out_channels=1)))
    mods = {"hdn": types.ModuleType("hdn"), "hdn.core": types.ModuleType("hdn.core"), "hdn.core.config": types.ModuleType("hdn.core.config")}
    mods["hdn"].core, mods["hdn.core"].config, mods["hdn.core.config"].cfg = mods["hdn.core"], mods["hdn.core.config"], node
    for name, m in mods.items():
        monkeypatch.setitem(sys.modules, name, m)
    cfg, ref = LP.reference_config()
    assert ref is node and cfg.instance_size == 303 and cfg.cls_out_channels == 1 and cfg.window_influence == 0.4
    del node.POINT                                           # a node that lacks what TrackerConfig itself reads: the defaults, no exception
    cfg, ref = LP.reference_config()
    assert cfg == TrackerConfig() and ref is None


def test_validate_frame_capacity():
    for bad in ((0, 5), (5, 0), (-1, 640)):
        with pytest.raises(ValueError, match="frame_capacity must be"):
            LP.validate_frame_capacity(bad)
    assert LP.validate_frame_capacity((360.0, 640)) == (360, 640)
    assert LP.validate_frame_capacity(None) is None


def test_uploader_refuses_before_the_first_cuda_call():
    up, f = LP.FrameUploader(2), np.zeros((4, 6, 3), np.uint8)
    with pytest.raises(ValueError, match="advances 2 sequences per step, got 1 frames"):
        up([f], None)
    with pytest.raises(TypeError, match=r"expected uint8 \[H,W,C\] frames, got float32"):
        up([f.astype(np.float32), f], None)
    with pytest.raises(TypeError, match=r"expected uint8 \[H,W,C\] frames"):
        up([f[0], f[0]], None)                                                   # frames of the wrong rank
    with pytest.raises(ValueError, match=r"all frames of a step must be uint8 \(4, 6, 3\).*frame 1 is uint8 \(3, 6, 3\)"):
        up([f, f[:3]], None)
    with pytest.raises(ValueError, match="frame 1 is int16"):
        up([f, f.astype(np.int16)], None)
    with pytest.raises(TypeError, match=r"expected a uint8 \[2,H,W,C\] tensor of frames, got torch.uint8 \(2, 4, 6\)"):
        up(torch.zeros((2, 4, 6), dtype=torch.uint8), None)                      # a tensor of the wrong rank
    with pytest.raises(TypeError, match=r"tensor of frames, got torch.float32"):
        up(torch.zeros((2, 4, 6, 3)), None)
    with pytest.raises(TypeError, match=r"tensor of frames"):
        up(torch.zeros((3, 4, 6, 3), dtype=torch.uint8), None)                   # the wrong count
    assert up._staging is None and up._copy_done is None                         # nothing was allocated for a refused step
    if not torch.cuda.is_available():
        from hdn_amd._lib import HdnHipError
        for good in ([f, f], torch.zeros((2, 4, 6, 3), dtype=torch.uint8)):
            with pytest.raises(HdnHipError, match="no CPU fallback"):
                up(good, None)


def test_upload_arena_checks_the_list_and_the_slots_sizes():
    from hdn_amd import frame as FR
    arena = FR.FrameArena(2, 8, 8, 3, device="cpu")
    a, b = np.full((4, 6, 3), 7, np.uint8), np.full((8, 5, 3), 9, np.uint8)
    for bad in ([a], [a, b, a], torch.zeros((2, 4, 6, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="takes a list of 2 frames"):
            LP.upload_arena(arena, bad, same_size=False)
    assert LP.upload_arena(arena, [a, b], same_size=False) is arena and arena.size(0) == (4, 6) and arena.size(1) == (8, 5)
    with pytest.raises(ValueError, match=r"slot 1 runs a sequence of \(8, 5\) frames, got a frame of \(4, 6\)"):
        LP.upload_arena(arena, [a, a], same_size=True)
    LP.upload_arena(arena, [a + 1, b], same_size=True)
    assert int(arena.frame(0)[0, 0, 0]) == 8 and int(arena.frame(1)[0, 0, 0]) == 9


def test_result_builders_and_track_state_row():
    row = np.array([10, 20, 30, 18, 32, 44, 8, 40, 0.75], np.float32)             # corners (10,20) (30,18) (32,44) (8,40), best_score
    r = LP.homography_result(row, 4)
    assert set(r) == {"bbox_aligned", "best_score", "polygon", "points", "bbox"}
    assert r["points"].shape == (4, 2) and r["points"].dtype == np.float32 and r["polygon"] is r["points"] and r["points"][2, 1] == 44
    assert r["bbox"] == [8, 18, 24, 26] and r["bbox_aligned"] == r["bbox"] and r["best_score"] == np.float32(0.75)
    h = np.arange(20, dtype=np.float64) + 0.5
    s = LP.similarity_result(h)
    assert set(s) == {"bbox", "bbox_aligned", "best_score", "rot", "polygon"}
    assert s["bbox"] == [0.5, 1.5, 2.5, 3.5] and s["bbox_aligned"] == [4.5, 5.5, 6.5, 7.5] and s["rot"] == 9.5
    assert type(s["best_score"]) is np.float32 and s["best_score"] == 8.5
    assert s["polygon"].shape == (4, 2) and s["polygon"][0, 0] == 10.5 and s["polygon"][3, 1] == 17.5 and not np.shares_memory(s["polygon"], h)
    t = np.zeros(48)
    t[:14] = [100, 50, 30, 20, 0.25, -1.5, 1.1, 0.9, 1.05, 3, 1, 0, 1, 17]
    st = LP.track_state_row(t)
    assert st == {"center_pos": st["center_pos"], "size": st["size"], "rot": 0.25, "lp_shift": [0, -1.5], "scale": 1.1, "v": 0.9, "window_scale_factor": 1.05,
                  "lost_count": 3, "last_lost": True, "rot_is_float32": False, "lp_shift_is_float32": True, "frames": 17}
    assert list(st["center_pos"]) == [100, 50] and list(st["size"]) == [30, 20] and not np.shares_memory(st["center_pos"], t)
    assert type(st["lost_count"]) is int and type(st["last_lost"]) is bool and type(st["rot"]) is float


def test_geometry_and_const_row_are_what_homotracker_init_spelled_out():
    """hdn_amd.tracker._geometry / _const_row (shared by HomoTracker and BatchedHomoTracker) against the single tracker's former inline arithmetic
    (hdn_tracker_proj_e2e.py:66-84, :251-258), value for value: float32 matrices, float32 inverses, widened to float64."""
    from hdn_amd import frame as FR
    from hdn_amd.similarity import TrackerConfig
    from hdn_amd.tracker import TRACK_CONST_DOUBLES, _const_row, _geometry
    c, poly, gate = TrackerConfig(), [301.7, 215.2, 151.3, 97.9, 0.3], 2.5
    pos, size, s_z, s_z_sm = _geometry(poly, c)
    init_pos, sz = np.array([poly[0], poly[1]], np.float64), np.array([poly[2], poly[3]], np.float64)
    w_z, h_z = sz[0] + c.context_amount * np.sum(sz), sz[1] + c.context_amount * np.sum(sz)
    assert (pos == init_pos).all() and (size == sz).all() and pos.dtype == size.dtype == np.float64
    assert float(s_z) == float(np.floor(np.sqrt(w_z * h_z))) and float(s_z_sm) == float(np.floor(np.sqrt(sz[0] * sz[1])))
    zp = FR.crop_points(pos, float(s_z_sm), 360, 640)
    cw, ch, E = zp[2] - zp[0] + 1, zp[3] - zp[1] + 1, c.exemplar_size
    S = np.diag([E / cw, E / ch, 1.0]).astype(np.float32)
    Sh = np.array([[1, 0, -zp[0]], [0, 1, -zp[1]], [0, 0, 1]], np.float32)
    want = np.zeros(TRACK_CONST_DOUBLES, np.float64)
    want[0:9], want[9:18] = np.linalg.inv(S).astype(np.float64).reshape(-1), S.astype(np.float64).reshape(-1)
    want[18:27], want[27:36] = np.linalg.inv(Sh).astype(np.float64).reshape(-1), Sh.astype(np.float64).reshape(-1)
    want[36] = gate
    got = _const_row(zp, E, gate)
    assert got.dtype == np.float64 and got.shape == want.shape and (got == want).all()
    assert np.linalg.inv(S).dtype == np.float32                                   # (numpy's dtype rule: the inverses are float32 too)


def test_lockstep_trackers_inherit_the_frame_body_and_the_device_classes_are_constructors():
    """The lock-step classes run the single trackers' own frame body (function identity, not a copy kept in step by hand); MIOpen find mode is
    entered by the base classes, so the Device* classes define no init / track_new / reinit of their own; and the public constructors take what
    they took before the classes were put under one base."""
    import inspect
    from hdn_amd.batched_tracker import BatchedDeviceTracker, BatchedHomoTracker
    from hdn_amd.simi_tracker import BatchedSimiTracker, DeviceTrackerSimi, SimiTracker
    from hdn_amd.tracker import DeviceTrackerHomo, HomoTracker
    assert BatchedHomoTracker._body is HomoTracker._body and BatchedHomoTracker._capture is HomoTracker._capture
    assert BatchedSimiTracker._body is SimiTracker._body
    assert HomoTracker._per_sample is False and BatchedHomoTracker._per_sample is True        # sample 0's score / every sequence's own, at n = 1 too
    with pytest.raises(NotImplementedError, match="ONE sequence"):                             # (inherited by name only: it decodes one record)
        BatchedHomoTracker.similarity_state(None)
    for cls in (DeviceTrackerHomo, BatchedDeviceTracker, DeviceTrackerSimi):
        assert not {"init", "track_new", "reinit"} & set(vars(cls)), cls
    assert HomoTracker.miopen_find is False and SimiTracker.miopen_find is False
    want = {
        HomoTracker: "(self, hm_net, iterations=1, similarity=None, score_gate=2.5, graph=False, cfg=None)",
        BatchedHomoTracker: "(self, hm_net, n, iterations=1, similarity=None, score_gate=2.5, graph=False, cfg=None, frame_capacity=None)",
        DeviceTrackerHomo: "(self, model, graph=None, iterations=1, cfg=None, fold_backbone=None, hip_trunk=None)",
        BatchedDeviceTracker: "(self, model, n, graph=None, iterations=1, cfg=None, fold_backbone=None, hip_trunk=None, frame_capacity=None)",
        SimiTracker: "(self, model, cfg=None, graph=False, scale_score_thresh=0.5, batch_template=None)",
        BatchedSimiTracker: "(self, model, n, cfg=None, graph=False, scale_score_thresh=0.5, batch_template=None, frame_capacity=None)",
        DeviceTrackerSimi: "(self, model, graph=None, cfg=None, fold_backbone=None, batch_template=None)",
    }
    for cls, sig in want.items():
        params = inspect.signature(cls.__init__).parameters.values()
        assert "(" + ", ".join(p.name if p.default is p.empty else f"{p.name}={p.default!r}" for p in params) + ")" == sig, cls


def test_device_setup_fills_in_what_was_not_given(monkeypatch):
    """The Device* constructors' preamble: a cfg handed in is kept and the reference's node is not looked up; None reads it; graph None reads
    HDN_TRACKER_GRAPH; the model is put in eval mode."""
    from hdn_amd.similarity import TrackerConfig
    monkeypatch.setattr(LP, "reference_config", lambda: (TrackerConfig(instance_size=303), "node"))
    monkeypatch.setenv("HDN_FOLD_BACKBONE", "0")
    model = torch.nn.Conv2d(1, 1, 1).train()
    mine = TrackerConfig(instance_size=271)
    monkeypatch.setenv("HDN_TRACKER_GRAPH", "0")
    assert LP.device_setup(model, mine, None, None) == (mine, None, False, False, []) and not model.training
    assert LP.device_setup(model, mine, True, False)[:3] == (mine, None, True)
    monkeypatch.delenv("HDN_TRACKER_GRAPH")
    cfg, ref, graph, find, folded = LP.device_setup(model, None, None, False)
    assert cfg.instance_size == 303 and ref == "node" and graph is True and find is False and folded == []


def test_step_enters_find_mode_around_the_capture_and_the_body(monkeypatch):
    """The shared step of either tracker kind raises cudnn.benchmark (when miopen_find is set, as the Device* constructors do) around the graph
    capture AND the frame body, puts it back, and goes on eagerly after a refused capture; with the class default nothing is touched."""
    from hdn_amd.simi_tracker import SimiTracker
    from hdn_amd.tracker import HomoTracker
    cudnn, seen = torch.backends.cudnn, []
    monkeypatch.setattr(cudnn, "benchmark", False)
    for base, rest, out in ((HomoTracker, (True,), (torch.zeros(1, 9), torch.zeros(()))), (SimiTracker, ((4, 6, 3),), torch.zeros(1, 20))):
        class Fake(base):
            def __init__(self):
                self.use_graph, self._graph = True, None

            def _capture(self, *_):
                seen.append(("capture", cudnn.benchmark))
                self.use_graph = False                       # (what a refused stream capture leaves behind)

            def _frames(self, imgs, into=None):
                return imgs

            def _body(self, frames):
                seen.append(("body", frames, cudnn.benchmark))
                return out
        for find in (True, False):
            t = Fake()
            if find:
                t.miopen_find = True
            t._step("frame", *rest)
            assert seen == [("capture", find), ("body", "frame", find)] and cudnn.benchmark is False and t.use_graph is False, (base, find)
            seen.clear()
