"""CPU tests of the similarity-only tracker's slots (tests/test_gpu_simi_update_ragged.py and tests/test_gpu_simi_tracker_stream.py run them on the
device): the export hdn_simi_track_update_ragged_f64, every error code it returns before a launch (made-up addresses: nothing is launched or
read), BatchedSimiTracker's frame_capacity / reinit preconditions, and track_videos over a recording fake whose init takes hdnTracker's
signature (init(imgs, bboxes, polys, gt_points, first_points)).  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE = -1, -2
NAME = "hdn_simi_track_update_ragged_f64"
ARGS = ("const double* state, double* tr, double* seq, double* out, const int* dims, int B, int Hmax, int Wmax, double scale_score_thresh, "
        "double context_amount, double instance_exemplar_ratio, void* stream")


def _lib():
    from hdn_amd import _lib as L
    return L.load()


def test_symbol_is_in_the_library_the_header_and_the_binding_and_the_abi_is_still_10():
    from hdn_amd import _lib as L
    lib = _lib()
    assert getattr(lib, NAME) is not None
    header = open(os.path.join(ROOT, "include", "hdn_hip.h")).read()
    m = re.search(r"int " + NAME + r"\(([^;]*)\);", header)
    assert m is not None, "not declared in include/hdn_hip.h"
    assert " ".join(m.group(1).split()) == ARGS
    restype, argtypes = L.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == 12
    assert argtypes[5:8] == [ctypes.c_int] * 3 and argtypes[8:11] == [ctypes.c_double] * 3 and argtypes[11] is ctypes.c_void_p
    assert lib.hdn_abi_version() == 10 and L.ABI_VERSION == 10
    assert "#define HDN_ABI_VERSION 10" in header


def test_ragged_update_refuses_bad_arguments_before_any_launch():
    run = _lib().hdn_simi_track_update_ragged_f64
    ptrs = [ctypes.c_void_p(v << 34) for v in (1, 2, 3, 4, 5)]        # state, tr, seq, out, dims
    B, Hm, Wm = 6, 360, 640
    for k in range(5):                                               # each null pointer, dims included
        args = list(ptrs)
        args[k] = None
        assert run(*args, B, Hm, Wm, 0.5, 0.5, 2.0, None) == E_NULL, k
    for shape in ((0, Hm, Wm), (-1, Hm, Wm), (B, 0, Wm), (B, Hm, 0), (B, -3, Wm), (B, Hm, -3)):
        assert run(*ptrs, *shape, 0.5, 0.5, 2.0, None) == E_SHAPE, shape
    for ratio in (0.0, -2.0, float("nan")):                          # "not > 0"
        assert run(*ptrs, B, Hm, Wm, 0.5, 0.5, ratio, None) == E_SHAPE, ratio
    assert run(None, *ptrs[1:], 0, Hm, Wm, 0.5, 0.5, 2.0, None) == E_NULL          # null before shape, as the existing entry
    # the existing entry answers the same for what they share
    old = _lib().hdn_simi_track_update_f64
    assert old(*ptrs[:4], 0, Wm, Hm, 0.5, 0.5, 2.0, None) == E_SHAPE and old(*ptrs[:4], B, Wm, Hm, 0.5, 0.5, 0.0, None) == E_SHAPE
    assert old(ptrs[0], None, *ptrs[2:4], B, Wm, Hm, 0.5, 0.5, 2.0, None) == E_NULL


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))


def test_batched_simi_tracker_frame_capacity_and_reinit_preconditions():
    from hdn_amd.simi_tracker import BatchedSimiTracker
    net = _Net()
    for bad in ((0, 5), (5, 0), (-1, 640)):
        with pytest.raises(ValueError):
            BatchedSimiTracker(net, 2, frame_capacity=bad)
    t = BatchedSimiTracker(net, 2, frame_capacity=(360.0, 640))
    assert t.frame_capacity == (360, 640) and t._arena is None
    assert BatchedSimiTracker(net, 2).frame_capacity is None
    img, poly = np.zeros((8, 8, 3), np.uint8), [4, 4, 3, 2, 0.0]
    with pytest.raises(RuntimeError):                  # arena mode, but no init() yet
        t.reinit(0, img, [2, 3, 3, 2], poly, None, (2.5, 3.0))
    with pytest.raises(RuntimeError):                  # no arena mode
        BatchedSimiTracker(net, 2).reinit(0, img, [2, 3, 3, 2], poly, None, (2.5, 3.0))
    with pytest.raises(ValueError, match="slot 1"):    # a first_point of None: refused before anything is built
        t.init([img, img], [[2, 3, 3, 2]] * 2, [poly] * 2, [None, None], [(2.5, 3.0), None])
    assert t._arena is None and t.host_syncs == 0


class _FakeSimiTracker:
    """Records what track_videos does with the tracker's three methods; init takes hdnTracker's arguments (imgs, bboxes, polys, *rest with
    first_points last), as BatchedSimiTracker.init does.  A frame is np.uint8 [2, 2, 3] filled with (video, index, 0)."""

    def __init__(self, n, frame_capacity=None):
        self.n, self.frame_capacity = n, frame_capacity
        self.host_syncs = 0
        self.calls, self.slot_video, self.fed = [], [None] * n, {}

    @staticmethod
    def _id(img):
        return int(img[0, 0, 0]), int(img[0, 0, 1])

    def _start(self, slot, img, init):
        v, i = self._id(img)
        assert i == 0 and init == v
        self.slot_video[slot] = v
        self.fed.setdefault(v, []).append((0, slot))

    def init(self, imgs, bboxes, polys, *rest):
        assert rest, "first_points are required"
        first_points = rest[-1]
        assert len(imgs) == len(bboxes) == len(polys) == len(first_points) == self.n and all(fp is not None for fp in first_points)
        assert len(rest) == 2 and rest[0] == bboxes == polys == first_points       # (gt_points in front, the launchers' spelling)
        self.calls.append(("init", [self._id(im)[0] for im in imgs]))
        self.host_syncs += 1
        for b, im in enumerate(imgs):
            self._start(b, im, bboxes[b])

    def reinit(self, slot, img, bbox, poly, gt_points, first_point=None):
        assert first_point is not None and bbox == poly == gt_points == first_point
        self.calls.append(("reinit", slot, self._id(img)[0]))
        self.host_syncs += 1
        self._start(slot, img, bbox)

    def track_new(self, fr_idx, imgs, gt_box=None, gt_poly=None, gt_points=None, sync=True):
        assert len(imgs) == self.n
        ids = [self._id(im) for im in imgs]
        self.calls.append(("step", ids))
        self.host_syncs += 1
        for b, (v, i) in enumerate(ids):
            assert v == self.slot_video[b], "a slot is fed the frames of the video it was (re-)initialised with"
            self.fed.setdefault(v, []).append((i, b))
        return [{"video": v, "frame": i, "slot": b} for b, (v, i) in enumerate(ids)]


def _videos(lengths, hw=(2, 2)):
    def frames(v, T):
        for i in range(T):
            f = np.zeros(hw + (3,), np.uint8)
            f[..., 0], f[..., 1] = v, i
            yield f
    return [(frames(v, T), {"bbox": v, "poly": v, "gt_points": v, "first_point": v}) for v, T in enumerate(lengths)]


def test_track_videos_drives_a_tracker_with_the_simi_signature():
    from hdn_amd import track_videos
    lengths = [4, 7, 3, 6, 5]
    t = _FakeSimiTracker(2, frame_capacity=(4, 4))
    res = track_videos(t, _videos(lengths))
    assert [len(r) for r in res] == [T - 1 for T in lengths]
    for v, r in enumerate(res):                                      # input order, that video's frames in order
        assert [(d["video"], d["frame"]) for d in r] == [(v, i) for i in range(1, lengths[v])]
    for v, T in enumerate(lengths):                                  # every frame once, in order, to ONE slot (then idle re-feeds of the last one)
        seen, slots = [i for i, _ in t.fed[v]], {b for _, b in t.fed[v]}
        assert len(slots) == 1, (v, slots)
        assert seen[:T] == list(range(T)) and all(i == T - 1 for i in seen[T:]), (v, seen)
    assert t.calls[0] == ("init", [0, 1])
    assert [c for c in t.calls if c[0] == "reinit"] == [("reinit", 0, 2), ("reinit", 0, 3), ("reinit", 1, 4)]
    assert len([c for c in t.calls if c[0] == "step"]) == 10 and t.host_syncs == 10 + 3 + 1
    # BatchedSimiTracker offers what the driver talks to
    from hdn_amd.simi_tracker import BatchedSimiTracker
    bt = BatchedSimiTracker(_Net(), 2, frame_capacity=(4, 4))
    assert bt.n == 2 and bt.frame_capacity == (4, 4) and all(callable(getattr(bt, name)) for name in ("init", "track_new", "reinit"))
    with pytest.raises(ValueError, match="video 2"):                 # above the capacity: refused by the driver, before init
        track_videos(bt, _videos([3, 3]) + _videos([2], hw=(5, 4)))
    assert bt._arena is None and bt.host_syncs == 0
