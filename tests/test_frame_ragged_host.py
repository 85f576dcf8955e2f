"""CPU tests of the ragged frame kernels' host side and of the video scheduler (tests/test_gpu_frame_ragged.py and tests/test_gpu_tracker_stream.py run
them on the device): the three new exports, every error code that returns before a launch (made-up addresses: nothing is launched or read),
FrameArena's capacity check, and track_videos over a recording fake tracker.  No kernel is launched here."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_LIMIT, E_ALIAS = -1, -2, -3, -4
NAMES = ("hdn_subwindow_ragged_f32", "hdn_frame_warp_perspective_ragged_u8", "hdn_frame_warp_affine_cubic_ragged_u8")


def _lib():
    from hdn_amd import _lib as L
    return L.load()


def test_ragged_symbols_are_in_the_library_the_header_and_the_binding_and_the_abi_is_still_10():
    from hdn_amd import _lib as L
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "hdn_hip.h")).read()
    for name in NAMES:
        assert getattr(lib, name) is not None, name
        assert name in L.SIGNATURES and ("int " + name + "(") in header, name
    assert lib.hdn_abi_version() == 10 and L.ABI_VERSION == 10


def test_ragged_warps_refuse_bad_arguments_before_any_launch():
    lib = _lib()
    src, dims, M, dst = (ctypes.c_void_p(v << 34) for v in (1, 2, 3, 4))
    B, Hm, Wm, C = 6, 48, 160, 3
    stride = Hm * Wm * C
    for name, width in (("hdn_frame_warp_perspective_ragged_u8", 9), ("hdn_frame_warp_affine_cubic_ragged_u8", 6)):
        run = getattr(lib, name)
        for args in ((None, stride, dims, M, width, dst), (src, stride, None, M, width, dst), (src, stride, dims, None, width, dst),
                     (src, stride, dims, M, width, None)):
            assert run(*args, B, Hm, Wm, C, None) == E_NULL, name
        for shape in ((0, Hm, Wm, C), (B, 0, Wm, C), (B, Hm, 0, C), (B, Hm, Wm, 0)):
            assert run(src, stride, dims, M, width, dst, *shape, None) == E_SHAPE, (name, shape)
        assert run(src, stride, dims, M, width - 1, dst, B, Hm, Wm, C, None) == E_SHAPE                 # the records overlap
        assert run(src, stride - 1, dims, M, width, dst, B, Hm, Wm, C, None) == E_SHAPE                 # one byte short of the capacity
        assert run(src, stride, dims, M, width, dst, B, Hm, Wm, 5, None) == E_LIMIT
        assert run(src, 1 << 40, dims, M, width, dst, B, 1 << 15, (1 << 15) + 1, C, None) == E_LIMIT
        assert run(src, stride, dims, M, width, dst, 65536, Hm, Wm, C, None) == E_LIMIT
        # alias, over WHOLE arenas: the same arena, and an output that begins inside the input's last slot
        assert run(src, stride, dims, M, width, src, B, Hm, Wm, C, None) == E_ALIAS
        assert run(src, stride, dims, M, width, ctypes.c_void_p((1 << 34) + B * stride - 1), B, Hm, Wm, C, None) == E_ALIAS
        assert run(ctypes.c_void_p((4 << 34) + B * (stride + 7) - 1), stride + 7, dims, M, width, dst, B, Hm, Wm, C, None) == E_ALIAS


def test_ragged_subwindow_refuses_bad_arguments_before_any_launch():
    lib = _lib()
    run = lib.hdn_subwindow_ragged_f32
    fr, dims, par, out = (ctypes.c_void_p(v << 34) for v in (1, 2, 3, 4))
    B, Hm, Wm, C = 6, 48, 160, 3
    stride = Hm * Wm * C
    for args in ((None, stride, dims, par, 6, out), (fr, stride, None, par, 6, out), (fr, stride, dims, None, 6, out), (fr, stride, dims, par, 6, None)):
        assert run(*args, B, Hm, Wm, C, 127, 0, None) == E_NULL
    for tail in ((0, Hm, Wm, C, 127, 0), (B, 0, Wm, C, 127, 0), (B, Hm, 0, C, 127, 0), (B, Hm, Wm, 0, 127, 0), (B, Hm, Wm, C, 0, 0),
                 (B, Hm, Wm, C, 127, 2), (B, Hm, Wm, 4, 127, 1)):
        assert run(fr, 1 << 20, dims, par, 8, out, *tail, None) == E_SHAPE, tail
    assert run(fr, stride, dims, par, 5, out, B, Hm, Wm, C, 127, 0, None) == E_SHAPE                    # params_stride < 3 + C
    assert run(fr, stride - 1, dims, par, 6, out, B, Hm, Wm, C, 127, 0, None) == E_SHAPE                # one byte short of the capacity
    assert run(fr, stride, dims, par, 8, out, B, Hm, Wm, 5, 127, 0, None) == E_LIMIT
    assert run(fr, stride, dims, par, 6, out, B, Hm, Wm, C, 4097, 0, None) == E_LIMIT
    assert run(fr, 1 << 40, dims, par, 6, out, B, 1 << 15, (1 << 15) + 1, C, 127, 0, None) == E_LIMIT
    assert run(fr, stride, dims, par, 6, out, 65536, Hm, Wm, C, 127, 0, None) == E_LIMIT
    assert run(fr, stride, dims, par, 6, ctypes.c_void_p((1 << 34) + B * stride - 4), B, Hm, Wm, C, 127, 0, None) == E_ALIAS


def test_frame_arena_refuses_a_frame_above_capacity_before_touching_dims():
    """(A host arena: same bookkeeping, no kernel takes it.)"""
    from hdn_amd import _lib as L
    from hdn_amd import frame as FR
    a = FR.FrameArena(3, 48, 160, device="cpu")
    assert a.slot_stride == 48 * 160 * 3 and tuple(a.dims.shape) == (3, 2) and a.dims.dtype == torch.int32 and not a.dims.any()
    g = np.random.default_rng(0)
    f0, f1 = g.integers(0, 256, (9, 70, 3), dtype=np.uint8), g.integers(0, 256, (48, 160, 3), dtype=np.uint8)
    a.set(0, f0)
    a.set(1, f1)
    assert a.dims.tolist() == [[9, 70], [48, 160], [0, 0]] and a.size(0) == (9, 70)
    assert np.array_equal(a.frame(0).numpy(), f0) and np.array_equal(a.frame(1).numpy(), f1)
    before, data = a.dims.clone(), a.data.clone()
    for bad in (np.zeros((49, 160, 3), np.uint8), np.zeros((48, 161, 3), np.uint8), np.zeros((9, 70, 4), np.uint8), np.zeros((0, 70, 3), np.uint8)):
        with pytest.raises(ValueError):
            a.set(0, bad)
        with pytest.raises(ValueError):          # set_all checks every frame before it writes the first
            a.set_all([f1, f0, bad])
    with pytest.raises(TypeError):
        a.set(0, np.zeros((9, 70, 3), np.float32))
    with pytest.raises(ValueError):
        a.set_all([f0, f1])
    assert torch.equal(a.dims, before) and torch.equal(a.data, data) and a.size(0) == (9, 70)
    with pytest.raises(ValueError):
        a.frame(2)                               # an empty slot
    b = a.like()
    assert b.dims is a.dims and (b.n, b.Hmax, b.Wmax, b.C, b.slot_stride) == (a.n, a.Hmax, a.Wmax, a.C, a.slot_stride) and b.data is not a.data
    a.set(0, f1)                                 # a slot changes its size: the arena made by like() sees it
    assert b.size(0) == (48, 160) and tuple(b.frame(0).shape) == (48, 160, 3)
    with pytest.raises(L.HdnHipError):           # no CPU fallback
        FR.warp_perspective(a, np.tile(np.eye(3).reshape(-1), 3))


class _FakeTracker:
    """Records what track_videos does with the tracker's three methods; a frame is np.uint8 [2, 2, 3] filled with (video, index, 0)."""

    def __init__(self, n, frame_capacity=None):
        self.n, self.frame_capacity = n, frame_capacity
        self.host_syncs = 0
        self.calls, self.slot_video = [], [None] * n
        self.fed = {}                  # video -> list of (frame index, slot)

    @staticmethod
    def _id(img):
        return int(img[0, 0, 0]), int(img[0, 0, 1])

    def _start(self, slot, img, init):
        v, i = self._id(img)
        assert i == 0 and init == v
        self.slot_video[slot] = v
        self.fed.setdefault(v, []).append((0, slot))

    def init(self, imgs, bboxes, polys, gt_points, first_points=None):
        assert len(imgs) == len(bboxes) == len(polys) == len(gt_points) == len(first_points) == self.n
        assert bboxes == polys == gt_points == first_points
        self.calls.append(("init", [self._id(im)[0] for im in imgs]))
        self.host_syncs += 1
        for b, im in enumerate(imgs):
            self._start(b, im, bboxes[b])

    def reinit(self, slot, img, bbox, poly, gt_points, first_point=None):
        assert bbox == poly == gt_points == first_point
        self.calls.append(("reinit", slot, self._id(img)[0]))
        self.host_syncs += 1
        self._start(slot, img, bbox)

    def track_new(self, fr_idx, imgs, sync=True):
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


def test_track_videos_schedules_five_videos_through_two_slots():
    import hdn_amd
    from hdn_amd.batched_tracker import track_videos
    assert hdn_amd.track_videos is track_videos
    lengths = [4, 7, 3, 6, 5]
    t = _FakeTracker(2)
    res = track_videos(t, _videos(lengths))
    # results: input order, one per frame after the first, that video's frames in order
    assert [len(r) for r in res] == [T - 1 for T in lengths]
    for v, r in enumerate(res):
        assert [(d["video"], d["frame"]) for d in r] == [(v, i) for i in range(1, lengths[v])]
    # every frame of every video was fed exactly once, in order, to ONE slot - leaving out the idle re-feeds of a video's last frame
    steps = [c for c in t.calls if c[0] == "step"]
    for v, T in enumerate(lengths):
        seen, slots = [i for i, _ in t.fed[v]], {b for _, b in t.fed[v]}
        assert len(slots) == 1, (v, slots)
        assert seen[:T] == list(range(T)) and all(i == T - 1 for i in seen[T:]), (v, seen)
    # re-inits: exactly 3, videos 2, 3, 4 in that order, each into the slot whose video had just ended
    assert [c for c in t.calls if c[0] == "reinit"] == [("reinit", 0, 2), ("reinit", 0, 3), ("reinit", 1, 4)]
    assert t.calls[0] == ("init", [0, 1])
    # slot 0: 3 + 2 + 5 steps, slot 1: 6 + 4 steps
    assert len(steps) == 10 and steps[-1][1] == [(3, 5), (4, 4)] and steps[3][1] == [(2, 1), (1, 4)]
    assert t.host_syncs == 1 + len(steps) + 3
    # an idle slot (queue empty, the other still running) is fed its last frame again and its result is dropped: slot 0 after 3 + 2 steps of 6
    t3 = _FakeTracker(2)
    res3 = track_videos(t3, _videos(lengths[:3]))
    steps3 = [c[1] for c in t3.calls if c[0] == "step"]
    assert len(steps3) == 6 and steps3[4] == [(2, 2), (1, 5)] and steps3[5] == [(2, 2), (1, 6)]
    assert [len(r) for r in res3] == [3, 6, 2] and [d["frame"] for d in res3[2]] == [1, 2]
    # the callback form
    got, t2 = [], _FakeTracker(2)
    res2 = track_videos(t2, _videos(lengths), on_result=lambda v, i, r: got.append((v, i, r["video"], r["frame"])))
    assert res2 == [[] for _ in lengths] and t2.calls == t.calls
    assert sorted(got) == [(v, i, v, i) for v, T in enumerate(lengths) for i in range(1, T)]


def test_track_videos_with_no_video_fewer_videos_than_slots_and_a_video_above_capacity():
    from hdn_amd.batched_tracker import track_videos
    t = _FakeTracker(2)
    assert track_videos(t, []) == [] and t.calls == []
    t = _FakeTracker(3)
    res = track_videos(t, _videos([3, 2]))
    assert [len(r) for r in res] == [2, 1]
    assert t.calls[0] == ("init", [0, 1, 1])                      # the spare slot runs a copy of the last video; its results are dropped
    assert [c[1] for c in t.calls if c[0] == "step"] == [[(0, 1), (1, 1), (1, 0)], [(0, 2), (1, 1), (1, 0)]]
    assert not [c for c in t.calls if c[0] == "reinit"]
    t = _FakeTracker(1)                                           # a one-frame video yields an empty list and costs no step
    res = track_videos(t, _videos([1, 3]))
    assert [len(r) for r in res] == [0, 2] and t.calls == [("init", [0]), ("reinit", 0, 1), ("step", [(1, 1)]), ("step", [(1, 2)])]
    t = _FakeTracker(2, frame_capacity=(4, 4))
    vids = _videos([3, 3]) + _videos([2], hw=(5, 4))
    with pytest.raises(ValueError):
        track_videos(t, vids)
    assert t.calls == []                                          # before anything was launched
