"""Videos of different sizes and lengths streamed through the slots of the similarity-only tracker (hdn_amd.simi_tracker.BatchedSimiTracker in arena
mode: frame_capacity, reinit, track_videos) - TRACKS['hdnTracker'], the reference's default cfg.TRACK.TYPE, whose users split a dataset by hand
across processes (tools/test.py:91-103).

Every sequence is held to its own B = 1 run through SimiTracker (no arena: the frame size a launch argument) and to the CPU restatement of the loop
(oracle.tracker_oracle.SimiTrackerOracle), with the bounds of tests/test_gpu_simi_tracker.py::test_batched_simi_tracker_equals_single_runs_and_cpu_loop
for eager and graph alike: the polygon within 2e-3 px on the first three frames after a (re-)init and 5e-2 px after, rot within 2e-4 of the B = 1
run.  The B = 1 runs are computed on a copy of the model (they reassign model.zf)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = [(360, 640), (300, 480), (270, 400)]
TARGETS = [(150, 100), (120, 90), (100, 130)]
CAPACITY = (360, 640)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class _World:
    """The stand-in model, the synthetic sequences, their B = 1 device runs and their CPU loops, each computed once."""

    def __init__(self, dev):
        from test_gpu_simi_tracker import _standin
        self.dev = dev
        self.twin, self.cpu, self.cfg = _standin(dev, loc_scale_lp=0.3)
        self.twin_single = copy.deepcopy(self.twin)         # the B = 1 runs' own model: they reassign zf / zf_lp
        self._seqs, self._single, self._cpu = {}, {}, {}

    def seq(self, size, target, seed, T):
        from synth_sequence import make_sequence
        key = (size, target, seed, T)
        if key not in self._seqs:
            self._seqs[key] = make_sequence(n_frames=T, frame_hw=SIZES[size], target_wh=TARGETS[target], seed=seed)
        return key, self._seqs[key]

    def single(self, key, cpu=True):
        """(B = 1 device results, CPU loop results) of the sequence, frames 1 .. T - 1 (cpu=False: the device run alone, None for the other)."""
        from hdn_amd.simi_tracker import SimiTracker
        from oracle.tracker_oracle import SimiTrackerOracle
        if key not in self._single:
            frames, _, init = self._seqs[key]
            fp = np.array([init["first_point"]])
            t = SimiTracker(self.twin_single, cfg=self.cfg)
            t.init(frames[0], init["bbox"], init["poly"], fp)
            self._single[key] = [t.track_new(i, frames[i]) for i in range(1, len(frames))]
            self._cpu[key] = [None] * (len(frames) - 1)
            if cpu:
                r = SimiTrackerOracle(self.cpu)
                r.init(frames[0], init["bbox"], init["poly"], fp)
                self._cpu[key] = [r.track_new(i, frames[i]) for i in range(1, len(frames))]
        return self._single[key], self._cpu[key]

    def tracker(self, n, graph, capacity=CAPACITY):
        from hdn_amd.simi_tracker import BatchedSimiTracker
        return BatchedSimiTracker(self.twin, n, cfg=self.cfg, graph=graph, frame_capacity=capacity)


@pytest.fixture(scope="module")
def world(dev):
    return _World(dev)


def _init_args(seqs):
    return ([s[0][0] for s in seqs], [s[2]["bbox"] for s in seqs], [s[2]["poly"] for s in seqs], [s[2]["gt_points"] for s in seqs],
            [s[2]["first_point"] for s in seqs])


def _check(res, ref, k, where, worst):
    """k: frames since the sequence's (re-)init, 0 = the first tracked frame; ref = (B = 1 result, CPU loop result)."""
    single, cpu = ref
    ds = float(np.max(np.abs(res["polygon"] - single["polygon"])))
    dc = float(np.max(np.abs(res["polygon"] - cpu["polygon"]))) if cpu is not None else 0.0
    dr = abs(float(res["rot"]) - float(single["rot"]))
    worst[0], worst[1], worst[2] = max(worst[0], ds), max(worst[1], dc), max(worst[2], dr)
    bound = 2e-3 if k < 3 else 5e-2
    assert ds <= bound and dc <= bound, (where, k, ds, dc)
    assert dr <= 2e-4, (where, k, dr)


def _report(what, graph, worst):
    print(f"{what} ({'hipGraph' if graph else 'eager'}): worst polygon distance {worst[0]:.2e} px to the B=1 runs, {worst[1]:.2e} px to the CPU loop; "
          f"rot {worst[2]:.1e}")


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_mixed_frame_sizes_in_one_batch(world, graph):
    """(a) n = 3, one sequence per frame size, 5 steps: every sequence within the bounds; one host read per step."""
    T = 6
    keys, seqs = zip(*[world.seq(b, b, 80 + b, 10) for b in range(3)])
    refs = [world.single(k) for k in keys]
    bt = world.tracker(3, graph)
    bt.init(*_init_args(seqs))
    assert [bt._arena.size(b) for b in range(3)] == SIZES and bt.frame_hw == SIZES
    assert [int(z.shape[0]) for z in world.twin.zf] == [3] * len(world.twin.zf)
    s0, worst = bt.host_syncs, [0.0, 0.0, 0.0]
    for i in range(1, T):
        res = bt.track_new(i, [s[0][i] for s in seqs])
        assert len(res) == 3 and set(res[0]) == {"bbox", "bbox_aligned", "best_score", "rot", "polygon"}
        for b in range(3):
            _check(res[b], (refs[b][0][i - 1], refs[b][1][i - 1]), i - 1, ("a", b), worst)
    assert bt.host_syncs - s0 == T - 1
    assert (bt._graph is not None) == graph
    _report("mixed sizes (n=3)", graph, worst)
    with pytest.raises(ValueError, match="slot 1"):          # a running slot keeps its frame size
        bt.track_new(99, [seqs[0][0][1], seqs[0][0][1], seqs[2][0][1]])
    with pytest.raises(ValueError):
        bt.track_new(99, [seqs[0][0][1]] * 2)


def _rows(bt, twin):
    """The per-sequence tensors a re-init writes: name -> (tensor, clone), the sequence along dim 0."""
    out = {"track": bt.track, "seq": bt.seq, "state": bt.state}
    for name in ("zf", "zf_lp"):
        z = getattr(twin, name)
        for l, t in enumerate(z if isinstance(z, (list, tuple)) else [z]):
            out[f"{name}[{l}]"] = t
    return {k: (v, v.clone()) for k, v in out.items()}


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_reinit_one_slot_mid_run(world, graph):
    """(b) n = 3, 9 steps; after step 4 slot 1 is handed a new sequence of another size and another texture.  Slots 0 and 2 stay within the bounds
    of their uninterrupted runs, slot 1 from step 5 on within those of a fresh B = 1 run of the new sequence.  The re-init touches row 1 only,
    replaces no tensor and, in graph mode, does not re-capture.  (Template-branch features of the heads that a replayed graph read from a stale
    cache would make slot 1 fail here.)"""
    T, cut = 10, 4
    keys, seqs = zip(*[world.seq(b, b, 80 + b, T) for b in range(3)])
    refs = [world.single(k) for k in keys]
    new_key, new_seq = world.seq(2, 0, 91, T - cut)          # (270, 400) into the slot that ran (300, 480); another seed = another texture
    new_ref = world.single(new_key)
    bt = world.tracker(3, graph)
    bt.init(*_init_args(seqs))
    worst, worst_new = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    s0 = bt.host_syncs
    for i in range(1, cut + 1):
        res = bt.track_new(i, [s[0][i] for s in seqs])
        for b in range(3):
            _check(res[b], (refs[b][0][i - 1], refs[b][1][i - 1]), i - 1, ("b", b), worst)
    g_before, rows = bt._graph, _rows(bt, world.twin)
    objs = {k: v[0] for k, v in rows.items()}
    frames, _, init = new_seq
    bt.reinit(1, frames[0], init["bbox"], init["poly"], init["gt_points"], init["first_point"])
    assert bt._graph is g_before and (g_before is not None) == graph
    assert bt._arena.size(1) == SIZES[2] and bt._arena.dims.tolist() == [list(SIZES[0]), list(SIZES[2]), list(SIZES[2])]
    assert bt._first.dims is bt._arena.dims and np.array_equal(bt._first.frame(1).cpu().numpy(), frames[0])
    now = _rows(bt, world.twin)
    assert set(now) == set(rows)
    for name, (t, was) in rows.items():
        assert now[name][0] is objs[name], name                                  # the same tensors, written in place
        assert torch.equal(t[0], was[0]) and torch.equal(t[2], was[2]), name    # rows 0 and 2: bit-equal
        assert not torch.equal(t[1], was[1]), name                               # row 1: the new sequence's
    assert bt.track is objs["track"] and bt.seq is objs["seq"] and bt.state is objs["state"]
    assert not bool(bt.state[1].any())
    for i in range(cut + 1, T):
        k = i - cut                                      # the new sequence's frame index
        res = bt.track_new(i, [seqs[0][0][i], frames[k], seqs[2][0][i]])
        for b in (0, 2):
            _check(res[b], (refs[b][0][i - 1], refs[b][1][i - 1]), i - 1, ("b", b), worst)
        _check(res[1], (new_ref[0][k - 1], new_ref[1][k - 1]), k - 1, ("b", "re-inited slot 1"), worst_new)
    assert bt._graph is g_before
    assert bt.host_syncs - s0 == (T - 1) + 1             # one read per step + the re-init's channel average
    _report("re-init mid-run (n=3), slots 0 and 2", graph, worst)
    _report("re-init mid-run (n=3), slot 1 after its re-init", graph, worst_new)
    with pytest.raises(ValueError):                      # above the capacity: refused before anything is written
        bt.reinit(1, np.zeros((CAPACITY[0] + 1, 64, 3), np.uint8), init["bbox"], init["poly"], init["gt_points"], init["first_point"])
    assert bt._arena.size(1) == SIZES[2]
    with pytest.raises(ValueError, match="slot 1"):
        bt.reinit(1, frames[0], init["bbox"], init["poly"], init["gt_points"], None)
    with pytest.raises(IndexError):
        bt.reinit(3, frames[0], init["bbox"], init["poly"], init["gt_points"], init["first_point"])


def test_track_videos_streams_five_videos_through_two_slots(world):
    """(c) track_videos, n = 2, five videos of lengths 4, 7, 3, 6, 5 and two frame sizes, one hipGraph per step: every frame of every video within
    the bounds of its own B = 1 run; host reads = steps + re-inits + init's one."""
    from hdn_amd import track_videos
    lengths, sizes = [4, 7, 3, 6, 5], [0, 1, 1, 0, 1]
    keys, seqs = zip(*[world.seq(sizes[v], v % 3, 100 + v, lengths[v]) for v in range(5)])
    refs = [world.single(k, cpu=False) for k in keys]          # (each video against its own B = 1 run; (a) and (b) hold the CPU loop too)
    bt = world.tracker(2, True)
    res = track_videos(bt, [(s[0], s[2]) for s in seqs])
    assert bt._graph is not None and [len(r) for r in res] == [3, 6, 2, 5, 4]
    worst = [0.0, 0.0, 0.0]
    for v in range(5):
        for k, r in enumerate(res[v]):
            _check(r, (refs[v][0][k], refs[v][1][k]), k, ("c", v), worst)
    assert bt.host_syncs == 10 + 3 + 1                   # slot 0: 3 + 2 + 5 steps, slot 1: 6 + 4; three re-inits; init's channel averages
    _report("track_videos (n=2, five videos)", True, worst)
    small = world.tracker(2, True, capacity=SIZES[1])
    with pytest.raises(ValueError, match="video 0"):
        track_videos(small, [(s[0], s[2]) for s in seqs])
    assert small._arena is None and small.host_syncs == 0           # before the first launch
