"""Videos of different sizes and lengths streamed through the slots of the lock-step tracker (hdn_amd.batched_tracker in arena mode: frame_capacity,
reinit, track_videos) - what the reference's users do by splitting the dataset by hand across processes (tools/test.py:91-103).

Every sequence is held to its own B = 1 run through hdn_amd.tracker.HomoTracker, with the bounds of tests/test_gpu_batched_tracker.py (set from
observation for exactly this comparison - another batch size, the same kernels; the frame kernels are bit-exact per slot, so the ragged path adds
nothing to them): eager 2e-4 px on the first three frames and 5e-3 px after, one hipGraph per step 1e-3 px and 2e-2 px, best_score within 1e-5 (eager).
For a slot that was handed a new video, "the first three frames" count from the re-init."""
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
TARGETS = [(150, 100), (120, 90), (100, 130)]          # (of test_gpu_batched_tracker._sequences' list: those that fit every size above)
CAPACITY = (360, 640)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class _World:
    """The stand-in similarity model + homography estimator, the synthetic sequences and their B = 1 runs, each computed once."""

    def __init__(self, dev):
        from test_gpu_batched_tracker import _similarity_twin
        self.dev = dev
        self.twin, _, _, self.cfg = _similarity_twin(dev)
        self._seqs, self._single = {}, {}

    def seq(self, size, target, seed, T):
        from synth_sequence import make_sequence
        key = (size, target, seed, T)
        if key not in self._seqs:
            self._seqs[key] = make_sequence(n_frames=T, frame_hw=SIZES[size], target_wh=TARGETS[target], seed=seed)
        return key, self._seqs[key]

    def single(self, key):
        """track_new's results of the sequence's own B = 1 run, frames 1 .. T - 1."""
        from hdn_amd.similarity import DeviceSimilarity
        from hdn_amd.tracker import HomoTracker
        if key not in self._single:
            frames, _, init = self._seqs[key]
            t = HomoTracker(self.twin.hm_net, similarity=DeviceSimilarity(self.twin, self.cfg), cfg=self.cfg)
            t.init(frames[0], init["bbox"], init["poly"], init["gt_points"], init["first_point"])
            self._single[key] = [t.track_new(i, frames[i]) for i in range(1, len(frames))]
        return self._single[key]

    def tracker(self, n, graph, capacity=CAPACITY):
        from hdn_amd.batched_tracker import BatchedHomoTracker
        from hdn_amd.similarity import DeviceSimilarity
        return BatchedHomoTracker(self.twin.hm_net, n, similarity=DeviceSimilarity(self.twin, self.cfg), cfg=self.cfg, graph=graph,
                                  frame_capacity=capacity)


@pytest.fixture(scope="module")
def world(dev):
    return _World(dev)


def _bound(graph, k):
    """k: frames since the sequence's (re-)init, 0 = the first tracked frame."""
    return ((1e-3 if k < 3 else 2e-2) if graph else (2e-4 if k < 3 else 5e-3))


def _init_args(seqs):
    return ([s[0][0] for s in seqs], [s[2]["bbox"] for s in seqs], [s[2]["poly"] for s in seqs], [s[2]["gt_points"] for s in seqs],
            [s[2]["first_point"] for s in seqs])


def _check(res, ref, graph, k, where, worst):
    from synth_sequence import success_4pts_error
    e = success_4pts_error(res["points"], ref["points"])
    worst[0] = max(worst[0], e)
    assert e <= _bound(graph, k), (where, k, e)
    if not graph:
        assert abs(float(res["best_score"]) - float(ref["best_score"])) <= 1e-5, (where, k)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_mixed_frame_sizes_in_one_batch(world, graph):
    """(a) n = 3, one sequence per frame size, with the similarity branch: every sequence within the bounds of its own B = 1 run; one host read per step."""
    T = 6
    keys, seqs = zip(*[world.seq(b, b, 80 + b, 10) for b in range(3)])
    single = [world.single(k) for k in keys]
    bt = world.tracker(3, graph)
    bt.init(*_init_args(seqs))
    assert [bt._arena.size(b) for b in range(3)] == SIZES
    s0, worst = bt.host_syncs, [0.0]
    for i in range(1, T):
        res = bt.track_new(i, [s[0][i] for s in seqs])
        for b in range(3):
            _check(res[b], single[b][i - 1], graph, i - 1, ("a", b), worst)
    assert bt.host_syncs - s0 == T - 1
    assert (bt._graph is not None) == graph
    print(f"mixed sizes (n=3, {'hipGraph' if graph else 'eager'}): worst corner distance to the B=1 runs {worst[0]:.2e} px")
    with pytest.raises(ValueError, match="slot 1"):          # a running slot keeps its frame size
        bt.track_new(99, [seqs[0][0][1], seqs[0][0][1], seqs[2][0][1]])
    with pytest.raises(ValueError):
        bt.track_new(99, [seqs[0][0][1]] * 2)


def _rows(bt, twin):
    """The per-sequence tensors a re-init writes, as clones: name -> tensor with the sequence along dim 0."""
    out = {"H_total": bt.H_total, "state": bt.similarity.state, "seq": bt.similarity.seq, "params0": bt.similarity._params0, "consts": bt._consts,
           "const_params": bt._const_params, "init_points": bt.init_points, "init_homo_tmp": bt.init_homo_tmp, "init_patch_1": bt.init_patch_1}
    for name in ("zf", "zf_lp"):
        z = getattr(twin, name)
        for l, t in enumerate(z if isinstance(z, (list, tuple)) else [z]):
            out[f"{name}[{l}]"] = t
    for name in ("head", "head_lp"):
        for l, t in enumerate(getattr(twin, name)._hdn_template_cache.kern):
            out[f"{name}.kern[{l}]"] = t
    return {k: (v, v.clone()) for k, v in out.items()}


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_reinit_one_slot_mid_run(world, graph):
    """(b) n = 3, 9 steps; after step 4 slot 1 is handed a new sequence of another size and another texture.  Slots 0 and 2 stay within the bounds of
    their uninterrupted B = 1 runs, slot 1 from step 5 on within those of a fresh B = 1 run of the new sequence.  The re-init touches row 1 only,
    replaces no tensor and, in graph mode, does not re-capture.  (A stale template-kernel cache in the heads - which a replayed graph keeps reading -
    makes slot 1 fail here.)"""
    T, cut = 10, 4
    keys, seqs = zip(*[world.seq(b, b, 80 + b, T) for b in range(3)])
    single = [world.single(k) for k in keys]
    new_key, new_seq = world.seq(2, 0, 91, T - cut)          # (270, 400) into the slot that ran (300, 480); another seed = another texture
    new_single = world.single(new_key)
    bt = world.tracker(3, graph)
    bt.init(*_init_args(seqs))
    worst, worst_new = [0.0], [0.0]
    s0 = bt.host_syncs
    for i in range(1, cut + 1):
        res = bt.track_new(i, [s[0][i] for s in seqs])
        for b in range(3):
            _check(res[b], single[b][i - 1], graph, i - 1, ("b", b), worst)
    g_before, rows = bt._graph, _rows(bt, world.twin)
    objs = {k: v[0] for k, v in rows.items()}
    frames, _, init = new_seq
    bt.reinit(1, frames[0], init["bbox"], init["poly"], init["gt_points"], init["first_point"])
    assert bt._graph is g_before and (g_before is not None) == graph
    assert bt._arena.size(1) == SIZES[2] and bt._arena.dims.tolist() == [list(SIZES[0]), list(SIZES[2]), list(SIZES[2])]
    now = _rows(bt, world.twin)
    for name, (t, was) in rows.items():
        assert now[name][0] is objs[name], name                                  # the same tensors, written in place
        assert torch.equal(t[0], was[0]) and torch.equal(t[2], was[2]), name    # rows 0 and 2: bit-equal
        if name != "state":
            assert not torch.equal(t[1], was[1]), name                           # row 1: the new sequence's
    assert torch.equal(bt.H_total[1], torch.eye(3, dtype=torch.float64, device=bt.H_total.device)) and not bool(bt.similarity.state[1].any())
    for i in range(cut + 1, T):
        k = i - cut                                      # the new sequence's frame index
        res = bt.track_new(i, [seqs[0][0][i], frames[k], seqs[2][0][i]])
        for b in (0, 2):
            _check(res[b], single[b][i - 1], graph, i - 1, ("b", b), worst)
        _check(res[1], new_single[k - 1], graph, k - 1, ("b", "re-inited slot 1"), worst_new)
    assert bt._graph is g_before
    assert bt.host_syncs - s0 == (T - 1) + 1             # one read per step + the re-init's channel average
    print(f"re-init mid-run (n=3, {'hipGraph' if graph else 'eager'}): worst corner distance to the B=1 runs {worst[0]:.2e} px (slots 0, 2), "
          f"{worst_new[0]:.2e} px (slot 1 after its re-init)")
    with pytest.raises(ValueError):                      # the point count is the tracker's
        bt.reinit(1, frames[0], init["bbox"], init["poly"], np.asarray(init["gt_points"]).reshape(-1, 2)[:3])
    with pytest.raises(ValueError):                      # above the capacity: refused before anything is written
        bt.reinit(1, np.zeros((CAPACITY[0] + 1, 64, 3), np.uint8), init["bbox"], init["poly"], init["gt_points"])
    assert bt._arena.size(1) == SIZES[2]


def test_track_videos_streams_five_videos_through_two_slots(world):
    """(c) track_videos, n = 2, five videos of lengths 4, 7, 3, 6, 5 and two frame sizes, one hipGraph per step: every frame of every video within the
    bounds of its own B = 1 run; host reads = steps + re-inits + init's one."""
    from hdn_amd import track_videos
    lengths, sizes = [4, 7, 3, 6, 5], [0, 1, 1, 0, 1]
    keys, seqs = zip(*[world.seq(sizes[v], v % 3, 100 + v, lengths[v]) for v in range(5)])
    single = [world.single(k) for k in keys]
    bt = world.tracker(2, True)
    res = track_videos(bt, [(s[0], s[2]) for s in seqs])
    assert bt._graph is not None and [len(r) for r in res] == [T - 1 for T in lengths]
    worst = [0.0]
    for v in range(5):
        for k, r in enumerate(res[v]):
            _check(r, single[v][k], True, k, ("c", v), worst)
    assert bt.host_syncs == 10 + 3 + 1                   # slot 0: 3 + 2 + 5 steps, slot 1: 6 + 4; three re-inits; init's channel averages
    print(f"track_videos (n=2, five videos, hipGraph): worst corner distance to the B=1 runs {worst[0]:.2e} px")
    small = world.tracker(2, True, capacity=SIZES[1])
    with pytest.raises(ValueError, match="video 0"):
        track_videos(small, [(s[0], s[2]) for s in seqs])
    assert small._arena is None and small.host_syncs == 0           # before the first launch
