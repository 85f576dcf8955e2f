"""A body that cannot be captured as a hipGraph (a host read inside the model, as in tests/test_gpu_tracker.py::
test_graph_capture_failure_falls_back_to_eager for HomoTracker) in the other trackers that go through hdn_amd._loop.capture_graph:
BatchedHomoTracker (plain and arena mode), SimiTracker, BatchedSimiTracker (plain and arena mode).  Each warns once, goes on eagerly with the
state the warm-up runs advanced put back, reads the host as often as an eager tracker, and gives what a graph=False run of the same tracker gives."""
import copy
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

HW, N = (180, 320), 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def seqs():
    from synth_sequence import make_sequence
    return [make_sequence(n_frames=4, frame_hw=HW, target_wh=(80, 60), seed=5 + b) for b in range(N)]


class HostRead(torch.nn.Module):       # stands for reference-side code that synchronises
    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        float(x.sum())                 # device -> host read: illegal during capture
        return self.inner(x)


def _init_args(seqs):
    return ([s[0][0] for s in seqs], [s[2]["bbox"] for s in seqs], [s[2]["poly"] for s in seqs], [s[2]["gt_points"] for s in seqs],
            [s[2]["first_point"] for s in seqs])


def _run(make, init, step, T, batched):
    """An eager tracker and a graph=True one (each on its own copy of the model) over frames 1 .. T - 1 -> (eager results, fallen-back results,
    the two trackers).  The first graphed step must warn exactly once, the later ones not at all."""
    eager = make(False)
    init(eager)
    want = [step(eager, i) for i in range(1, T)]
    trk = make(True)
    init(trk)
    with pytest.warns(UserWarning, match="could not be captured") as rec:
        got = [step(trk, 1)]
    said = [str(w.message) for w in rec if "could not be captured" in str(w.message)]
    assert len(said) == 1 and ("the batched per-frame body" in said[0]) == batched and ("the per-frame body" in said[0]) == (not batched), said
    assert trk.use_graph is False and trk._graph is None
    with warnings.catch_warnings(record=True) as later:
        warnings.simplefilter("always")
        got += [step(trk, i) for i in range(2, T)]
    assert not [w for w in later if "could not be captured" in str(w.message)]
    assert trk.use_graph is False and trk._graph is None
    assert trk.host_syncs == eager.host_syncs
    return want, got, eager, trk


@pytest.mark.parametrize("capacity", [None, HW], ids=["plain", "arena"])
def test_batched_homo_tracker_capture_failure_falls_back_to_eager(dev, seqs, capacity):
    from test_gpu_batched_tracker import _similarity_twin
    from hdn_amd.batched_tracker import BatchedHomoTracker
    from hdn_amd.similarity import DeviceSimilarity
    twin, _, _, cfg = _similarity_twin(dev)
    twin.hm_net.ShareFeature = HostRead(twin.hm_net.ShareFeature)

    def make(graph):
        m = copy.deepcopy(twin)
        return BatchedHomoTracker(m.hm_net, N, similarity=DeviceSimilarity(m, cfg), cfg=cfg, graph=graph, frame_capacity=capacity)

    want, got, eager, trk = _run(make, lambda t: t.init(*_init_args(seqs)), lambda t, i: t.track_new(i, [s[0][i] for s in seqs]), 4, batched=True)
    worst = 0.0
    for a, b in zip(got, want):
        for ra, rb in zip(a, b):
            worst = max(worst, float(np.abs(ra["points"] - rb["points"]).max()))
            np.testing.assert_allclose(ra["points"], rb["points"], rtol=0, atol=2e-3)
    print(f"BatchedHomoTracker ({'arena' if capacity else 'plain'}) after a failed capture vs eager: worst corner difference {worst:.1e} px")


def _same_records(got, want):
    for a, b in zip(got, want):
        for ra, rb in zip(*((a, b) if isinstance(a, list) else ([a], [b]))):
            assert set(ra) == set(rb) == {"bbox", "bbox_aligned", "best_score", "rot", "polygon"}
            for k in ra:            # the eager twin runs the same kernels in the same order: no tolerance
                assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])), (k, ra[k], rb[k])


def _simi_model(dev):
    from test_gpu_simi_tracker import _standin
    twin, _, cfg = _standin(dev, loc_scale_lp=0.3)
    twin.backbone[1] = HostRead(twin.backbone[1])
    return twin, cfg


def test_simi_tracker_capture_failure_falls_back_to_eager(dev, seqs):
    from hdn_amd.simi_tracker import SimiTracker
    twin, cfg = _simi_model(dev)
    frames, _, init = seqs[0]
    fp = np.array([init["first_point"]])
    want, got, eager, trk = _run(lambda graph: SimiTracker(copy.deepcopy(twin), cfg=cfg, graph=graph),
                                 lambda t: t.init(frames[0], init["bbox"], init["poly"], fp), lambda t, i: t.track_new(i, frames[i]), 4, batched=False)
    _same_records(got, want)
    assert torch.equal(trk.track, eager.track) and torch.equal(trk.state, eager.state)


@pytest.mark.parametrize("capacity", [None, HW], ids=["plain", "arena"])
def test_batched_simi_tracker_capture_failure_falls_back_to_eager(dev, seqs, capacity):
    from hdn_amd.simi_tracker import BatchedSimiTracker
    twin, cfg = _simi_model(dev)
    want, got, eager, trk = _run(lambda graph: BatchedSimiTracker(copy.deepcopy(twin), N, cfg=cfg, graph=graph, frame_capacity=capacity),
                                 lambda t: t.init(*_init_args(seqs)), lambda t, i: t.track_new(i, [s[0][i] for s in seqs]), 4, batched=True)
    _same_records(got, want)
    assert torch.equal(trk.track, eager.track) and torch.equal(trk.state, eager.state)
