"""hdn_simi_track_update_ragged_f64 (-m gpu): the similarity-only tracker's update kernel with every slot's frame size read from the arena's device
table.  The oracle is the project's own hdn_simi_track_update_f64 called on one row with that slot's (W_b, H_b): the two kernels share one device
function, so every row is compared with torch.equal.  B = 6 hand-made records whose sizes make the width clamp alone, the height clamp alone, both
and neither occur; no record is square, so an (H, W) swap or a neighbour's record changes a result."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

B = 6
DIMS = [(360, 640), (20, 640), (360, 30), (9, 70), (48, 160), (17, 65)]       # (H_b, W_b)
CAP = (360, 640)
# boxes (w, h) and the decoded scale S[46], chosen against DIMS: slot 0 neither clamp; 1 and 4 the height alone (38 * 1.1 > 20, 44 * 1.15 > 48); 2 the
# width alone (48 * 0.95 > 30); 3 the height, then the 10 px floor (9 -> 10); 5 both (58 * 1.15 > 65, 36 * 1.15 > 17)
BOXES = [(50, 40), (52, 38), (48, 42), (50, 40), (46, 44), (58, 36)]
SCALES = [1.0, 1.1, 0.95, 1.2, 1.15, 1.15]
THRESH, CONTEXT, RATIO = 0.5, 0.5, 2.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _inputs(dev):
    """(state [B,48], tr [B,48], seq [B,8]) float64 on the device; boxes of about 50 x 40, S[46] (the scale) in [0.9, 1.2], S[47] 0 or 1."""
    from hdn_amd.simi_tracker import sequence_records
    from hdn_amd.similarity import TrackerConfig
    g = np.random.default_rng(20261018)
    state = g.uniform(-1.0, 1.0, (B, 48))
    state[:, 2:4] = g.uniform(20.0, 300.0, (B, 2))          # the decoded centre
    state[:, 5], state[:, 7] = g.uniform(0.2, 1.0, B), g.uniform(0.2, 1.0, B)     # best_score, pscore (both sides of the threshold)
    state[:, 17] = g.uniform(-0.2, 0.2, B)                  # rot_delta
    state[:, 46] = SCALES
    state[:, 47] = np.array([0, 1, 0, 0, 1, 0], np.float64)
    tr, seq = [], []
    for b in range(B):
        w, h = BOXES[b][0] + g.uniform(-0.5, 0.5), BOXES[b][1] + g.uniform(-0.5, 0.5)
        cx, cy = g.uniform(60, 200, 2)
        poly = [cx, cy, w, h, float(g.uniform(-0.3, 0.3))]
        t, s, _, _ = sequence_records(poly, (cx - w / 2, cy - h / 2), g.uniform(90, 130, 3), TrackerConfig())
        tr.append(t)
        seq.append(s)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    return to(state), to(np.stack(tr)), to(np.stack(seq))


def _ragged(state, tr, seq, out, dims, cap=CAP):
    from hdn_amd import _lib
    with _lib.device_guard(state.device):
        _lib.check(_lib.load().hdn_simi_track_update_ragged_f64(_lib.ptr(state), _lib.ptr(tr), _lib.ptr(seq), _lib.ptr(out), _lib.ptr(dims), state.shape[0],
                                                                cap[0], cap[1], THRESH, CONTEXT, RATIO, _lib.stream_ptr(state.device)), "ragged update")


def _single_rows(state, tr, seq, sizes):
    """The existing entry on every row alone, B = 1, with (img_w, img_h) = (W_b, H_b) -> (tr, seq, out) stacked."""
    from hdn_amd import _lib
    lib = _lib.load()
    T, Q, O = tr.clone(), seq.clone(), torch.zeros((state.shape[0], 20), dtype=torch.float64, device=state.device)
    for b, (H, W) in enumerate(sizes):
        s, t, q, o = state[b:b + 1].clone(), T[b:b + 1].clone(), Q[b:b + 1].clone(), O[b:b + 1].clone()
        with _lib.device_guard(state.device):
            _lib.check(lib.hdn_simi_track_update_f64(_lib.ptr(s), _lib.ptr(t), _lib.ptr(q), _lib.ptr(o), 1, W, H, THRESH, CONTEXT, RATIO,
                                                     _lib.stream_ptr(state.device)), "update")
        T[b], Q[b], O[b] = t[0], q[0], o[0]
    return T, Q, O


@pytest.fixture(scope="module")
def case(dev):
    state, tr, seq = _inputs(dev)
    ref = _single_rows(state, tr, seq, DIMS)          # computed once, never written
    return state, tr, seq, ref


def test_every_slot_equals_the_single_call_at_its_own_size(dev, case):
    state, tr0, seq0, (rt, rq, ro) = case
    tr, seq, out = tr0.clone(), seq0.clone(), torch.zeros((B, 20), dtype=torch.float64, device=dev)
    dims = torch.tensor(DIMS, dtype=torch.int32, device=dev)
    _ragged(state, tr, seq, out, dims)
    for b in range(B):
        assert torch.equal(tr[b], rt[b]) and torch.equal(seq[b], rq[b]) and torch.equal(out[b], ro[b]), b
    # the clamps were met: the new size is the frame's own width / height somewhere, and somewhere it is not
    w, h = tr[:, 2].cpu().numpy(), tr[:, 3].cpu().numpy()
    wc = [bool(w[b] == DIMS[b][1]) for b in range(B)]
    hc = [bool(h[b] == DIMS[b][0]) for b in range(B)]
    print("width clamped:", wc, "height clamped:", hc)
    assert any(wc) and any(hc)
    kinds = set(zip(wc, hc))
    assert kinds == {(True, False), (False, True), (True, True), (False, False)}, kinds
    # with the capacity as every slot's size (what a launch-argument kernel would do) the rows differ
    ct, cq, co = _single_rows(state, tr0, seq0, [CAP] * B)
    assert not torch.equal(ct, rt) and not torch.equal(co, ro) and not torch.equal(cq, rq)
    for b in range(B):
        if wc[b] or hc[b]:
            assert not torch.equal(ct[b], rt[b]), b


@pytest.mark.parametrize("bad", [(0, 5), (CAP[0] + 1, CAP[1])], ids=["empty", "above-capacity"])
def test_a_slot_whose_record_does_not_fit_is_skipped(dev, case, bad):
    state, tr0, seq0, (rt, rq, ro) = case
    tr, seq, out = tr0.clone(), seq0.clone(), torch.zeros((B, 20), dtype=torch.float64, device=dev)
    nan = torch.tensor(0x7FF8DEADBEEF0001, dtype=torch.int64, device=dev)
    for t in (tr, seq, out):
        t[2].view(torch.int64).copy_(nan + torch.arange(t.shape[1], device=dev))
    before = [t[2].view(torch.int64).clone() for t in (tr, seq, out)]
    dims = torch.tensor(DIMS, dtype=torch.int32, device=dev)
    dims[2].copy_(torch.tensor(bad, dtype=torch.int32))
    _ragged(state, tr, seq, out, dims)
    for t, was in zip((tr, seq, out), before):
        assert torch.equal(t[2].view(torch.int64), was)
    for b in (0, 1, 3, 4, 5):
        assert torch.equal(tr[b], rt[b]) and torch.equal(seq[b], rq[b]) and torch.equal(out[b], ro[b]), b


def test_a_captured_graph_follows_the_size_table(dev, case):
    state, tr0, seq0, (rt, rq, ro) = case
    tr, seq, out = tr0.clone(), seq0.clone(), torch.zeros((B, 20), dtype=torch.float64, device=dev)
    dims = torch.tensor(DIMS, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _ragged(state, tr, seq, out, dims)           # (warm-up: the module is loaded before the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _ragged(state, tr, seq, out, dims)
    tr.copy_(tr0), seq.copy_(seq0), out.zero_()
    graph.replay()
    for b in range(B):
        assert torch.equal(tr[b], rt[b]) and torch.equal(seq[b], rq[b]) and torch.equal(out[b], ro[b]), b
    # slots 1 and 4 swap their sizes IN PLACE; the inputs are restored; the same graph is replayed
    sizes = list(DIMS)
    sizes[1], sizes[4] = sizes[4], sizes[1]
    d1 = dims[1].clone()
    dims[1].copy_(dims[4])
    dims[4].copy_(d1)
    assert dims.tolist() == [list(s) for s in sizes]
    tr.copy_(tr0), seq.copy_(seq0), out.zero_()
    graph.replay()
    st, sq, so = _single_rows(state, tr0, seq0, sizes)
    for b in range(B):
        assert torch.equal(tr[b], st[b]) and torch.equal(seq[b], sq[b]) and torch.equal(out[b], so[b]), b
    assert not torch.equal(st[1], rt[1]) and not torch.equal(st[4], rt[4])          # the swap changed both slots' results
