"""The ragged frame kernels (hdn_*_ragged_*: B slots of frames of DIFFERENT sizes, every slot's (H, W) read from device memory) on the device.
The oracle is the project's own for the batch entries: per slot bit-identical to the single-frame call on that slot's frame alone.

Capacity (48, 160); the slot sizes are the smallest at which the per-slot arithmetic can go wrong: full capacity, bh = 9 with one 70-wide block,
exactly one 64-wide block, one pixel into a second block and one row over 16, W < 64, and the smallest frame."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HMAX, WMAX = 48, 160
SIZES = [(48, 160), (9, 70), (16, 64), (17, 65), (33, 20), (2, 3)]
FILL = 0xA5
CROPS = ((127, 0), (255, 0), (127, 1))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _frames(g, sizes):
    return [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _records(g, sizes, dev):
    """Per-slot matrices as tests/test_gpu_batched_tracker.py draws them, the translations scaled to the frame; slot 3's perspective matrix and
    slot 4's rotation map partly outside the frame (BORDER_REPLICATE)."""
    n = len(sizes)
    Hs = np.tile(np.eye(3), (n, 1, 1))
    rot = np.zeros((n, 6))
    par = np.zeros((n, 6))
    for b, (h, w) in enumerate(sizes):
        Hs[b, :2, 2] = g.normal(0, 0.03, 2) * (w, h)
        Hs[b, :2, :2] += g.normal(0, 0.03, (2, 2))
        Hs[b, 2, :2] = g.normal(0, 1e-5, 2)
        a = g.normal(0, 0.1)
        rot[b] = [np.cos(a), -np.sin(a), g.normal(0, 0.02) * w, np.sin(a), np.cos(a), g.normal(0, 0.02) * h]
        par[b] = [g.uniform(0.3, 0.7) * w, g.uniform(0.3, 0.7) * h, g.uniform(0.5, 1.5) * max(h, w), *g.uniform(90, 130, 3)]
    Hs[3, :2, 2] = (0.6 * sizes[3][1], -0.4 * sizes[3][0])
    rot[4, 2], rot[4, 5] = -0.5 * sizes[4][1], 0.3 * sizes[4][0]
    return tuple(torch.from_numpy(a.reshape(n, -1)).to(dev) for a in (Hs, rot, par))


def _single(FR, frame, Hd, Rd, Pd):
    """The single-frame calls on one dense frame: (perspective, cubic, crops..., search info)."""
    out = [FR.warp_perspective(frame, Hd), FR.warp_affine_cubic(frame, Rd)]
    out += [FR.get_subwindow(frame, None, sz, None, None, params=Pd, islog=islog)[0] for sz, islog in CROPS]
    out.append(FR.get_search_info(frame, None, None, None, model_sz=127, params=Pd)[0])
    return out


def _filled(arena):
    out = arena.like()
    out.data.fill_(FILL)
    return out


def _ragged(FR, arena, Hd, Rd, Pd):
    """The same calls on the whole arena: (perspective arena, cubic arena, crops..., search info), the output arenas pre-filled with 0xA5."""
    out = [FR.warp_perspective(arena, Hd, out=_filled(arena)), FR.warp_affine_cubic(arena, Rd, out=_filled(arena))]
    out += [FR.get_subwindow(arena, None, sz, None, None, params=Pd, islog=islog) for sz, islog in CROPS]
    out.append(FR.get_search_info(arena, None, None, None, model_sz=127, params=Pd))
    return out


def _assert_slot_exact(got, want, b, sizes, what=""):
    h, w = sizes[b]
    for k in range(2):                     # the two warps: the frame, and not one byte of the slot beyond it
        assert torch.equal(got[k].data[b, :h * w * 3].view(h, w, 3), want[k]), (what, b, k)
        assert bool((got[k].data[b, h * w * 3:] == FILL).all()), (what, b, k, "stray write")
    for k in range(2, len(want)):
        assert torch.equal(got[k][b], want[k]), (what, b, k)


@pytest.fixture(scope="module")
def case(dev):
    """One arena, its records and the single-frame results, computed once and left unchanged."""
    from hdn_amd import frame as FR
    g = np.random.default_rng(11)
    frames = _frames(g, SIZES)
    arena = FR.FrameArena(len(SIZES), HMAX, WMAX, device=dev)
    arena.set_all(frames)
    Hd, Rd, Pd = _records(g, SIZES, dev)
    want = [_single(FR, arena.frame(b).clone(), Hd[b], Rd[b], Pd[b]) for b in range(len(SIZES))]
    return frames, Hd, Rd, Pd, want


def _arena(FR, frames, dev):
    arena = FR.FrameArena(len(frames), HMAX, WMAX, device=dev)
    arena.set_all(frames)
    return arena


def test_ragged_frame_kernels_bit_exact_per_slot_and_no_stray_writes(dev, case):
    from hdn_amd import frame as FR
    frames, Hd, Rd, Pd, want = case
    arena = _arena(FR, frames, dev)
    assert arena.dims.tolist() == [list(s) for s in SIZES]
    for b, f in enumerate(frames):
        assert torch.equal(arena.frame(b).cpu(), torch.from_numpy(f))
    got = _ragged(FR, arena, Hd, Rd, Pd)
    assert got[0].dims is arena.dims and got[2].shape == (len(SIZES), 3, 127, 127) and got[4].shape == (len(SIZES), 6, 127, 127)
    for b in range(len(SIZES)):
        _assert_slot_exact(got, want[b], b, SIZES)
    # the border case does leave the frame: slot 3's perspective warp takes its left 0.6 W columns from outside (BORDER_REPLICATE)
    assert float(Hd[3, 2]) > 0.5 * SIZES[3][1]


@pytest.mark.parametrize("record", [(0, 5), (HMAX + 1, WMAX)])
def test_ragged_frame_kernels_skip_a_slot_whose_record_does_not_fit(dev, case, record):
    """dims is device data the host never sees: slot 2 (not the last) is given a bad record by writing the device table directly.  It is skipped -
    its warp outputs keep their fill, its crops theirs - and the slot behind it, where a broken guard of (Hmax + 1, Wmax) would spill, is exact."""
    from hdn_amd import frame as FR
    frames, Hd, Rd, Pd, want = case
    arena = _arena(FR, frames, dev)
    bad = 2
    arena.dims[bad] = torch.tensor(record, dtype=torch.int32, device=dev)
    got = [FR.warp_perspective(arena, Hd, out=_filled(arena)), FR.warp_affine_cubic(arena, Rd, out=_filled(arena))]
    for k in range(2):
        assert bool((got[k].data[bad] == FILL).all()), (record, k)
    # the crops of the skipped slot are not written either: run the entry on a pre-filled output
    from hdn_amd import _lib
    lib = _lib.load()
    for mode, ch in ((0, 3), (1, 1)):
        out = torch.full((len(SIZES), ch, 127, 127), -7.0, dtype=torch.float32, device=dev)
        rc = lib.hdn_subwindow_ragged_f32(_lib.ptr(arena.data), arena.slot_stride, _lib.ptr(arena.dims), _lib.ptr(Pd), 6, _lib.ptr(out), len(SIZES),
                                          HMAX, WMAX, 3, 127, mode, _lib.stream_ptr(dev))
        assert rc == 0
        assert bool((out[bad] == -7.0).all()), (record, mode)
        k = 2 if mode == 0 else 5
        for b in range(len(SIZES)):
            if b != bad:
                assert torch.equal(out[b], want[b][k]), (record, mode, b)
    for b in range(len(SIZES)):
        if b != bad:
            h, w = SIZES[b]
            for k in range(2):
                assert torch.equal(got[k].data[b, :h * w * 3].view(h, w, 3), want[b][k]), (record, b, k)
                assert bool((got[k].data[b, h * w * 3:] == FILL).all()), (record, b, k)


def test_ragged_frame_kernels_replayed_as_a_graph_after_slots_changed_size(dev, case):
    """The three ragged calls captured ONCE as a hipGraph, replayed after frames and dims of two slots were changed in place, (16, 64) <-> (33, 20):
    every slot equals the single-frame calls for its CURRENT size."""
    from hdn_amd import frame as FR
    frames, Hd, Rd, Pd, want = case
    arena = _arena(FR, frames, dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _ragged(FR, arena, Hd, Rd, Pd)                # (lazy initialisations outside the capture: the cubic table, the log-polar maps)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        wp = FR.warp_perspective(arena, Hd)
        wa = FR.warp_affine_cubic(arena, Rd)
        crops = [FR.get_subwindow(arena, None, sz, None, None, params=Pd, islog=islog) for sz, islog in CROPS]
        si = FR.get_search_info(arena, None, None, None, model_sz=127, params=Pd)
    got = [wp, wa] + crops + [si]
    for o in (wp, wa):
        o.data.fill_(FILL)
    graph.replay()
    for b in range(len(SIZES)):
        _assert_slot_exact(got, want[b], b, SIZES, "first replay")
    # slots 2 and 4 swap sizes: new frames, the same matrices and crop records
    g = np.random.default_rng(12)
    sizes = list(SIZES)
    sizes[2], sizes[4] = SIZES[4], SIZES[2]
    new = {2: g.integers(0, 256, sizes[2] + (3,), dtype=np.uint8), 4: g.integers(0, 256, sizes[4] + (3,), dtype=np.uint8)}
    for b, f in new.items():
        arena.set(b, f)
    assert arena.dims.tolist() == [list(s) for s in sizes]
    for o in (wp, wa):
        o.data.fill_(FILL)
    graph.replay()
    torch.cuda.synchronize()
    for b in range(len(SIZES)):
        w = _single(FR, torch.from_numpy(new[b]).to(dev), Hd[b], Rd[b], Pd[b]) if b in new else want[b]
        _assert_slot_exact(got, w, b, sizes, "after the change")
        assert wp.size(b) == sizes[b] and tuple(wp.frame(b).shape) == sizes[b] + (3,)
