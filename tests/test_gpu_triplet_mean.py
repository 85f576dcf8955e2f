"""csrc/triplet_loss.hip's flag-selected means on the device against tests/triplet_mean_cases.py: every case forward and backward (raw ABI, every
subset of the three gradients, NaN-filled outputs: every element is written), two calls bit-equal, hdn_amd.triplet_l1_mean and its autograd path
against the explicit backward, one graph capture of forward + backward replayed while flags and data are rewritten in place (every set emptied and
refilled), the refusals."""
import itertools

import numpy as np
import pytest
import torch

import triplet_mean_cases as MC
from hdn_amd import triplet_l1_mean, triplet_l1_mean_backward  # noqa: F401  (the module is about them: without them nothing here is collected)

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0ABCD
E_NULL, E_SHAPE, E_LIMIT, E_ALIAS = -1, -2, -3, -4
SUBSETS = [s for s in itertools.product((True, False), repeat=3) if any(s)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b)) if a.dtype == torch.float32 else torch.equal(a, b)


def _nan(shape, dev):
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    out.view(torch.int32).fill_(NAN_BITS)
    return out


def _dev(c, dev):
    return [t.to(dev) for t in (c.a, c.p, c.n, c.if_pos, c.if_unsup)]


def _raw_forward(c, t, dev):
    """One raw call into NaN-filled outputs -> (out [1], counts [2], partial [N R])."""
    from hdn_amd import _lib
    partial, out = _nan((c.N * c.R,), dev), _nan((1,), dev)
    counts = torch.full((2,), -7, dtype=torch.int32, device=dev)
    _lib.launch("triplet_l1_mean", dev, _lib.load().hdn_triplet_l1_mean_f32, *[_lib.ptr(v) for v in t], _lib.ptr(partial), _lib.ptr(out),
                _lib.ptr(counts), c.N, c.R, c.D, c.rule, c.denom, c.margin, c.eps)
    return out, counts, partial


def _raw_backward(c, t, g, dev, need=(True, True, True)):
    from hdn_amd import _lib
    grads = [_nan(c.a.shape, dev) if w else None for w in need]
    _lib.launch("triplet_l1_mean_backward", dev, _lib.load().hdn_triplet_l1_mean_bwd_f32, *[_lib.ptr(v) for v in t], _lib.ptr(g),
                *[_lib.opt(x) for x in grads], c.N, c.R, c.D, c.rule, c.denom, c.margin, c.eps)
    return grads


@pytest.mark.parametrize("name", MC.NAMES)
def test_every_case_forward_and_backward(dev, name):
    c = MC.CASES[name]
    t, g = _dev(c, dev), c.g.to(dev)
    keep = [v.clone() for v in t]
    out, counts, partial = _raw_forward(c, t, dev)
    out2, counts2, partial2 = _raw_forward(c, t, dev)
    grads = _raw_backward(c, t, g, dev)
    grads2 = _raw_backward(c, t, g, dev)
    torch.cuda.synchronize()
    tr = c.truth()
    ratio = MC.check_value(c, out.cpu()[0], counts.cpu().tolist(), "raw")
    print(f"TRIPLET_MEAN {name}: value {float(out):.9g} value64 {tr['value']:.9g} |err| / bound {ratio:.3f} counts {counts.cpu().tolist()}")
    assert _same(out, out2) and _same(counts, counts2) and _same(partial, partial2)                 # two calls are bit-equal
    assert not bool((_bits(partial) == NAN_BITS).any())                                             # every row of the scratch is written ...
    unused = torch.from_numpy(~tr["used"]).to(dev).repeat_interleave(c.R)
    assert not bool((partial[unused] != 0).any()) and bool(torch.isfinite(partial).all())           # ... with 0 for a sample that is not read
    if c.exact:
        assert np.float32(float(out)).tobytes() == MC.restate32(c).tobytes()                         # the rule's division order, in the bits
    for a, b in zip(grads, grads2):
        assert _same(a, b) and not bool((_bits(a) == NAN_BITS).any())                                # every element written, the same bits
    c_got = MC.check_grads(c, [x.cpu() for x in grads], "raw")
    if tr["n_sel"] == 0:
        assert c_got is None and all(not bool((x != 0).any()) for x in grads)                        # empty selection: zero gradients
    for x in grads:
        assert not bool((x[torch.from_numpy(~tr["used"]).to(dev)] != 0).any())                       # also where the unused sample holds NaN
    for v, k in zip(t, keep):
        assert _same(v, k)                                                                           # the inputs are untouched
    for need in SUBSETS[1:]:                                                                         # every subset gives the all-three call's bits
        sub = _raw_backward(c, t, g, dev, need)
        for w, x, full in zip(need, sub, grads):
            assert (x is None) == (not w) and (x is None or _same(x, full)), need


@pytest.mark.parametrize("name", [n for n in MC.NAMES if n.startswith("f_")])
def test_python_layer_and_autograd_agree_with_the_explicit_backward(dev, name):
    import hdn_amd
    c = MC.CASES[name]
    t, g = _dev(c, dev), c.g.to(dev)
    raw_out, raw_counts, _ = _raw_forward(c, t, dev)
    raw_grads = _raw_backward(c, t, g, dev)
    value, counts = hdn_amd.triplet_l1_mean(*t, c.rule, denom=c.denom, margin=c.margin, eps=c.eps)
    assert value.dim() == 0 and counts.dtype == torch.int32 and tuple(counts.shape) == (2,) and not value.requires_grad
    assert _same(value.reshape(1), raw_out) and _same(counts, raw_counts)
    for need in SUBSETS:
        py = hdn_amd.triplet_l1_mean_backward(*t, g, c.rule, denom=c.denom, margin=c.margin, eps=c.eps, need_anchor=need[0],
                                              need_positive=need[1], need_negative=need[2])
        leaves = [v.clone().requires_grad_(w) for v, w in zip(t[:3], need)]
        v4 = [x.unsqueeze(1) for x in leaves]                                                        # [N,1,R,D], the reference's layout
        out, cnt = hdn_amd.triplet_l1_mean(*v4, t[3], t[4], c.rule, denom=c.denom, margin=c.margin, eps=c.eps)
        assert out.requires_grad and not cnt.requires_grad and _same(out.detach().reshape(1), raw_out)
        (out * g[0]).backward()                                                                      # the upstream gradient is g exactly
        for w, x, leaf, full in zip(need, py, leaves, raw_grads):
            assert (x is None) == (not w) and (leaf.grad is None) == (not w)
            if w:
                assert _same(x, full) and _same(leaf.grad, full), (name, need)


def test_a_zero_upstream_gradient_gives_zeros_not_nan(dev):
    """What torch.where gating passes to a term that is gated off: with an empty selection (and with a full one) the gradients are exactly zero."""
    import hdn_amd
    for name in ("f_3x3x65_none_with_neg_r1", "f_3x3x65_none_no_neg_r1", "f_3x3x65_none_with_neg_r0", "f_3x3x65_all_r0"):
        c = MC.CASES[name]
        t = _dev(c, dev)
        leaves = [v.clone().requires_grad_(True) for v in t[:3]]
        value, counts = hdn_amd.triplet_l1_mean(*leaves, t[3], t[4], c.rule)
        gated = torch.where(counts[0] > 0, value, torch.zeros_like(value)) * 0.0
        gated.backward()
        assert bool(torch.isfinite(value)) and all(not bool((x.grad != 0).any()) for x in leaves), name


def test_forward_and_backward_in_a_graph_follow_flags_and_data_rewritten_in_place(dev):
    """One capture of forward and explicit backward; then flags, data and grad_out are overwritten in place with other cases' of the same shape -
    every set emptied and refilled - and the graph is replayed: it gives what an eager call gives, bit for bit."""
    import hdn_amd
    for rule in (0, 1):
        seq = [f"f_9x3x127_{p}_r{rule}" for p in ("alternating", "all", "none_with_neg", "quirk", "none_no_neg", "first", "half", "nan_unused",
                                                    "last", "alternating")]
        first = MC.CASES[seq[0]]
        st = [v.clone() for v in _dev(first, dev)]
        g = first.g.to(dev).clone()

        def step():
            value, counts = hdn_amd.triplet_l1_mean(*st, rule)
            return [value, counts, *hdn_amd.triplet_l1_mean_backward(*st, g, rule)]

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()                                                              # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="global"):             # a stray host read or upload fails the capture
            outs = step()
        seen = set()
        for name in seq:
            c = MC.CASES[name]
            for dst, src in zip(st, _dev(c, dev)):
                dst.copy_(src)
            g.copy_(c.g.to(dev))
            graph.replay()
            torch.cuda.synchronize()
            got = [o.clone() for o in outs]
            eager = step()
            torch.cuda.synchronize()
            for a, b in zip(got, eager):
                assert _same(a, b), name
            MC.check_value(c, got[0].cpu(), got[1].cpu().tolist(), "replay")
            MC.check_grads(c, [x.cpu() for x in got[2:]], "replay")
            seen.add(tuple(int(v > 0) for v in got[1].cpu().tolist()))
        assert seen == {(1, 1), (1, 0), (0, 1), (0, 0)}                         # both sets were emptied and refilled


def test_refusals_return_their_codes_and_launch_nothing(dev):
    import hdn_amd
    from hdn_amd import _lib as L
    c = MC.CASES["f_3x3x65_alternating_r0"]
    t = _dev(c, dev)
    lib = L.load()
    partial, out = torch.full((c.N * c.R,), -5.0, device=dev), torch.full((1,), -5.0, device=dev)
    counts = torch.full((2,), -7, dtype=torch.int32, device=dev)
    gr = [torch.full(c.a.shape, -5.0, device=dev) for _ in range(3)]
    g = c.g.to(dev)
    p = [L.ptr(v) for v in t]
    o = [L.ptr(partial), L.ptr(out), L.ptr(counts)]
    dims, tail = (c.N, c.R, c.D), (c.denom, c.margin, c.eps, None)
    f, b = lib.hdn_triplet_l1_mean_f32, lib.hdn_triplet_l1_mean_bwd_f32
    for i in range(5):
        q = list(p)
        q[i] = None
        assert f(*q, *o, *dims, 0, *tail) == E_NULL and b(*q, L.ptr(g), *[L.ptr(x) for x in gr], *dims, 0, *tail) == E_NULL
    assert f(*p, None, o[1], o[2], *dims, 0, *tail) == E_NULL and b(*p, None, *[L.ptr(x) for x in gr], *dims, 0, *tail) == E_NULL
    for rule in (2, -1):
        assert f(*p, *o, *dims, rule, *tail) == E_SHAPE and b(*p, L.ptr(g), *[L.ptr(x) for x in gr], *dims, rule, *tail) == E_SHAPE
    assert f(*p, *o, 0, c.R, c.D, 0, *tail) == E_SHAPE and b(*p, L.ptr(g), None, None, None, *dims, 0, *tail) == E_SHAPE
    assert f(*p, *o, 65537, c.R, c.D, 0, *tail) == E_LIMIT and b(*p, L.ptr(g), *[L.ptr(x) for x in gr], 65537, c.R, c.D, 0, *tail) == E_LIMIT
    assert f(*p, p[0], o[1], o[2], *dims, 0, *tail) == E_ALIAS and f(*p, o[0], o[1], p[3], *dims, 0, *tail) == E_ALIAS
    assert b(*p, L.ptr(g), p[1], None, None, *dims, 0, *tail) == E_ALIAS and b(*p, L.ptr(g), L.ptr(gr[0]), L.ptr(gr[0]), None, *dims, 0, *tail) == E_ALIAS
    torch.cuda.synchronize()
    assert all(bool((x == -5).all()) for x in [partial, out, *gr]) and bool((counts == -7).all())    # nothing was launched
    with pytest.raises(ValueError, match="HDN_E_LIMIT"):
        z = torch.zeros(65537, 1, 1, device=dev)
        hdn_amd.triplet_l1_mean(z, z, z, torch.ones(65537, device=dev), torch.ones(65537, device=dev), 0)
    with pytest.raises(L.HdnHipError):
        hdn_amd.triplet_l1_mean(t[0], t[1], t[2], t[3].cpu(), t[4], 0)                                # a flag on the host is not uploaded
    with pytest.raises(ValueError, match="rule"):
        hdn_amd.triplet_l1_mean(*t, 2)
