"""hdn_head_tail_batch_f32 (csrc/head_tail.hip; hdn_amd.heads.head_tail_batch) on the GPU: exact addressing at every tile and edge situation, float64
parity at PyTorch's own fp32 error, batch invariance against hdn_head_tail_f32 bit for bit, the range guard, and the place hdn_amd.heads uses it behind
HDN_HIP_HEADS=2 / head._hdn_hip_heads = 2 (everything behind the correlations at B > 1): parity through both heads with the launches counted, the
packed head's cache semantics, and a hipGraph of both heads."""
import copy
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import head_batch_cases as HB
import head_tail_batch_cases as HT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _packed(w1, b1, wf, bf, oc, ol, dev):
    """A _PackedHead with what head_tail / head_tail_batch read."""
    from hdn_amd import heads as HD
    pk = HD._PackedHead()
    pk.w1, pk.b1, pk.wf, pk.bf = (t.float().to(dev).contiguous() for t in (w1, b1, wf, bf))
    pk.oc, pk.ol, pk.hidden = oc, ol, w1.shape[1]
    pk.w1p = HD._pack_w1(pk.w1)
    return pk


def _run(feats, pk, n, B, Ho=None):
    """head_tail_batch on feats [2n, B, H, P] (as [2n, B, H, Ho, P / Ho]) -> (cls [B, oc, P], loc [B, ol, P])."""
    from hdn_amd import heads as HD
    G, _, H, P = feats.shape
    Ho = Ho or 1
    c, l = HD.head_tail_batch(feats.view(G, B, H, Ho, P // Ho), pk, n, B)
    assert c.shape == (B, pk.oc, Ho, P // Ho) and l.shape == (B, pk.ol, Ho, P // Ho) and c.is_contiguous() and l.is_contiguous()
    assert c.untyped_storage().data_ptr() == l.untyped_storage().data_ptr() and l.data_ptr() == c.data_ptr() + 4 * c.numel()      # one buffer
    return c.view(B, pk.oc, P), l.view(B, pk.ol, P)


# ----------------------------------------------------------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("case", HT.CASES, ids=HT.case_id)
def test_addressing_is_exact(dev, case):
    """Integer feats with another code per image, group and level, one-hot w1 with another column per group, +-1 wf: cls / loc == the integer
    expectation by torch.equal - a wrong image or group pointer, row block or pixel tile fails, and the first wrong (branch, image, row, pixel) is named."""
    H, P, n, oc, ol, B = case
    feats, w1, b1, wf, bf, want = HT.exact_case(*case)
    pk = _packed(w1, b1, wf, bf, oc, ol, dev)
    Ho = next(d for d in (31, 25, 13, 8, 5, 1) if P % d == 0)                  # (any [Ho, Wo] with Ho Wo = P: the kernel sees pixels)
    got = _run(feats.float().to(dev), pk, n, B, Ho)
    for br, name in enumerate(("cls", "loc")):
        msg = HT.first_difference(got[br].cpu(), want[br].float())
        assert msg is None, f"head tail batch {case} branch {br} ({name}): {msg}"


# ----------------------------------------------------------------------------------------------------------------- 2 / 3. float64, invariance
_RUNS = {}


def _random_run(case, dev):
    """The random data of a case, its packed weights and its batched result (computed once)."""
    if case not in _RUNS:
        H, P, n, oc, ol, B = case
        data = HT.random_case(H, P, n, oc, ol, B, seed=H + 7 * P + B)
        pk = _packed(*data[1:], oc, ol, dev)
        fd = data[0].to(dev)
        _RUNS[case] = (data, pk, fd, _run(fd, pk, n, B))
    return _RUNS[case]


def _check_f64(got, data, oc, ol, what):
    """got (cls [B, oc, P], loc [B, ol, P]) float64 on the CPU: per image and branch err <= 4 e_ref + 1e-6 scale, e_ref = PyTorch-CPU fp32 on the same
    two products (the bound of test_head_tail_one_launch_vs_float64)."""
    ref = HT.tail(*(t.double() for t in data))
    ref32 = HT.tail(*data).double()
    for b in range(ref.shape[0]):
        for br, rows in enumerate((oc, ol)):
            r, r32 = ref[b, br, :rows], ref32[b, br, :rows]
            e_ref, scale, err = float((r32 - r).abs().max()), float(r.abs().max()), float((got[br][b] - r).abs().max())
            print(f"{what} image {b} branch {br}: err {err:.3e}  e_ref {e_ref:.3e}  scale {scale:.3e}")
            assert err <= 4 * e_ref + 1e-6 * scale, (what, b, br, err, e_ref, scale)


@pytest.mark.parametrize("case", HT.CASES, ids=HT.case_id)
def test_against_float64_and_deterministic(dev, case):
    H, P, n, oc, ol, B = case
    data, pk, fd, got = _random_run(case, dev)
    _check_f64([g.cpu().double() for g in got], data, oc, ol, f"head tail batch {case}")
    again = _run(fd, pk, n, B)                                                 # run twice: bit-equal
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


@pytest.mark.parametrize("case", HT.CASES, ids=HT.case_id)
def test_batch_invariance_against_the_single_image_entry(dev, case):
    """Image b of the batched result is bit-equal to hdn_head_tail_f32 (head_tail) on feats[:, b] alone: the written rows where oc != ol, and at
    B = 1 with oc == ol the old entry's whole [2, n_out, P] buffer."""
    from hdn_amd import heads as HD
    H, P, n, oc, ol, B = case
    data, pk, fd, got = _random_run(case, dev)
    for b in range(B):
        one = HD.head_tail(fd[:, b].contiguous().view(2 * n, H, P, 1), pk, n)                   # [2, om, P]
        for br, rows in enumerate((oc, ol)):
            msg = HT.first_difference(got[br][b].cpu(), one[br, :rows].cpu(), "(row, pixel)")
            assert msg is None, f"{case} image {b} branch {br}: {msg}"


def test_one_image_with_equal_out_counts_is_the_old_entrys_buffer(dev):
    from hdn_amd import heads as HD
    H, P, n, oc, B = 256, 64, 2, 4, 1
    data = HT.random_case(H, P, n, oc, oc, B, seed=99)
    pk = _packed(*data[1:], oc, oc, dev)
    fd = data[0].to(dev)
    c, l = _run(fd, pk, n, B)
    one = HD.head_tail(fd[:, 0].contiguous().view(2 * n, H, P, 1), pk, n)
    whole = torch.as_strided(c, (2, oc, P), (oc * P, P, 1))                    # cls and loc are adjacent in one buffer: [2, n_out, P]
    assert torch.equal(whole, one)


# ----------------------------------------------------------------------------------------------------------------- 4. range
def test_range(dev):
    """One element of 1e7 (inside the two-piece format's 1.67e7) in the LAST image: finite and inside the float64 bound; 2e7 with the guard on is
    refused with HDN_E_LIMIT whichever image holds it (the guard looks at all images of all groups)."""
    from hdn_amd import _lib
    H, P, n, oc, ol, B = 128, 40, 2, 2, 4, 3
    data = list(HT.random_case(H, P, n, oc, ol, B, seed=77))
    pk = _packed(*data[1:], oc, ol, dev)
    data[0][3, B - 1, 100, 39] = 1.0e7
    got = _run(data[0].to(dev), pk, n, B)
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
    _check_f64([g.cpu().double() for g in got], data, oc, ol, "1e7")
    lib = _lib.load()
    prev = lib.hdn_set_check_range(1)
    try:
        data[0][3, B - 1, 100, 39] = 1.0
        assert torch.isfinite(_run(data[0].to(dev), pk, n, B)[0]).all()        # the guard passes data in range
        for g, b in ((0, 0), (1, 1), (3, B - 1)):
            bad = data[0].clone()
            bad[g, b, 5, 7] = 2.0e7
            with pytest.raises(ValueError, match="HDN_E_LIMIT"):
                _run(bad.to(dev), pk, n, B)
    finally:
        lib.hdn_set_check_range(prev)


# ----------------------------------------------------------------------------------------------------------------- 5. through the heads
class _Spies:
    """Counts what a forward launches: the correlation launch (with its outs), head_tail_batch, _packed_forward and the Conv2d modules of the `head`
    Sequentials (forward hooks)."""

    def __init__(self, monkeypatch, head):
        from hdn_amd import heads as HD
        self.xcorr, self.tail, self.packed, self.head_convs = [], [], [], []
        real_x, real_t, real_p = HD.xcorr_depthwise_multi, HD.head_tail_batch, HD._packed_forward

        def xcorr(srch, kern, **kw):
            self.xcorr.append((list(srch), list(kern), kw.get("outs")))
            return real_x(srch, kern, **kw)

        def tail(feats, pk, n, B):
            self.tail.append((tuple(feats.shape), B))
            return real_t(feats, pk, n, B)

        def packed(*a, **k):
            self.packed.append(1)
            return real_p(*a, **k)
        monkeypatch.setattr(HD, "xcorr_depthwise_multi", xcorr)
        monkeypatch.setattr(HD, "head_tail_batch", tail)
        monkeypatch.setattr(HD, "_packed_forward", packed)
        self.hooks = [m.register_forward_hook(lambda mod, i, o: self.head_convs.append(mod))
                      for box in (head.box2, head.box3, head.box4) for br in (box.cls, box.loc) for m in br.head if isinstance(m, nn.Conv2d)]
        assert len(self.hooks) == 12

    def remove(self):
        for h in self.hooks:
            h.remove()


def _oracle(m, z, x, circular):
    """(float64 forward, fp32 forward) of the modules' present state on the CPU (oracle.multi_ban on the deep-copied state)."""
    from oracle import hdn_oracle as O
    cpu = copy.deepcopy(m).cpu()
    sd64 = {k: v.detach().clone() for k, v in copy.deepcopy(cpu).double().state_dict().items()}
    sd32 = {k: v.detach().clone() for k, v in cpu.state_dict().items()}
    with torch.no_grad():
        return (O.multi_ban([t.double() for t in z], [t.double() for t in x], sd64, circular), O.multi_ban(z, x, sd32, circular))


def _check_heads(got, ref, ref32, what):
    """err <= 4 e_ref + 1e-5 scale, the bound of test_through_the_heads (tests/test_gpu_head_batch.py) for the multi-layer chain."""
    for name, g, r, r32 in zip(("cls", "loc"), got, ref, ref32):
        g = g.cpu().double()
        assert g.shape == r.shape
        e_ref, scale, err = float((r32.double() - r).abs().max()), float(r.abs().max()), float((g - r).abs().max())
        print(f"{what} {name}: err {err:.3e}  e_ref {e_ref:.3e}  scale {scale:.3e}")
        assert err <= 4 * e_ref + 1e-5 * scale, (what, name, err, e_ref, scale)


_HEADS = {}


def _setup(cls_name, B, dev):
    """A seeded head on the CPU, its inputs and the oracle's two forwards (computed once per head and batch, never changed)."""
    key = (cls_name, B)
    if key not in _HEADS:
        circular = cls_name == "MultiCircBAN"
        m = HB.seeded_head(cls_name)
        z, x = HB.head_inputs(circular, B, seed=5 + B)
        _HEADS[key] = (m, z, x, _oracle(m, z, x, circular))
    m, z, x, refs = _HEADS[key]
    return copy.deepcopy(m).to(dev), [t.to(dev) for t in z], [t.to(dev) for t in x], refs


@pytest.mark.parametrize("cls_name", ["MultiBAN", "MultiCircBAN"])
def test_through_the_heads_three_launches(dev, cls_name, monkeypatch):
    """B = 3 at level 2: cls / loc against the float64 oracle forward; contiguous, of the reference's shapes, views of one buffer; ONE correlation launch
    whose outs tile one buffer, ONE head_tail_batch, and no Conv2d of a `head` Sequential runs."""
    B = 3
    md, z, x, (ref, ref32) = _setup(cls_name, B, dev)
    md._hdn_hip_heads = 2
    spies = _Spies(monkeypatch, md)
    got = md(z, x)
    spies.remove()
    _check_heads(got, ref, ref32, f"{cls_name} level 2 B={B}")
    c, l = got
    assert c.is_contiguous() and l.is_contiguous() and c.shape[:2] == (B, 2) and l.shape[:2] == (B, 4 if cls_name == "MultiCircBAN" else 2)
    assert c.untyped_storage().data_ptr() == l.untyped_storage().data_ptr() and l.data_ptr() == c.data_ptr() + 4 * c.numel()
    assert len(spies.xcorr) == 1 and len(spies.tail) == 1 and not spies.packed and not spies.head_convs
    srch, kern, outs = spies.xcorr[0]
    assert outs is not None and len(outs) == len(srch) == len(kern) == 6
    assert all(o.is_contiguous() and o.shape == (B, 256) + tuple(c.shape[2:]) for o in outs)
    step = outs[0].numel() * 4
    assert [o.data_ptr() for o in outs] == [outs[0].data_ptr() + i * step for i in range(6)]          # stacked order, one buffer
    assert all(o.untyped_storage().data_ptr() == outs[0].untyped_storage().data_ptr() for o in outs)
    assert spies.tail[0] == ((6, B, 256) + tuple(c.shape[2:]), B)
    pk = md._hdn_packed_head
    assert pk is not None and pk.w1p is not None and md._hdn_search_pack.ok


@pytest.mark.parametrize("cls_name", ["MultiBAN", "MultiCircBAN"])
@pytest.mark.parametrize("how", ["level1", "no_head_tail"])
def test_level_one_and_the_opt_out_keep_the_level_one_path(dev, cls_name, how, monkeypatch):
    """_hdn_hip_heads = 1, and _hdn_no_head_tail = True at level 2: the batched tail is not reached, the `head` modules run, the same bound holds."""
    B = 3
    md, z, x, (ref, ref32) = _setup(cls_name, B, dev)
    md._hdn_hip_heads = 1 if how == "level1" else 2
    if how == "no_head_tail":
        md._hdn_no_head_tail = True
    spies = _Spies(monkeypatch, md)
    got = md(z, x)
    spies.remove()
    _check_heads(got, ref, ref32, f"{cls_name} {how} B={B}")
    assert not spies.tail and not spies.packed and len(spies.xcorr) == 1 and len(spies.head_convs) == 12
    assert md._hdn_search_pack.ok                                              # conv_search on the batched kernel, as at level 1


def test_one_image_at_level_two_takes_the_packed_forward(dev, monkeypatch):
    md, z, x, (ref, ref32) = _setup("MultiBAN", 1, dev)
    md._hdn_hip_heads = 2
    spies = _Spies(monkeypatch, md)
    got = md(z, x)
    spies.remove()
    _check_heads(got, ref, ref32, "MultiBAN level 2 B=1")
    assert len(spies.packed) == 1 and not spies.tail and not spies.head_convs


# ----------------------------------------------------------------------------------------------------------------- 6. cache semantics
def test_packed_head_follows_in_place_changes(dev, monkeypatch):
    """After an in-place change of a head[3].bias, of a head[1] running statistic or of loc_scale the next forward at level 2 re-packs and matches the
    float64 forward of the changed modules; an unchanged head keeps its pack."""
    B, cls_name = 3, "MultiCircBAN"
    md, z, x, (ref, ref32) = _setup(cls_name, B, dev)
    zc, xc = [t.cpu() for t in z], [t.cpu() for t in x]
    md._hdn_hip_heads = 2
    spies = _Spies(monkeypatch, md)
    first = [t.clone() for t in md(z, x)]
    pk = md._hdn_packed_head
    md(z, x)
    assert md._hdn_packed_head is pk and len(spies.tail) == 2                  # nothing changed: nothing re-packed
    changes = [lambda: md.box3.loc.head[3].bias.add_(0.75), lambda: md.box2.cls.head[1].running_mean.sub_(0.4),
               lambda: md.box4.cls.head[1].running_var.mul_(1.7), lambda: md.loc_scale.mul_(-1.5)]
    last = first
    for i, change in enumerate(changes):
        with torch.no_grad():
            change()
        got = md(z, x)
        assert md._hdn_packed_head is not pk and md._hdn_packed_head.w1p is not None, i
        pk = md._hdn_packed_head
        r, r32 = _oracle(md, zc, xc, True)
        _check_heads(got, r, r32, f"after change {i}")
        assert not (torch.equal(got[0], last[0]) and torch.equal(got[1], last[1])), i
        last = [t.clone() for t in got]
    spies.remove()
    assert len(spies.tail) == 2 + len(changes) and not spies.head_convs


# ----------------------------------------------------------------------------------------------------------------- 7. capture
def test_both_heads_in_one_graph(dev):
    """Both heads at B = 3, level 2, captured in one hipGraph after a warm-up forward: the replay is bit-equal to eager."""
    B = 3
    heads = [HB.seeded_head("MultiBAN", 3).to(dev), HB.seeded_head("MultiCircBAN", 4).to(dev)]
    ins = [HB.head_inputs(False, B, 31), HB.head_inputs(True, B, 32)]
    zs = [[t.to(dev) for t in z] for z, _ in ins]
    xs = [[t.to(dev) for t in x] for _, x in ins]
    nxt = [[t.to(dev) for t in HB.head_inputs(c, B, s)[1]] for c, s in ((False, 41), (True, 42))]
    for h in heads:
        h._hdn_hip_heads = 2

    def frame():
        return [h(z, x) for h, z, x in zip(heads, zs, xs)]

    eager0 = [[o.clone() for o in pair] for pair in frame()]                   # (also the warm-up: template cache and packs)
    for x, other in zip(xs, nxt):
        for a, b in zip(x, other):
            a.copy_(b)
    eager1 = [[o.clone() for o in pair] for pair in frame()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        frame()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = frame()
    g.replay()
    torch.cuda.synchronize()
    for pair, want in zip(outs, eager1):
        for o, w in zip(pair, want):
            assert torch.equal(o, w), float((o - w).abs().max())
    for x, (_, first) in zip(xs, ins):                                         # the first search features again, through the same graph
        for a, b in zip(x, first):
            a.copy_(b.to(dev))
    g.replay()
    torch.cuda.synchronize()
    for pair, want in zip(outs, eager0):
        for o, w in zip(pair, want):
            assert torch.equal(o, w), float((o - w).abs().max())
    assert not torch.equal(eager0[0][0], eager1[0][0])
