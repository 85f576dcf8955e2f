"""hdn_head_conv3x3_batch_f32 (csrc/head_conv.hip; hdn_amd.heads.head_conv_batch) on the GPU: exact addressing at every tile and edge situation,
float64 parity at PyTorch's own fp32 error, batch invariance against hdn_head_conv3x3_f32 bit for bit, the range guard, and the two places
hdn_amd.heads uses it behind HDN_HIP_HEADS / head._hdn_hip_heads (the template branch at any batch, conv_search at B > 1): parity through the
heads, the template cache's semantics, and a hipGraph that refreshes the template in place."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import head_batch_cases as HB

pytestmark = pytest.mark.gpu
CL = torch.channels_last


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _to(x, dev, nhwc):
    x = x.float().to(dev)
    return x.contiguous(memory_format=CL) if nhwc else x


def _pack(ws, bs, dev):
    from hdn_amd import heads as HD
    return HD._pack_conv_search([w.to(dev) for w in ws]), (bs if torch.is_tensor(bs) else torch.stack(bs)).float().to(dev)


def _by_image(y):
    """[n, groups, B, CG, Ho, Wo] -> [n, B, CO, Ho, Wo]."""
    n, G, B, CG, Ho, Wo = y.shape
    return y.permute(0, 2, 1, 3, 4, 5).reshape(n, B, G * CG, Ho, Wo)


# ----------------------------------------------------------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("case", HB.CASES, ids=HB.case_id)
def test_addressing_is_exact(dev, case):
    """Integer data in [0, 15], one-hot weights with another (channel, tap) code per level, integer bias: out == relu(x[b, src, y + ky, x + kx] + bias)
    on every image, by torch.equal - a wrong group offset, batch stride, image-to-tile map or level pointer fails."""
    from hdn_amd import heads as HD
    Hi, Wi, n, B, CO, groups, nhwc = case
    xs, ws, bs, want = HB.exact_case(Hi, Wi, n, B, CO)
    wsp, bsp = _pack(ws, bs, dev)
    got = HD.head_conv_batch([_to(x, dev, nhwc) for x in xs], wsp, bsp, groups=groups)
    assert got.shape == (n, groups, B, CO // groups, Hi - 2, Wi - 2) and got.is_contiguous()
    msg = HB.first_difference(_by_image(got).cpu(), want.float())
    assert msg is None, f"head conv batch {case}: {msg}"


@pytest.mark.parametrize("nhwc", [False, True])
def test_batch_slice_of_a_larger_tensor_is_read_in_place(dev, nhwc, monkeypatch):
    """Inputs t[1:3] of 4-image tensors (level 1 at another offset of its parent): exact, and the kernel got the views' own addresses and the
    parents' batch stride - no copy."""
    from hdn_amd import _lib, heads as HD
    Hi, Wi, n, CO = 7, 7, 2, 64
    xs4, ws, bs, want4 = HB.exact_case(Hi, Wi, n, 4, CO)
    wsp, bsp = _pack(ws, bs, dev)
    parents = [_to(x, dev, nhwc) for x in xs4]
    views = [p[1:3] for p in parents]
    lib, seen = _lib.load(), {}
    real = lib.hdn_head_conv3x3_batch_f32

    def spy(xs, w, b, out, n_, B_, g_, CO_, Hi_, Wi_, nhwc_, xbs, stream):
        seen.update(ptrs=[xs[i] for i in range(n_)], xbs=xbs, nhwc=nhwc_, B=B_)
        return real(xs, w, b, out, n_, B_, g_, CO_, Hi_, Wi_, nhwc_, xbs, stream)
    monkeypatch.setattr(lib, "hdn_head_conv3x3_batch_f32", spy)
    got = HD.head_conv_batch(views, wsp, bsp, groups=2)
    assert seen["ptrs"] == [v.data_ptr() for v in views] and seen["xbs"] == 256 * Hi * Wi and seen["nhwc"] == int(nhwc) and seen["B"] == 2
    msg = HB.first_difference(_by_image(got).cpu(), want4[:, 1:3].float())
    assert msg is None, msg
    # every second image: batch stride 2 images
    got = HD.head_conv_batch([p[::2] for p in parents], wsp, bsp, groups=1)
    assert seen["xbs"] == 2 * 256 * Hi * Wi and seen["ptrs"] == [p.data_ptr() for p in parents]
    msg = HB.first_difference(_by_image(got).cpu(), want4[:, ::2].float())
    assert msg is None, msg


# ----------------------------------------------------------------------------------------------------------------- 2 / 3. float64, invariance
_RUNS = {}


def _random_run(case, dev):
    """The random data of a case, its batched result (computed once) and the packed weights."""
    from hdn_amd import heads as HD
    if case not in _RUNS:
        Hi, Wi, n, B, CO, groups, nhwc = case
        xs, ws, bs = HB.random_case(Hi, Wi, n, B, CO, seed=Hi * 1000 + Wi * 10 + B + CO)
        wsp, bsp = _pack(ws, bs, dev)
        xd = [_to(x, dev, nhwc) for x in xs]
        got = HD.head_conv_batch(xd, wsp, bsp, groups=groups)
        _RUNS[case] = (xs, ws, bs, xd, wsp, bsp, got)
    return _RUNS[case]


def _check_f64(got, xs, ws, bs, what, rel=1e-6):
    """got [n, B, CO, Ho, Wo] (float64, CPU): per image and level err <= 4 e_ref + rel scale, e_ref = PyTorch-CPU fp32 on the same convolution."""
    for i in range(len(xs)):
        ref = HB.conv_relu(xs[i].double(), ws[i].double(), bs[i].double())
        ref32 = HB.conv_relu(xs[i], ws[i], bs[i]).double()
        for b in range(xs[i].shape[0]):
            e_ref, scale = float((ref32[b] - ref[b]).abs().max()), float(ref[b].abs().max())
            err = float((got[i, b] - ref[b]).abs().max())
            print(f"{what} level {i} image {b}: err {err:.3e}  e_ref {e_ref:.3e}  scale {scale:.3e}")
            assert err <= 4 * e_ref + rel * scale, (what, i, b, err, e_ref, scale)


@pytest.mark.parametrize("case", HB.CASES, ids=HB.case_id)
def test_against_float64_and_deterministic(dev, case):
    from hdn_amd import heads as HD
    xs, ws, bs, xd, wsp, bsp, got = _random_run(case, dev)
    _check_f64(_by_image(got).cpu().double(), xs, ws, bs, f"head conv batch {case}")
    assert torch.equal(HD.head_conv_batch(xd, wsp, bsp, groups=case[5]), got)          # run twice: bit-equal


@pytest.mark.parametrize("case", HB.CASES, ids=HB.case_id)
def test_batch_invariance_against_the_single_image_entry(dev, case):
    """Image b of the batched result is bit-equal to hdn_head_conv3x3_f32 (head_conv_search) on that image alone."""
    from hdn_amd import heads as HD
    xs, ws, bs, xd, wsp, bsp, got = _random_run(case, dev)
    pk = HD._PackedHead()
    pk.wsp, pk.bsp = wsp, bsp
    got = _by_image(got)
    for b in range(case[3]):
        one = HD.head_conv_search([x[b:b + 1] for x in xd], pk)                          # [n, CO, Ho, Wo]
        msg = HB.first_difference(got[:, b].cpu(), one.cpu(), "(level, channel, y, x)")
        assert msg is None, f"{case} image {b}: {msg}"


# ----------------------------------------------------------------------------------------------------------------- 4. range
def test_range(dev):
    """One element of 1e7 (inside the two-piece format's 1.67e7) in the LAST image: finite and inside the float64 bound; 2e7 with the guard on is
    refused with HDN_E_LIMIT, in a dense batch and in a batch slice (the guard looks at every image)."""
    from hdn_amd import _lib, heads as HD
    Hi, Wi, n, B, CO = 9, 14, 1, 2, 64
    xs, ws, bs = HB.random_case(Hi, Wi, n, B, CO, seed=77)
    wsp, bsp = _pack(ws, bs, dev)
    xs[0][1, 200, 8, 13] = 1.0e7
    got = HD.head_conv_batch([xs[0].to(dev)], wsp, bsp)
    assert torch.isfinite(got).all()
    _check_f64(_by_image(got).cpu().double(), xs, ws, bs, "1e7")
    lib = _lib.load()
    prev = lib.hdn_set_check_range(1)
    try:
        xs[0][1, 200, 8, 13] = 2.0e7
        with pytest.raises(ValueError, match="HDN_E_LIMIT"):
            HD.head_conv_batch([xs[0].to(dev)], wsp, bsp)
        four = torch.cat([xs[0], xs[0]]).to(dev)                                         # images 1 and 3 hold the element
        with pytest.raises(ValueError, match="HDN_E_LIMIT"):
            HD.head_conv_batch([four[1::2]], wsp, bsp)
        assert torch.isfinite(HD.head_conv_batch([four[::2]], wsp, bsp)).all()           # images 0 and 2 do not
    finally:
        lib.hdn_set_check_range(prev)


# ----------------------------------------------------------------------------------------------------------------- 5. through the heads
def _spy_xcorr(monkeypatch):
    from hdn_amd import heads as HD
    calls, real = [], HD.xcorr_depthwise_multi

    def spy(srch, kern, **kw):
        calls.append((list(srch), list(kern)))
        return real(srch, kern, **kw)
    monkeypatch.setattr(HD, "xcorr_depthwise_multi", spy)
    return calls


def _one_buffer(ts):
    """The tensors are contiguous and tile ONE buffer back to back (views of one launch's output: no copy was made)."""
    assert all(t.is_contiguous() for t in ts)
    ptrs = sorted(t.data_ptr() for t in ts)
    step = ts[0].numel() * 4
    assert ptrs == [ptrs[0] + i * step for i in range(len(ts))], [p - ptrs[0] for p in ptrs]
    assert all(t.untyped_storage().data_ptr() == ts[0].untyped_storage().data_ptr() for t in ts)


@pytest.mark.parametrize("cls_name,B,packed", [("MultiBAN", 1, True), ("MultiBAN", 1, False), ("MultiBAN", 3, None),
                                               ("MultiCircBAN", 1, True), ("MultiCircBAN", 1, False), ("MultiCircBAN", 3, None)])
def test_through_the_heads(dev, cls_name, B, packed, monkeypatch):
    """cls / loc of a seeded head with the switch on against the float64 CPU forward of the same modules (oracle.multi_ban on the deep-copied
    .double() state), err <= 4 e_ref + 1e-5 scale with e_ref from the fp32 CPU forward: the project's bound for multi-layer chains.  The template
    tensors handed to the correlation launch are views of one buffer; at B > 1 so are the search tensors."""
    from oracle import hdn_oracle as O
    circular = cls_name == "MultiCircBAN"
    m = HB.seeded_head(cls_name)
    z, x = HB.head_inputs(circular, B, seed=5 + B)
    sd64 = {k: v.detach().clone() for k, v in copy.deepcopy(m).double().state_dict().items()}
    sd32 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref = O.multi_ban([t.double() for t in z], [t.double() for t in x], sd64, circular)
        ref32 = O.multi_ban(z, x, sd32, circular)
    md = m.to(dev)
    md._hdn_hip_heads = True
    if packed is False:
        md._hdn_no_packed_head = True
    calls = _spy_xcorr(monkeypatch)
    got = md([t.to(dev) for t in z], [t.to(dev) for t in x])
    assert len(calls) == 1
    srch, kern = calls[0]
    assert len(kern) == 6 and all(k.shape == (B, 256, kern[0].shape[2], kern[0].shape[3]) for k in kern)
    _one_buffer(kern)
    assert md._hdn_template_pack is not None and md._hdn_template_pack.ok
    if B > 1:
        _one_buffer(srch)
        assert md._hdn_search_pack is not None and md._hdn_search_pack.ok
    if packed:
        assert getattr(md, "_hdn_packed_head", None) is not None
    for name, g, r, r32 in zip(("cls", "loc"), got, ref, ref32):
        g = g.cpu().double()
        assert g.shape == r.shape
        e_ref, scale, err = float((r32.double() - r).abs().max()), float(r.abs().max()), float((g - r).abs().max())
        print(f"{cls_name} B={B} packed={packed} {name}: err {err:.3e}  e_ref {e_ref:.3e}  scale {scale:.3e}")
        assert err <= 4 * e_ref + 1e-5 * scale, (name, err, e_ref, scale)


# ----------------------------------------------------------------------------------------------------------------- 5b. predicates and packs
# What the parent of the heads' untangling answered (head_batch_cases.stage_case, hidden 32, [B, 256, 5, 5]); the only launches are the packers' uploads.
# _packable_any_batch asks for the module layout and one shape, nothing of channel counts, levels or the patch: those are _search_pack's.  (hidden48: the
# pack is built, 2 x 48 = 96 channels being a multiple of 32, although the kernel wants each half tile-aligned: characterised here, not endorsed.)
LAYOUT_REFUSED = {"bias", "stride2", "padding1", "dilation2", "groups2", "bn_training", "bn_not_affine", "bn_no_running_stats", "identity", "length4"}
SEARCH_PACKABLE = {name: name not in LAYOUT_REFUSED | {"two_shapes"} for name in HB.STAGE_CASES}
SEARCH_PACK = {name: name in ("reference", "hidden48", "side17") for name in HB.STAGE_CASES}
TEMPLATE_PACK = {name: name in ("reference", "side17") for name in HB.STAGE_CASES}


def _rehead(hd, i, **kw):
    c = hd[i]
    hd[i] = torch.nn.Conv2d(c.in_channels, c.out_channels, **{"kernel_size": 1, "bias": c.bias is not None, **kw})


# one mutation of box2.loc's 1x1 head each (a Sequential(Conv2d, BatchNorm2d, ReLU, Conv2d with bias))
HEAD_MUTATIONS = {
    "bias0": lambda hd: _rehead(hd, 0, bias=True),
    "kernel0": lambda hd: _rehead(hd, 0, kernel_size=3, padding=1),
    "bn_training": lambda hd: hd[1].train(),
    "bn_not_affine": lambda hd: hd.__setitem__(1, torch.nn.BatchNorm2d(hd[1].num_features, affine=False).eval()),
    "bn_no_running_stats": lambda hd: hd.__setitem__(1, torch.nn.BatchNorm2d(hd[1].num_features, track_running_stats=False).eval()),
    "identity": lambda hd: hd.__setitem__(2, torch.nn.Identity()),
    "length5": lambda hd: hd.append(torch.nn.Identity()),
    "no_bias3": lambda hd: _rehead(hd, 3, bias=False),
    "kernel3": lambda hd: _rehead(hd, 3, kernel_size=3, padding=1),
}


@pytest.mark.parametrize("B", [1, 2])
def test_search_predicates_and_pack_truth_table(dev, B):
    from hdn_amd import heads as HD
    assert list(SEARCH_PACKABLE) == HB.STAGE_CASES
    any_batch, b1, pack = {}, {}, {}
    with torch.no_grad():
        for name in HB.STAGE_CASES:
            m, boxes, x = HB.stage_case(name, "conv_search", B=B, dev=dev)
            any_batch[name], b1[name] = HD._packable_any_batch(m, boxes, x), HD._packable(m, boxes, x)
            pack[name] = HD._search_pack(m, boxes, x) is not None
            assert (getattr(m._hdn_search_pack, "wsp", None) is not None) == m._hdn_search_pack.ok == pack[name], name
        for name, mutate in HEAD_MUTATIONS.items():
            m, boxes, x = HB.stage_case("reference", "conv_search", B=B, dev="cpu")
            mutate(m.box2.loc.head)
            m, x = m.to(dev), [t.to(dev) for t in x]
            got = HD._packable_any_batch(m, boxes, x), HD._packable(m, boxes, x), HD._search_pack(m, boxes, x)
            assert got == (False, False, None), (name, got)
    assert any_batch == SEARCH_PACKABLE
    assert b1 == {name: ok and B == 1 for name, ok in SEARCH_PACKABLE.items()}
    assert pack == SEARCH_PACK


def test_template_pack_truth_table(dev):
    from hdn_amd import heads as HD
    got = {}
    with torch.no_grad():
        for name in HB.STAGE_CASES:
            m, boxes, z = HB.stage_case(name, "conv_kernel", B=2, dev=dev)
            got[name] = HD._template_pack(m, boxes, [br for box in boxes for br in (box.cls, box.loc)], z) is not None
            assert (getattr(m._hdn_template_pack, "wsp", None) is not None) == m._hdn_template_pack.ok == got[name], name
    assert got == TEMPLATE_PACK


def test_pack_keys_follow_in_place_weight_updates(dev):
    """Each pack is kept while its own side's tensors stand and rebuilt, under another key, after an in-place update of one of them."""
    from hdn_amd import heads as HD
    m, boxes, x = HB.stage_case("reference", "conv_search", B=2, dev=dev)
    branches = [br for box in boxes for br in (box.cls, box.loc)]
    with torch.no_grad():
        sp, tp = HD._search_pack(m, boxes, x), HD._template_pack(m, boxes, branches, x)
        assert HD._search_pack(m, boxes, x) is sp and HD._template_pack(m, boxes, branches, x) is tp
        m.box2.loc.conv_kernel[0].weight.mul_(0.5)                                       # the template side only
        tp2 = HD._template_pack(m, boxes, branches, x)
        assert tp2 is not tp and tp2.key != tp.key and tp2.ok and not torch.equal(tp2.ws[0], tp.ws[0])
        assert HD._search_pack(m, boxes, x) is sp
        m.box2.cls.conv_search[1].running_var.add_(0.25)                                 # the search side only: a BatchNorm buffer counts
        sp2 = HD._search_pack(m, boxes, x)
        assert sp2 is not sp and sp2.key != sp.key and sp2.ok and not torch.equal(sp2.ws[0], sp.ws[0])
        assert HD._template_pack(m, boxes, branches, x) is tp2
        m.loc_scale.mul_(2.0)                                                            # the head's own parameters are in the search pack's key
        assert HD._search_pack(m, boxes, x) is not sp2 and HD._template_pack(m, boxes, branches, x) is tp2


# ----------------------------------------------------------------------------------------------------------------- 6. cache semantics
def test_template_cache_semantics_with_the_switch_on(dev, monkeypatch):
    from hdn_amd import heads as HD
    m = HB.seeded_head("MultiBAN").to(dev)
    m._hdn_hip_heads = True
    z, x = HB.head_inputs(False, 1, seed=21)
    z2, _ = HB.head_inputs(False, 1, seed=22)
    z, x, z2 = [t.to(dev) for t in z], [t.to(dev) for t in x], [t.to(dev) for t in z2]
    launches, real = [], HD.head_conv_batch

    def counted(x_fs, *a, **k):
        launches.append(tuple(x_fs[0].shape))
        return real(x_fs, *a, **k)
    monkeypatch.setattr(HD, "head_conv_batch", counted)

    def fresh_kernels(head, zz):
        f = copy.deepcopy(head)
        HD.invalidate_template_cache(f)
        f._hdn_hip_heads = True
        f([t.clone() for t in zz], x)
        return f._hdn_template_cache.kern

    out1 = m(z, x)
    assert launches == [(1, 256, 7, 7)]                                                  # one launch for the 6 template convolutions
    cache, pack, p0 = m._hdn_template_cache, m._hdn_template_pack, m._hdn_template_cache.kern[0].data_ptr()
    out2 = m(z, x)                                                                       # the same template: nothing new
    assert len(launches) == 1 and m._hdn_template_cache is cache and cache.kern[0].data_ptr() == p0
    assert torch.equal(out1[0], out2[0]) and torch.equal(out1[1], out2[1])
    for a, b in zip(z, z2):                                                              # an in-place refresh is a new template
        a.copy_(b)
    m(z, x)
    assert len(launches) == 2 and m._hdn_template_cache is not cache and m._hdn_template_pack is pack
    n0 = len(launches)
    want = fresh_kernels(m, z2)
    del launches[n0:]
    assert all(torch.equal(a, b) for a, b in zip(m._hdn_template_cache.kern, want))
    sd = {k: v.clone() for k, v in m.state_dict().items()}                               # new conv_kernel weights: re-packed, and followed
    sd["box3.loc.conv_kernel.0.weight"] *= -0.5
    sd["box2.cls.conv_kernel.1.running_mean"] += 0.25
    m.load_state_dict(sd)
    before = [k.clone() for k in m._hdn_template_cache.kern]
    m(z, x)
    assert len(launches) == n0 + 1 and m._hdn_template_pack is not pack and m._hdn_template_pack.ok
    n1 = len(launches)
    want = fresh_kernels(m, z)
    del launches[n1:]
    kern = m._hdn_template_cache.kern
    assert all(torch.equal(a, b) for a, b in zip(kern, want))
    changed = [not torch.equal(a, b) for a, b in zip(kern, before)]                      # (cls, loc) per level: box2.cls and box3.loc moved
    assert changed == [True, False, False, True, False, False], changed
    with torch.no_grad():
        ref = m.box3.loc.conv_kernel(z[1])                                               # the modules' own forward with the new weights
    assert float((kern[3] - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    HD.invalidate_template_cache(m)
    assert m._hdn_template_pack is None and m._hdn_template_cache is None


# ----------------------------------------------------------------------------------------------------------------- 7. capture
def test_template_refresh_and_both_heads_in_one_graph(dev):
    """One hipGraph holding an in-place template refresh + fused_forward of both heads at B = 1, replayed with two templates: each replay is
    bit-equal to the eager result for that template."""
    heads = [HB.seeded_head("MultiBAN", 3).to(dev), HB.seeded_head("MultiCircBAN", 4).to(dev)]
    ins = [HB.head_inputs(False, 1, 31), HB.head_inputs(True, 1, 32)]
    tmpl = [[[t.to(dev) for t in HB.head_inputs(c, 1, s)[0]] for c, s in ((False, 41 + k), (True, 51 + k))] for k in range(2)]   # [template][head][level]
    zs = [[t.to(dev) for t in z] for z, _ in ins]
    xs = [[t.to(dev) for t in x] for _, x in ins]
    src = [[torch.empty_like(t) for t in z] for z in zs]
    for h in heads:
        h._hdn_hip_heads = True

    def frame():
        outs = []
        for h, z, s, x in zip(heads, zs, src, xs):
            for a, b in zip(z, s):
                a.copy_(b)                                                               # the template refresh, in place
            outs.append(h(z, x))
        return outs

    def load(k):
        for s, t in zip(src, tmpl[k]):
            for a, b in zip(s, t):
                a.copy_(b)

    eager = []
    for k in range(2):
        load(k)
        eager.append([[o.clone() for o in pair] for pair in frame()])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        frame()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = frame()
    for k in (1, 0, 1):
        load(k)
        g.replay()
        torch.cuda.synchronize()
        for hi, (pair, want) in enumerate(zip(outs, eager[k])):
            for o, w in zip(pair, want):
                assert torch.equal(o, w), (k, hi, float((o - w).abs().max()))
    assert not torch.equal(eager[0][0][0], eager[1][0][0])
