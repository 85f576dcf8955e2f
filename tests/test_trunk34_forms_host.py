"""CPU tests beside tests/test_gpu_trunk34_forms.py.  The exact addressing tests there compare kernels with expectations built by integer indexing
(tests/trunk34_forms.py); here every one of those expectations is checked, at B = 2 and the smallest shape of its kernel, against a float64
F.conv2d / max_pool2d / baddbmm with the same one-hot weights - so the tests' reference is verified independently of any kernel.  The batch
lists of the GPU tests are checked against the library's host queries as well (no kernel is launched)."""
import torch
import torch.nn.functional as F

import trunk34_forms as T
from trunk34_forms import _codes


def _same(want_int, ref64):
    assert want_int.dtype == torch.int64 and ref64.dtype == torch.float64 and tuple(want_int.shape) == tuple(ref64.shape)
    assert int(want_int.abs().max()) < 1 << 53 and bool(want_int.ne(0).any())
    assert torch.equal(want_int.double(), ref64), T.first_difference(want_int.double(), ref64)


def test_case_lists_cover_every_form():
    """The same check as the *_cases_cover_every_form tests of the GPU file, in the suite that runs without a GPU."""
    T.check_all_coverage()


def test_stride1_expectation_equals_float64_conv2d():
    """relu(pick3x3 + bias (+ residual)) == relu(conv2d(x, one-hot, bias, padding 1) (+ residual)) in float64, (S, C) = (4, 512), B = 2."""
    B, S, C = 2, 4, 512
    xi, ri, bi = _codes((B, S, S, C)), _codes((B, S, S, C), 40503, 2003, 1001), T.bias_int(C)
    w, src, tap = T.onehot3x3(C, C)
    assert int(w.sum()) == C and bool((w.flatten(1).sum(1) == 1).all()) and len(set(tap.tolist())) == 9
    raw = T.pick3x3(xi, src, tap)
    conv = F.conv2d(T.nchw(xi).double(), w.double(), bi.double(), padding=1)
    _same(torch.relu(raw + bi).permute(0, 3, 1, 2), torch.relu(conv))
    _same(torch.relu(raw + bi + ri).permute(0, 3, 1, 2), torch.relu(conv + T.nchw(ri).double()))
    assert int(xi.abs().max()) < 1 << 21 and int(ri.abs().max()) <= 1001 and int(bi.abs().max()) <= 100


def test_stride2_expectations_equal_float64_conv2d():
    """Both outputs of the stride-2 + downsample kernels: (S, CI) = (4, 256), B = 2; the downsample output keeps its negative values."""
    B, S, CI = 2, 4, 256
    xi, bi = _codes((B, 2 * S, 2 * S, CI)), T.bias_int(2 * CI)
    w, src, tap = T.onehot3x3(2 * CI, CI)
    wd, srcd = T.onehot1x1(2 * CI, CI)
    assert bool((src != srcd).any())
    _same(torch.relu(T.pick3x3(xi, src, tap, 2) + bi).permute(0, 3, 1, 2), torch.relu(F.conv2d(T.nchw(xi).double(), w.double(), bi.double(), stride=2, padding=1)))
    ds = T.pick1x1s2(xi, srcd).permute(0, 3, 1, 2)
    _same(ds, F.conv2d(T.nchw(xi).double(), wd.double(), None, stride=2))
    assert int(ds.min()) < 0


def test_stem_expectation_equals_float64_conv_and_pool():
    B = 2
    xi, bi = _codes((B, 2, 127, 127)), T.bias_int(64)
    w, ci, ky, kx = T.stem_onehot()
    assert bool((w.flatten(1).sum(1) == 1).all()) and set(ky.tolist()) == set(kx.tolist()) == set(range(7))
    # (the position repeats every 14 channels; the bias tells those channels apart)
    assert len(set(zip(ci.tolist(), ky.tolist(), kx.tolist(), bi.tolist()))) == 64
    ref = F.max_pool2d(torch.relu(F.conv2d(xi.double(), w.double(), bi.double(), stride=2, padding=3)), 3, 2, 1)
    want = T.stem_expected(xi, ci, ky, kx, bi)
    assert tuple(want.shape) == (B, 64, 32, 32)
    _same(want, ref)


def test_head_conv_expectation_equals_float64_conv2d():
    Hi, Wi, n, CO = 9, 14, 2, 64
    xs, ws, bs, want = T.head_conv_case(Hi, Wi, n, CO)
    assert not torch.equal(ws[0], ws[1]) and not torch.equal(xs[0], xs[1]) and not torch.equal(bs[0], bs[1])
    ref = torch.stack([torch.relu(F.conv2d(xs[l].double(), ws[l].double(), bs[l].double()))[0] for l in range(n)])
    _same(want, ref)


def test_head_tail_expectation_equals_float64_baddbmm():
    H, P, n, om = 128, 7, 2, 8
    feats, w1, b1, wf, bf, want = T.head_tail_case(H, P, n, om)
    assert bool((w1.sum(2) == 1).all()) and bool((wf.abs().sum(2) == 8).all()) and set(wf.unique().tolist()) == {-1.0, 0.0, 1.0}
    hid = torch.baddbmm(b1.double(), w1.double(), feats.double()).relu()
    _same(want, torch.baddbmm(bf.double(), wf.double(), hid.view(2, n * H, P)))
    assert int(hid.max()) * 8 + 20 < 1 << 24


def test_chained_expectations_equal_float64_conv2d():
    """Every intermediate of the two chained cases, (S, C) = (4, 512) and (S, CI) = (4, 256) at B = 2, against float64 convolutions."""
    f = lambda t: T.nchw(t).double()
    p = lambda t: t.permute(0, 3, 1, 2)
    conv = lambda x, w, **kw: F.conv2d(x, w.double(), None, **kw)
    bv = lambda b: b.double().view(1, -1, 1, 1)
    c = T.chain1_case(2, 4, 512)
    raw0 = conv(f(c["xi"]), c["w"][0], padding=1)
    a = torch.relu(raw0 + bv(c["b"][0]) + f(c["ri"]))
    raw1 = conv(a, c["w"][1], padding=1)
    for name, ref in (("raw0", raw0), ("a", a), ("raw1", raw1), ("out", torch.relu(raw1 + bv(c["b"][1]) + a))):
        _same(p(c[name]), ref)
    c = T.chain2_case(2, 4, 256)
    raw0 = conv(f(c["xi"]), c["w"][0], padding=1)
    a = torch.relu(raw0 + bv(c["b"][0]) + f(c["ri"]))
    raw1, d = conv(a, c["w"][1], stride=2, padding=1), conv(a, c["wd"], stride=2)
    y = torch.relu(raw1 + bv(c["b"][1]))
    raw2 = conv(y, c["w"][2], padding=1)
    out = torch.relu(raw2 + bv(c["b"][2]) + d)
    for name, ref in (("raw0", raw0), ("a", a), ("raw1", raw1), ("d", d), ("y", y), ("raw2", raw2), ("out", out), ("raw3", conv(out, c["w"][3], padding=1))):
        _same(p(c[name]), ref)
