"""GPU tests of the ResNet-34 trunk's and the heads' matrix-core kernels in EVERY launch form: hdn_conv3x3_bias_relu_f32, hdn_conv3x3_v2_f32,
hdn_conv3x3s2_ds_f32, hdn_conv3x3_chain_f32 / hdn_conv3x3_finish_f32 (csrc/conv3x3.hip), hdn_conv3x3s2_v2_f32 (csrc/conv3x3s2.hip),
hdn_trunk_stem_mfma_f32, hdn_head_conv3x3_f32 and hdn_head_tail_f32 - against float64 on all images of the batch, in exact (tolerance-free)
addressing tests, and at large magnitudes with the range guard off.

The batch lists and the integer-indexed expectations live in tests/trunk34_forms.py; tests/test_trunk34_forms_host.py checks those expectations
against float64 on the CPU.  The host queries (hdn_conv3x3_workspace_bytes, hdn_conv3x3_v2_workspace_bytes, hdn_conv3x3_chain_slices) are used for
one thing only: the *_cases_cover_every_form tests prove with them that the lists reach every form.  No expected value comes from a query."""
import pytest
import torch
import torch.nn.functional as F

import trunk34_forms as T
from test_gpu_trunk50_forms import _codes, _held, check_per_image

pytestmark = pytest.mark.gpu

CL = torch.channels_last

S1_FLAT = T.flat(T.S1_CASES, T.S1_EXTRA)
V2_FLAT = T.flat(T.V2_CASES, T.V2_EXTRA)
S2_FLAT = T.flat(T.S2_CASES)
S2V2_FLAT = T.flat(T.S2V2_CASES)
CHAIN1_FLAT = T.flat(T.CHAIN1_CASES)
CHAIN2_FLAT = T.flat(T.CHAIN2_CASES)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _cl(t):
    return t.contiguous(memory_format=CL)


def _scales():
    from hdn_amd.trunk import ACT_SCALE_LOG2
    return 2.0 ** -ACT_SCALE_LOG2, 2.0 ** ACT_SCALE_LOG2


def _exact(what, got, want):
    """got (device, NCHW view) == want (CPU float32, NCHW view), or an AssertionError naming the first wrong (image, channel, y, x)."""
    msg = T.first_difference(got.cpu(), want)
    if msg is not None:
        raise AssertionError(f"{what}: {msg}")


# ----------------------------------------------------------------------------------------------------------------- coverage
def test_conv3x3_cases_cover_every_form():
    """S1_CASES / V2_CASES reach every K-slice form of hdn_conv3x3_bias_relu_f32 and hdn_conv3x3_v2_f32, each batch the first of its form."""
    T.check_stride1_coverage()
    from hdn_amd.trunk import V2_MIN_BATCH
    assert V2_MIN_BATCH == 24 and all(B >= V2_MIN_BATCH for _, _, B in V2_FLAT + S2V2_FLAT)


def test_conv3x3s2_ds_cases_cover_every_form():
    """S2_CASES reach every K-slice form of hdn_conv3x3s2_ds_f32 (hdn_conv3x3s2_v2_f32 has one form per shape: S2V2_CASES)."""
    T.check_stride2_coverage()


def test_chain_cases_cover_every_form():
    """One batch per distinct hdn_conv3x3_chain_slices in 1 .. CHAIN_MAX_BATCH, both strides; the chained form splits K as the unchained one at
    least for B <= 12 (where the chain tests assert bit-identity)."""
    from hdn_amd.trunk import CHAIN_MAX_BATCH
    assert CHAIN_MAX_BATCH == T.CHAIN_MAX
    T.check_chain_coverage()


# ----------------------------------------------------------------------------------------------------------------- float64 sweeps
def _stride1_vs_float64(dev, S, C, B, v2):
    from hdn_amd.trunk import conv3x3_bias_relu, pack_conv3x3, pack_conv3x3_v2
    g = torch.Generator().manual_seed(3400 + S + 3 * C + 7 * B + v2)
    w = torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(C, generator=g) * 0.1
    x = torch.randn(B, C, S, S, generator=g).clamp_min_(0)
    r = torch.randn(B, C, S, S, generator=g)
    wp, bd = pack_conv3x3(w).to(dev), b.to(dev)
    kw = {"wpacked_v2": pack_conv3x3_v2(w).to(dev)} if v2 else {}
    xd, rd = _cl(x.to(dev)), _cl(r.to(dev))
    y, y0 = conv3x3_bias_relu(xd, wp, bd, rd, **kw), conv3x3_bias_relu(xd, wp, bd, **kw)
    assert torch.equal(y, conv3x3_bias_relu(xd, wp, bd, rd, **kw)) and torch.equal(y0, conv3x3_bias_relu(xd, wp, bd, **kw))   # deterministic
    assert y.is_contiguous(memory_format=CL) and tuple(y.shape) == (B, C, S, S)
    sc, un = _scales()
    xs, rs = _cl(xd * sc), _cl(rd * sc)
    yd = conv3x3_bias_relu(xs, wp, bd * sc, rs, act_domain=1, **kw) * un
    yd0 = conv3x3_bias_relu(xs, wp, bd * sc, act_domain=1, **kw) * un
    conv, conv32 = F.conv2d(x.double(), w.double(), b.double(), padding=1), F.conv2d(x, w, b, padding=1)
    t, ref, t0, ref0 = torch.relu(conv + r.double()), torch.relu(conv32 + r), torch.relu(conv), torch.relu(conv32)
    what = f"{'conv3x3_v2' if v2 else 'conv3x3'} ({S}, {C}) z={(T.z_v2 if v2 else T.z_s1)(B, S, C)} B={B}"
    check_per_image(what + " residual domain 0", y, t, ref)
    check_per_image(what + " residual domain 1", yd, t, ref)
    check_per_image(what + " plain domain 0", y0, t0, ref0)
    check_per_image(what + " plain domain 1", yd0, t0, ref0)


@pytest.mark.parametrize("S,C,B", S1_FLAT)
def test_conv3x3_every_form_vs_float64(dev, S, C, B):
    """hdn_conv3x3_bias_relu_f32 in the form batch B selects against a float64 convolution on EVERY image: per image within 4x the error of PyTorch's
    CPU fp32 convolution + 1e-5 of the image's output scale; with and without residual, act_domain 0 and 1, two calls bit-equal."""
    _stride1_vs_float64(dev, S, C, B, False)


@pytest.mark.parametrize("S,C,B", V2_FLAT)
def test_conv3x3_v2_every_form_vs_float64(dev, S, C, B):
    """hdn_conv3x3_v2_f32 likewise (B >= V2_MIN_BATCH: both sides of every k_slices_v2 switch up to 64)."""
    _stride1_vs_float64(dev, S, C, B, True)


def _stride2_vs_float64(dev, S, CI, B, v2):
    from hdn_amd.trunk import conv3x3s2_ds, pack_conv3x3s2_ds, pack_conv3x3s2_ds_v2
    g = torch.Generator().manual_seed(3500 + S + 3 * CI + 7 * B + v2)
    CO = 2 * CI
    w = torch.randn(CO, CI, 3, 3, generator=g) * (2.0 / (9 * CI)) ** 0.5
    wd = torch.randn(CO, CI, 1, 1, generator=g) * (1.0 / CI) ** 0.5
    b = torch.randn(CO, generator=g) * 0.1
    x = torch.randn(B, CI, 2 * S, 2 * S, generator=g).clamp_min_(0)
    wp, bd = pack_conv3x3s2_ds(w, wd).to(dev), b.to(dev)
    kw = {"wpacked_v2": pack_conv3x3s2_ds_v2(w, wd).to(dev)} if v2 else {}
    xd = _cl(x.to(dev))
    y, ds = conv3x3s2_ds(xd, wp, bd, **kw)
    y2, ds2 = conv3x3s2_ds(xd, wp, bd, **kw)
    assert torch.equal(y, y2) and torch.equal(ds, ds2)                                                  # deterministic
    assert tuple(y.shape) == tuple(ds.shape) == (B, CO, S, S) and y.is_contiguous(memory_format=CL) and ds.is_contiguous(memory_format=CL)
    sc, un = _scales()
    y1, ds1 = conv3x3s2_ds(_cl(xd * sc), wp, bd * sc, act_domain=1, **kw)
    t, ref = torch.relu(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1)), torch.relu(F.conv2d(x, w, b, stride=2, padding=1))
    td, refd = F.conv2d(x.double(), wd.double(), None, stride=2), F.conv2d(x, wd, None, stride=2)
    what = f"{'conv3x3s2_v2' if v2 else 'conv3x3s2_ds'} ({S}, {CI}) " + ("" if v2 else f"z={T.z_s2(B, S, CI)} ") + f"B={B}"
    check_per_image(what + " conv domain 0", y, t, ref)
    check_per_image(what + " conv domain 1", y1 * un, t, ref)
    check_per_image(what + " downsample domain 0", ds, td, refd)
    check_per_image(what + " downsample domain 1", ds1 * un, td, refd)


@pytest.mark.parametrize("S,CI,B", S2_FLAT)
def test_conv3x3s2_ds_every_form_vs_float64(dev, S, CI, B):
    """hdn_conv3x3s2_ds_f32 in the form batch B selects: both outputs against float64 convolutions on every image, both act_domains, bit-equal calls."""
    _stride2_vs_float64(dev, S, CI, B, False)


@pytest.mark.parametrize("S,CI,B", S2V2_FLAT)
def test_conv3x3s2_v2_vs_float64_on_every_image(dev, S, CI, B):
    _stride2_vs_float64(dev, S, CI, B, True)


def _per_image_2e5(what, got, truth):
    """The chain tests' bound, per image: err <= 2e-5 of the image's max |truth|."""
    got = got.detach().cpu().double()
    assert got.shape == truth.shape and torch.isfinite(got).all(), what
    err, scale = (got - truth).abs().flatten(1).amax(1), truth.abs().flatten(1).amax(1)
    i = int(torch.argmax(err / scale))
    print(f"FORMS {what}: worst image {i} of {got.shape[0]}: err {float(err[i]):.3e}, scale {float(scale[i]):.3f}, bound {2e-5 * float(scale[i]):.3e}")
    assert bool((err <= 2e-5 * scale).all()), (what, i, float(err[i]), float(scale[i]))


@pytest.mark.parametrize("S,C,B", CHAIN1_FLAT)
def test_chain_two_blocks_every_form_vs_float64(dev, S, C, B):
    """Two BasicBlocks as four chained launches (chain_conv / LazyAct) at one batch per distinct hdn_conv3x3_chain_slices: per image within 2e-5 of
    the image's scale of float64, bit-identical to the unchained launches where both split K alike (asserted to be so for B <= 12)."""
    from hdn_amd.trunk import LazyAct, chain_conv, conv3x3_bias_relu, pack_conv3x3
    g = torch.Generator().manual_seed(3600 + 7 * C + B)
    ws = [torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5 for _ in range(4)]
    bs = [torch.randn(C, generator=g) * 0.1 for _ in range(4)]
    x = torch.randn(B, C, S, S, generator=g).clamp_min_(0)
    wp, bd = [pack_conv3x3(w).to(dev) for w in ws], [b.to(dev) for b in bs]
    xd = _cl(x.to(dev))
    y1 = conv3x3_bias_relu(conv3x3_bias_relu(xd, wp[0], bd[0]), wp[1], bd[1], xd)
    y2 = conv3x3_bias_relu(conv3x3_bias_relu(y1, wp[2], bd[2]), wp[3], bd[3], y1)
    s1, _, _ = chain_conv(xd, wp[0])
    s2, _, _ = chain_conv(LazyAct(s1, bd[0]), wp[1])
    s3, _, y1c = chain_conv(LazyAct(s2, bd[1], xd), wp[2], 1, want_x=True)
    s4, _, _ = chain_conv(LazyAct(s3, bd[2]), wp[3])
    y2c = LazyAct(s4, bd[3], y1c).finish()
    same_split = T.z_chain(B, S, C, 1) == T.z_s1(B, S, C)
    assert s1.shape[0] == T.z_chain(B, S, C, 1)
    if B <= T.CHAIN_SAME_SPLIT_UP_TO:
        assert same_split, (S, C, B)
    if same_split:
        assert torch.equal(y1c, y1) and torch.equal(y2c, y2)
    xt = x.double()
    cv = lambda t, i: F.conv2d(t, ws[i].double(), bs[i].double(), padding=1)
    t1 = torch.relu(cv(torch.relu(cv(xt, 0)), 1) + xt)
    t2 = torch.relu(cv(torch.relu(cv(t1, 2)), 3) + t1)
    what = f"chain ({S}, {C}) z={s1.shape[0]} B={B}"
    _per_image_2e5(what + " block 1", y1c, t1)
    _per_image_2e5(what + " block 2", y2c, t2)


@pytest.mark.parametrize("S,CI,B", CHAIN2_FLAT)
def test_chain_downsample_block_every_form_vs_float64(dev, S, CI, B):
    """The first block of layer2..4 chained (stride-2 convolution + downsample branch from a LazyAct input, the downsample SLICES as the block's
    residual) at one batch per distinct hdn_conv3x3_chain_slices - B = 13 included, which no other test runs at stride 2."""
    from hdn_amd.trunk import LazyAct, chain_conv, conv3x3_bias_relu, conv3x3s2_ds, pack_conv3x3, pack_conv3x3s2_ds
    g = torch.Generator().manual_seed(3700 + 11 * CI + B)
    CO = 2 * CI
    w0 = torch.randn(CI, CI, 3, 3, generator=g) * (2.0 / (9 * CI)) ** 0.5
    w1 = torch.randn(CO, CI, 3, 3, generator=g) * (2.0 / (9 * CI)) ** 0.5
    wd = torch.randn(CO, CI, 1, 1, generator=g) * (1.0 / CI) ** 0.5
    w2 = torch.randn(CO, CO, 3, 3, generator=g) * (2.0 / (9 * CO)) ** 0.5
    b0, b1, b2 = (torch.randn(c, generator=g) * 0.1 for c in (CI, CO, CO))
    x = torch.randn(B, CI, 2 * S, 2 * S, generator=g).clamp_min_(0)
    r = torch.randn(B, CI, 2 * S, 2 * S, generator=g)
    xd, rd = _cl(x.to(dev)), _cl(r.to(dev))
    p0, p1, p2 = pack_conv3x3(w0).to(dev), pack_conv3x3s2_ds(w1, wd).to(dev), pack_conv3x3(w2).to(dev)
    b0d, b1d, b2d = b0.to(dev), b1.to(dev), b2.to(dev)
    a = conv3x3_bias_relu(xd, p0, b0d, rd)
    y, idt = conv3x3s2_ds(a, p1, b1d)
    out = conv3x3_bias_relu(y, p2, b2d, idt)
    s0, _, _ = chain_conv(xd, p0)
    s1, sd, _ = chain_conv(LazyAct(s0, b0d, rd), p1, 2)
    s2, _, _ = chain_conv(LazyAct(s1, b1d), p2)
    outc = LazyAct(s2, b2d, sd).finish()
    assert s1.shape[0] == sd.shape[0] == T.z_chain(B, S, CI, 2)
    same_split = (T.z_chain(B, 2 * S, CI, 1) == T.z_s1(B, 2 * S, CI) and T.z_chain(B, S, CI, 2) == T.z_s2(B, S, CI)
                  and T.z_chain(B, S, CO, 1) == T.z_s1(B, S, CO))
    if B <= T.CHAIN_SAME_SPLIT_UP_TO:
        assert same_split, (S, CI, B)
    if same_split:
        assert torch.equal(outc, out)
    at = torch.relu(F.conv2d(x.double(), w0.double(), b0.double(), padding=1) + r.double())
    yt = torch.relu(F.conv2d(at, w1.double(), b1.double(), stride=2, padding=1))
    tt = torch.relu(F.conv2d(yt, w2.double(), b2.double(), padding=1) + F.conv2d(at, wd.double(), None, stride=2))
    _per_image_2e5(f"chain downsample block ({S}, {CI}) z={s1.shape[0]} B={B}", outc, tt)


# ----------------------------------------------------------------------------------------------------------------- exact addressing
def _stride1_exact(dev, S, C, B, v2):
    from hdn_amd.trunk import conv3x3_bias_relu, pack_conv3x3, pack_conv3x3_v2
    xi, ri, bi = _codes((B, S, S, C)), _codes((B, S, S, C), 40503, 2003, 1001), T.bias_int(C)
    w, src, tap = T.onehot3x3(C, C)
    raw = T.pick3x3(xi, src, tap)
    want_res, want_plain = T.nchw(torch.relu(raw + bi + ri)), T.nchw(torch.relu(raw + bi))
    wp = pack_conv3x3(w).to(dev)
    kw = {"wpacked_v2": pack_conv3x3_v2(w).to(dev)} if v2 else {}
    xd, rd, bd = T.nchw(xi).to(dev), T.nchw(ri).to(dev), bi.float().to(dev)
    assert xd.is_contiguous(memory_format=CL) and rd.is_contiguous(memory_format=CL)
    sc, _ = _scales()
    name = f"{'conv3x3_v2' if v2 else 'conv3x3'} ({S}, {C}) B={B} z={(T.z_v2 if v2 else T.z_s1)(B, S, C)}"
    for dom, k in ((0, 1.0), (1, sc)):
        _exact(f"{name} domain {dom} residual", conv3x3_bias_relu(xd * k, wp, bd * k, rd * k, act_domain=dom, **kw) / k, want_res)
        _exact(f"{name} domain {dom} plain", conv3x3_bias_relu(xd * k, wp, bd * k, act_domain=dom, **kw) / k, want_plain)


@pytest.mark.parametrize("S,C,B", S1_FLAT)
def test_conv3x3_addressing_is_exact(dev, S, C, B):
    """Integer activations |x| < 2^21 (exact under the x 2^-8 two-fp16-piece split), one 1.0 per output channel at input channel (5 co + 3) mod C and
    tap co mod 9, integer bias |b| <= 100 and residual |r| <= 1001: out[b, co, y, x] = relu(x[b, ci, y + ky - 1, x + kx - 1] (zero outside) + bias
    (+ residual)) exactly, every other partial sum an exact zero in every wave and K slice.  torch.equal against integer indexing on a zero-padded
    tensor, in every form of hdn_conv3x3_bias_relu_f32, both act_domains: a swapped tap, image, channel or slice anywhere in the batch fails."""
    _stride1_exact(dev, S, C, B, False)


@pytest.mark.parametrize("S,C,B", V2_FLAT)
def test_conv3x3_v2_addressing_is_exact(dev, S, C, B):
    _stride1_exact(dev, S, C, B, True)


def _stride2_exact(dev, S, CI, B, v2):
    from hdn_amd.trunk import conv3x3s2_ds, pack_conv3x3s2_ds, pack_conv3x3s2_ds_v2
    CO = 2 * CI
    xi, bi = _codes((B, 2 * S, 2 * S, CI)), T.bias_int(CO)
    w, src, tap = T.onehot3x3(CO, CI)
    wd, srcd = T.onehot1x1(CO, CI)
    want, want_ds = T.nchw(torch.relu(T.pick3x3(xi, src, tap, 2) + bi)), T.nchw(T.pick1x1s2(xi, srcd))
    assert float(want_ds.min()) < 0                                         # no bias, no ReLU: negative values survive
    wp = pack_conv3x3s2_ds(w, wd).to(dev)
    kw = {"wpacked_v2": pack_conv3x3s2_ds_v2(w, wd).to(dev)} if v2 else {}
    xd, bd = T.nchw(xi).to(dev), bi.float().to(dev)
    assert xd.is_contiguous(memory_format=CL)
    sc, _ = _scales()
    name = f"{'conv3x3s2_v2' if v2 else 'conv3x3s2_ds'} ({S}, {CI}) B={B}" + ("" if v2 else f" z={T.z_s2(B, S, CI)}")
    for dom, k in ((0, 1.0), (1, sc)):
        y, ds = conv3x3s2_ds(xd * k, wp, bd * k, act_domain=dom, **kw)
        _exact(f"{name} domain {dom} conv", y / k, want)
        _exact(f"{name} domain {dom} downsample", ds / k, want_ds)


@pytest.mark.parametrize("S,CI,B", S2_FLAT)
def test_conv3x3s2_ds_addressing_is_exact(dev, S, CI, B):
    """As test_conv3x3_addressing_is_exact for both outputs of hdn_conv3x3s2_ds_f32 in every form; the downsample weights are one-hot at ANOTHER
    input channel, (7 co + 1) mod CI, and that output has no bias and no ReLU."""
    _stride2_exact(dev, S, CI, B, False)


@pytest.mark.parametrize("S,CI,B", S2V2_FLAT)
def test_conv3x3s2_v2_addressing_is_exact(dev, S, CI, B):
    _stride2_exact(dev, S, CI, B, True)


def _nhwc_sum(slices):
    """[z, B, S, S, C] raw K slices -> their sum as an NCHW view (exact here: all but one slice of every element are exact zeros)."""
    return slices.sum(0).permute(0, 3, 1, 2)


@pytest.mark.parametrize("S,C,B", CHAIN1_FLAT)
def test_chain_addressing_is_exact(dev, S, C, B):
    """conv -> lazy conv with want_x -> finish on the integer construction (tests/trunk34_forms.py: chain1_case, |x| < 2^20 so that every activation
    that is split again stays below 2^22): the activation written on the way (x_out), the final activation and each slice tensor summed over z,
    all torch.equal to integer indexing; both act_domains."""
    from hdn_amd.trunk import LazyAct, chain_conv, pack_conv3x3
    c = T.chain1_case(B, S, C)
    p0, p1 = (pack_conv3x3(w).to(dev) for w in c["w"])
    xd, rd = T.nchw(c["xi"]).to(dev), T.nchw(c["ri"]).to(dev)
    sc, _ = _scales()
    for dom, k in ((0, 1.0), (1, sc)):
        b0, b1 = (b.float().to(dev) * k for b in c["b"])
        name = f"chain ({S}, {C}) B={B} z={T.z_chain(B, S, C, 1)} domain {dom}"
        s0, _, none = chain_conv(xd * k, p0, act_domain=dom)
        assert none is None
        s1, _, xo = chain_conv(LazyAct(s0, b0, rd * k), p1, 1, want_x=True, act_domain=dom)
        out = LazyAct(s1, b1, xo).finish()
        _exact(name + " slices of conv 0", _nhwc_sum(s0) / k, T.nchw(c["raw0"]))
        _exact(name + " x_out", xo / k, T.nchw(c["a"]))
        _exact(name + " slices of conv 1", _nhwc_sum(s1) / k, T.nchw(c["raw1"]))
        _exact(name + " finish", out / k, T.nchw(c["out"]))


@pytest.mark.parametrize("S,CI,B", CHAIN2_FLAT)
def test_chain_downsample_block_addressing_is_exact(dev, S, CI, B):
    """The stride-2 block chained on the integer construction (chain2_case): a lazy input with an activation residual into the stride-2 launch
    (x_out, both slice tensors), its slices into the block's second convolution (x_out), the downsample SLICES as the residual of finish() and of
    the next block's first convolution (x_out again) - every tensor torch.equal to integer indexing; both act_domains."""
    from hdn_amd.trunk import LazyAct, chain_conv, pack_conv3x3, pack_conv3x3s2_ds
    c = T.chain2_case(B, S, CI)
    w0, w1, w2, w3 = c["w"]
    p0, p1, p2, p3 = pack_conv3x3(w0).to(dev), pack_conv3x3s2_ds(w1, c["wd"]).to(dev), pack_conv3x3(w2).to(dev), pack_conv3x3(w3).to(dev)
    xd, rd = T.nchw(c["xi"]).to(dev), T.nchw(c["ri"]).to(dev)
    sc, _ = _scales()
    for dom, k in ((0, 1.0), (1, sc)):
        b0, b1, b2 = (b.float().to(dev) * k for b in c["b"])
        name = f"chain downsample block ({S}, {CI}) B={B} z={T.z_chain(B, S, CI, 2)} domain {dom}"
        s0, _, _ = chain_conv(xd * k, p0, act_domain=dom)
        s1, sd, xo = chain_conv(LazyAct(s0, b0, rd * k), p1, 2, want_x=True, act_domain=dom)
        s2, _, yo = chain_conv(LazyAct(s1, b1), p2, 1, want_x=True, act_domain=dom)
        out = LazyAct(s2, b2, sd).finish()
        s3, _, oo = chain_conv(LazyAct(s2, b2, sd), p3, 1, want_x=True, act_domain=dom)
        for what, got, key in (("slices of conv 0", _nhwc_sum(s0), "raw0"), ("x_out of the stride-2 launch", xo, "a"),
                               ("slices of the stride-2 conv", _nhwc_sum(s1), "raw1"), ("downsample slices", _nhwc_sum(sd), "d"),
                               ("x_out of conv 2", yo, "y"), ("slices of conv 2", _nhwc_sum(s2), "raw2"), ("finish", out, "out"),
                               ("x_out of the next block", oo, "out"), ("slices of the next block", _nhwc_sum(s3), "raw3")):
            _exact(f"{name} {what}", got / k, T.nchw(c[key]))


@pytest.mark.parametrize("B", [1, 8, 48])
def test_stem_addressing_is_exact(dev, B):
    """hdn_trunk_stem_mfma_f32 through FusedStem at the 4 / 8 / 16-rows-per-workgroup forms, both out_domains: integer images, the one 1.0 of channel
    co at (ci, ky, kx) = (co mod 2, (co // 2) mod 7, (3 co + 1) mod 7), integer bias; expected = max_pool2d(3, 2, 1) of the ReLU'd integer tensor
    computed on int64.  A leak from the eighth (padding) kernel column, from the K = 98 -> 112 pad or from the carried pool row fails torch.equal."""
    from hdn_amd import trunk
    xi, bi = _codes((B, 2, 127, 127)), T.bias_int(64)
    w, ci, ky, kx = T.stem_onehot()
    want = T.stem_expected(xi, ci, ky, kx, bi).float()
    conv = torch.nn.Conv2d(2, 64, 7, 2, 3)
    conv.weight.data, conv.bias.data = w, bi.float()
    assert B >= trunk.STEM_MFMA_MIN_BATCH
    sc, un = _scales()
    for dom, k in ((0, 1.0), (1, un)):
        st = trunk.FusedStem(conv, True, out_domain=dom).to(dev)
        y = st(xi.float().to(dev))
        assert y.is_contiguous(memory_format=CL)
        _exact(f"stem B={B} out_domain {dom}", y * k, want)


@pytest.mark.parametrize("nhwc", [False, True])
@pytest.mark.parametrize("Hi,Wi,n,CO", [(9, 14, 2, 64), (33, 20, 4, 96), (31, 31, 3, 512)])
def test_head_conv_addressing_is_exact(dev, Hi, Wi, n, CO, nhwc):
    """hdn_head_conv3x3_f32: every level with its own codes, one-hot and bias; out[l, co, y, x] = relu(x_l[src, y + ky, x + kx] + b_l[co]) exactly -
    a level, channel, tap or pixel mix-up fails.  NCHW and channels-last inputs."""
    from hdn_amd import heads as HD
    xs, ws, bs, want = T.head_conv_case(Hi, Wi, n, CO)
    pk = HD._PackedHead()
    pk.wsp = HD._pack_conv_search([w.to(dev) for w in ws])
    pk.bsp = bs.float().to(dev)
    xd = [_cl(x.float().to(dev)) if nhwc else x.float().to(dev) for x in xs]
    got = HD.head_conv_search(xd, pk)
    msg = T.first_difference(got.cpu(), want.float())
    assert msg is None, f"head conv ({Hi}, {Wi}, {n}, {CO}) nhwc={nhwc}: (level, channel, y, x): {msg}"


@pytest.mark.parametrize("H,P,n,om", [(128, 7, 2, 8), (256, 33, 1, 4), (256, 169, 3, 4)])
def test_head_tail_addressing_is_exact(dev, H, P, n, om):
    """hdn_head_tail_f32: w1 one-hot per hidden row with an integer b1, wf in {-1, 0, 1} with 8 non-zeros per row, integer inputs |x| < 2^17: every
    partial sum of the fp32 second product is an integer below 2^24, so the result is exact in any summation order."""
    from hdn_amd import heads as HD
    feats, w1, b1, wf, bf, want = T.head_tail_case(H, P, n, om)
    pk = HD._PackedHead()
    pk.w1, pk.b1, pk.wf, pk.bf = w1.to(dev), b1.float().to(dev), wf.to(dev), bf.float().to(dev)
    pk.w1p = HD._pack_w1(pk.w1)
    got = HD.head_tail(feats.float().view(2 * n, H, P, 1).to(dev), pk, n).cpu()
    if not torch.equal(got, want.float()):
        bad = (got != want.float()).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"head tail ({H}, {P}, {n}): {bad.shape[0]} of {got.numel()} outputs differ; first (branch, row, pixel) = {i}: "
                             f"got {float(got[i])!r}, want {float(want[i])!r}")


# ----------------------------------------------------------------------------------------------------------------- large magnitudes, guard off
def test_large_magnitudes_across_forms_with_the_guard_off(dev):
    """test_fp16_piece_range_guard runs hdn_conv3x3_bias_relu_f32 in one sliced form and hdn_conv3x3s2_ds_f32 at B = 3 only.  One element of 7e4 and of
    1e7 in the LAST image, in a z > 1 form and at z = 1 of each, both act_domains: finite, and the outputs the element reaches and the others each
    within the float64 bound against their own scale."""
    from hdn_amd import _lib
    from hdn_amd.trunk import conv3x3_bias_relu, conv3x3s2_ds, pack_conv3x3, pack_conv3x3s2_ds
    lib = _lib.load()
    sc, un = _scales()
    prev = lib.hdn_set_check_range(0)
    try:
        g = torch.Generator().manual_seed(34)
        S, C = 16, 128
        w = torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
        b = torch.randn(C, generator=g) * 0.1
        wp, bd = pack_conv3x3(w).to(dev), b.to(dev)
        for B, z in ((3, 8), (50, 1)):
            assert T.z_s1(B, S, C) == z
            x = torch.randn(B, C, S, S, generator=g).clamp_min_(0)
            for big in (7.0e4, 1.0e7):
                xb = x.clone()
                xb[B - 1, 17, 3, 5] = big
                t, ref = torch.relu(F.conv2d(xb.double(), w.double(), b.double(), padding=1)), torch.relu(F.conv2d(xb, w, b, padding=1))
                reached = torch.zeros_like(t, dtype=torch.bool)
                reached[B - 1, :, 2:5, 4:7] = True
                xd = _cl(xb.to(dev))
                _held(conv3x3_bias_relu(xd, wp, bd), t, ref, reached, f"conv3x3 z={z} {big:g} domain 0")
                _held(conv3x3_bias_relu(_cl(xd * sc), wp, bd * sc, act_domain=1) * un, t, ref, reached, f"conv3x3 z={z} {big:g} domain 1")
        S, CI = 16, 64
        w2 = torch.randn(2 * CI, CI, 3, 3, generator=g) * (2.0 / (9 * CI)) ** 0.5
        wd = torch.randn(2 * CI, CI, 1, 1, generator=g) * (1.0 / CI) ** 0.5
        b2 = torch.randn(2 * CI, generator=g) * 0.1
        wp2, bd2 = pack_conv3x3s2_ds(w2, wd).to(dev), b2.to(dev)
        for B, z in ((3, 4), (25, 1)):
            assert T.z_s2(B, S, CI) == z
            x = torch.randn(B, CI, 2 * S, 2 * S, generator=g).clamp_min_(0)
            for big in (7.0e4, 1.0e7):
                xb = x.clone()
                xb[B - 1, 17, 8, 10] = big
                t, ref = torch.relu(F.conv2d(xb.double(), w2.double(), b2.double(), stride=2, padding=1)), torch.relu(F.conv2d(xb, w2, b2, stride=2, padding=1))
                td, refd = F.conv2d(xb.double(), wd.double(), None, stride=2), F.conv2d(xb, wd, None, stride=2)
                # input pixel (8, 10), both even: under a 3 x 3 / stride 2 / padding 1 window only as the centre tap, 2 oy - 1 + ky = 8 -> (oy, ky) =
                # (4, 1), 2 ox - 1 + kx = 10 -> (ox, kx) = (5, 1); and the pixel the 1x1 / stride 2 branch reads for output (4, 5)
                reached = torch.zeros_like(t, dtype=torch.bool)
                reached[B - 1, :, 4, 5] = True
                reach_d = torch.zeros_like(td, dtype=torch.bool)
                reach_d[B - 1, :, 4, 5] = True
                xd = _cl(xb.to(dev))
                for dom, k in ((0, 1.0), (1, sc)):
                    y, ds = conv3x3s2_ds(_cl(xd * k), wp2, bd2 * k, act_domain=dom)
                    _held(y / k, t, ref, reached, f"conv3x3s2_ds z={z} {big:g} domain {dom} conv")
                    _held(ds / k, td, refd, reach_d, f"conv3x3s2_ds z={z} {big:g} domain {dom} downsample")
    finally:
        lib.hdn_set_check_range(prev)
    torch.cuda.synchronize()
