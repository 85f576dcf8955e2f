"""GPU tests of the two ResNet-50 trunk kernels in EVERY launch form: hdn_conv1x1_f32 (csrc/conv1x1.hip, Cfg<NT, WM, WN, KW> by batch and shape) and
hdn_conv3x3s2_f32 (csrc/conv3x3s2.hip, K slices by batch) against float64 on all images of the batch, an exact (tolerance-free) addressing test,
large magnitudes with the range guard off, and the folded trunk at batches between the ones tests/test_gpu_trunk50*.py run.

The two host queries (hdn_conv1x1_form, hdn_conv3x3s2_workspace_bytes) are used for one thing only: the *_covers_every_form tests prove with them
that the batch lists below reach every form.  If the fill threshold of a kernel moves, those tests fail and say which list to re-pick.  No expected
value comes from a query."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from test_gpu_trunk50 import SHAPES as TRUNK_1X1                      # every 1x1 convolution of the trunk: (CI, CO, S, stride)

pytestmark = pytest.mark.gpu

CL = torch.channels_last

# ----------------------------------------------------------------------------------------------------------------- the cases
# hdn_conv3x3s2_f32, (S, C) -> batches: each the first batch of a form past the first (the table in docs/PARITY.md), and at S = 4 each = 1 mod 4:
# the last 4-image tile holds one image (B = 5: the first form with such a tile)
S2_CASES = {(16, 128): [3, 16, 32, 64], (8, 256): [3, 16, 32, 64, 128], (4, 512): [1, 5, 13, 29, 61, 125, 253]}
S2_FORMS = {(16, 128): ["4x3", "4x1", "2x1", "fused"], (8, 256): ["8x3", "8x1", "4x1", "2x1", "fused"],
            (4, 512): ["16x3", "16x1", "8x1", "4x1", "2x1", "fused"]}
S2_FLAT = [(S, C, B) for (S, C), bs in S2_CASES.items() for B in bs]

# hdn_conv1x1_f32 off the trunk, (CI, CO, S, stride, B): M = B So^2 = 147, 147, 125, 147, 25, 48, 125, 9 - none a multiple of its form's pixel tile
# (a tail under each of the four KW = 1 forms), the CO % 64 != 0 form three times (the last: it wins over the small-M form), odd sides at stride 2
OFF_TRUNK = [(64, 64, 7, 1, 3), (64, 128, 7, 1, 3), (64, 256, 5, 1, 5), (64, 96, 7, 1, 3), (96, 160, 5, 1, 1), (64, 128, 7, 2, 3), (64, 256, 9, 2, 5),
             (128, 96, 3, 1, 1)]
OFF_TRUNK_FORMS = ["Cfg<2,4,1,1>", "Cfg<2,2,2,1>", "Cfg<2,1,4,1>", "Cfg<1,4,1,1>", "Cfg<1,4,1,1>", "Cfg<2,2,2,1>", "Cfg<2,1,4,1>", "Cfg<1,4,1,1>"]
ALL_1X1_FORMS = {"Cfg<2,4,1,1>", "Cfg<2,2,2,1>", "Cfg<2,1,4,1>", "Cfg<1,4,1,1>", "Cfg<1,1,1,4>"}
SWITCH_MAX = 256                                                     # a small-M -> large switch is run on both sides where it lies at B <= this


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _lib():
    from hdn_amd import _lib as L
    return L.load()


def form_1x1(B, S, CI, CO, stride):
    v = _lib().hdn_conv1x1_form(B, S, CI, CO, stride)
    assert v > 0, (v, B, S, CI, CO, stride)
    return f"Cfg<{v & 255},{(v >> 8) & 255},{(v >> 16) & 255},{v >> 24}>"


def pixel_tile_1x1(form):
    return 32 * int(form[4:-1].split(",")[1])                        # 32 WM


def form_s2(B, S, C):
    n = _lib().hdn_conv3x3s2_workspace_bytes(B, S, C)
    assert n >= 0 and n % (B * S * S * C * 4) == 0, (n, B, S, C)
    z = n // (B * S * S * C * 4)
    if z == 0:
        return "fused"
    zt = 3 if z % 3 == 0 else 1
    return f"{z // zt}x{zt}"


def switch_batch(CI, CO, S, stride):
    """The first batch at which a shape leaves the small-M form, None if it never is in it or stays in it up to SWITCH_MAX."""
    if form_1x1(1, S, CI, CO, stride) != "Cfg<1,1,1,4>":
        return None
    for B in range(2, SWITCH_MAX + 1):
        if form_1x1(B, S, CI, CO, stride) != "Cfg<1,1,1,4>":
            return B
    return None


def batches_1x1(CI, CO, S, stride):
    bs = [3, 17]
    sw = switch_batch(CI, CO, S, stride)
    if sw is not None:
        bs += [sw - 1, sw]
    return sorted(set(bs))


def check_per_image(what, got, truth, ref32):
    """got (device or CPU), the float64 truth and PyTorch's CPU fp32 result, all [B, C, H, W]: for every image err <= 4 e_ref + 1e-5 scale, e_ref the
    fp32 reference's own error and scale = max |truth| of that image (the bound of test_conv3x3_matrix_core_vs_float64).  Returns the figures of the
    image that comes closest to its bound."""
    got = got.detach().cpu().double()
    assert got.shape == truth.shape, (what, got.shape, truth.shape)
    assert torch.isfinite(got).all(), what
    d = (got - truth).abs()
    err = d.flatten(1).amax(1)
    e_ref = (ref32.double() - truth).abs().flatten(1).amax(1)
    scale = truth.abs().flatten(1).amax(1)
    bound = 4 * e_ref + 1e-5 * scale
    i = int(torch.argmax(err / bound))
    c, y, x = np.unravel_index(int(torch.argmax(d[i])), tuple(d.shape[1:]))
    print(f"FORMS {what}: worst image {i} of {got.shape[0]}: err {float(err[i]):.3e}, e_ref {float(e_ref[i]):.3e}, scale {float(scale[i]):.3f}, "
          f"bound {float(bound[i]):.3e}")
    assert bool((err <= bound).all()), (what, f"{int((err > bound).sum())} images over their bound; worst (image, channel, y, x) = {(i, int(c), int(y), int(x))}: "
                                              f"got {float(got[i, c, y, x])!r}, truth {float(truth[i, c, y, x])!r}, err {float(err[i]):.3e}, "
                                              f"e_ref {float(e_ref[i]):.3e}, scale {float(scale[i]):.3f}, bound {float(bound[i]):.3e}")


# ----------------------------------------------------------------------------------------------------------------- coverage
def test_conv3x3s2_cases_cover_every_form():
    """The batches of S2_CASES reach every K-slice form of hdn_conv3x3s2_f32 at every shape, and the exact test and the sweep use this list."""
    for (S, C), want in S2_FORMS.items():
        hit = [form_s2(B, S, C) for B in S2_CASES[(S, C)]]
        print(f"FORMS coverage conv3x3s2 (S, C) = ({S}, {C}): " + ", ".join(f"B={B}: {f}" for B, f in zip(S2_CASES[(S, C)], hit)))
        assert list(dict.fromkeys(hit)) == want, (f"hdn_conv3x3s2_f32 ({S}, {C}): the batches {S2_CASES[(S, C)]} run {hit}, wanted {want}: re-pick S2_CASES "
                                                   "(has HDN_S2_FILL moved?)")
        for B, f in zip(S2_CASES[(S, C)], hit):
            if f != want[0]:
                assert form_s2(B - 1, S, C) != f, (S, C, B)                             # the FIRST batch of its form
    assert all(B % 4 == 1 for B in S2_CASES[(4, 512)])


def test_conv1x1_cases_cover_every_form():
    """The trunk shapes at their batches and the off-trunk cases reach all five forms of hdn_conv1x1_f32; every form has a case whose M is no multiple of
    its pixel tile 32 WM (clamped row loads, guarded stores); both sides of every small-M -> large switch at B <= 256 are among the trunk cases."""
    hit, tails, switches = {}, set(), 0
    for CI, CO, S, stride in TRUNK_1X1:
        sw = switch_batch(CI, CO, S, stride)
        switches += sw is not None
        for B in batches_1x1(CI, CO, S, stride):
            f = form_1x1(B, S, CI, CO, stride)
            hit.setdefault(f, []).append((CI, CO, S, stride, B))
            if (B * ((S - 1) // stride + 1) ** 2) % pixel_tile_1x1(f):
                tails.add(f)
        if sw is not None:
            assert form_1x1(sw - 1, S, CI, CO, stride) == "Cfg<1,1,1,4>" != form_1x1(sw, S, CI, CO, stride)
    got = [form_1x1(B, S, CI, CO, stride) for CI, CO, S, stride, B in OFF_TRUNK]
    assert got == OFF_TRUNK_FORMS, f"off-trunk cases run {got}, wanted {OFF_TRUNK_FORMS}: re-pick OFF_TRUNK (has FILL of conv1x1.hip moved?)"
    for (CI, CO, S, stride, B), f in zip(OFF_TRUNK, got):
        hit.setdefault(f, []).append((CI, CO, S, stride, B))
        M = B * ((S - 1) // stride + 1) ** 2
        assert M % pixel_tile_1x1(f), (CI, CO, S, stride, B, M, f)
        tails.add(f)
    for f in sorted(hit):
        print(f"FORMS coverage conv1x1 {f}: {len(hit[f])} cases, tail: {f in tails}, e.g. (CI, CO, S, stride, B) = {hit[f][0]}, {hit[f][-1]}")
    print(f"FORMS coverage conv1x1: {switches} trunk shapes switch small-M -> large at B <= {SWITCH_MAX}")
    assert set(hit) == ALL_1X1_FORMS, f"forms never run: {ALL_1X1_FORMS - set(hit)}"
    assert tails == ALL_1X1_FORMS, f"forms without a partial pixel tile: {ALL_1X1_FORMS - tails}"
    assert switches == 12, switches


# ----------------------------------------------------------------------------------------------------------------- float64 sweeps
@pytest.mark.parametrize("S,C,B", S2_FLAT)
def test_conv3x3s2_every_form_vs_float64(dev, S, C, B):
    """hdn_conv3x3s2_f32 in the form batch B selects, against a float64 convolution on EVERY image: per image within 4x the error of PyTorch's CPU fp32
    convolution + 1e-5 of the image's output scale; act_domain 0 and 1; two calls bit-equal.  Inputs as test_conv3x3s2_vs_float64's."""
    from hdn_amd.trunk import ACT_SCALE_LOG2, conv3x3s2, pack_conv3x3s2
    g = torch.Generator().manual_seed(1000 + S + 3 * C + B)
    w = torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(C, generator=g) * 0.1
    x = torch.randn(B, C, 2 * S, 2 * S, generator=g).clamp_min_(0)
    wp, bd = pack_conv3x3s2(w).to(dev), b.to(dev)
    xd = x.to(dev).contiguous(memory_format=CL)
    y = conv3x3s2(xd, wp, bd)
    assert torch.equal(y, conv3x3s2(xd, wp, bd))                                 # deterministic
    assert y.is_contiguous(memory_format=CL) and tuple(y.shape) == (B, C, S, S)
    sc = 2.0 ** -ACT_SCALE_LOG2
    yd = conv3x3s2((xd * sc).contiguous(memory_format=CL), wp, bd * sc, act_domain=1) * 2.0 ** ACT_SCALE_LOG2
    t = torch.relu(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1))
    ref = torch.relu(F.conv2d(x, w, b, stride=2, padding=1))
    form = form_s2(B, S, C)
    for name, got in (("domain 0", y), ("domain 1", yd)):
        check_per_image(f"conv3x3s2 ({S}, {C}) form {form} B={B} {name}", got, t, ref)


def _conv1x1_vs_float64(dev, CI, CO, S, stride, B):
    from hdn_amd.trunk import ACT_SCALE_LOG2, conv1x1, pack_conv1x1
    g = torch.Generator().manual_seed(2000 + CI + 3 * CO + 7 * S + 11 * stride + B)
    So = (S - 1) // stride + 1
    w = torch.randn(CO, CI, 1, 1, generator=g) * (2.0 / CI) ** 0.5
    b = torch.randn(CO, generator=g) * 0.1
    x = torch.randn(B, CI, S, S, generator=g).clamp_min_(0)
    r = torch.randn(B, CO, So, So, generator=g)
    wp, bd = pack_conv1x1(w).to(dev), b.to(dev)
    xd, rd = x.to(dev).contiguous(memory_format=CL), r.to(dev).contiguous(memory_format=CL)
    y = conv1x1(xd, wp, bd, rd, stride=stride, relu=True)
    y0 = conv1x1(xd, wp, bd, stride=stride, relu=False)
    assert torch.equal(y, conv1x1(xd, wp, bd, rd, stride=stride, relu=True))          # deterministic
    assert torch.equal(y0, conv1x1(xd, wp, bd, stride=stride, relu=False))
    assert y.is_contiguous(memory_format=CL) and tuple(y.shape) == (B, CO, So, So)
    sc = 2.0 ** -ACT_SCALE_LOG2
    yd = conv1x1((xd * sc).contiguous(memory_format=CL), wp, bd * sc, (rd * sc).contiguous(memory_format=CL), stride=stride, relu=True,
                 act_domain=1) * 2.0 ** ACT_SCALE_LOG2
    yd0 = conv1x1((xd * sc).contiguous(memory_format=CL), wp, bd * sc, stride=stride, relu=False, act_domain=1) * 2.0 ** ACT_SCALE_LOG2
    conv = F.conv2d(x.double(), w.double(), b.double(), stride=stride)
    conv32 = F.conv2d(x, w, b, stride=stride)
    t, ref = torch.relu(conv + r.double()), torch.relu(conv32 + r)
    what = f"conv1x1 {CI}->{CO} @{S}/{stride} form {form_1x1(B, S, CI, CO, stride)} B={B} M={B * So * So}"
    check_per_image(what + " residual+relu domain 0", y, t, ref)
    check_per_image(what + " residual+relu domain 1", yd, t, ref)
    check_per_image(what + " plain domain 0", y0, conv, conv32)
    check_per_image(what + " plain domain 1", yd0, conv, conv32)


@pytest.mark.parametrize("CI,CO,S,stride", TRUNK_1X1)
def test_conv1x1_trunk_shapes_between_the_tested_batches(dev, CI, CO, S, stride):
    """Every 1x1 convolution of the trunk at B = 3 and 17 and on both sides of its small-M -> large switch (where that lies at B <= 256), against
    float64 on every image: with residual + ReLU and without both, act_domain 0 and 1, two calls bit-equal."""
    for B in batches_1x1(CI, CO, S, stride):
        _conv1x1_vs_float64(dev, CI, CO, S, stride, B)


@pytest.mark.parametrize("CI,CO,S,stride,B", OFF_TRUNK)
def test_conv1x1_partial_tiles_and_odd_sides(dev, CI, CO, S, stride, B):
    """Shapes no trunk has but the ABI accepts: M no multiple of the pixel tile under each KW = 1 form (the clamped row load and the `mm < M` store
    guard), CO % 64 != 0, odd sides at stride 2 (So = (S - 1) / 2 + 1)."""
    _conv1x1_vs_float64(dev, CI, CO, S, stride, B)


# ----------------------------------------------------------------------------------------------------------------- exact addressing
def _codes(shape, mul=2654435761, mod=4194301, off=2097150):
    """Integers of |v| <= off spread over the linear index of `shape` (int64)."""
    n = int(np.prod(shape))
    return ((torch.arange(n, dtype=torch.int64) * mul) % mod - off).reshape(shape)


EXACT_1X1 = OFF_TRUNK + [(2048, 512, 4, 1, 1), (2048, 512, 4, 1, 3), (256, 64, 32, 1, 3), (64, 64, 32, 1, 17), (256, 128, 32, 1, 32), (512, 256, 16, 1, 64),
                         (1024, 2048, 8, 2, 127)]


def test_exact_1x1_cases_cover_every_form():
    hit = {form_1x1(B, S, CI, CO, stride) for CI, CO, S, stride, B in EXACT_1X1}
    print("FORMS coverage exact conv1x1:", sorted(hit))
    assert hit == ALL_1X1_FORMS, ALL_1X1_FORMS - hit


@pytest.mark.parametrize("CI,CO,S,stride,B", EXACT_1X1)
def test_conv1x1_addressing_is_exact(dev, CI, CO, S, stride, B):
    """Integer activations |x| < 2^22 (exact under the x 2^-8 two-fp16-piece split), exactly one 1.0 per output channel at input channel (5 co + 3) mod CI,
    integer bias and residual: every output is ONE input element + bias (+ residual), ReLU'd, every other partial sum an exact zero in every wave and
    K slice.  The expected tensor is built by integer indexing; torch.equal, so one wrong (image, pixel, channel) anywhere fails.  Both act_domains
    (domain 1 is fed codes 2^-8 and answers x 2^-8: exact both ways)."""
    from hdn_amd.trunk import ACT_SCALE_LOG2, conv1x1, pack_conv1x1
    So = (S - 1) // stride + 1
    xi = _codes((B, S, S, CI))                                                   # NHWC
    ri = _codes((B, So, So, CO), 40503, 2003, 1001)
    bi = (torch.arange(CO, dtype=torch.int64) * 37) % 201 - 100
    src = (5 * torch.arange(CO) + 3) % CI
    w = torch.zeros(CO, CI)
    w[torch.arange(CO), src] = 1.0
    picked = xi[:, ::stride, ::stride, :][..., src] + bi                         # [B, So, So, CO]
    assert picked.shape == (B, So, So, CO)
    want_res = torch.relu(picked + ri).float().permute(0, 3, 1, 2)
    want_plain = picked.float().permute(0, 3, 1, 2)
    wp = pack_conv1x1(w).to(dev)
    xd = xi.float().permute(0, 3, 1, 2).to(dev)
    rd = ri.float().permute(0, 3, 1, 2).to(dev)
    bd = bi.float().to(dev)
    assert xd.is_contiguous(memory_format=CL) and rd.is_contiguous(memory_format=CL)
    sc = 2.0 ** -ACT_SCALE_LOG2
    for dom, k in ((0, 1.0), (1, sc)):
        y = conv1x1(xd * k, wp, bd * k, rd * k, stride=stride, relu=True, act_domain=dom).cpu() / k
        y0 = conv1x1(xd * k, wp, bd * k, stride=stride, relu=False, act_domain=dom).cpu() / k
        for name, got, want in (("residual+relu", y, want_res), ("plain", y0, want_plain)):
            if not torch.equal(got, want):
                bad = (got != want).nonzero()
                i, c, yy, xx = bad[0].tolist()
                raise AssertionError(f"conv1x1 {CI}->{CO} @{S}/{stride} B={B} {form_1x1(B, S, CI, CO, stride)} domain {dom} {name}: {bad.shape[0]} of "
                                     f"{got.numel()} outputs differ; first (image, channel, y, x) = {(i, c, yy, xx)}: got {float(got[i, c, yy, xx])!r}, "
                                     f"want {float(want[i, c, yy, xx])!r}")


@pytest.mark.parametrize("S,C,B", S2_FLAT)
def test_conv3x3s2_addressing_is_exact(dev, S, C, B):
    """As test_conv1x1_addressing_is_exact for hdn_conv3x3s2_f32 in every K-slice form: the one 1.0 of output channel co sits at input channel
    (5 co + 3) mod C, tap co mod 9, so out[b, co, oy, ox] = relu(x[b, ci, 2 oy + ky - 1, 2 ox + kx - 1] (a padding zero outside) + bias[co]) exactly:
    an image, channel, tap, padding or slice mix-up anywhere in the batch fails torch.equal."""
    from hdn_amd.trunk import ACT_SCALE_LOG2, conv3x3s2, pack_conv3x3s2
    xi = _codes((B, 2 * S, 2 * S, C))                                            # NHWC
    bi = (torch.arange(C, dtype=torch.int64) * 37) % 201 - 100
    src, tap = (5 * torch.arange(C) + 3) % C, torch.arange(C) % 9
    w = torch.zeros(C, C, 3, 3)
    w[torch.arange(C), src, tap // 3, tap % 3] = 1.0
    xp = F.pad(xi, (0, 0, 1, 1, 1, 1))                                           # one pixel of zeros around [.., 2S, 2S, ..]
    want = torch.empty(B, S, S, C, dtype=torch.int64)
    for t in range(9):
        ky, kx = t // 3, t % 3
        co = (tap == t).nonzero().flatten()
        want[..., co] = xp[:, ky:ky + 2 * S:2, kx:kx + 2 * S:2, :][..., src[co]]
    want = torch.relu(want + bi).float().permute(0, 3, 1, 2)
    wp = pack_conv3x3s2(w).to(dev)
    xd, bd = xi.float().permute(0, 3, 1, 2).to(dev), bi.float().to(dev)
    assert xd.is_contiguous(memory_format=CL)
    sc = 2.0 ** -ACT_SCALE_LOG2
    for dom, k in ((0, 1.0), (1, sc)):
        got = conv3x3s2(xd * k, wp, bd * k, act_domain=dom).cpu() / k
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            i, c, yy, xx = bad[0].tolist()
            raise AssertionError(f"conv3x3s2 ({S}, {C}) B={B} form {form_s2(B, S, C)} domain {dom}: {bad.shape[0]} of {got.numel()} outputs differ; first "
                                 f"(image, channel, y, x) = {(i, c, yy, xx)}: got {float(got[i, c, yy, xx])!r}, want {float(want[i, c, yy, xx])!r}")


# ----------------------------------------------------------------------------------------------------------------- large magnitudes, guard off
def _held(y, t64, ref32, reached, what):
    """test_fp16_piece_range_guard's check: finite, and the outputs the large element reaches and the others each within the float64 bound against
    their own scale."""
    y, t64, ref32 = y.detach().cpu().double(), t64.double(), ref32.double()
    assert torch.isfinite(y).all(), what
    for name, m in (("reached", reached), ("others", ~reached)):
        assert m.any()
        e_ref, scale = float((ref32[m] - t64[m]).abs().max()), float(t64[m].abs().max())
        err = float((y[m] - t64[m]).abs().max())
        print(f"FORMS range {what} {name}: err {err:.3e}, e_ref {e_ref:.3e}, scale {scale:.4g}, bound {4 * e_ref + 1e-5 * scale:.3e}")
        assert err <= 4 * e_ref + 1e-5 * scale, (what, name, err, e_ref, scale)


def test_large_magnitudes_with_the_guard_off(dev):
    """include/hdn_hip.h: with the range guard off hdn_conv1x1_f32 and hdn_conv3x3s2_f32 are finite and fp32-accurate for |x| < 1.67e7.  One element of
    7e4 and of 1e7 (-1e7 for the 1x1 without ReLU) in the LAST image: hdn_conv3x3s2_f32 in a sliced and in the fused form, hdn_conv1x1_f32 in the
    small-M and in a large form, both act_domains each; 1.6e7 stays finite."""
    from hdn_amd.trunk import ACT_SCALE_LOG2, conv1x1, conv3x3s2, pack_conv1x1, pack_conv3x3s2
    lib = _lib()
    sc, un = 2.0 ** -ACT_SCALE_LOG2, 2.0 ** ACT_SCALE_LOG2
    prev = lib.hdn_set_check_range(0)
    try:
        g = torch.Generator().manual_seed(77)
        S, C = 16, 128
        w = torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
        b = torch.randn(C, generator=g) * 0.1
        wp, bd = pack_conv3x3s2(w).to(dev), b.to(dev)
        for B, want_form in ((3, "4x3"), (64, "fused")):
            assert form_s2(B, S, C) == want_form
            x = torch.randn(B, C, 2 * S, 2 * S, generator=g).clamp_min_(0)
            for big in (7.0e4, 1.0e7):
                xb = x.clone()
                xb[B - 1, 17, 7, 9] = big                                        # input pixel (7, 9): the windows of outputs (3..4, 4..5)
                t = torch.relu(F.conv2d(xb.double(), w.double(), b.double(), stride=2, padding=1))
                ref = torch.relu(F.conv2d(xb, w, b, stride=2, padding=1))
                reached = torch.zeros_like(t, dtype=torch.bool)
                reached[B - 1, :, 3:5, 4:6] = True
                xd = xb.to(dev).contiguous(memory_format=CL)
                _held(conv3x3s2(xd, wp, bd), t, ref, reached, f"conv3x3s2 {want_form} {big:g} domain 0")
                _held(conv3x3s2((xd * sc).contiguous(memory_format=CL), wp, bd * sc, act_domain=1) * un, t, ref, reached,
                      f"conv3x3s2 {want_form} {big:g} domain 1")
            xb = x.clone()
            xb[B - 1, 17, 7, 9] = 1.6e7
            xd = xb.to(dev).contiguous(memory_format=CL)
            assert torch.isfinite(conv3x3s2(xd, wp, bd)).all()
            assert torch.isfinite(conv3x3s2((xd * sc).contiguous(memory_format=CL), wp, bd * sc, act_domain=1)).all()
        CI, CO, S1 = 256, 64, 32
        w1 = torch.randn(CO, CI, 1, 1, generator=g) * (2.0 / CI) ** 0.5
        b1 = torch.randn(CO, generator=g) * 0.1
        wp1, bd1 = pack_conv1x1(w1).to(dev), b1.to(dev)
        for B, want_form in ((2, "Cfg<1,1,1,4>"), (64, "Cfg<2,4,1,1>")):
            assert form_1x1(B, S1, CI, CO, 1) == want_form
            x = torch.randn(B, CI, S1, S1, generator=g).clamp_min_(0)
            r = torch.randn(B, CO, S1, S1, generator=g)
            rd = r.to(dev).contiguous(memory_format=CL)
            for big, full in ((7.0e4, True), (-1.0e7, False)):                  # with residual + ReLU / without both
                xb = x.clone()
                xb[B - 1, 201, 30, 29] = big
                conv, conv32 = F.conv2d(xb.double(), w1.double(), b1.double()), F.conv2d(xb, w1, b1)
                t, ref = (torch.relu(conv + r.double()), torch.relu(conv32 + r)) if full else (conv, conv32)
                reached = torch.zeros_like(t, dtype=torch.bool)
                reached[B - 1, :, 30, 29] = True
                xd = xb.to(dev).contiguous(memory_format=CL)
                for dom, k in ((0, 1.0), (1, sc)):
                    xk = (xd * k).contiguous(memory_format=CL)
                    got = conv1x1(xk, wp1, bd1 * k, (rd * k).contiguous(memory_format=CL) if full else None, relu=full, act_domain=dom) / k
                    _held(got, t, ref, reached, f"conv1x1 {want_form} {big:g} domain {dom}")
            xb = x.clone()
            xb[B - 1, 201, 30, 29] = -1.6e7
            xd = xb.to(dev).contiguous(memory_format=CL)
            assert torch.isfinite(conv1x1(xd, wp1, bd1, relu=False)).all()
            assert torch.isfinite(conv1x1((xd * sc).contiguous(memory_format=CL), wp1, bd1 * sc, relu=False, act_domain=1)).all()
    finally:
        lib.hdn_set_check_range(prev)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------- the trunk between the tested batches
@pytest.fixture(scope="module")
def trunk50(dev):
    import make_golden as mg
    from hdn_amd.trunk import fold_for_inference, resnet50_homo
    seeded = lambda: mg.seeded_trunk_state_(resnet50_homo().eval())
    fast = fold_for_inference(seeded().to(dev), channels_last=True, fused_stem=True, fused_epilogue=True)
    return fast, seeded().double()


@pytest.mark.parametrize("B", [5, 16, 33])
def test_folded_resnet50_trunk_between_the_tested_batches(dev, trunk50, monkeypatch, B):
    """The folded HIP ResNet-50 trunk at B = 5, 16 (BatchedDeviceTracker's benchmarked n) and 33 - both sides of V2_MIN_BATCH = 24 and of several
    1x1 / stride-2 form switches - with torch.nn.functional.conv2d raising, against the float64 forward of the same seeded model on EVERY image:
    within 1e-4 of the image's max |truth|."""
    fast, m64 = trunk50

    def no_conv2d(*a, **k):
        raise AssertionError("F.conv2d called by the folded ResNet-50 trunk")

    x = torch.from_numpy(np.random.default_rng(500 + B).standard_normal((B, 2, 127, 127)).astype(np.float32))
    monkeypatch.setattr(torch.nn.functional, "conv2d", no_conv2d)
    with torch.no_grad():
        y = fast(x.to(dev)).cpu().double()
    monkeypatch.undo()
    with torch.no_grad():
        t = m64(x.double())
    assert y.shape == t.shape == (B, 2048, 4, 4) and torch.isfinite(y).all()
    d = (y - t).abs()
    err, scale = d.flatten(1).amax(1), t.abs().flatten(1).amax(1)
    i = int(torch.argmax(err / scale))
    c, yy, xx = np.unravel_index(int(torch.argmax(d[i])), tuple(d.shape[1:]))
    print(f"FORMS trunk B={B}: worst image {i}: err {float(err[i]):.3e}, bound {1e-4 * float(scale[i]):.3e}")
    assert bool((err <= 1e-4 * scale).all()), (B, "worst (image, channel, y, x)", (i, int(c), int(yy), int(xx)), float(err[i]), float(scale[i]))
