"""hdn_simi_stem_f32 (csrc/simi_stem.hip: conv 7x7 / stride 2 / padding 0 + shift + ReLU + maxpool 3 / 2 / 1 of the similarity backbone in one launch) on
the device: against float64 at every size of tests/simi_full_cases.py (the smallest, the workload's 127 and 255, one on each side of every boundary of
the workgroup's column tiling), bit-equality across calls and batch sizes, exact results with integer data, every one of the 147 taps named by the
output, the set of outputs one bright pixel reaches, the range guard.  The integer expectations are checked against float64 on the CPU by
tests/test_simi_full_host.py."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import simi_full_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BATCHES = (1, 2, 5)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def chain(x, w, b):
    return F.max_pool2d(torch.relu(F.conv2d(x, w, b, stride=2)), 3, 2, 1)


@functools.lru_cache(maxsize=None)
def weights():
    g = torch.Generator().manual_seed(21)
    return torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5, torch.randn(64, generator=g) * 0.2


@functools.lru_cache(maxsize=None)
def problem(S, pixels):
    """(x [5,3,S,S], float64 chain, CPU fp32 chain) once per size and input scale; the B = 1 / 2 calls take its first images."""
    w, b = weights()
    x = torch.randn(max(BATCHES), 3, S, S, generator=torch.Generator().manual_seed(S + 7 * pixels))
    if pixels:
        x = x * 60 + 110
        b = b * 100
    return x, b, chain(x.double(), w.double(), b.double()), chain(x, w, b)


def check_per_image(what, got, truth, ref32):
    """For every image on its own: err <= 4 e_ref + 1e-5 scale (e_ref: the same chain in fp32 on the CPU; scale: the image's max |truth|)."""
    got = got.detach().cpu().double()
    assert got.shape == truth.shape and torch.isfinite(got).all(), what
    err = (got - truth).abs().flatten(1).amax(1)
    e_ref = (ref32.double() - truth).abs().flatten(1).amax(1)
    scale = truth.abs().flatten(1).amax(1)
    bound = 4 * e_ref + 1e-5 * scale
    i = int(torch.argmax(err / bound))
    print(f"FORMS simi_stem {what}: worst image {i} of {got.shape[0]}: err {float(err[i]):.3e}, e_ref {float(e_ref[i]):.3e}, scale {float(scale[i]):.3f}, "
          f"bound {float(bound[i]):.3e}, err/bound {float(err[i] / bound[i]):.3f}")
    assert bool((err <= bound).all()), (what, i, float(err[i]), float(e_ref[i]), float(scale[i]), float(bound[i]))


@pytest.mark.parametrize("S", SC.STEM_SIZES)
def test_simi_stem_vs_float64(dev, S):
    """Every image within 4 e_ref + 1e-5 scale of float64 max_pool2d(relu(conv2d(x, w) + b), 3, 2, 1), inputs at unit scale and at randn 60 + 110, B = 1, 2, 5
    (the grid is 2 B Sp workgroups: odd and even counts of rows); two calls bit-equal; image 0 of the B = 5 call bit-equal to the same image at B = 1."""
    from hdn_amd.trunk import pack_simi_stem, simi_stem
    w, _ = weights()
    wp = pack_simi_stem(w).to(dev)
    Sc, Sp = SC.stem_sides(S)
    for pixels in (0, 1):
        x, b, t64, r32 = problem(S, pixels)
        xd, bd = x.to(dev), b.to(dev)
        outs = {}
        for B in BATCHES:
            got = simi_stem(xd[:B].contiguous(), wp, bd)
            assert got.shape == (B, 64, Sp, Sp) and got.is_contiguous(memory_format=CL)
            assert torch.equal(got, simi_stem(xd[:B].contiguous(), wp, bd)), (S, B)
            check_per_image(f"S {S} ({Sc}, {Sp}) B {B} pixels {pixels}", got, t64[:B], r32[:B])
            outs[B] = got
        assert torch.equal(outs[5][:1], outs[1]) and torch.equal(outs[5][:2], outs[2]), S


@pytest.mark.parametrize("S", SC.STEM_EXACT_SIZES)
def test_simi_stem_is_exact_on_integers(dev, S):
    """Integer pixels 0..255, weights in {-1, 0, 1} (no two channels and no two taps alike), integer bias: every piece, product and partial sum is exact
    (below 147 x 255 < 2^24), so the output must EQUAL the integer truth — a wrong tap, row, column, tile or pool neighbour shows as a wrong integer."""
    from hdn_amd.trunk import pack_simi_stem, simi_stem
    B = 2
    x, w, b, want = SC.stem_integer_problem(B, S)
    got = simi_stem(x.float().to(dev), pack_simi_stem(w.float()).to(dev), b.float().to(dev)).cpu()
    want = want.float()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i, c, yy, xx = bad[0].tolist()
        raise AssertionError(f"S {S}: {bad.shape[0]} of {got.numel()} outputs differ; first (image, channel, y, x) = {(i, c, yy, xx)}: "
                             f"got {float(got[i, c, yy, xx])!r}, want {float(want[i, c, yy, xx])!r}")


def test_every_tap_is_read_where_the_layout_says(dev):
    """One weight w[co][ci][ky][kx] = 1 per output channel on an image whose pixel value names (ci, y, x): the output names the tap that was read — all 147
    taps, 64 per launch."""
    from hdn_amd.trunk import pack_simi_stem, simi_stem
    x, ws, wants = SC.stem_tap_problem(13)
    xd, zero = x.float().to(dev), torch.zeros(64, device=dev)
    for l, (w, want) in enumerate(zip(ws, wants)):
        got = simi_stem(xd, pack_simi_stem(w.float()).to(dev), zero).cpu()
        if not torch.equal(got, want.float()):
            bad = (got != want.float()).nonzero()
            _, co, p, q = bad[0].tolist()
            t = 64 * l + co
            raise AssertionError(f"tap (ci, ky, kx) = {(t // 49, (t // 7) % 7, t % 7)}: pooled ({p}, {q}) is {float(got[0, co, p, q])!r}, "
                                 f"want {float(want[0, co, p, q])!r} (pixel code 1 + (ci 13 + y) 13 + x)")


@pytest.mark.parametrize("S,y0,x0", [(13, 0, 0), (13, 12, 5), (13, 6, 6), (27, 13, 26), (27, 9, 14), (69, 33, 68), (133, 70, 128)])
def test_one_bright_pixel_reaches_only_its_outputs(dev, S, y0, x0):
    """A single bright pixel in a zero image, all-positive weights, zero bias: exactly the pooled outputs whose pool window covers a conv output whose 7x7
    window covers the pixel are nonzero — in the image that holds it, in every channel."""
    from hdn_amd.trunk import pack_simi_stem, simi_stem
    w = torch.rand(64, 3, 7, 7, generator=torch.Generator().manual_seed(1)) + 0.5
    x = torch.zeros(3, 3, S, S)
    x[1, 2, y0, x0] = 200.0
    got = simi_stem(x.to(dev), pack_simi_stem(w).to(dev), torch.zeros(64, device=dev)).cpu()
    hit = SC.stem_reached(S, y0, x0)
    assert not bool(got[0].any()) and not bool(got[2].any())
    assert torch.equal(got[1] != 0, hit.unsqueeze(0).expand(64, -1, -1)), (S, y0, x0)


def test_simi_stem_range_guard(dev):
    """The range guard (hdn_set_check_range) on x.  The stem takes real units (act_domain 0), where the pieces hold x 2^-8: with the guard on, 2e7 (beyond
    65,520 x 256) is refused with HDN_E_LIMIT and nothing is launched, and 7e4 — refused by the kernels' scaled domain — is inside the range here; with
    the guard off, an image with a 6e4 pixel is finite and meets the float64 bound."""
    from hdn_amd import _lib
    from hdn_amd.trunk import pack_simi_stem, simi_stem
    lib = _lib.load()
    w, b = weights()
    S = 27
    x = torch.randn(2, 3, S, S, generator=torch.Generator().manual_seed(8)) * 60 + 110
    wp, bd = pack_simi_stem(w).to(dev), b.to(dev)
    prev = lib.hdn_set_check_range(1)
    try:
        xb = x.clone()
        xb[1, 1, 9, 14] = 2.0e7
        with pytest.raises(ValueError):
            simi_stem(xb.to(dev), wp, bd)
        xb[1, 1, 9, 14] = 7.0e4
        assert torch.isfinite(simi_stem(xb.to(dev), wp, bd)).all()
        lib.hdn_set_check_range(0)
        xb[1, 1, 9, 14] = 6.0e4
        got = simi_stem(xb.to(dev), wp, bd)
        check_per_image("range 6e4", got, chain(xb.double(), w.double(), b.double()), chain(xb, w, b))
    finally:
        lib.hdn_set_check_range(prev)
    torch.cuda.synchronize()


def test_simi_stem_wrapper_refuses_what_the_kernel_does_not_take(dev):
    from hdn_amd.trunk import pack_simi_stem, simi_stem
    w, b = weights()
    wp, bd = pack_simi_stem(w).to(dev), b.to(dev)
    for bad in (torch.zeros(1, 3, 6, 6), torch.zeros(1, 3, 256, 256), torch.zeros(1, 2, 31, 31), torch.zeros(1, 3, 31, 33)):
        with pytest.raises(ValueError):
            simi_stem(bad.to(dev), wp, bd)
    with pytest.raises(ValueError):
        simi_stem(torch.zeros(1, 3, 31, 31, device=dev).contiguous(memory_format=CL), wp, bd)
    with pytest.raises(ValueError):
        simi_stem(torch.zeros(1, 3, 31, 31, device=dev), wp[:-8], bd)
