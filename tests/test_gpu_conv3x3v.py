"""hdn_conv3x3v_f32 (csrc/conv3x3d.hip with the padding-0 pixel map: stride 1 / 2, the two 3x3 convolutions of layer2's first block) on the device:
against float64 in every launch form, exact addressing with integer data, one nonzero input pixel, the range guard.  The float64 side is F.conv2d on
the CPU, computed once per case and shared by the relu / bias / act_domain variants; the integer expectations are tests/simi_full_cases.py's, which
tests/test_simi_full_host.py checks against float64 without a GPU."""
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


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def form_name(B, S, CI, CO, st):
    from hdn_amd import _lib
    return SC.v_form_name(_lib.load().hdn_conv3x3v_form(B, S, CI, CO, st))


@functools.lru_cache(maxsize=None)
def problem(B, S, CI, CO, st):
    """(x, w, bias, float64 convolution, CPU fp32 convolution) of a case, computed once: post-ReLU-like inputs, He-scaled weights."""
    g = torch.Generator().manual_seed(1000 * S + CI + CO + st + B)
    x = torch.randn(B, CI, S, S, generator=g).clamp_min_(0)
    w = torch.randn(CO, CI, 3, 3, generator=g) * (2.0 / (9 * CI)) ** 0.5
    b = torch.randn(CO, generator=g) * 0.2
    return x, w, b, F.conv2d(x.double(), w.double(), None, st), F.conv2d(x, w, None, st)


def check_per_image(what, got, truth, ref32):
    """For every image of the batch on its own: err <= 4 e_ref + 1e-5 scale, e_ref the error of PyTorch's CPU fp32 convolution on that image and scale
    its max |truth| (the project's bound: tests/test_gpu_conv3x3d.py).  Prints the image closest to its bound; returns the largest err / bound."""
    got = got.detach().cpu().double()
    assert got.shape == truth.shape and torch.isfinite(got).all(), what
    err = (got - truth).abs().flatten(1).amax(1)
    e_ref = (ref32.double() - truth).abs().flatten(1).amax(1)
    scale = truth.abs().flatten(1).amax(1)
    bound = 4 * e_ref + 1e-5 * scale
    i = int(torch.argmax(err / bound))
    print(f"FORMS conv3x3v {what}: worst image {i} of {got.shape[0]}: err {float(err[i]):.3e}, e_ref {float(e_ref[i]):.3e}, scale {float(scale[i]):.3f}, "
          f"bound {float(bound[i]):.3e}, err/bound {float(err[i] / bound[i]):.3f}")
    assert bool((err <= bound).all()), (what, i, float(err[i]), float(e_ref[i]), float(scale[i]), float(bound[i]))
    return float((err / bound).max())


def test_cases_cover_every_form():
    """The five forms of dispatch() (A / B, each whole or K-split, and C), each case under the form the list names (host query only)."""
    for name, cases in SC.V_CASES.items():
        for c in cases:
            assert form_name(*c) == name, (c, form_name(*c), name)
    assert set(SC.V_CASES) == {"A", "A split", "B", "B split", "C"}


@pytest.mark.parametrize("B,S,CI,CO,st", SC.V_ALL)
def test_conv3x3v_vs_float64(dev, B, S, CI, CO, st):
    """Every image within 4 e_ref + 1e-5 scale of float64, with and without ReLU, with a bias and with NULL, in both activation domains; two calls are
    bit-equal (K-split forms add their slices in a fixed order)."""
    from hdn_amd.trunk import ACT_SCALE_LOG2, conv3x3v, pack_conv3x3d
    sc = 2.0 ** -ACT_SCALE_LOG2
    x, w, b, t64, r32 = problem(B, S, CI, CO, st)
    So = SC.v_out_side(S, st)
    wp, xd, bd = pack_conv3x3d(w).to(dev), x.to(dev).contiguous(memory_format=CL), b.to(dev)
    name = f"{(B, S, CI, CO, st)} {form_name(B, S, CI, CO, st)}"
    for bias in (True, False):
        t, r = (t64 + b.double().view(1, -1, 1, 1), r32 + b.view(1, -1, 1, 1)) if bias else (t64, r32)
        for relu in (False, True):
            tt, rr = (torch.relu(t), torch.relu(r)) if relu else (t, r)
            for dom, k in ((0, 1.0), (1, sc)):
                args = ((xd * k).contiguous(memory_format=CL), wp, (bd * k) if bias else None)
                got = conv3x3v(*args, stride=st, relu=relu, act_domain=dom)
                assert got.shape == (B, CO, So, So) and got.is_contiguous(memory_format=CL)
                again = conv3x3v(*args, stride=st, relu=relu, act_domain=dom)
                assert torch.equal(got, again), name
                check_per_image(f"{name} bias {bias} relu {relu} domain {dom}", got / k, tt, rr)


@pytest.mark.parametrize("B,S,CI,CO,st", SC.V_EXACT)
def test_conv3x3v_addressing_is_exact(dev, B, S, CI, CO, st):
    """Integer inputs in [-4, 4] and integer weights in [-2, 2]: every piece, product and partial sum is exact, so the output must EQUAL the integer
    truth — a wrong tap, stride, offset or slice shows as a wrong integer, not as a rounding."""
    from hdn_amd.trunk import ACT_SCALE_LOG2, conv3x3v, pack_conv3x3d
    sc = 2.0 ** -ACT_SCALE_LOG2
    x, w, b, want = SC.v_integer_problem(B, S, CI, CO, st)
    assert int(want.abs().max()) < 2 ** 20
    x, w, b, want = x.float(), w.float(), b.float(), want.float()
    wp, xd, bd = pack_conv3x3d(w).to(dev), x.to(dev).contiguous(memory_format=CL), b.to(dev)
    for dom, k in ((0, 1.0), (1, sc)):
        got = conv3x3v((xd * k).contiguous(memory_format=CL), wp, bd * k, stride=st, relu=False, act_domain=dom).cpu() / k
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            i, c, yy, xx = bad[0].tolist()
            raise AssertionError(f"{(B, S, CI, CO, st)} {form_name(B, S, CI, CO, st)} domain {dom}: {bad.shape[0]} of {got.numel()} outputs differ; first "
                                 f"(image, channel, y, x) = {(i, c, yy, xx)}: got {float(got[i, c, yy, xx])!r}, want {float(want[i, c, yy, xx])!r}")


@pytest.mark.parametrize("st", [1, 2])
def test_one_input_pixel_reaches_only_its_outputs(dev, st):
    """One nonzero input element at a corner, an edge and an interior position (and, at stride 2, on an odd row and column): exactly the outputs (oy, ox)
    with st oy + ky == y0 and st ox + kx == x0 are nonzero, each w[co][c][ky][kx] times it, only in that image.  At stride 2 a pixel on an odd row and
    column reaches at most one output (ky = kx = 1)."""
    from hdn_amd.trunk import conv3x3v, pack_conv3x3d
    B, S, CI, CO = 3, 9, 64, 32
    So = SC.v_out_side(S, st)
    w = torch.randint(1, 6, (CO, CI, 3, 3), generator=torch.Generator().manual_seed(st)).float()
    wp = pack_conv3x3d(w).to(dev)
    for (b0, c0, y0, x0) in ((1, 37, 4, 4), (2, 5, 0, 0), (0, 63, 8, 3), (1, 9, 3, 5), (0, 1, 8, 8)):
        x = torch.zeros(B, CI, S, S)
        x[b0, c0, y0, x0] = 3.0
        got = conv3x3v(x.to(dev).contiguous(memory_format=CL), wp, None, stride=st, relu=False).cpu()
        want = torch.zeros(B, CO, So, So)
        n = 0
        for ky in range(3):
            for kx in range(3):
                yy, xx = y0 - ky, x0 - kx
                if yy % st == 0 and xx % st == 0 and 0 <= yy // st < So and 0 <= xx // st < So:
                    want[b0, :, yy // st, xx // st] = 3.0 * w[:, c0, ky, kx]
                    n += 1
        if st == 2 and y0 % 2 and x0 % 2:
            assert n == 1
        if (y0, x0) == (4, 4):
            assert n == (9 if st == 1 else 4)
        if (y0, x0) in ((0, 0), (8, 8)):
            assert n == 1
        assert int((got != 0).any(1).sum()) == n, (st, (b0, c0, y0, x0), int((got != 0).any(1).sum()), n)
        assert torch.equal(got, want), (st, (b0, c0, y0, x0))


def test_conv3x3v_range_guard(dev):
    """The fp16-piece range guard (hdn_set_check_range): with it on, a stored 7e4 in the scaled domain (where the first piece is fp16(x) itself) is refused
    with HDN_E_LIMIT and nothing is launched; with it off, 6e4 — in either domain — is finite and meets the float64 bound, on the outputs the large
    element reaches and on the others, each against its own scale."""
    from hdn_amd import _lib
    from hdn_amd.trunk import conv3x3v, pack_conv3x3d
    lib = _lib.load()
    B, S, CI, CO, st = 2, 15, 128, 128, 2
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, CI, S, S, generator=g).clamp_min_(0)
    w = torch.randn(CO, CI, 3, 3, generator=g) * (2.0 / (9 * CI)) ** 0.5
    b = torch.randn(CO, generator=g) * 0.2
    wp, bd = pack_conv3x3d(w).to(dev), b.to(dev)
    prev = lib.hdn_set_check_range(1)
    try:
        xb = x.clone()
        xb[B - 1, 77, 6, 9] = 7.0e4
        with pytest.raises(ValueError):
            conv3x3v(xb.to(dev).contiguous(memory_format=CL), wp, bd, stride=st, act_domain=1)
        assert torch.isfinite(conv3x3v(x.to(dev).contiguous(memory_format=CL), wp, bd, stride=st)).all()
        lib.hdn_set_check_range(0)
        xb[B - 1, 77, 6, 9] = 6.0e4
        t = torch.relu(F.conv2d(xb.double(), w.double(), b.double(), st))
        r = torch.relu(F.conv2d(xb, w, b, st))
        reached = torch.zeros_like(t, dtype=torch.bool)
        for yy in (2, 3):                                     # 2 oy + ky == 6 (ky = 2, 0), 2 ox + kx == 9 (kx = 1)
            reached[B - 1, :, yy, 4] = True
        moved = (t != torch.relu(F.conv2d(x.double(), w.double(), b.double(), st))).any(1)
        assert bool(moved.any()) and not bool((moved & ~reached.any(1)).any())          # the large element changes those two positions only
        xd = xb.to(dev).contiguous(memory_format=CL)
        for dom in (0, 1):            # (domain 1: the same numbers read as stored values; the convolution is linear and the bias is handed over as is)
            y = conv3x3v(xd, wp, bd, stride=st, act_domain=dom).cpu().double()
            assert torch.isfinite(y).all()
            for name, m in (("reached", reached), ("others", ~reached)):
                e_ref, scale = float((r.double()[m] - t[m]).abs().max()), float(t[m].abs().max())
                err = float((y[m] - t[m]).abs().max())
                print(f"FORMS conv3x3v range domain {dom} {name}: err {err:.3e}, e_ref {e_ref:.3e}, scale {scale:.4g}, bound {4 * e_ref + 1e-5 * scale:.3e}")
                assert err <= 4 * e_ref + 1e-5 * scale, (dom, name, err, e_ref, scale)
    finally:
        lib.hdn_set_check_range(prev)
    torch.cuda.synchronize()
