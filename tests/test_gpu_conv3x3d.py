"""hdn_conv3x3d_f32 (csrc/conv3x3d.hip: the dilated 3x3 convolution of the similarity backbone on the matrix cores) on the device: against float64 in
every launch form, exact addressing with integer data, argument errors, the range guard.  The float64 side is F.conv2d on the CPU, computed once per
case and shared by the relu / bias / act_domain variants."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last

# (B, S, CI, CO, d): the smallest shapes that reach each way of going wrong
CASES = [(1, 3, 64, 64, 4), (2, 2, 32, 32, 2),            # side at or below the dilation: only the centre tap is in bounds
         (2, 5, 32, 96, 2),                               # one K chunk per tap, CO no multiple of 64, two images in one pixel tile
         (3, 7, 96, 32, 1),                               # M = 147: a partial tile
         (1, 15, 128, 256, 4), (2, 15, 256, 128, 2),      # the 127-px crop's side
         (2, 31, 64, 128, 4), (1, 31, 256, 256, 2),       # the 255-px crop's side, the real layer-3 shape
         (1, 5, 1024, 128, 2),                            # long K
         (1, 5, 64, 2048, 1),                             # wide N
         (1, 63, 64, 64, 1),                              # layer 1
         # the smallest case of each form the list above does not reach (all of it is K-split A or B):
         (3, 63, 32, 96, 1),                              # A unsplit: 94 x 3 = 282 workgroups
         (1, 63, 32, 512, 1),                             # B unsplit: 32 x 8 = 256 workgroups
         (1, 63, 32, 1024, 1)]                            # C: 32 x 8 = 256 workgroups of 128 x 128
ALL_FORMS = {"A", "A split", "B", "B split", "C"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _lib():
    from hdn_amd import _lib as L
    return L.load()


def form_name(B, S, CI, CO, d):
    v = _lib().hdn_conv3x3d_form(B, S, CI, CO, d)
    assert v > 0, (v, B, S, CI, CO, d)
    cfg = (v & 15, (v >> 4) & 15, (v >> 8) & 15, (v >> 12) & 15)
    name = {(1, 1, 4, 1): "A", (1, 2, 4, 1): "B", (2, 2, 2, 2): "C"}[cfg]
    return name + (" split" if (v >> 16) > 1 else "")


@functools.lru_cache(maxsize=None)
def problem(B, S, CI, CO, d):
    """(x, w, bias, float64 convolution, CPU fp32 convolution) of a case, computed once: post-ReLU-like inputs, He-scaled weights."""
    g = torch.Generator().manual_seed(1000 * S + CI + CO + d + B)
    x = torch.randn(B, CI, S, S, generator=g).clamp_min_(0)
    w = torch.randn(CO, CI, 3, 3, generator=g) * (2.0 / (9 * CI)) ** 0.5
    b = torch.randn(CO, generator=g) * 0.2
    t64 = F.conv2d(x.double(), w.double(), None, 1, d, d)
    r32 = F.conv2d(x, w, None, 1, d, d)
    return x, w, b, t64, r32


def check_per_image(what, got, truth, ref32):
    """For every image of the batch on its own: err <= 4 e_ref + 1e-5 scale, e_ref the error of PyTorch's CPU fp32 convolution on that image and scale
    its max |truth| (the bound of tests/test_gpu_trunk50_forms.py).  Returns the largest err / bound."""
    got = got.detach().cpu().double()
    assert got.shape == truth.shape and torch.isfinite(got).all(), what
    err = (got - truth).abs().flatten(1).amax(1)
    e_ref = (ref32.double() - truth).abs().flatten(1).amax(1)
    scale = truth.abs().flatten(1).amax(1)
    bound = 4 * e_ref + 1e-5 * scale
    i = int(torch.argmax(err / bound))
    print(f"CONV3X3D {what}: worst image {i} of {got.shape[0]}: err {float(err[i]):.3e}, e_ref {float(e_ref[i]):.3e}, scale {float(scale[i]):.3f}, "
          f"bound {float(bound[i]):.3e}")
    assert bool((err <= bound).all()), (what, i, float(err[i]), float(e_ref[i]), float(scale[i]), float(bound[i]))
    return float((err / bound).max())


def test_cases_cover_every_form():
    """dispatch() of csrc/conv3x3d.hip has five forms (A / B, each whole or K-split, and C); the case list reaches every one (host query only)."""
    seen = {form_name(*c) for c in CASES}
    assert seen == ALL_FORMS, seen


@pytest.mark.parametrize("B,S,CI,CO,d", CASES)
def test_conv3x3d_vs_float64(dev, B, S, CI, CO, d):
    """Every image within 4 e_ref + 1e-5 scale of float64, with and without ReLU, with a bias and with NULL, in both activation domains; two calls are
    bit-equal (K-split forms add their slices in a fixed order)."""
    from hdn_amd.trunk import ACT_SCALE_LOG2, conv3x3d, pack_conv3x3d
    sc = 2.0 ** -ACT_SCALE_LOG2
    x, w, b, t64, r32 = problem(B, S, CI, CO, d)
    wp, xd, bd = pack_conv3x3d(w).to(dev), x.to(dev).contiguous(memory_format=CL), b.to(dev)
    name = f"{(B, S, CI, CO, d)} {form_name(B, S, CI, CO, d)}"
    for bias in (True, False):
        t, r = (t64 + b.double().view(1, -1, 1, 1), r32 + b.view(1, -1, 1, 1)) if bias else (t64, r32)
        for relu in (False, True):
            tt, rr = (torch.relu(t), torch.relu(r)) if relu else (t, r)
            for dom, k in ((0, 1.0), (1, sc)):
                args = ((xd * k).contiguous(memory_format=CL), wp, (bd * k) if bias else None)
                got = conv3x3d(*args, dilation=d, relu=relu, act_domain=dom)
                assert got.shape == (B, CO, S, S) and got.is_contiguous(memory_format=CL)
                again = conv3x3d(*args, dilation=d, relu=relu, act_domain=dom)
                assert torch.equal(got, again), name
                check_per_image(f"{name} bias {bias} relu {relu} domain {dom}", got / k, tt, rr)


@pytest.mark.parametrize("B,S,CI,CO,d", [(2, 5, 32, 96, 2), (1, 31, 64, 64, 4), (3, 7, 96, 32, 1)])
def test_conv3x3d_addressing_is_exact(dev, B, S, CI, CO, d):
    """Integer inputs in [-4, 4] and integer weights in [-2, 2]: every piece, product and partial sum is exact, so the output must EQUAL the integer
    truth — a wrong tap, offset, border or slice shows as a wrong integer, not as a rounding."""
    from hdn_amd.trunk import ACT_SCALE_LOG2, conv3x3d, pack_conv3x3d
    sc = 2.0 ** -ACT_SCALE_LOG2
    g = torch.Generator().manual_seed(5 + S)
    x = torch.randint(-4, 5, (B, CI, S, S), generator=g).float()
    w = torch.randint(-2, 3, (CO, CI, 3, 3), generator=g).float()
    b = torch.randint(-9, 10, (CO,), generator=g).float()
    want = F.conv2d(x.double(), w.double(), b.double(), 1, d, d).float()
    assert float(want.abs().max()) < 2 ** 20
    wp, xd, bd = pack_conv3x3d(w).to(dev), x.to(dev).contiguous(memory_format=CL), b.to(dev)
    for dom, k in ((0, 1.0), (1, sc)):
        got = conv3x3d((xd * k).contiguous(memory_format=CL), wp, bd * k, dilation=d, relu=False, act_domain=dom).cpu() / k
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            i, c, yy, xx = bad[0].tolist()
            raise AssertionError(f"{(B, S, CI, CO, d)} {form_name(B, S, CI, CO, d)} domain {dom}: {bad.shape[0]} of {got.numel()} outputs differ; first "
                                 f"(image, channel, y, x) = {(i, c, yy, xx)}: got {float(got[i, c, yy, xx])!r}, want {float(want[i, c, yy, xx])!r}")


@pytest.mark.parametrize("d", [1, 2, 4])
def test_one_input_pixel_reaches_its_nine_outputs(dev, d):
    """One nonzero input element: exactly the outputs at (y0 - (ky - 1) d, x0 - (kx - 1) d) are nonzero, each w[co][c][ky][kx] times it — nine positions
    for an interior pixel, fewer at the border — and only in that image."""
    from hdn_amd.trunk import conv3x3d, pack_conv3x3d
    B, S, CI, CO = 3, 9, 64, 32
    g = torch.Generator().manual_seed(d)
    w = torch.randint(1, 6, (CO, CI, 3, 3), generator=g).float()
    wp = pack_conv3x3d(w).to(dev)
    for (b0, c0, y0, x0) in ((1, 37, 4, 4), (2, 5, 0, 8), (0, 63, 8, 3)):
        x = torch.zeros(B, CI, S, S)
        x[b0, c0, y0, x0] = 3.0
        got = conv3x3d(x.to(dev).contiguous(memory_format=CL), wp, None, dilation=d, relu=False).cpu()
        want = torch.zeros(B, CO, S, S)
        n = 0
        for ky in range(3):
            for kx in range(3):
                yy, xx = y0 - (ky - 1) * d, x0 - (kx - 1) * d
                if 0 <= yy < S and 0 <= xx < S:
                    want[b0, :, yy, xx] = 3.0 * w[:, c0, ky, kx]
                    n += 1
        assert n == 9 if (y0, x0) == (4, 4) else n < 9
        assert int((got != 0).any(1).sum()) == n, (d, (b0, c0, y0, x0), int((got != 0).any(1).sum()), n)
        assert torch.equal(got, want), (d, (b0, c0, y0, x0))


def test_conv3x3d_argument_errors(dev):
    """Each return code once, nothing launched: NULL, shape, limit (misaligned pointer, short workspace), alias; the wrapper's own checks."""
    from hdn_amd import _lib
    from hdn_amd.trunk import conv3x3d, pack_conv3x3d
    lib = _lib.load()
    B, S, CI, CO, d = 2, 5, 32, 96, 2
    # x and out are cut from ONE allocation with a gap: `x + 1 float` then overlaps nothing, wherever the caching allocator put the tests before this one
    # (with two allocations `out` can lie right behind `x`, and the entry point rightly answers HDN_E_ALIAS before it looks at the alignment)
    n_x, n_out, gap = B * S * S * CI, B * S * S * CO, 64
    arena = torch.empty(n_x + gap + n_out, device=dev)
    x = arena[:n_x].view(B, S, S, CI).permute(0, 3, 1, 2).copy_(torch.rand(B, CI, S, S, device=dev))
    out = arena[n_x + gap:].view(B, S, S, CO).permute(0, 3, 1, 2)
    assert x.is_contiguous(memory_format=CL) and out.is_contiguous(memory_format=CL)
    wp = pack_conv3x3d(torch.randn(CO, CI, 3, 3) * 0.05).to(dev)
    b = torch.zeros(CO, device=dev)
    nws = lib.hdn_conv3x3d_workspace_bytes(B, S, CI, CO, d)
    assert nws > 0
    ws = torch.empty(nws // 4, device=dev)
    p, s, f = _lib.ptr, _lib.stream_ptr(dev), lib.hdn_conv3x3d_f32
    assert f(None, p(wp), p(b), p(out), p(ws), nws, B, S, CI, CO, d, 1, 0, s) == -1
    assert f(p(x), p(wp), p(b), p(out), None, 0, B, S, CI, CO, d, 1, 0, s) == -1                            # a K-split form without its workspace
    assert f(p(x), p(wp), p(b), p(out), p(ws), nws, B, S, CI, CO, 3, 1, 0, s) == -2
    assert f(p(x), p(wp), p(b), p(out), p(ws), nws, B, S, 48, CO, d, 1, 0, s) == -2
    assert f(p(x), p(wp), p(b), p(out), p(ws), nws, B, S, CI, CO, d, 2, 0, s) == -2
    assert f(p(x), p(wp), p(b), p(out), p(ws), nws, B, S, CI, CO, d, 1, 2, s) == -2
    assert f(ctypes.c_void_p(x.data_ptr() + 4), p(wp), p(b), p(out), p(ws), nws, B, S, CI, CO, d, 1, 0, s) == -3   # x + 1 float: misaligned
    assert f(p(x), p(wp), p(b), p(out), p(ws), nws - 4, B, S, CI, CO, d, 1, 0, s) == -3
    assert f(p(x), p(wp), p(b), p(x), p(ws), nws, B, S, CI, CO, d, 1, 0, s) == -4                           # out == x
    assert f(p(x), p(wp), p(b), p(out), p(out), nws, B, S, CI, CO, d, 1, 0, s) == -4                        # ws == out
    with pytest.raises(ValueError):
        conv3x3d(x.contiguous(), wp, b, dilation=d)                       # NCHW input
    with pytest.raises(ValueError):
        conv3x3d(x, wp[:-8], b, dilation=d)
    with pytest.raises(ValueError):
        conv3x3d(x, wp, b, dilation=3)
    torch.cuda.synchronize()
    assert f(p(x), p(wp), p(b), p(out), p(ws), nws, B, S, CI, CO, d, 1, 0, s) == 0
    torch.cuda.synchronize()


def test_conv3x3d_range_guard(dev):
    """The fp16-piece range guard (hdn_set_check_range): with it on, a stored 7e4 in the scaled domain (where the first piece is fp16(x) itself: the
    limit is 65,520) and 2e7 in real units are refused with HDN_E_LIMIT and nothing is launched; with it off, 6e4 — in either domain — is finite and
    meets the float64 bound, on the outputs the large element reaches and on the others, each against its own scale."""
    from hdn_amd import _lib
    from hdn_amd.trunk import conv3x3d, pack_conv3x3d
    lib = _lib.load()
    B, S, CI, CO, d = 2, 15, 128, 256, 4
    x, w, b, _, _ = problem(1, S, CI, CO, d)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, CI, S, S, generator=g).clamp_min_(0)
    wp, bd = pack_conv3x3d(w).to(dev), b.to(dev)
    prev = lib.hdn_set_check_range(1)
    try:
        for big, dom in ((7.0e4, 1), (2.0e7, 0)):
            xb = x.clone()
            xb[B - 1, 77, 6, 9] = big
            with pytest.raises(ValueError):
                conv3x3d(xb.to(dev).contiguous(memory_format=CL), wp, bd, dilation=d, act_domain=dom)
        assert torch.isfinite(conv3x3d(x.to(dev).contiguous(memory_format=CL), wp, bd, dilation=d)).all()
        lib.hdn_set_check_range(0)
        xb = x.clone()
        xb[B - 1, 77, 6, 9] = 6.0e4
        t = torch.relu(F.conv2d(xb.double(), w.double(), b.double(), 1, d, d))
        r = torch.relu(F.conv2d(xb, w, b, 1, d, d))
        reached = torch.zeros_like(t, dtype=torch.bool)
        for yy in (2, 6, 10):
            for xx in (5, 9, 13):
                reached[B - 1, :, yy, xx] = True
        xd = xb.to(dev).contiguous(memory_format=CL)
        for dom in (0, 1):            # (domain 1: the same numbers read as stored values; the convolution is linear and the bias is handed over as is)
            y = conv3x3d(xd, wp, bd, dilation=d, act_domain=dom).cpu().double()
            assert torch.isfinite(y).all()
            for name, m in (("reached", reached), ("others", ~reached)):
                e_ref, scale = float((r.double()[m] - t[m]).abs().max()), float(t[m].abs().max())
                err = float((y[m] - t[m]).abs().max())
                print(f"CONV3X3D range domain {dom} {name}: err {err:.3e}, e_ref {e_ref:.3e}, scale {scale:.4g}, bound {4 * e_ref + 1e-5 * scale:.3e}")
                assert err <= 4 * e_ref + 1e-5 * scale, (dom, name, err, e_ref, scale)
    finally:
        lib.hdn_set_check_range(prev)
    torch.cuda.synchronize()
