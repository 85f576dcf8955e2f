"""Shared by tests/test_gpu_affine_stn.py and tests/test_affine_stn_host.py: the restatements, the float64 closed form with the magnitudes of the bound,
the fixtures and the device runners of the affine spatial transformer (hdn_affine_sample_f32, hdn_affine_sample_bwd_f32, hdn_amd.affine).  The
conventions are those of tests/geometry_bwd_cases.py (read its docstring first); its helpers (worst_ratio, k_bound, at_offset, untouched, OFFSETS, PAD,
FILL, first_difference) are used from there.  Nothing here launches a kernel except the run_* functions.

Restatements: stn_rs = the reference's three lines (theta.view, F.affine_grid, F.grid_sample with PyTorch's defaults) in any dtype; kernel_forward_np =
the statements of sample_point / sample_kernel (csrc/affine_stn.hip) one numpy operation at a time - the coordinate and w, 1 - w, n, 1 - n in float64 from the fp32 theta, each
rounded to fp32 once, the blend in fp32 - which the kernel's forward must equal bit for bit; coords = the coordinate statements in torch, each
op rounded in `dtype` (float64: the kernel's own).

Truth is float64: closed() returns, per element of out, grad_theta and grad_img, the sum and M, the sum of the absolute values of its terms (|grad_out|,
|I_a| + |I_b| for a difference of taps, absolute chain factors).  The host test pins it to float64 autograd through stn_rs at 1e-12 of M.

Cells: a bilinear derivative jumps where px or py crosses an integer, so truth and kernel must agree on the cell of every sample.  The kernel forms px,
py in float64 by the statements of coords(), so the cells its forward picks ARE the float64 cells, at every shape (255 -> 127, where no data keeps a
margin, and the identity, whose centre coordinates are integers exactly, included): closed() takes them from coords(..., cells), cells = float64, the
forward's own restatement.  PyTorch's fp32 path, which gives r_ref, rounds its coordinates in fp32: the random ('similarity', 'classes') fixtures of the
small shapes are redrawn until no px, py is within MARGIN = 1e-4 of an integer (the host test asserts it), so that r_ref is measured on the same cells
there; at 255 -> 127 some of its samples fall into a neighbouring cell and r_ref contains that.

Bound on random data, for out, grad_theta and grad_img: |got - truth| <= K M, K = max(4 r_ref, 2e-6), r_ref = the worst |g32 - truth| / M of PyTorch's
own fp32 CPU path (stn_rs in fp32 and its autograd) on the same fixture, computed here and printed by the tests.

Zeros-padding classes of a sample, per axis: 'in' (both taps inside), 'lo' (x0 = -1: the west / north tap outside), 'hi' (x0 = W - 1: the east / south
tap outside), 'dead' (not strictly inside (-1, W): every tap outside, the kernel's guard)."""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

import geometry_bwd_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 20261020
MARGIN = GC.MARGIN
# (B, C, H, W, Ho, Wo).  Output pixels per sample: 35, 64, 63, 1 (one 256-lane block, one partial per sample), 437 (two blocks, the second with a
# tail of 181), 16129 (64 blocks: exactly one per lane of the reducing wave, the last block holding one pixel).
SMALL_SHAPES = ((2, 3, 9, 11, 5, 7), (3, 1, 8, 8, 8, 8), (1, 2, 5, 4, 7, 9), (1, 1, 2, 2, 1, 1), (2, 2, 13, 17, 19, 23))
LARGE_SHAPE = (2, 3, 255, 255, 127, 127)
SHAPES = SMALL_SHAPES + (LARGE_SHAPE,)
KINDS = ("identity", "similarity", "classes")
# the classes a 'classes' fixture must populate between its samples: (x class, y class)
REQUIRED_CLASSES = (("in", "in"), ("lo", "in"), ("hi", "in"), ("in", "lo"), ("in", "hi"), "corner", "dead")
CLASS_SHAPES = ((2, 3, 9, 11, 5, 7), (3, 1, 8, 8, 8, 8), (2, 2, 13, 17, 19, 23), LARGE_SHAPE)     # enough samples to hold every class


# ================================================================================================================= restatements
def stn_rs(x, theta, size, dtype=torch.float64):
    """ModelBuilder.stn_with_theta's three lines in `dtype`."""
    theta = theta.to(dtype).view(-1, 2, 3)
    grid = F.affine_grid(theta, list(size), align_corners=False)
    return F.grid_sample(x.to(dtype), grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def coords(theta, H, W, Ho, Wo, dtype):
    """(X [Wo], Y [Ho], px, py [B,Ho,Wo]) by the statements of sample_point, each op rounded in `dtype`."""
    t = theta.detach().reshape(-1, 2, 3).to(dtype)
    X = (2 * torch.arange(Wo) + 1).to(dtype) / float(Wo) - 1.0
    Y = (2 * torch.arange(Ho) + 1).to(dtype) / float(Ho) - 1.0
    Xb, Yb = X.reshape(1, 1, Wo), Y.reshape(1, Ho, 1)
    c = lambda r, k: t[:, r, k].reshape(-1, 1, 1)
    gx = (c(0, 0) * Xb + c(0, 1) * Yb) + c(0, 2)
    gy = (c(1, 0) * Xb + c(1, 1) * Yb) + c(1, 2)
    return X, Y, ((gx + 1.0) * float(W) - 1.0) * 0.5, ((gy + 1.0) * float(H) - 1.0) * 0.5


def margin(theta, H, W, Ho, Wo):
    """The distance of the nearest finite px, py (float64) to an integer."""
    _, _, px, py = coords(theta, H, W, Ho, Wo, torch.float64)
    v = torch.cat([px.reshape(-1), py.reshape(-1)])
    v = v[v.isfinite() & (v.abs() < 1e9)]
    return float((v - v.round()).abs().min()) if v.numel() else float("inf")


def axis_class(p, n):
    """Per sample coordinate: 0 'in', 1 'lo', 2 'hi', 3 'dead' (the kernel's float comparisons, then floor)."""
    live = (p > -1.0) & (p < float(n))
    f = torch.where(live, p.floor(), torch.zeros_like(p))
    return torch.where(~live, 3, torch.where(f < 0, 1, torch.where(f + 1 >= n, 2, 0)))


def classes_present(theta, H, W, Ho, Wo, dtype=torch.float64):
    """Which of REQUIRED_CLASSES the samples of the fixture populate."""
    _, _, px, py = coords(theta, H, W, Ho, Wo, dtype)
    cx, cy = axis_class(px, W), axis_class(py, H)
    names = ("in", "lo", "hi")
    got = set()
    for a in range(3):
        for b in range(3):
            if bool(((cx == a) & (cy == b)).any()):
                got.add("corner" if a and b else (names[a], names[b]))
    if bool(((cx == 3) | (cy == 3)).any()):
        got.add("dead")
    if W == 1 or H == 1:
        got.discard("corner")
    return got


def kernel_forward_np(x, theta, Ho, Wo):
    """The forward by the kernel's own statements, one numpy operation at a time (coordinate float64, weights and blend fp32): -> out [B,C,Ho,Wo] float32."""
    f, d = np.float32, np.float64
    x = x.detach().numpy().astype(f)
    t = theta.detach().reshape(-1, 2, 3).numpy().astype(f).astype(d)
    B, C, H, W = x.shape
    with np.errstate(all="ignore"):
        X = ((2 * np.arange(Wo) + 1).astype(d) / d(Wo) - d(1)).reshape(1, 1, Wo)
        Y = ((2 * np.arange(Ho) + 1).astype(d) / d(Ho) - d(1)).reshape(1, Ho, 1)
        c = lambda r, k: t[:, r, k].reshape(B, 1, 1)
        gx = (c(0, 0) * X + c(0, 1) * Y) + c(0, 2)
        gy = (c(1, 0) * X + c(1, 1) * Y) + c(1, 2)
        px = ((gx + d(1)) * d(W) - d(1)) * d(0.5)
        py = ((gy + d(1)) * d(H) - d(1)) * d(0.5)
        live = (px > d(-1)) & (px < d(W)) & (py > d(-1)) & (py < d(H))
        xw = np.where(live, np.floor(px), d(0))
        yn = np.where(live, np.floor(py), d(0))
        dw, dn = np.where(live, px - xw, d(0)), np.where(live, py - yn, d(0))
    assert px.dtype == d and dw.dtype == d
    w, n, e, s = dw.astype(f), dn.astype(f), (d(1) - dw).astype(f), (d(1) - dn).astype(f)
    x0, y0 = xw.astype(np.int64), yn.astype(np.int64)
    west, east, north, south = live & (x0 >= 0), live & (x0 + 1 < W), live & (y0 >= 0), live & (y0 + 1 < H)
    xa, xb, ya, yb = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1), np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
    flat = x.reshape(B, C, H * W)

    def tap(yy, xx, ok):
        idx = np.broadcast_to((yy * W + xx).reshape(B, 1, Ho * Wo), (B, C, Ho * Wo))
        return np.where(ok.reshape(B, 1, Ho, Wo), np.take_along_axis(flat, idx, axis=2).reshape(B, C, Ho, Wo), f(0)).astype(f)

    v_nw, v_ne, v_sw, v_se = tap(ya, xa, north & west), tap(ya, xb, north & east), tap(yb, xa, south & west), tap(yb, xb, south & east)
    u = lambda a: a.reshape(B, 1, Ho, Wo)
    out = ((v_nw * u(s * e) + v_ne * u(s * w)) + v_sw * u(n * e)) + v_se * u(n * w)
    assert out.dtype == f
    return torch.from_numpy(out)


# ================================================================================================================= float64 closed form
def closed(x, theta, Ho, Wo, g, cells=torch.float64):
    """-> dict of float64 (truth, M) pairs: 'out' [B,C,Ho,Wo], 'theta' [B,2,3], 'img' [B,C,H,W].  cells: the dtype whose coordinates decide the guard
    and choose the cell of every sample."""
    B, C, H, W = x.shape
    xd, gd = x.detach().double(), g.detach().double()
    X, Y, px, py = coords(theta, H, W, Ho, Wo, torch.float64)
    _, _, cx, cy = coords(theta, H, W, Ho, Wo, cells)
    live = (cx > -1.0) & (cx < float(W)) & (cy > -1.0) & (cy < float(H))
    zero = torch.zeros_like(px)
    x0 = torch.where(live, cx.double().floor(), zero).long()
    y0 = torch.where(live, cy.double().floor(), zero).long()
    w = torch.where(live, px - x0.double(), zero)
    n = torch.where(live, py - y0.double(), zero)
    e, s = 1.0 - w, 1.0 - n
    west, east, north, south = live & (x0 >= 0), live & (x0 + 1 < W), live & (y0 >= 0), live & (y0 + 1 < H)
    xa, xb, ya, yb = x0.clamp(0, W - 1), (x0 + 1).clamp(0, W - 1), y0.clamp(0, H - 1), (y0 + 1).clamp(0, H - 1)
    flat = xd.reshape(B, C, H * W)
    P = Ho * Wo

    def idx(yy, xx):
        return (yy * W + xx).reshape(B, 1, P).expand(B, C, P)

    def take(yy, xx, ok):
        return flat.gather(2, idx(yy, xx)).reshape(B, C, Ho, Wo) * ok.double().unsqueeze(1)

    taps = ((ya, xa, north & west, s * e), (ya, xb, north & east, s * w), (yb, xa, south & west, n * e), (yb, xb, south & east, n * w))
    v_nw, v_ne, v_sw, v_se = (take(yy, xx, ok) for yy, xx, ok, _ in taps)
    u = lambda t: t.unsqueeze(1)
    terms = [v * u(wt) for v, (_, _, _, wt) in zip((v_nw, v_ne, v_sw, v_se), taps)]
    out, M_out = sum(terms), sum(t.abs() for t in terms)
    dpx = u(s) * (v_ne - v_nw) + u(n) * (v_se - v_sw)
    dpy = u(e) * (v_sw - v_nw) + u(w) * (v_se - v_ne)
    apx = u(s.abs()) * (v_ne.abs() + v_nw.abs()) + u(n.abs()) * (v_se.abs() + v_sw.abs())
    apy = u(e.abs()) * (v_sw.abs() + v_nw.abs()) + u(w.abs()) * (v_se.abs() + v_ne.abs())
    basis = (X.reshape(1, 1, 1, Wo).expand(1, 1, Ho, Wo), Y.reshape(1, 1, Ho, 1).expand(1, 1, Ho, Wo), torch.ones(1, 1, Ho, Wo, dtype=torch.float64))
    rows, Mrows = [], []
    for d, a, half in ((dpx, apx, W / 2), (dpy, apy, H / 2)):
        rows.append(torch.stack([half * (gd * d * k).sum(dim=(1, 2, 3)) for k in basis], dim=1))
        Mrows.append(torch.stack([half * (gd.abs() * a * k.abs()).sum(dim=(1, 2, 3)) for k in basis], dim=1))
    gth, Mth = torch.stack(rows, dim=1), torch.stack(Mrows, dim=1)
    gim, Mim = torch.zeros(B, C, H * W, dtype=torch.float64), torch.zeros(B, C, H * W, dtype=torch.float64)
    for yy, xx, ok, wt in taps:
        term = (gd * u(wt * ok.double())).reshape(B, C, P)
        gim.scatter_add_(2, idx(yy, xx), term)
        Mim.scatter_add_(2, idx(yy, xx), term.abs())
    return {"out": (out, M_out), "theta": (gth, Mth), "img": (gim.reshape(B, C, H, W), Mim.reshape(B, C, H, W))}


def autograd(x, theta, size, g, dtype):
    """(out, grad_theta [B,2,3], grad_x) of stn_rs and sum(stn_rs * g) by torch autograd in `dtype` on the CPU."""
    xr, tr = x.detach().to(dtype).requires_grad_(True), theta.detach().reshape(-1, 2, 3).to(dtype).requires_grad_(True)
    out = stn_rs(xr, tr, size, dtype)
    out.backward(g.to(dtype))
    return out.detach(), tr.grad, xr.grad


# ================================================================================================================= fixtures
def _similarity(rng, B):
    """Rotation + scale + shift as combine_affine_c0_v2 (hdn/utils/transform.py:442-481) builds affine_m: [[a, b, tx], [c, d, ty]] with a = d = sc cos,
    c = -b = sc sin, sc = out_sz / in_sz * scale (about one half), a normalised shift."""
    sc = 0.5 * rng.uniform(0.8, 1.25, B)
    rot = rng.uniform(-0.35, 0.35, B)
    tx, ty = rng.uniform(-0.15, 0.15, B), rng.uniform(-0.15, 0.15, B)
    a, c = sc * np.cos(rot), sc * np.sin(rot)
    return torch.from_numpy(np.stack([a, -c, tx, c, a, ty], axis=1).astype(np.float32)).reshape(B, 2, 3)


def _overshoot(rng, B):
    """A grid 1.3 - 1.7 times the image, slightly rotated and shifted: samples on every side of every border."""
    sc = rng.uniform(1.3, 1.7, B)
    rot = rng.uniform(-0.2, 0.2, B)
    tx, ty = rng.uniform(-0.1, 0.1, B), rng.uniform(-0.1, 0.1, B)
    a, c = sc * np.cos(rot), sc * np.sin(rot)
    return torch.from_numpy(np.stack([a, -c, tx, c, a, ty], axis=1).astype(np.float32)).reshape(B, 2, 3)


@functools.lru_cache(maxsize=None)
def make_theta(kind, shape):
    """theta [B,2,3] of a fixture.  'similarity' / 'classes' are redrawn (fixed seed) until, at a small shape, no coordinate is within MARGIN of an
    integer and, for 'classes' at a shape of CLASS_SHAPES, every class of REQUIRED_CLASSES is populated in float64 and in fp32."""
    B, C, H, W, Ho, Wo = shape
    if kind == "identity":
        return torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]).repeat(B, 1, 1)
    rng = np.random.default_rng(SEED + 1009 * H + 101 * W + 11 * Ho + 7 * Wo + B + 3 * C + (kind == "classes"))
    small = shape in SMALL_SHAPES
    for _ in range(20000):
        theta = _similarity(rng, B) if kind == "similarity" else _overshoot(rng, B)
        if small and not margin(theta, H, W, Ho, Wo) > MARGIN:
            continue
        if kind == "classes" and shape in CLASS_SHAPES and not all(
                set(REQUIRED_CLASSES) <= classes_present(theta, H, W, Ho, Wo, dt) for dt in (torch.float64, torch.float32)):
            continue
        return theta
    raise AssertionError(f"no {kind} theta for {shape}")


@functools.lru_cache(maxsize=None)
def problem(kind, shape):
    """N(0,1) image and grad_out -> (x, theta, g, closed(...))."""
    B, C, H, W, Ho, Wo = shape
    rng = np.random.default_rng(SEED + 31 * H + 17 * W + 5 * Ho + 3 * Wo + B + 7 * C + 100003 * KINDS.index(kind))
    x = torch.from_numpy(rng.standard_normal((B, C, H, W), dtype=np.float32))
    g = torch.from_numpy(rng.standard_normal((B, C, Ho, Wo), dtype=np.float32))
    theta = make_theta(kind, shape)
    return x, theta, g, closed(x, theta, Ho, Wo, g)


@functools.lru_cache(maxsize=None)
def r_ref(kind, shape):
    """{'out', 'theta', 'img'} -> r_ref: PyTorch's own fp32 CPU path (stn_rs and its autograd) on the same fixture against the float64 truth."""
    B, C, H, W, Ho, Wo = shape
    x, theta, g, truth = problem(kind, shape)
    o32, t32, x32 = autograd(x, theta, (B, C, Ho, Wo), g, torch.float32)
    return {k: GC.worst_ratio(v, *truth[k]) for k, v in (("out", o32), ("theta", t32), ("img", x32))}


def poisoned(theta, b, how):
    """theta with sample b made unusable: 'shift' = a shift of 1e30, 'nan' = NaN entries, 'inf' = +-inf entries."""
    t = theta.clone()
    if how == "shift":
        t[b, 0, 2] = 1e30
    elif how == "nan":
        t[b, 0, 1] = float("nan")
        t[b, 1, 2] = float("nan")
    else:
        t[b, 0, 0] = float("inf")
        t[b, 1, 2] = float("-inf")
    return t


# ================================================================================================================= on the device
def run_forward(x, theta, Ho, Wo, dev, offsets=(0, 0, 0, 0, 0)):
    """One raw call of hdn_affine_sample_f32: out from NaN inside 0xA5 margins.  -> (out on the CPU, were all bytes outside it left alone?)."""
    from hdn_amd import _lib
    B, C, H, W = x.shape
    xd, td = GC.at_offset(x, offsets[0], dev)[0], GC.at_offset(theta, offsets[1], dev)[0]
    n = B * C * Ho * Wo
    ov, ob = GC.at_offset(n, offsets[3], dev, margin=GC.PAD, fill=GC.FILL)
    rc = _lib.load().hdn_affine_sample_f32(_lib.ptr(xd), _lib.ptr(td), _lib.ptr(ov), B, C, H, W, Ho, Wo, _lib.stream_ptr(dev))
    _lib.check(rc, "hdn_affine_sample_f32")
    torch.cuda.synchronize(dev)
    return ov.cpu().view(B, C, Ho, Wo), GC.untouched(ob.cpu(), GC.PAD + offsets[3], GC.PAD + offsets[3] + n)


def run_backward(x, theta, g, dev, offsets=(0, 0, 0, 0, 0), need_theta=True, need_x=True):
    """One raw call of hdn_affine_sample_bwd_f32: outputs from NaN inside 0xA5 margins (so the zero-fill of grad_img must cover exactly the buffer), an
    output that is not asked for NULL and its buffer 0xA5 everywhere, the workspace NaN.  -> (grad_theta | None [B,2,3], grad_x | None, clean)."""
    from hdn_amd import _lib
    lib = _lib.load()
    B, C, H, W = x.shape
    Ho, Wo = g.shape[2:]
    xd, td, gd = GC.at_offset(x, offsets[0], dev)[0], GC.at_offset(theta, offsets[1], dev)[0], GC.at_offset(g, offsets[2], dev)[0]
    gtv, gtb, gxv, gxb = GC._outputs(B * 6, x.numel(), offsets, dev, need_theta, need_x)
    nbytes = lib.hdn_affine_sample_bwd_workspace_bytes(B, Ho, Wo)
    ws = torch.full((nbytes // 4,), float("nan"), device=dev)
    rc = lib.hdn_affine_sample_bwd_f32(_lib.ptr(xd), _lib.ptr(td), _lib.ptr(gd), _lib.ptr(gtv) if need_theta else None,
                                       _lib.ptr(gxv) if need_x else None, _lib.ptr(ws) if need_theta else None, nbytes, B, C, H, W, Ho, Wo,
                                       _lib.stream_ptr(dev))
    _lib.check(rc, "hdn_affine_sample_bwd_f32")
    gt, gx, clean = GC._finish(dev, gtv, gtb, B * 6, offsets[3], need_theta, gxv, gxb, x.numel(), offsets[4], need_x)
    return (gt.view(B, 2, 3) if need_theta else None), (gx.view(B, C, H, W) if need_x else None), clean
