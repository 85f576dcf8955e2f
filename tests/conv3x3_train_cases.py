"""Cases, float64 truths and a float64 emulation of the kernels for the heads' 3x3 convolutions in training (hdn_conv3x3v_dgrad_f32,
hdn_conv3x3v_wgrad_f32, hdn_grad_scale_f32, hdn_pack_conv3x3d_dev_f32), shared by tests/test_conv3x3_train_host.py (no GPU) and
tests/test_gpu_conv3x3_train.py.

The truths are index arithmetic over nine strided views (no convolution routine).  `emulate` restates what the kernels compute — fp16 pieces, three
piece products into hi / lo, the K slices of wgrad — in float64, and takes a `fault`: each FAULTS entry is a wrong kernel one could plausibly write, and
tests/test_conv3x3_train_host.py shows that each fails the very checks (`check_*` below) the device results have to pass."""
import math

import torch

# ---------------------------------------------------------------------------------------------------------------- case lists, by launch form
# (B, S, CI, CO) of the convolution: x [B, CI, S, S], weight [CO, CI, 3, 3], dy [B, CO, S - 2, S - 2].
# dgrad runs conv3x3d.hip's dispatch over M = B S^2 pixels, N = CI, K = 9 CO: forms A / B / C, A and B whole or K-split.
DGRAD_CASES = {
    "A split": [(2, 3, 32, 32), (2, 5, 32, 96), (3, 7, 96, 32), (9, 5, 32, 32)],
    "B split": [(3, 9, 64, 64), (1, 31, 128, 128), (2, 7, 256, 256), (2, 31, 256, 256), (2, 15, 256, 256)],   # the last three: the workload's maps
    "A": [(8, 64, 32, 32)],          # M = 32,768: 256 pixel tiles
    "B": [(8, 64, 64, 32)],
    "C": [(8, 64, 128, 32)],
}
# wgrad: W = 4 / 2 / 1 waves (the largest W with 32 W | CO), whole (one K slice: a single unit, or >= 256 tiles) or split over units of (8 images, row)
WGRAD_CASES = {
    "W1": [(2, 3, 32, 32)],
    "W2": [(8, 3, 32, 64)],
    "W4": [(3, 3, 64, 128)],
    "W1 split": [(2, 5, 32, 96), (3, 7, 96, 32), (9, 5, 32, 32), (8, 64, 32, 32)],
    "W2 split": [(3, 9, 64, 64)],
    "W4 split": [(1, 31, 128, 128), (2, 7, 256, 256), (2, 31, 256, 256), (2, 15, 256, 256), (17, 12, 32, 128)],
}
RANDOM_CASES = sorted({c for cs in list(DGRAD_CASES.values()) + list(WGRAD_CASES.values()) for c in cs})
EXACT_CASES = [(2, 3, 32, 32), (2, 5, 32, 96), (3, 7, 96, 32), (3, 9, 64, 64), (1, 31, 128, 128), (5, 15, 256, 256)]
PACK_CASES = [(32, 32), (96, 32), (32, 96), (128, 256), (256, 256)]      # (CO, CI)


def dgrad_form_name(v):
    assert v > 0, v
    cfg = (v & 15, (v >> 4) & 15, (v >> 8) & 15, (v >> 12) & 15)
    return {(1, 1, 4, 1): "A", (1, 2, 4, 1): "B", (2, 2, 2, 2): "C"}[cfg] + (" split" if (v >> 16) > 1 else "")


def wgrad_form_name(v):
    assert v > 0, v
    return f"W{v & 0xffff}" + (" split" if (v >> 16) > 1 else "")


def wgrad_plan(B, S, CI, CO):
    """(W, units, units per slice, Z) — the rule of csrc/conv3x3_train.hip, restated: it reads (B, S, CI, CO) and nothing else."""
    W = 4 if CO % 128 == 0 else 2 if CO % 64 == 0 else 1
    units = -(-B // 8) * (S - 2)
    wgs = (CO // (32 * W)) * (CI // 32)
    z = 1 if wgs >= 256 else -(-256 // wgs)
    z = min(z, 16, units)
    ups = -(-units // z)
    return W, units, ups, -(-units // ups)


# ------------------------------------------------------------------------------------------------------------------------------ float64 truths
def taps():
    return [(ky, kx) for ky in range(3) for kx in range(3)]


def conv_truth(x, w):
    Ho, Wo = x.shape[2] - 2, x.shape[3] - 2
    return sum(torch.einsum("biyx,oi->boyx", x[:, :, ky:ky + Ho, kx:kx + Wo], w[:, :, ky, kx]) for ky, kx in taps())


def gx_truth(dy, w, S):
    So = S - 2
    gx = torch.zeros(dy.shape[0], w.shape[1], S, S, dtype=dy.dtype)
    for ky, kx in taps():
        gx[:, :, ky:ky + So, kx:kx + So] += torch.einsum("boyx,oi->biyx", dy, w[:, :, ky, kx])
    return gx


def gw_truth(x, dy, mask=None):
    """sum over pixels of dy x(window); mask [B, So, So] (bool) restricts the pixels (a K slice)."""
    So = dy.shape[2]
    if mask is not None:
        dy = dy * mask[:, None].to(dy.dtype)
    gw = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=dy.dtype)
    for ky, kx in taps():
        gw[:, :, ky, kx] = torch.einsum("boyx,biyx->oi", dy, x[:, :, ky:ky + So, kx:kx + So])
    return gw


def w_dgrad(w):
    """w'[ci][co][ky][kx] = w[co][ci][2 - ky][2 - kx]: the weight whose packed stream (mode 1) the dgrad kernel reads."""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def pad2(dy, rows=(2, 2), cols=(2, 2)):
    return torch.nn.functional.pad(dy, (cols[0], cols[1], rows[0], rows[1]))


# ------------------------------------------------------------------------------------------------------------------- exponent rule and the split
def exponent_rule(amax):
    """e with amax 2^e in [2^14, 2^15), from the exponent FIELD of the fp32 amax alone; 0 for 0, inf, NaN; a subnormal counts as 2^-126."""
    bits = int(torch.tensor([amax], dtype=torch.float32).view(torch.int32).item()) & 0x7fffffff
    f = bits >> 23
    if bits == 0 or f == 255:
        return 0
    return 141 - max(f, 1)


def grad_exponent(g):
    a = g.abs().max().item() if not torch.isnan(g).any() else float("nan")
    return exponent_rule(a)


def split16(v, e):
    """fp32-valued float64 tensor v -> the two fp16 pieces of v 2^e, as float64: p0 = fp16(v 2^e), p1 = fp16((v 2^e - p0) 2^11)."""
    vs = torch.ldexp(v.double(), torch.tensor(e))
    p0 = vs.float().half().double()
    p1 = ((vs - p0) * 2048.0).float().half().double()
    return p0, p1


def joined(p0, p1, e):
    return torch.ldexp(p0 + p1 / 2048.0, torch.tensor(-e))


def piece_bound(v, amax):
    return torch.maximum(v.abs().double() * 2.0 ** -22, torch.full_like(v, amax * 2.0 ** -50, dtype=torch.float64))


# -------------------------------------------------------------------------------------------------------------------------------- problems
def integer_problem(B, S, CI, CO):
    """x in [-4, 4], w in [-2, 2], dy in [-3, 3], integers (int64) with their exact y, gx, gw."""
    g = torch.Generator().manual_seed(7 * S + CI + 3 * CO + B)
    x = torch.randint(-4, 5, (B, CI, S, S), generator=g)
    w = torch.randint(-2, 3, (CO, CI, 3, 3), generator=g)
    dy = torch.randint(-3, 4, (B, CO, S - 2, S - 2), generator=g)
    return x, w, dy, conv_truth(x, w), gx_truth(dy, w, S), gw_truth(x, dy)


def random_problem(B, S, CI, CO, dy_scale=1e-6):
    """Post-ReLU-like x, He-scaled w, a gradient of a mean loss's magnitude."""
    g = torch.Generator().manual_seed(1000 * S + CI + CO + B)
    x = torch.randn(B, CI, S, S, generator=g).clamp_min_(0)
    w = torch.randn(CO, CI, 3, 3, generator=g) * (2.0 / (9 * CI)) ** 0.5
    dy = torch.randn(B, CO, S - 2, S - 2, generator=g) * dy_scale
    return x, w, dy


# ----------------------------------------------------------------------------------------------------------- the kernels, emulated in float64
FAULTS = ("unflipped taps", "untransposed weights", "missing halo row", "missing halo column", "slice boundary off by one", "dropped lo",
          "fixed 2^-8 gradient split", "slice order by arrival")


def emulate(x, w, dy, fault=None, call=0):
    """(gx, gw) as the kernels compute them, accumulations in float64 (slice partials of wgrad rounded to fp32 and added in slice order in fp32, as
    the finish pass does).  x, w, dy: float32 tensors.  fault: None or one of FAULTS; call: the call number (for the arrival-order fault)."""
    B, CI, S, _ = x.shape
    CO, So = w.shape[0], S - 2
    e = -8 if fault == "fixed 2^-8 gradient split" else grad_exponent(dy)
    a0, a1 = split16(dy.double(), e)
    if fault == "dropped lo":
        a1 = torch.zeros_like(a1)
    # dgrad: full correlation with the pieces of w'
    wp = w_dgrad(w)
    if fault == "unflipped taps":
        wp = w.transpose(0, 1).contiguous()
    if fault == "untransposed weights":
        assert CI == CO
        wp = w.flip(2, 3).contiguous()
    q0, q1 = split16(wp.double(), 0)
    if fault == "dropped lo":
        q1 = torch.zeros_like(q1)
    rows, cols = (2, 2), (2, 2)
    if fault == "missing halo row":
        rows = (2, 1)
    if fault == "missing halo column":
        cols = (1, 2)

    def full(d, q):
        out = conv_truth(pad2(d, rows, cols), q)      # a halo of fewer than 2 + 2 rows / columns leaves the outputs on that side unproduced (zero)
        return torch.nn.functional.pad(out, (2 - cols[0], 2 - cols[1], 2 - rows[0], 2 - rows[1]))

    hi, lo = full(a0, q0), full(a0, q1) + full(a1, q0)
    gx = joined(hi, lo, e).float()
    # wgrad: K slices of whole (8 images, output row) units
    b0, b1 = split16(x.double(), -8)
    if fault == "dropped lo":
        b1 = torch.zeros_like(b1)
    W, units, ups, Z = wgrad_plan(B, S, CI, CO)
    parts = []
    for z in range(Z):
        mask = torch.zeros(B, So, So, dtype=torch.bool)
        for u in range(z * ups, min(units, (z + 1) * ups)):
            bg, oy = divmod(u, So)
            mask[8 * bg:8 * bg + 8, oy] = True
        if fault == "slice boundary off by one" and z > 0:
            u = z * ups
            bg, oy = divmod(u, So)
            mask[8 * bg, oy, 0] = False       # the slice starts one pixel late: its first pixel belongs to nobody
        hi = gw_truth(b0, a0, mask)
        lo = gw_truth(b1, a0, mask) + gw_truth(b0, a1, mask)
        parts.append(joined(hi, lo, e - 8).float())
    order = list(range(Z))
    if fault == "slice order by arrival" and call % 2:
        order = order[::-1]
    gw = parts[order[0]].clone()
    for z in order[1:]:
        gw = gw + parts[z]
    return gx, gw


# ------------------------------------------------------------------------------------------------------ the checks device results have to pass
def bound_check(what, got, truth, ref32, dims):
    """err <= 4 e_ref + 1e-5 scale, with err, e_ref (PyTorch's own fp32 CPU backward against float64) and scale = max |truth| taken over `dims` (per
    image for gx: dims (1, 2, 3); per output channel for gw).  Returns (ok, worst err / bound)."""
    got = got.detach().cpu().double()
    if got.shape != truth.shape or not bool(torch.isfinite(got).all()):
        return False, float("inf")
    err = (got - truth).abs().amax(dims)
    e_ref = (ref32.double() - truth).abs().amax(dims)
    scale = truth.abs().amax(dims)
    bound = 4 * e_ref + 1e-5 * scale
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    print(f"FORMS conv3x3 train {what}: worst err/bound {float(ratio.max()):.3f} (err {float(err.max()):.3e}, scale {float(scale.max()):.3e})")
    return bool((err <= bound).all()), float(ratio.max())


def reference_backward(x, w, dy):
    """(float64 gx, gw by index arithmetic; PyTorch's fp32 CPU autograd gx, gw) of a case."""
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    torch.nn.functional.conv2d(xr, wr).backward(dy)
    return gx_truth(dy.double(), w.double(), x.shape[2]), gw_truth(x.double(), dy.double()), xr.grad, wr.grad


def check_random(fn, cases, dy_scale=1e-6):
    """fn(x, w, dy) -> (gx, gw), float32.  Every case within the bound, per image (gx) and per output channel (gw)."""
    ok = True
    for c in cases:
        x, w, dy = random_problem(*c, dy_scale=dy_scale)
        gx64, gw64, gx32, gw32 = reference_backward(x, w, dy)
        gx, gw = fn(x, w, dy)
        ok &= bound_check(f"{c} gx", gx, gx64, gx32, (1, 2, 3))[0]
        ok &= bound_check(f"{c} gw", gw, gw64, gw32, (1, 2, 3))[0]
    return ok


def check_exact(fn, cases):
    """Integer problems: gx and gw EQUAL the integer truth."""
    ok = True
    for c in cases:
        x, w, dy, _, gx, gw = integer_problem(*c)
        got_gx, got_gw = fn(x.float(), w.float(), dy.float())
        ok &= torch.equal(got_gx.cpu().double(), gx.double()) and torch.equal(got_gw.cpu().double(), gw.double())
    return ok


def check_repeatable(fn, case):
    """Two calls are bit-equal."""
    x, w, dy = random_problem(*case)
    a, b = fn(x, w, dy), fn(x, w, dy)
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def all_checks(fn_factory):
    """fn_factory() -> a fresh fn.  The host-sized subset of what tests/test_gpu_conv3x3_train.py asks of the device, as one verdict per check."""
    small = [(2, 5, 32, 96), (3, 9, 64, 64), (9, 5, 32, 32)]
    return {
        "exact": check_exact(fn_factory(), [(2, 5, 32, 96), (3, 7, 32, 32), (9, 5, 32, 32)]),
        "bound": check_random(fn_factory(), small, dy_scale=1e-7),
        "repeatable": check_repeatable(fn_factory(), (9, 5, 32, 32)),
    }


def integer_sum_limit(B, S, CI, CO):
    """An upper bound of every |sum| of an integer problem (forward, gx, gw)."""
    return max(9 * CI * 4 * 2, 9 * CO * 3 * 2, B * (S - 2) ** 2 * 3 * 4)


assert math.log2(integer_sum_limit(5, 15, 256, 256)) < 24
