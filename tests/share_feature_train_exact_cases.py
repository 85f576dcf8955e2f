"""Shared by tests/test_gpu_share_feature_train_exact.py and tests/test_share_feature_train_exact_host.py: the exact fixtures, the restatements and
the raw-ABI runners of PreShareFeature's training kernels (csrc/share_feature_train.hip).  Nothing here launches a kernel except the run_*
functions.  The bound fixtures (one maximum per tensor, a ReLU margin) are tests/share_feature_train_cases.py; nothing here needs a margin.

A. Order-free exact fixtures: fp32 is exact on them in ANY summation order, so the device must be torch.equal to a float64 / int64 truth.
  A1 dyadic(): integer image in [-4, 4], grad_out in [-3, 3], weights in [-2, 2], gamma in {0.5, 1, 2}, integer bias and running mean in [-2, 2],
     eps = 2^-10 in every layer and running variance 4^k - 2^-10 (4^k in {1, 4, 16, 64}, layer 3: 256): (double)var + eps is exactly 4^k, invstd a
     power of two, and every product and partial sum a dyadic number far inside 24 bits (the host test proves it: stock fp32 == stock float64 on
     every tensor, and sum |dc a| 2^r < 2^24 per weight, 2^-r the terms' resolution).  Truth: float64 autograd through the stock nn.Sequential in
     eval mode.  A draw is accepted only if every layer's share of z > 0 lies in SHARE = [0.2, 0.8]: no layer dead, none linear.  A layer with
     ONE pre-activation (H W = 1, layer 3) has share 0 or 1; there the rule is "alive" (z > 0), so the backward runs through it.  And only if
     order_free_margin() < 1: at two 127 x 127 images some draws' weight-gradient terms outgrow 24 bits.  Neither rule looks at a kernel.
     DYADIC_CASES holds the first accepted seed offset per shape; the host test re-derives it.
  A2 onehot_problem(s, shape): weights with a single 1, data that are integer codes, statistics frozen to alpha = 1, beta = 0 (mean 0, variance 1 - 2^-10,
     gamma 1, bias 0; set BETA_SET: bias 3 in layers 1 and 2, so beta = 3 > 0).  Tap rule, set s = 0 .. 35, t = 9 ci + k:
         w1[co, 0, k]  = 1  at  k = (s + 2 co) mod 9
         w2[co, ci, k] = 1  at  t = (s + 5 co) mod 36
         w3[0, ci, k]  = 1  at  k = (s + ci) mod 9      for every ci
     Layers 1 and 2 have one 1 per output channel; layer 3 has one output channel, so one 1 per output channel would meet a single one of its
     72 taps per set and starve seven of layer 2's eight channels of gradient: it holds one 1 per INPUT channel instead (c3 is then a sum of
     eight codes, still index arithmetic).  Sets 0 .. 35 meet every (co, ci, k) of all three layers (the host test counts them), forward and,
     since every channel of dc2 and dc1 is fed, backward.  Codes: x = +-(1 + ((b H + y) W + x) mod 1021), negative where (b + y + 2 x) mod 5 = 0
     (those die in layer 1's ReLU and leave exact zeros behind: the kink); grad_out = ((7 (b H W + pix) + 3 b) mod 5) - 2.  Truth: chain() on int64.
  A3 dyadic()'s integers with BATCH statistics: c1 is an integer plane, so sum c and sum c^2 are exact integers in any order and layer 1's
     mean / invstd / unbiased variance must be bit-equal to stats_statements() on them.

B. check_stages(): every stage restated in numpy from the DEVICE's own upstream outputs (saved, stats, grad_gamma / grad_bias), on N(0, 1) data,
   batch and frozen statistics, no ReLU margin.  fp32 operations are individually rounded numpy ones; fma32() is fp32(float64(a) float64(b) +
   float64(c)), re-evaluated on fractions where the float64 sum is an inexact fp32 tie.  Planes must match as numbers, every element (-0 == +0:
   fmaxf may return either zero).  Reductions are enclosed: see enclose_sum().  gw: |gw - exact| <= GW_ROUNDINGS 2^-24 sum |dc a| per weight.

C. chain(mutant=...) restates five wrong kernels for the host test; no mutated kernel is ever built for the GPU."""
import fractions
import functools
import math

import numpy as np
import torch

import share_feature_train_cases as C

f32, f64 = np.float32, np.float64
LAYERS, PXB, THREADS = C.LAYERS, C.PX_PER_WORKGROUP, 256
EPS_DYADIC = 2.0 ** -10
SHARE = (0.2, 0.8)
EXACT_SEED = 20261020
MAX_OFFSET = 64
# both sides of every boundary of the one launch form: H W = 1, 2, 255 | 256 | 257, 1023 | 1024 | 1025, 2049 at B = 1 (H = 1 and W = 1 among the
# factorisations), three workgroups per image, 64 | 65 and 256 | 257 workgroups, and two images of the step's real size
DYADIC_CASES = {
    (1, 1, 1): 8, (1, 1, 2): 0, (1, 2, 1): 0, (1, 15, 17): 0, (1, 1, 255): 0, (1, 16, 16): 0, (1, 256, 1): 8, (1, 1, 257): 5, (1, 257, 1): 2,
    (1, 33, 31): 0, (1, 32, 32): 0, (1, 1024, 1): 0, (1, 25, 41): 0, (1, 1, 1025): 1, (1, 3, 683): 1, (1, 2049, 1): 10, (3, 33, 65): 0,
    (64, 1, 2): 4, (65, 1, 2): 1, (256, 1, 2): 1, (257, 1, 2): 2, (2, 127, 127): 2,
}
STAGE_CASES = list(DYADIC_CASES)                # B runs A1's shapes; (2, 127, 127) with batch statistics is among them
STAGE_SEED = 20261021
ONEHOT_SETS = 36
BETA_SET = 36                                   # one extra set: set 0's weights with beta = 3 in layers 1 and 2
ONEHOT_SHAPES = [(2, 5, 7), (1, 3, 343)]        # one workgroup per image; two workgroups, the second one ragged
EPS_A3 = (1e-5, 1e-3, 1e-1)
EPS_A3_PERMUTED = (1e-1, 1e-5, 1e-3)
A3_CASES = [(1, 1, 2), (1, 16, 16), (1, 1, 257), (1, 25, 41), (3, 33, 65), (65, 1, 2), (257, 1, 2), (2, 127, 127)]
# roundings on the longest path of one weight-gradient entry, counted in conv_weight_adjoint_kernel / weight_finish_kernel: a thread chains its 4
# pixels' fmas (4), the wave's xor tree 32 .. 1 (6), the waves 1 .. 3 through LDS (3), the float64 sum across workgroups rounded once (1)
GW_ROUNDINGS = 4 + 6 + 3 + 1
FMA_TIES = [0]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32))


def workgroup_of(pix):
    return pix // PXB, pix % THREADS


# ================================================================================================================= A1 / A3: the dyadic fixture
def dyadic(B, H, W, seed):
    """The fixture dict of share_feature_train_cases.draw() (fp32 CPU tensors), every entry a small integer or dyadic number."""
    rng = np.random.default_rng(seed)
    ints = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(f64)
    fix = {"x": ints(-4, 4, (B, 1, H, W)), "g": ints(-3, 3, (B, 1, H, W)), "w1": ints(-2, 2, (4, 1, 3, 3)), "w2": ints(-2, 2, (8, 4, 3, 3)),
           "w3": ints(-2, 2, (1, 8, 3, 3)), "gamma": rng.choice([0.5, 1.0, 2.0], 13), "bias": ints(-2, 2, 13), "rmean": ints(-2, 2, 13)}
    k = rng.integers(0, 4, 13)
    k[12] = 4
    fix["rvar"] = 4.0 ** k - EPS_DYADIC
    assert np.array_equal(fix["rvar"].astype(f32).astype(f64), fix["rvar"])
    return {n: T(v) for n, v in fix.items()}


def shares(zs):
    return [float((z > 0).double().mean()) for z in zs]


def shares_ok(zs):
    """Every layer's share of z > 0 in SHARE; a layer of one pre-activation must be alive."""
    return all((s == 1.0) if z.numel() == 1 else (SHARE[0] <= s <= SHARE[1]) for z, s in zip(zs, shares(zs)))


def saved_of(cs):
    """The three convolutions' outputs [B, CO, H, W] -> the kernel's `saved`: c1 | c2 | c3, each plane-major per image."""
    return torch.cat([c.reshape(-1) for c in cs])


@functools.lru_cache(maxsize=None)
def dyadic_problem(shape, offset):
    """(fixture, float64 truth): stock()'s dict of the eval-mode nn.Sequential plus 'saved' and 'stats01'."""
    fix = dyadic(*shape, EXACT_SEED + offset)
    truth = C.stock(fix, torch.float64, train=False, running=C.running_of(fix), eps=EPS_DYADIC)
    truth["saved"] = saved_of(truth["c"])
    truth["stats01"] = torch.cat([fix["rmean"].double(), 1.0 / torch.sqrt(fix["rvar"].double() + EPS_DYADIC)])
    return fix, truth


def first_dyadic_offset(shape):
    for off in range(MAX_OFFSET):
        fix, truth = dyadic_problem(shape, off)
        if shares_ok(truth["z"]) and order_free_margin(fix) < 1.0:
            return off
    return None


EXACT_TENSORS = ("y", "saved", "stats01", "gx", "gw1", "gw2", "gw3", "gg1", "gg2", "gg3", "gb1", "gb2", "gb3")


def device_dict(res):
    """run_raw()'s result -> the tensors by name (y, saved, stats, stats01, gx, gw1..3, gg1..3, gb1..3)."""
    out = {"y": res["y"], "saved": res["saved"], "stats": res["stats"], "stats01": res["stats"][:26]}
    if res.get("gx") is not None:
        out["gx"] = res["gx"]
    if res.get("gp") is not None:
        out.update(C.split_params(res["gp"]))
    return out


def plane_layout(name, B, H, W):
    """[(sub-name, CO, first float)] of a tensor made of planes."""
    n = B * H * W
    return {"y": [("y", 1, 0)], "gx": [("gx", 1, 0)], "saved": [("saved c1", 4, 0), ("saved c2", 8, 4 * n), ("saved c3", 1, 12 * n)]}.get(name)


def first_mismatch(name, got, want, shape, taps=None):
    """None, or the first wrong element of a tensor by name: planes as image, channel, row, column, workgroup pix // 1024 and thread pix % 256 of
    the launch form, and - taps: {sub-name: [tap text per channel]} - the one-hot tap that feeds it."""
    got, want = np.asarray(got, f64).reshape(-1), np.asarray(want, f64).reshape(-1)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = np.flatnonzero(~(got == want))
    if bad.size == 0:
        return None
    i, (B, H, W) = int(bad[0]), shape
    layout = plane_layout(name, B, H, W)
    if layout is None:
        return f"{name}[{i}]: got {got[i]!r} want {want[i]!r} ({bad.size} of {got.size} wrong)"
    sub, co, base = [l for l in layout if l[2] <= i][-1]
    b, ch, y, x = np.unravel_index(i - base, (B, co, H, W))
    wg, th = workgroup_of(int(y) * W + int(x))
    tap = "" if not taps or sub not in taps else f", tap {taps[sub][int(ch)]}"
    return (f"{sub}: image {b} channel {ch} row {y} column {x} (workgroup {wg} of the image, thread {th}){tap}: got {got[i]!r} want {want[i]!r} "
            f"({bad.size} of {got.size} wrong)")


def compare_exact(got, truth, names, shape, taps=None):
    """The list of first mismatches, one per wrong tensor."""
    return [m for m in (first_mismatch(n, got[n].numpy(), truth[n].numpy() if torch.is_tensor(truth[n]) else truth[n], shape, taps) for n in names)
            if m]


# ================================================================================================================= the chain, order-free
def shift_conv(a, w, sign=1, pad=None):
    """out[b, co, y, x] = sum over ci, k of w[co, ci, k] a[b, ci, y + sign (ky - 1), x + sign (kx - 1)]; outside the plane a is 0, or pad[ci]."""
    B, CI, H, W = a.shape
    ap = np.zeros((B, CI, H + 2, W + 2), a.dtype)
    if pad is not None:
        ap[:] = np.asarray(pad, a.dtype).reshape(1, CI, 1, 1)
    ap[:, :, 1:H + 1, 1:W + 1] = a
    out = np.zeros((B, w.shape[0], H, W), a.dtype)
    for co, ci, ky, kx in zip(*np.nonzero(w)):
        dy, dx = sign * (ky - 1) + 1, sign * (kx - 1) + 1
        out[:, co] += w[co, ci, ky, kx] * ap[:, ci, dy:dy + H, dx:dx + W]
    return out


def shift_dot(dc, a, keep=None, pad=None):
    """gw[co, ci, ky, kx] = sum over b, p of dc[b, co](p) a[b, ci](p + k); keep: a [B, H, W] mask of the pixels that take part."""
    B, CI, H, W = a.shape
    ap = np.zeros((B, CI, H + 2, W + 2), a.dtype)
    if pad is not None:
        ap[:] = np.asarray(pad, a.dtype).reshape(1, CI, 1, 1)
    ap[:, :, 1:H + 1, 1:W + 1] = a
    d = dc if keep is None else dc * keep[:, None].astype(dc.dtype)
    out = np.zeros((dc.shape[1], CI, 3, 3), a.dtype)
    for ky in range(3):
        for kx in range(3):
            out[:, :, ky, kx] = np.einsum("bohw,bihw->oi", d, ap[:, :, ky:ky + H, kx:kx + W])
    return out


def last_workgroup_mask(B, H, W):
    """[B, H, W]: False on the pixels of the launch's last workgroup (image B - 1, pixels from the last multiple of 1024 on)."""
    keep = np.ones((B, H * W), bool)
    keep[B - 1, ((H * W - 1) // PXB) * PXB:] = False
    return keep.reshape(B, H, W)


MUTANTS = ("padding", "mask", "adjoint", "unbiased", "drop-stats", "drop-bn", "drop-weight")


def chain(fix, dtype=f64, mutant=None):
    """PreShareFeature forward and backward with FROZEN statistics, order-free, in `dtype` (float64 on a dyadic fixture, int64 on a one-hot set:
    exact either way).  fix: numpy arrays x, g, w1..3 and per channel alpha[13], beta[13], mean[13], invstd[13].
    mutant: None or one of MUTANTS' first three / 'drop-bn' / 'drop-weight' - a wrong kernel restated (the host test shows which fixture rejects it):
      padding      a tap outside the plane reads relu(beta), the activation of a zero PRE-activation, instead of 0
      mask         dz = g [z >= 0]
      adjoint      the data adjoint gathers dc at p + k instead of p - k
      drop-bn      the last workgroup's partial is left out of S1 / S2;  drop-weight: out of the weight gradients
    -> dict y, saved, gx, gw1..3, gg1..3, gb1..3, z (list)."""
    x, g = fix["x"].astype(dtype), fix["g"].astype(dtype)
    ws = [fix["w%d" % l].astype(dtype) for l in (1, 2, 3)]
    al, be, mean, invstd = (fix[k].astype(dtype) for k in ("alpha", "beta", "mean", "invstd"))
    B, _, H, W = x.shape
    per = lambda v, lo, hi: v[lo:hi].reshape(1, -1, 1, 1)
    relu = lambda v: np.maximum(v, 0)
    keep = last_workgroup_mask(B, H, W)
    a, acts, pads, cs, zs = x, [], [], [], []
    for l, (lo, hi) in enumerate(LAYERS):
        pad = None if l == 0 or mutant != "padding" else relu(be[LAYERS[l - 1][0]:LAYERS[l - 1][1]])
        c = shift_conv(a, ws[l], 1, pad)
        z = c * per(al, lo, hi) + per(be, lo, hi)
        acts.append(a), pads.append(pad), cs.append(c), zs.append(z)
        a = relu(z)
    out = {"y": a, "saved": np.concatenate([c.reshape(-1) for c in cs]), "z": zs}
    grad = g
    for l in (2, 1, 0):
        lo, hi = LAYERS[l]
        mask = (zs[l] >= 0) if mutant == "mask" else (zs[l] > 0)
        dz = grad * mask
        xh = (cs[l] - per(mean, lo, hi)) * per(invstd, lo, hi)
        part = dz * keep[:, None] if mutant == "drop-bn" else dz
        out["gb%d" % (l + 1)], out["gg%d" % (l + 1)] = part.sum(axis=(0, 2, 3)), (part * xh).sum(axis=(0, 2, 3))
        dc = per(al, lo, hi) * dz
        out["gw%d" % (l + 1)] = shift_dot(dc, acts[l], keep if mutant == "drop-weight" else None, pads[l])
        grad = shift_conv(dc, np.ascontiguousarray(ws[l].transpose(1, 0, 2, 3)), 1 if mutant == "adjoint" else -1)
    out["gx"] = grad
    return out


def frozen_tables(fix, eps):
    """numpy float64 alpha, beta, mean, invstd [13] of a torch fixture with frozen statistics (exact on a dyadic fixture)."""
    eps = np.repeat(np.array(C.per_layer(eps), f64), [4, 8, 1])
    gamma, bias, mean, var = (fix[k].double().numpy() for k in ("gamma", "bias", "rmean", "rvar"))
    invstd = 1.0 / np.sqrt(var + eps)
    alpha = gamma * invstd
    return {"alpha": alpha, "beta": bias - mean * alpha, "mean": mean, "invstd": invstd}


def resolution(t):
    """The least r with every entry of t a multiple of 2^-r."""
    t, r = t[t != 0], 0
    while t.size and not np.array_equal(np.ldexp(t, r), np.rint(np.ldexp(t, r))):
        r += 1
    return r


def order_free_margin(fix):
    """The largest sum |dc| |a| 2^(r_dc + r_a) / 2^24 over the weights of a dyadic fixture, 2^-r_dc and 2^-r_a the resolutions of the dc plane and
    the activation plane of that weight.  Below 1, every partial sum of the weight's terms dc a - in any order, through any fma chain - is a
    multiple of 2^-(r_dc + r_a) below 2^24 of them: an fp32 number, so the weight gradients are order-free.  (The planes themselves and S1 / S2
    need no such rule: their sums have at most 72 terms, or are carried in float64.)"""
    d = {k: fix[k].double().numpy() for k in ("x", "g", "w1", "w2", "w3")}
    d.update(frozen_tables(fix, EPS_DYADIC))
    out, grad, worst = chain(d), d["g"], 0.0
    acts = [d["x"]] + [np.maximum(z, 0) for z in out["z"][:2]]
    for l in (2, 1, 0):
        lo, hi = LAYERS[l]
        dc = d["alpha"][lo:hi].reshape(1, -1, 1, 1) * grad * (out["z"][l] > 0)
        mag = shift_dot(np.abs(dc), np.abs(acts[l])).max(axis=(2, 3))
        for co in range(hi - lo):
            for ci in range(acts[l].shape[1]):
                worst = max(worst, float(np.ldexp(mag[co, ci], resolution(dc[:, co]) + resolution(acts[l][:, ci]) - 24)))
        grad = shift_conv(dc, np.ascontiguousarray(d["w%d" % (l + 1)].transpose(1, 0, 2, 3)), -1)
    return worst


def chain_of(fix, eps, dtype=f64, mutant=None):
    """chain() on a torch fixture with frozen statistics."""
    d = {k: fix[k].double().numpy() for k in ("x", "g", "w1", "w2", "w3")}
    d.update(frozen_tables(fix, eps))
    return chain(d, dtype, mutant)


# ------------------------------------------------------------------------------------------------------------------------ the kernel's statements
def stats_statements(s, q, n, eps, unbiased=True):
    """stats_finish_kernel's float64 statements on the sums s = sum c, q = sum c^2 of n values: (mean, invstd, unbiased variance) as fp32, and the
    float64 (mean, var).  eps arrives through the C ABI as a float.  Every statement is monotone in s or q, rounding included."""
    n, eps = float(n), float(f32(eps))
    mean = f64(s) / n
    var = max(f64(q) / n - mean * mean, 0.0)
    uvar = var * (n / (n - 1.0)) if unbiased else var
    return f32(mean), f32(1.0 / math.sqrt(var + eps)), f32(uvar), mean, var


def layer1_batch_stats(fix, eps1, mutant=None):
    """A3: (c1 as int64 [B, 4, H, W], the [3, 4] fp32 rows mean / invstd / unbiased variance of layer 1) of a dyadic fixture with batch statistics,
    from exact integer sums.  mutant 'unbiased': the factor n / (n - 1) dropped; 'drop-stats': the last workgroup's partial left out."""
    x, w1 = fix["x"].numpy().astype(np.int64), fix["w1"].numpy().astype(np.int64)
    B, _, H, W = x.shape
    c1 = shift_conv(x, w1)
    part = c1 * last_workgroup_mask(B, H, W)[:, None] if mutant == "drop-stats" else c1
    rows = np.zeros((3, 4), f32)
    for co in range(4):
        s, q = int(part[:, co].sum()), int((part[:, co] ** 2).sum())
        assert abs(s) < 2 ** 53 and q < 2 ** 53
        rows[:, co] = stats_statements(s, q, B * H * W, eps1, unbiased=mutant != "unbiased")[:3]
    return c1, rows


# ================================================================================================================= A2: one-hot sets
def onehot_taps(s):
    """The tap rule of the docstring: ([k per co], [(ci, k) per co], [k per ci]) of set s."""
    s = 0 if s == BETA_SET else s
    return [(s + 2 * co) % 9 for co in range(4)], [divmod((s + 5 * co) % 36, 9) for co in range(8)], [(s + ci) % 9 for ci in range(8)]


def onehot_weights(s):
    t1, t2, t3 = onehot_taps(s)
    w1, w2, w3 = np.zeros((4, 1, 9), np.int64), np.zeros((8, 4, 9), np.int64), np.zeros((1, 8, 9), np.int64)
    for co, k in enumerate(t1):
        w1[co, 0, k] = 1
    for co, (ci, k) in enumerate(t2):
        w2[co, ci, k] = 1
    for ci, k in enumerate(t3):
        w3[0, ci, k] = 1
    return w1.reshape(4, 1, 3, 3), w2.reshape(8, 4, 3, 3), w3.reshape(1, 8, 3, 3)


def onehot_tap_names(s):
    t1, t2, t3 = onehot_taps(s)
    kk = lambda k: f"(ky {k // 3}, kx {k % 3})"
    return {"saved c1": [f"w1[{co}, 0] {kk(k)}" for co, k in enumerate(t1)], "saved c2": [f"w2[{co}, {ci}] {kk(k)}" for co, (ci, k) in enumerate(t2)],
            "saved c3": ["w3[0, ci] k = (s + ci) mod 9, every ci"], "y": ["w3[0, ci] k = (s + ci) mod 9, every ci"],
            "gx": ["w1[co, 0] k = (s + 2 co) mod 9, every co"]}


@functools.lru_cache(maxsize=None)
def onehot_problem(s, shape):
    """(torch fixture for the device, int64 truth as numpy: chain()'s dict plus 'stats01') of one-hot set s."""
    B, H, W = shape
    b, y, x = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    pix = (b * H + y) * W + x
    code = (1 + pix % 1021) * np.where((b + y + 2 * x) % 5 == 0, -1, 1)
    grad = (7 * pix + 3 * b) % 5 - 2
    w1, w2, w3 = onehot_weights(s)
    bias = np.zeros(13, np.int64)
    if s == BETA_SET:
        bias[:12] = 3
    ints = {"x": code.reshape(B, 1, H, W), "g": grad.reshape(B, 1, H, W), "w1": w1, "w2": w2, "w3": w3, "alpha": np.ones(13, np.int64), "beta": bias,
            "mean": np.zeros(13, np.int64), "invstd": np.ones(13, np.int64)}
    truth = chain(ints, np.int64)
    truth["stats01"] = np.concatenate([np.zeros(13), np.ones(13)])
    fix = {k: T(ints[k]) for k in ("x", "g", "w1", "w2", "w3")}
    fix.update(gamma=torch.ones(13), bias=T(bias), rmean=torch.zeros(13), rvar=torch.full((13,), 1.0 - EPS_DYADIC))
    return fix, truth, ints


# ================================================================================================================= B: stage restatements
def round_tie(exact, tie):
    """The fp32 nearest to the fraction `exact`, which is not `tie`, the float64 midpoint of two neighbouring fp32 numbers it was rounded to."""
    v = f32(tie)
    other = np.nextafter(v, f32(np.inf) if tie > float(v) else f32(-np.inf))
    lo, hi = (v, other) if v < other else (other, v)
    return hi if exact > fractions.Fraction(tie) else lo


def fma32(a, b, c):
    """fp32 fma as fp32(float64(a) float64(b) + float64(c)): the product is exact, the sum rounded to float64 and then to fp32.  The two roundings
    differ from one only if the float64 sum was itself rounded (TwoSum error != 0) and lies half way between two fp32 numbers (low 29 bits
    1000...0): those elements are re-evaluated on fractions and counted in FMA_TIES."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    with np.errstate(all="ignore"):
        p, c64 = a.astype(f64) * b.astype(f64), c.astype(f64)
        s = p + c64
        bp = s - p
        err = (p - (s - bp)) + (c64 - bp)
    out = s.astype(f32)
    tie = ((np.ascontiguousarray(s).view(np.int64) & (2 ** 29 - 1)) == 2 ** 28) & (err != 0) & np.isfinite(s)
    if tie.any():
        out, flat = np.ascontiguousarray(out), [v.reshape(-1) for v in (a, b, c, s)]
        for i in np.flatnonzero(tie):
            exact = fractions.Fraction(float(flat[0][i])) * fractions.Fraction(float(flat[1][i])) + fractions.Fraction(float(flat[2][i]))
            out.reshape(-1)[i] = round_tie(exact, float(flat[3][i]))
            FMA_TIES[0] += 1
    return out


def make_ab(gamma, bias, mean, invstd):
    """make_ab of the kernel file: alpha = gamma invstd, beta = fma(-mean, alpha, bias)."""
    alpha = (gamma.astype(f32) * invstd.astype(f32)).astype(f32)
    return alpha, fma32(-mean.astype(f32), alpha, bias.astype(f32))


def padded(a):
    B, CI, H, W = a.shape
    ap = np.zeros((B, CI, H + 2, W + 2), f32)
    ap[:, :, 1:H + 1, 1:W + 1] = a
    return ap


def conv_chain(a, w):
    """conv_stats_kernel's sum: the accumulator starts at 0; ci ascending, then k = 0 .. 8; acc = fma(w[co][ci][k], a, acc), a = 0 outside."""
    B, CI, H, W = a.shape
    ap, acc = padded(a), np.zeros((B, w.shape[0], H, W), f32)
    for ci in range(CI):
        for k in range(9):
            acc = fma32(w[:, ci, k // 3, k % 3].reshape(1, -1, 1, 1), ap[:, ci, k // 3:k // 3 + H, k % 3:k % 3 + W][:, None], acc)
    return acc


def adjoint_chain(dc, w):
    """conv_data_adjoint_kernel's sum: co ascending, then k; acc[ci] = fma(w[co][ci][k], dc[co](p - k), acc[ci]), 0 outside."""
    B, CO, H, W = dc.shape
    dp, acc = padded(dc), np.zeros((B, w.shape[1], H, W), f32)
    for co in range(CO):
        for k in range(9):
            dy, dx = 2 - k // 3, 2 - k % 3                 # p - k: row y - (ky - 1) is row y + 1 - (ky - 1) of the padded plane
            acc = fma32(w[co, :, k // 3, k % 3].reshape(1, -1, 1, 1), dp[:, co, dy:dy + H, dx:dx + W][:, None], acc)
    return acc


def activation(c, alpha, beta):
    """act_at inside the plane: relu(fma(c, alpha, beta)) per channel."""
    return np.maximum(fma32(c, alpha.reshape(1, -1, 1, 1), beta.reshape(1, -1, 1, 1)), f32(0))


def enclose_sum(terms):
    """[lo, hi] around a float64 sum, in any order, of the exactly representable `terms`: their exact sum (math.fsum) widened by
    n 2^-53 sum |term|, the a-priori bound of n - 1 float64 additions.  Integer terms below 2^53 in all: every partial sum is exact, a point."""
    t = np.asarray(terms, f64).reshape(-1)
    s, mag = math.fsum(t.tolist()), math.fsum(np.abs(t).tolist())
    if mag < 2.0 ** 53 and np.array_equal(t, np.rint(t)):
        return s, s
    w = t.size * 2.0 ** -53 * mag
    return np.nextafter(s - w, -np.inf), np.nextafter(s + w, np.inf)


def enclose_stats(c, n, eps):
    """The enclosures [(lo, hi)] of mean, invstd and unbiased variance (fp32) of one channel's values c, through stats_statements(): each of its
    statements is monotone, and correct rounding keeps monotone, so the ends of the sums' enclosures give the ends of the results'."""
    c = np.asarray(c, f64).reshape(-1)
    (slo, shi), (qlo, qhi) = enclose_sum(c), enclose_sum(c * c)
    n_, e = float(n), float(f32(eps))
    mlo, mhi = slo / n_, shi / n_
    m2lo = 0.0 if mlo <= 0.0 <= mhi else min(mlo * mlo, mhi * mhi)
    m2hi = max(mlo * mlo, mhi * mhi)
    vlo, vhi = max(qlo / n_ - m2hi, 0.0), max(qhi / n_ - m2lo, 0.0)
    k = n_ / (n_ - 1.0)
    return [(f32(mlo), f32(mhi)), (f32(1.0 / math.sqrt(vhi + e)), f32(1.0 / math.sqrt(vlo + e))), (f32(vlo * k), f32(vhi * k))]


class Report:
    """What check_stages() found: `bad` (texts, the first wrong element of each stage), the count of enclosures and of those that were not points,
    and the worst ratio of a weight gradient's error to its bound."""

    def __init__(self):
        self.bad, self.enclosures, self.not_points, self.gw_ratio = [], 0, 0, 0.0

    def inside(self, name, got, lo, hi):
        self.enclosures += 1
        self.not_points += int(lo != hi)
        if not (lo <= got <= hi):
            self.bad.append(f"{name}: {got!r} outside [{lo!r}, {hi!r}]")

    def equal(self, name, got, want, shape):
        m = first_mismatch(name, got, want, shape)
        if m:
            self.bad.append(m)


def check_stages(fix, dev, frozen, eps):
    """B.  fix: the torch fixture; dev: device_dict() of one raw forward + backward on it (numpy-convertible CPU tensors); eps: per layer.
    Every stage is recomputed from dev's own upstream outputs.  -> Report."""
    rep = Report()
    eps = C.per_layer(eps)
    x, g = fix["x"].numpy(), fix["g"].numpy()
    ws = [fix["w%d" % l].numpy() for l in (1, 2, 3)]
    gamma, bias = fix["gamma"].numpy(), fix["bias"].numpy()
    B, _, H, W = x.shape
    n, shape = B * H * W, (B, H, W)
    saved, stats = dev["saved"].numpy(), dev["stats"].numpy()
    cs = [saved[0:4 * n].reshape(B, 4, H, W), saved[4 * n:12 * n].reshape(B, 8, H, W), saved[12 * n:].reshape(B, 1, H, W)]
    mean, invstd = stats[0:13], stats[13:26]
    alpha, beta = make_ab(gamma, bias, mean, invstd)
    # ---- forward
    a = x
    for l, (lo, hi) in enumerate(LAYERS):
        rep.equal("c%d from its input" % (l + 1), cs[l], conv_chain(a, ws[l]), shape)
        for ch in range(lo, hi):
            if frozen:
                want = [(fix["rmean"][ch].numpy(),) * 2, (f32(1.0 / math.sqrt(float(fix["rvar"][ch]) + float(f32(eps[l])))),) * 2,
                        (fix["rvar"][ch].numpy(),) * 2]
            else:
                want = enclose_stats(cs[l][:, ch - lo], n, eps[l])
            for row, (lo_, hi_) in enumerate(want):
                rep.inside(f"stats[{row}][{ch}]", stats[13 * row + ch], lo_, hi_)
        a = activation(cs[l], alpha[lo:hi], beta[lo:hi])
    rep.equal("y from c3", dev["y"].numpy().reshape(B, 1, H, W), a, shape)
    # ---- backward
    inv_n = f32(1.0 / float(n))
    grad = g
    for l in (2, 1, 0):
        lo, hi = LAYERS[l]
        per = lambda v: v[lo:hi].reshape(1, -1, 1, 1)
        z = fma32(cs[l], per(alpha), per(beta))
        dz = np.where(z > 0, grad, f32(0)).astype(f32)
        xh = ((cs[l] - per(mean)).astype(f32) * per(invstd)).astype(f32)
        gb, gg = dev["gb%d" % (l + 1)].numpy(), dev["gg%d" % (l + 1)].numpy()
        for co in range(hi - lo):
            rep.inside(f"gb{l + 1}[{co}]", gb[co], *map(f32, enclose_sum(dz[:, co])))
            rep.inside(f"gg{l + 1}[{co}]", gg[co], *map(f32, enclose_sum(dz[:, co].astype(f64) * xh[:, co].astype(f64))))
        v = dz
        if not frozen:   # bn_apply_kernel: S1, S2 are the fp32 values that went to grad_bias, grad_gamma
            s1n, s2n = (gb.astype(f32) * inv_n).astype(f32).reshape(1, -1, 1, 1), (gg.astype(f32) * inv_n).astype(f32).reshape(1, -1, 1, 1)
            v = ((dz - s1n).astype(f32) - (xh * s2n).astype(f32)).astype(f32)
        dc = (per(alpha) * v).astype(f32)
        # the weight gradient: an fp32 tree inside a workgroup, float64 across workgroups
        a_in = x if l == 0 else activation(cs[l - 1], alpha[LAYERS[l - 1][0]:LAYERS[l - 1][1]], beta[LAYERS[l - 1][0]:LAYERS[l - 1][1]])
        ap, gw = padded(a_in).astype(f64), dev["gw%d" % (l + 1)].numpy().astype(f64)
        d64 = dc.astype(f64)
        for ci in range(a_in.shape[1]):
            for k in range(9):
                prod = d64 * ap[:, ci, k // 3:k // 3 + H, k % 3:k % 3 + W][:, None]          # exact: 24 x 24 bits
                mag = np.abs(prod).sum(axis=(0, 2, 3))
                for co in range(hi - lo):
                    err, bound = abs(gw[co, ci, k // 3, k % 3] - math.fsum(prod[:, co].reshape(-1).tolist())), GW_ROUNDINGS * 2.0 ** -24 * mag[co]
                    if err > 0:
                        rep.gw_ratio = max(rep.gw_ratio, err / bound if bound > 0 else math.inf)
                    if not err <= bound:
                        rep.bad.append(f"gw{l + 1}[{co}, {ci}, {k // 3}, {k % 3}]: error {err:.3e} beyond {GW_ROUNDINGS} 2^-24 sum|dc a| = {bound:.3e}")
        grad = adjoint_chain(dc, ws[l])
    rep.equal("gx down from grad_out", dev["gx"].numpy().reshape(B, 1, H, W), grad, shape)
    return rep


def emulate(fix, frozen, eps):
    """A host model of the ten kernels - the restated fp32 stages chained, float64 sums where the kernels carry float64 - in run_raw()'s result
    form.  The host test feeds it to check_stages(); the weight gradients are float64 sums rounded once (inside their bound, not the device's bits)."""
    eps = C.per_layer(eps)
    x, g = fix["x"].numpy(), fix["g"].numpy()
    ws = [fix["w%d" % l].numpy() for l in (1, 2, 3)]
    gamma, bias = fix["gamma"].numpy(), fix["bias"].numpy()
    B, _, H, W = x.shape
    n = B * H * W
    stats, alpha, beta, cs, acts, a = np.zeros(39, f32), np.zeros(13, f32), np.zeros(13, f32), [], [], x
    for l, (lo, hi) in enumerate(LAYERS):
        c = conv_chain(a, ws[l])
        for ch in range(lo, hi):
            if frozen:
                stats[ch], stats[26 + ch] = fix["rmean"][ch], fix["rvar"][ch]
                stats[13 + ch] = f32(1.0 / math.sqrt(float(fix["rvar"][ch]) + float(f32(eps[l]))))
            else:
                v = c[:, ch - lo].astype(f64).reshape(-1)
                stats[ch], stats[13 + ch], stats[26 + ch] = stats_statements(v.sum(), (v * v).sum(), n, eps[l])[:3]
        alpha[lo:hi], beta[lo:hi] = make_ab(gamma[lo:hi], bias[lo:hi], stats[lo:hi], stats[13 + lo:13 + hi])
        acts.append(a), cs.append(c)
        a = activation(c, alpha[lo:hi], beta[lo:hi])
    gp, grad, inv_n = np.zeros(422, f32), g, f32(1.0 / float(n))
    gw_at = {0: (0, 36), 1: (36, 324), 2: (324, 396)}
    for l in (2, 1, 0):
        lo, hi = LAYERS[l]
        per = lambda v: v[lo:hi].reshape(1, -1, 1, 1)
        dz = np.where(fma32(cs[l], per(alpha), per(beta)) > 0, grad, f32(0)).astype(f32)
        xh = ((cs[l] - per(stats[0:13])).astype(f32) * per(stats[13:26])).astype(f32)
        s1 = dz.astype(f64).sum(axis=(0, 2, 3)).astype(f32)
        s2 = (dz.astype(f64) * xh.astype(f64)).sum(axis=(0, 2, 3)).astype(f32)
        gp[409 + lo:409 + hi], gp[396 + lo:396 + hi] = s1, s2
        v = dz
        if not frozen:
            v = ((dz - (s1 * inv_n).astype(f32).reshape(1, -1, 1, 1)).astype(f32) - (xh * (s2 * inv_n).astype(f32).reshape(1, -1, 1, 1)).astype(f32)).astype(f32)
        dc = (per(alpha) * v).astype(f32)
        gp[gw_at[l][0]:gw_at[l][1]] = shift_dot(dc.astype(f64), acts[l].astype(f64)).astype(f32).reshape(-1)
        grad = adjoint_chain(dc, ws[l])
    return {"y": T(a), "saved": T(np.concatenate([c.reshape(-1) for c in cs])), "stats": T(stats), "gx": T(grad), "gp": T(gp)}


@functools.lru_cache(maxsize=None)
def stage_fixture(shape):
    """B's fixture: share_feature_train_cases.draw() - N(0, 1) image and grad_out, Kaiming weights - at one seed, no margin rule."""
    return C.draw(*shape, STAGE_SEED)


# ================================================================================================================= on the device
def run_raw(fix, dev, offsets=C.OFFSETS[0], frozen=True, eps=EPS_DYADIC):
    """share_feature_train_cases.run_raw() (NaN outputs inside 0xA5 margins, NaN workspace) -> (device_dict(), clean)."""
    res, clean = C.run_raw(fix, dev, offsets, frozen=frozen, eps=eps)
    return device_dict(res), clean
