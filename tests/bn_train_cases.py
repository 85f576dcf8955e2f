"""Cases and problem builders of the training BatchNorm + ReLU kernels (hdn_bn_relu_train_fwd_f32 / _bwd_f32), shared by tests/test_bn_train_host.py
(no GPU: the builders against float64 autograd) and tests/test_gpu_bn_train.py.  A helper module, not a conftest.

A problem is flat: c [N = B P][C] (the channels-last map), gamma, beta [C], dy [B][C][P] (NCHW order; .permute(0, 2, 1) is its channels-last form),
running buffers rm0, rv0 [C].  shape4(B, P, C) is the [B, C, H, W] the Python wrappers take."""
import functools

import torch
import torch.nn.functional as F

FUSED_MAX_ROWS = 400           # bn_train.hip: form 0 (one launch) up to this N = B P, form 1 (partial sums, finish, apply) beyond
_B0 = FUSED_MAX_ROWS // 25     # the last batch of form 0 when B is walked at P = 25

BASE_CASES = [(2, 1, 32), (1, 2, 32), (3, 25, 32), (2, 25, 256), (5, 49, 96), (1, 169, 64), (2, 841, 64), (32, 25, 256)]
THRESHOLD_CASES = [(_B0, 25, 256), (_B0 + 1, 25, 256)]     # the last batch of form 0 and the first of form 1 (7 chunks, the last of 41 rows)
CASES = BASE_CASES + THRESHOLD_CASES
LARGE_MEAN_CASES = [(3, 25, 32), (2, 841, 64)]
# even N; the last two sit on either side of the threshold
EXACT_CASES = [(2, 1, 32), (1, 2, 32), (2, 25, 256), (2, 169, 96), (2, 841, 64), (32, 25, 256), (_B0, 25, 256), (_B0 + 2, 25, 256)]
EXACT_EPS, EXACT_MOMENTUM = 0.75, 0.5
EPS, MOMENTUM = 1e-5, 0.1
MARGIN = 1e-3

_SIDES = {1: (1, 1), 2: (1, 2), 25: (5, 5), 49: (7, 7), 169: (13, 13), 841: (29, 29)}


def shape4(B, P, C):
    H, W = _SIDES[P]
    return (B, C, H, W)


def as4(c_flat, B, P, C):
    """The channels-last [B, C, H, W] view of the flat [N][C] map (no copy)."""
    H, W = _SIDES[P]
    return c_flat.view(B, H, W, C).permute(0, 3, 1, 2)


def z64(c, gamma, beta, eps):
    c = c.double()
    mean, var = c.mean(0), c.var(0, unbiased=False)
    return (c - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def min_abs_z(c, gamma, beta, eps=EPS):
    return float(z64(c, gamma, beta, eps).abs().min())


def _fix_margin(c, gamma, beta, eps):
    """Move every c whose float64 |z| < MARGIN by 0.25 until none is left: a ReLU mask that flips under rounding changes S1 by a whole dy, which no
    tolerance covers.  The margin is a condition of the problem, not of the kernel."""
    for _ in range(50):
        bad = z64(c, gamma, beta, eps).abs() < MARGIN
        if not bool(bad.any()):
            return c
        c = torch.where(bad, c + 0.25, c)
    raise AssertionError("the margin fix-up did not end")


def _common(B, P, C, g):
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g)
    dy = torch.randn(B, C, P, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    return gamma, beta, dy, rm0, rv0


@functools.lru_cache(maxsize=None)
def random_problem(B, P, C, seed=0):
    """(a): c ~ 2 N(0, 1) + 0.5, gamma in [0.5, 1.5], beta ~ N(0, 1), every float64 |z| >= MARGIN."""
    g = torch.Generator().manual_seed(1000 * seed + B * 31 + P * 7 + C)
    c = 2.0 * torch.randn(B * P, C, generator=g) + 0.5
    gamma, beta, dy, rm0, rv0 = _common(B, P, C, g)
    return _fix_margin(c, gamma, beta, EPS), gamma, beta, dy, rm0, rv0


@functools.lru_cache(maxsize=None)
def large_mean_problem(B, P, C):
    """(c): c ~ 1000 + N(0, 1): a folded z or fp32 sums of squares cannot pass."""
    g = torch.Generator().manual_seed(77 + B * 31 + P * 7 + C)
    c = 1000.0 + torch.randn(B * P, C, generator=g)
    gamma, beta, dy, rm0, rv0 = _common(B, P, C, g)
    return _fix_margin(c, gamma, beta, EPS), gamma, beta, dy, rm0, rv0


def reference(problem, B, P, C, relu, eps=EPS, momentum=MOMENTUM, dtype=torch.float64, track=True):
    """F.batch_norm (training) [+ relu] and its autograd on the CPU in `dtype`: y [B][C][P], dc [N][C], dgamma, dbeta, mean, invstd, rm, rv."""
    c, gamma, beta, dy, rm0, rv0 = (t.to(dtype) for t in problem)
    x = c.view(B, P, C).permute(0, 2, 1).contiguous().requires_grad_(True)
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = (rm0.clone(), rv0.clone()) if track else (None, None)
    z = F.batch_norm(x, rm, rv, gm, bt, True, momentum, eps)
    y = torch.relu(z) if relu else z
    y.backward(dy)
    mean, var = c.mean(0), c.var(0, unbiased=False)
    return {"y": y.detach(), "dc": x.grad.permute(0, 2, 1).reshape(B * P, C), "dgamma": gm.grad, "dbeta": bt.grad, "mean": mean,
            "invstd": 1.0 / torch.sqrt(var + eps), "rm": rm, "rv": rv}


@functools.lru_cache(maxsize=None)
def references(kind, B, P, C, relu):
    """(float64 truth, PyTorch-CPU fp32) of a random (kind 'a') or large-mean ('c') problem, computed once."""
    prob = random_problem(B, P, C) if kind == "a" else large_mean_problem(B, P, C)
    return reference(prob, B, P, C, relu), reference(prob, B, P, C, relu, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def exact_problem(B, P, C, seed=0):
    """(b): c = m[ch] +- 0.5 in equal halves per channel (a seeded permutation), eps 0.75 (var + eps = 1, invstd = 1), gamma in {1, 2, 4}, integer beta,
    m and rm0, momentum 0.5; integer dy whose sums over the (sign of c - m) x (z > 0) groups of a channel are multiples of 4 N, so that S1 and S2 are
    multiples of 2 N with and without the ReLU and every quotient is an integer.  Returns (problem, expectations by relu); the expectations are closed
    forms in float64, not autograd."""
    N = B * P
    assert N % 2 == 0
    g = torch.Generator().manual_seed(500 + 1000 * seed + B * 31 + P * 7 + C)
    m = torch.randint(-4, 5, (C, ), generator=g).double()
    sign = torch.empty(N, C, dtype=torch.float64)
    half = torch.cat([torch.full((N // 2, ), 0.5), torch.full((N // 2, ), -0.5)]).double()
    for ch in range(C):
        sign[:, ch] = half[torch.randperm(N, generator=g)]
    c = m + sign
    gamma = torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64)[torch.randint(0, 3, (C, ), generator=g)]
    beta = torch.randint(-2, 3, (C, ), generator=g).double()
    rm0, rv0 = torch.randint(-3, 4, (C, ), generator=g).double(), torch.ones(C, dtype=torch.float64)
    z = sign * gamma + beta                                           # invstd = 1
    dy = torch.randint(-3, 4, (N, C), generator=g).double()
    for pos in (True, False):
        for on in (True, False):
            grp = ((sign > 0) == pos) & ((z > 0) == on)
            s = (dy * grp).sum(0)
            fix = s - torch.round(s / (4 * N)) * (4 * N)
            first = grp.to(torch.uint8).argmax(0)                     # the group's first row per channel (row 0 where the group is empty: fix = 0)
            dy[first, torch.arange(C)] -= fix
    expect = {}
    for relu in (0, 1):
        dz = dy * (z > 0) if relu else dy
        s1, s2 = dz.sum(0), (dz * sign).sum(0)
        assert bool(((s1 % (2 * N)) == 0).all()) and bool(((s2 % (2 * N)) == 0).all())
        expect[relu] = {"y": (torch.relu(z) if relu else z).view(B, P, C).permute(0, 2, 1).contiguous(), "dc": gamma * (dz - s1 / N - sign * s2 / N),
                        "dgamma": s2, "dbeta": s1, "mean": m, "invstd": torch.ones(C, dtype=torch.float64),
                        "rm": 0.5 * rm0 + 0.5 * m, "rv": 0.5 * rv0 + 0.5 * 0.25 * N / (N - 1)}
    prob = tuple(t.float() for t in (c, gamma, beta, dy.view(B, P, C).permute(0, 2, 1).contiguous(), rm0, rv0))
    return prob, expect


def bound(got, truth, ref32):
    """(err, 4 e_ref + 1e-5 scale): the project's bound per tensor, e_ref the error of PyTorch-CPU fp32 on the same problem, scale = max |truth|."""
    truth = truth.double()
    err = float((got.double() - truth).abs().max())
    e_ref, scale = float((ref32.double() - truth).abs().max()), float(truth.abs().max())
    return err, 4 * e_ref + 1e-5 * scale
