"""Shared by tests/test_gpu_share_feature_forms.py and tests/test_share_feature_host.py: an exact fixture for PreShareFeature (csrc/share_feature.hip), a
float64 reference that is independent of oracle.hdn_oracle.share_feature, the strip-height rule of the rows kernel restated, and the case tables that
reach every strip height, every end of a strip and every tile edge.  Nothing here launches a kernel except launch() and the __main__ block, which is the
child process of test_forced_strip_height_sweep_is_exact (HDN_SF_STRIP is read once per process).

The exact fixture: integer conv weights in [-2, 2], BatchNorm scales that are powers of two (2^-2 .. 2^-5), integer shifts, integer images in [-3, 3].
Every product and every partial sum of a layer is then an integer times a power of two (2^0 in layer 1, 2^-4 in layer 2, 2^-9 in layer 3 and 2^-11 after
the last scale, with the scales below) and stays far below 2^24 of these quanta, so fp32 gives the same result in any summation order, fused or not, and
a kernel has to be BIT-equal to the float64 chain.  exactness_headroom() works that out for an input instead of trusting this paragraph."""
import functools
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 20261019
SF_ALPHA, SF_BETA, N_PARAMS = 396, 409, 422          # include/hdn_hip.h: 13 scales at SF_ALPHA, 13 shifts at SF_BETA
# -log2 of the 13 scales and the 13 shifts (layer 1: 4, layer 2: 8, layer 3: 1).  The scales are a seeded draw from 2 .. 5; the shifts are then tuned on
# the float64 reference: ceil(-median) of a channel's scaled convolution in layers 1 and 2 (no channel is dead, the wide ones clip about half), and for
# the last layer, which the draw's 2^-5 and any integer shift left either never or always clipped, the scale 2^-2 and -round(median).
SCALE_EXPS = (4, 3, 3, 4, 5, 4, 2, 5, 2, 4, 4, 4, 2)
SHIFTS = (0, 0, 0, 0, 1, 1, 1, 0, 1, 0, 0, 1, -3)
CLIP_SHARE = (0.10, 0.90)                            # every ReLU clips a share of its values inside this interval (asserted by the host test)


# ----------------------------------------------------------------------------------------------------------------- parameters
def _block(ws, alpha, beta):
    """The kernel's 422-float block: the weight layout comes from hdn_amd.fold_params (on an identity BatchNorm), scales and shifts are written over."""
    import hdn_amd
    sd = {}
    for (conv, bn), w in zip(((0, 1), (3, 4), (6, 7)), ws):
        n = w.shape[0]
        sd[f"ShareFeature.{conv}.weight"] = w.float()
        sd[f"ShareFeature.{bn}.weight"], sd[f"ShareFeature.{bn}.running_var"] = torch.ones(n), torch.ones(n)
        sd[f"ShareFeature.{bn}.bias"], sd[f"ShareFeature.{bn}.running_mean"] = torch.zeros(n), torch.zeros(n)
    folded = hdn_amd.fold_params(sd).clone()
    assert folded.numel() == N_PARAMS and SF_BETA + 13 == N_PARAMS
    folded[SF_ALPHA:SF_ALPHA + 13] = alpha.float()
    folded[SF_BETA:SF_BETA + 13] = beta.float()
    return folded


@functools.lru_cache(maxsize=None)
def exact_params():
    """(ws: three float64 conv weights, alpha [13] float64, beta [13] float64, folded: the fp32 block) of the exact fixture."""
    g = np.random.default_rng(SEED)
    ws = [torch.from_numpy(g.integers(-2, 3, s)).double() for s in ((4, 1, 3, 3), (8, 4, 3, 3), (1, 8, 3, 3))]
    alpha = torch.tensor([2.0 ** -e for e in SCALE_EXPS], dtype=torch.float64)
    beta = torch.tensor(SHIFTS, dtype=torch.float64)
    return ws, alpha, beta, _block(ws, alpha, beta)


@functools.lru_cache(maxsize=None)
def ones_params():
    """All-ones weights, scale 1, shift 0: the output counts the 3-step paths from a pixel, nothing is clipped for a non-negative input."""
    ws = [torch.ones(4, 1, 3, 3, dtype=torch.float64), torch.ones(8, 4, 3, 3, dtype=torch.float64), torch.ones(1, 8, 3, 3, dtype=torch.float64)]
    alpha, beta = torch.ones(13, dtype=torch.float64), torch.zeros(13, dtype=torch.float64)
    return ws, alpha, beta, _block(ws, alpha, beta)


def exact_image(B, H, W):
    """Integer image in [-3, 3], fp32 [B, 1, H, W], another one per shape."""
    g = np.random.default_rng(SEED + 1000003 * B + 1009 * H + W)
    return torch.from_numpy(g.integers(-3, 4, (B, 1, H, W)).astype(np.float32))


# ----------------------------------------------------------------------------------------------------------------- references
def chain(x, ws, alpha, beta, dtype=torch.float64, pre=None):
    """3 x (conv3x3 with its own zero padding -> scale -> shift -> clamp at 0) in `dtype`; pre, if a list, receives the three pre-clamp tensors."""
    y, off = x.to(dtype), 0
    for w in ws:
        n = w.shape[0]
        y = F.conv2d(y, w.to(dtype), padding=1) * alpha[off:off + n].to(dtype).view(1, n, 1, 1) + beta[off:off + n].to(dtype).view(1, n, 1, 1)
        if pre is not None:
            pre.append(y)
        y = y.clamp_min(0)
        off += n
    return y


def reference64(x, params):
    ws, alpha, beta, _ = params
    return chain(x, ws, alpha, beta)


def exactness_headroom(x, params):
    """max over the layers of (a bound on every partial sum, in any order) / (2^24 quanta of that layer): below 1, fp32 holds every intermediate exactly.
    The bound is the chain on |x|, |w|, |shift| without the clamp; the quantum of a layer is the product of the smallest scales before it (all values
    are integers times powers of two), times the layer's own smallest scale after its BatchNorm."""
    ws, alpha, beta, _ = params
    y, off, q, worst = x.double().abs(), 0, 1.0, 0.0
    for w in ws:
        n = w.shape[0]
        acc = F.conv2d(y, w.abs(), padding=1)
        worst = max(worst, float(acc.max()) / (q * 2.0 ** 24))
        q *= float(alpha[off:off + n].min())
        y = acc * alpha[off:off + n].view(1, n, 1, 1) + beta[off:off + n].abs().view(1, n, 1, 1)
        worst = max(worst, float(y.max()) / (q * 2.0 ** 24))
        off += n
    return worst


def clip_shares(x, params):
    """Share of strictly negative pre-activations in front of each of the three ReLUs, on the float64 reference."""
    ws, alpha, beta, _ = params
    pre = []
    chain(x, ws, alpha, beta, pre=pre)
    return [float((p < 0).double().mean()) for p in pre]


def first_difference(got, want):
    """None if the [B, 1, H, W] tensors are bit-for-value equal, else (count, (image, row, column), got, want) of the first wrong output."""
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return None
    bad = (got != want).nonzero()
    b, _, r, c = bad[0].tolist()
    return int(bad.shape[0]), (b, r, c), float(got[b, 0, r, c]), float(want[b, 0, r, c])


# ----------------------------------------------------------------------------------------------------------------- the launch rule
def strip_rows(B, H):
    """Rows per wave of share_feature_rows_kernel, as launch_sf_rows (csrc/share_feature.hip) picks them without HDN_SF_STRIP: one row per wave up to
    1024 rows in all, else the smallest of 2, 4, 8, ... that keeps the launch inside 3072 waves, stopping once a strip holds the whole image."""
    n = 1 if B * H <= 1024 else 2
    while n < H and B * -(-H // n) > 3072:
        n *= 2
    return n


def strips(n, H):
    """[(ra, rb)] of the strips of n rows of an H-row image: output rows [ra, rb)."""
    return [(ra, min(ra + n, H)) for ra in range(0, H, n)]


# ----------------------------------------------------------------------------------------------------------------- the cases
ROWS_MAX_W = 128                                     # W <= 128: share_feature_rows_kernel; wider: share_feature_kernel on TILE_ROWS x TILE_COLS tiles
TILE_ROWS, TILE_COLS = 4, 128
PROD = [(B, 127, 127) for B in (1, 8, 9, 47, 64, 128)]
PROD_N = [1, 1, 2, 2, 4, 8]
N16 = [(1100, 17, 5), (4000, 3, 5)]                  # 16 rows per wave (two strips: 16 + 1); the n >= H stop (n = 4 over 3 rows, one strip)
N16_N = [16, 4]
SWEEP_B = 3
SWEEP_H = tuple(range(1, 27))
SWEEP_H_TALL = (33, 34, 35)                          # 16-row strips: the last-strip lengths 1, 2, 3 at the H mod 3 that 1 .. 26 does not pair them with
SWEEP_W = (1, 2, 3, 31, 32, 33, 63, 64, 65, 126, 127, 128)
FORCED_N = (1, 2, 4, 8, 16)
TILE = [(2, H, W) for W in (129, 130, 255, 256, 257, 384, 385) for H in (1, 3, 4, 5, 8, 9)]   # 384: the near side of the edge 385 is beyond


def sweep_sizes():
    return [(H, W) for H in SWEEP_H + SWEEP_H_TALL for W in SWEEP_W]


def bright_pixels(H, W):
    """Where test_one_bright_pixel_reaches_its_7x7_neighbourhood puts its pixel: the corners, the edge midpoints, and rows on both sides of a 4- and an
    8-row boundary crossed with columns on both sides of a DPP row (16 lanes = 32 columns), a half wave, the rows kernel's last lane and a 128-column
    tile."""
    pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]
    pts += [(r, c) for r in (3, 4, 7, 8) for c in (31, 32, 63, 64, 126, 127, 128, 255, 256) if r < H and c < W]
    return sorted(set(pts))


BRIGHT_SIZES = [(13, 127), (26, 128), (9, 257)]


# ----------------------------------------------------------------------------------------------------------------- on the device
def launch(x, folded, out):
    """hdn_share_feature_f32 through the C ABI on tensors of the caller's (x [B, 1, H, W] contiguous; out of the same size, written in place)."""
    from hdn_amd import _lib
    B, _, H, W = x.shape
    rc = _lib.load().hdn_share_feature_f32(_lib.ptr(x), _lib.ptr(folded), _lib.ptr(out), B, H, W, _lib.stream_ptr(x.device))
    _lib.check(rc, "PreShareFeature")
    return out


def run_poisoned(x, folded, dev):
    """The kernel's answer on the CPU, from an output buffer that held NaN: an output the kernel never wrote cannot pass for a right one."""
    xd = x.to(dev)
    out = torch.full_like(xd, float("nan"))
    return launch(xd, folded, out).cpu()


def sweep_failures(dev):
    """Every sweep size at SWEEP_B images on the exact fixture against float64: [[H, W, image, row, column]] of the first wrong output of each size."""
    params = exact_params()
    folded = params[3].to(dev)
    bad = []
    for H, W in sweep_sizes():
        x = exact_image(SWEEP_B, H, W)
        d = first_difference(run_poisoned(x, folded, dev), reference64(x, params).float())
        if d is not None:
            bad.append([H, W, *d[1]])
    return bad


if __name__ == "__main__":
    # the child of test_forced_strip_height_sweep_is_exact: HDN_SF_STRIP is set by the parent; one JSON line is the answer
    if not torch.cuda.is_available():
        sys.exit("no GPU")
    print(json.dumps({"strip": os.environ.get("HDN_SF_STRIP"), "sizes": len(sweep_sizes()), "failures": sweep_failures(torch.device("cuda:0"))}))
