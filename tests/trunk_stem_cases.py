"""Shared by tests/test_gpu_trunk_stem.py and tests/test_trunk_stem_host.py: the fixtures, truths, case lists and the raw-ABI runner of the trunk's first
stage, conv 7x7 / 2 / 3 + bias + ReLU + max pool 3 / 2 / 1, in its two forms - trunk_stem_kernel<NHWC, PR> (csrc/trunk_stem.hip, hdn_trunk_stem_f32: the
vector pipe, every size) and trunk_stem_mfma_kernel (csrc/trunk_stem_mfma.hip, hdn_trunk_stem_mfma_f32: the matrix cores, 127 x 127 channels-last).
Nothing here launches a kernel except run_stem, and no expected value comes from the library.

Truths.  One-hot sets: stem_expected of tests/trunk34_forms.py on int64 (one input element + bias per conv output: exact).  Dense fixture: integer x in
[-8, 8], w in [-3, 3], bias in [-20, 20]; |conv| <= 98 x 24 + 20 = 2,372 < 2^24, so fp32 is exact in any summation order and the truth is float64
max_pool2d(relu(conv2d)), compared by torch.equal.  Random data: float64, under check_per_image of tests/test_gpu_trunk50_forms.py.

The form rule (which kernel instantiation a shape takes) is restated here and compared with the sources as text (SOURCE_FACTS); the host test evaluates
it over the case lists.  lane_model restates the vector kernel's lane arithmetic (pair loads, the `sh` select, the wave shifts of the taps and of the
pool, the row select) in numpy for one purpose: the host test proves with it that the fixtures below reject a tap one column off, a missing `sh`
select, a pool neighbour from the wrong side and a padding row that is multiplied in instead of selected."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from geometry_bwd_cases import FILL, PAD, ROOT, at_offset, untouched
from test_gpu_trunk50_forms import _codes
from trunk34_forms import bias_int, first_difference, stem_expected  # noqa: F401 (first_difference: for the tests)

SEED = 20261020
CSRC = os.path.join(ROOT, "hdn_amd", "csrc")

# ================================================================================================================= the forms, restated
CO, CB, KS = 64, 16, 7                                     # output channels, channels per wave (the kernel's cb), kernel side
TAPS = 2 * KS * KS                                         # 98
W_MIN, W_MAX, B_MAX = 2, 128, 65535
WAVE = 64                                                  # one lane per conv column: Wc <= 64
SMALL_WAVES = 1024                                         # fewer waves of 4-row strips than this: 1-row strips
STRIP_ROWS = 4
MFMA_SIDE = 127
MFMA_ROWS = ((48, 16), (8, 8), (1, 4))                     # (from this batch on, conv rows per workgroup)
E_NULL, E_SHAPE, E_LIMIT, E_ALIAS = -1, -2, -3, -4

SOURCE_FACTS = (
    ("trunk_stem.hip", f"constexpr int CO = {CO}, CB = {CB}, KS = {KS}, NPAIR = CB / 2;"),
    ("trunk_stem.hip", "const int Hc = (H - 1) / 2 + 1, Wc = (W - 1) / 2 + 1, Hp = (Hc - 1) / 2 + 1, Wp = (Wc - 1) / 2 + 1;"),
    ("trunk_stem.hip", f"if (W < {W_MIN} || Wc > {WAVE} || B > {B_MAX} || (long long)H * W > (1LL << 24)) return HDN_E_LIMIT;"),
    ("trunk_stem.hip", f"const bool small = (long long)B * 4 * hdn::cdiv(Hp, {STRIP_ROWS}) < {SMALL_WAVES};"),
    ("trunk_stem.hip", f"const int pr = small ? 1 : {STRIP_ROWS};"),
    ("trunk_stem.hip", "const int strips = hdn::cdiv(Hp, pr);"),
    ("trunk_stem.hip", "const int cb = g & 3, s = (g >> 2) % strips_per_img, b = (g >> 2) / strips_per_img;"),
    ("trunk_stem.hip", "const bool sh = W >= 2 && 2 * lane == W - 1;"),
    ("trunk_stem.hip", "if (nhwc) { if (small) HDN_STEM_LAUNCH(true, 1); else HDN_STEM_LAUNCH(true, 4); }"),
    ("trunk_stem.hip", "else { if (small) HDN_STEM_LAUNCH(false, 1); else HDN_STEM_LAUNCH(false, 4); }"),
    ("trunk_stem.hip", "if (out == x) return HDN_E_ALIAS;"),
    ("trunk_stem_mfma.hip", f"constexpr int H = {MFMA_SIDE}, W = {MFMA_SIDE}, HC = 64, HP = 32, WP = 32, CO = {CO}, NSTEP = {KS};"),
    ("trunk_stem_mfma.hip", "const int rows = rows_env ? rows_env : (B >= %d ? %d : B >= %d ? %d : %d);"
     % (MFMA_ROWS[0][0], MFMA_ROWS[0][1], MFMA_ROWS[1][0], MFMA_ROWS[1][1], MFMA_ROWS[2][1])),
    ("../../include/hdn_hip.h", "#define HDN_E_NULL (%d)" % E_NULL), ("../../include/hdn_hip.h", "#define HDN_E_LIMIT (%d)" % E_LIMIT),
    ("../../include/hdn_hip.h", "#define HDN_E_ALIAS (%d)" % E_ALIAS), ("../../include/hdn_hip.h", "#define HDN_E_SHAPE (%d)" % E_SHAPE),
)


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def cdiv(a, b):
    return (a + b - 1) // b


def dims(H, W):
    """(Hc, Wc, Hp, Wp): the conv and the pooled size."""
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return Hc, Wc, (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1


def in_range(B, H, W):
    return B >= 1 and H >= 1 and W_MIN <= W <= W_MAX and dims(H, W)[1] <= WAVE and B <= B_MAX


def strip_rows(B, H, W):
    """Pooled rows per wave: 1 iff B 4 ceil(Hp / 4) < 1024."""
    return 1 if B * 4 * cdiv(dims(H, W)[2], STRIP_ROWS) < SMALL_WAVES else STRIP_ROWS


def strips(B, H, W):
    return cdiv(dims(H, W)[2], strip_rows(B, H, W))


def min_batch_of_4row_form(H, W):
    return cdiv(SMALL_WAVES, 4 * cdiv(dims(H, W)[2], STRIP_ROWS))


def sh_lane(W):
    """The lane whose pair would start at the row's last float (odd W): it reads one float earlier and shifts; None for an even W."""
    return (W - 1) // 2 if W % 2 else None


def mfma_rows(B):
    return next(rows for lo, rows in MFMA_ROWS if B >= lo)


def where(B, H, W, nhwc, idx, taps=None):
    """The form, layout, shape and owner of output element idx = (image, channel, pooled row, pooled column)."""
    b, c, p, q = (int(v) for v in idx)
    pr, n = strip_rows(B, H, W), strips(B, H, W)
    cb, s = c // CB, p // pr
    text = (f"{pr}-row strips, {'channels-last' if nhwc else 'NCHW'}, (B, H, W) = ({B}, {H}, {W}): image {b}, channel {c}, pooled (row, column) = ({p}, {q}); "
            f"wave (cb, strip) = ({cb}, {s}) = wave {(b * n + s) * 4 + cb} of {B * n * 4}, conv rows {2 * p - 1}..{2 * p + 1}, lanes {2 * q - 1}..{2 * q + 1} "
            f"(sh lane: {sh_lane(W)}, last conv lane {dims(H, W)[1] - 1})")
    if taps is not None:
        text += f", tap (ci, ky, kx) = ({int(taps[0][c])}, {int(taps[1][c])}, {int(taps[2][c])})"
    return text


def difference(got, want, B, H, W, nhwc, taps=None):
    """None if torch.equal, else first_difference's text with the owner of the first wrong element."""
    text = first_difference(got, want)
    if text is None or got.shape != want.shape:
        return text
    return text + " [" + where(B, H, W, nhwc, (got != want).nonzero()[0].tolist(), taps) + "]"


# ================================================================================================================= one-hot sets
N_SETS = 7


def onehot_tap(s):
    """The tap index of every output channel in set s: t = (16 s + co mod 16 + 5 (co // 16)) mod 98."""
    co = torch.arange(CO)
    return (16 * s + co % CB + 5 * (co // CB)) % TAPS


def onehot_set(s):
    """(w [64, 2, 7, 7], ci, ky, kx): the one 1.0 of channel co at tap t = onehot_tap(s)[co], (ci, ky, kx) = (t // 49, (t // 7) mod 7, t mod 7)."""
    t = onehot_tap(s)
    ci, ky, kx = t // (KS * KS), (t // KS) % KS, t % KS
    w = torch.zeros(CO, 2, KS, KS)
    w[torch.arange(CO), ci, ky, kx] = 1.0
    return w, ci, ky, kx


@functools.lru_cache(maxsize=4)
def onehot_case(s, B, H, W):
    """(x int64 [B,2,H,W] codes, w, (ci, ky, kx), bias int64 [64], want int64 [B,64,Hp,Wp]) of set s."""
    xi, bi = _codes((B, 2, H, W)), bias_int(CO, k=s)
    w, ci, ky, kx = onehot_set(s)
    return xi, w, (ci, ky, kx), bi, stem_expected(xi, ci, ky, kx, bi)


# ================================================================================================================= the dense integer fixture
X_MAX, W_ABS, B_ABS = 8, 3, 20
EXACT_BOUND = TAPS * X_MAX * W_ABS + B_ABS                 # 2,372


def _table(seed, shape, lo, hi):
    return torch.from_numpy(np.random.default_rng(SEED + seed).integers(lo, hi + 1, shape).astype(np.float32))


@functools.lru_cache(maxsize=None)
def dense_weights(nozero=False):
    """(w [64,2,7,7] integer in [-3, 3], bias [64] integer in [-20, 20]); nozero: w from {-3..-1, 1..3}."""
    w = _table(1, (CO, 2, KS, KS), -W_ABS, W_ABS)
    if nozero:
        m = _table(2, (CO, 2, KS, KS), 0, 2 * W_ABS - 1)                                         # 0..5 -> -3..-1, 1..3
        w = torch.where(m < W_ABS, m - W_ABS, m - W_ABS + 1)
    return w, _table(3, (CO,), -B_ABS, B_ABS)


def dense_image(B, H, W):
    """x [B,2,H,W] integer in [-8, 8]; the first images of a larger batch of the same (H, W) are the same."""
    rng = np.random.default_rng(SEED + 1009 * H + W)
    return torch.from_numpy(rng.integers(-X_MAX, X_MAX + 1, (B, 2, H, W)).astype(np.float32))


def truth64(x, w, b):
    """float64 max_pool2d(relu(conv2d(x, w, b, stride 2, padding 3)), 3, 2, 1)."""
    return F.max_pool2d(torch.relu(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=3)), 3, 2, 1)


@functools.lru_cache(maxsize=2)
def dense_case(B, H, W, nozero=False):
    """(x, w, bias, truth float64 [B,64,Hp,Wp])."""
    x = dense_image(B, H, W)
    w, b = dense_weights(nozero)
    return x, w, b, truth64(x, w, b)


# ================================================================================================================= case lists: (B, H, W)
ALL_WIDTHS = tuple((2, H, W) for H in (5, 6) for W in range(W_MIN, W_MAX + 1))                    # the 1-row form
HEIGHTS = tuple((2, H, W) for W in (7, 64) for H in range(1, 27))                                 # row -1 / last row / Hc parity in every residue
# the smallest batch of the 4-row form at each shape (256 for Hp <= 4, 128 for Hp 5..8, 86 for Hp = 9): every Hp mod 4, one to three strips; each shape
# also runs with one image fewer, in the 1-row form
STRIP4 = ((256, 1, 2), (256, 5, 3), (256, 9, 13), (256, 13, 128), (128, 17, 6), (128, 21, 127), (128, 29, 65), (86, 33, 31))
STRIP_CASES = tuple((B - d, H, W) for B, H, W in STRIP4 for d in (0, 1))
OFFSET_WIDTHS = tuple((2, 5, W) for W in (2, 3, 127, 128))
OFFSETS = tuple((xo, oo) for xo in range(4) for oo in range(4))                                   # float offsets of x and out in a 16-byte line
STRIP_OFFSETS = tuple((xo, 0) for xo in range(4)) + tuple((0, oo) for oo in range(1, 4)) + ((1, 2), (2, 3), (3, 1))   # the large strip shapes
ONEHOT_WIDTHS = tuple((2, 9, W) for W in (2, 3, 4, 5, 7, 8, 31, 32, 33, 63, 64, 65, 95, 96, 97, 125, 126, 127, 128))
ONEHOT_STRIP4 = ((256, 9, 13), (128, 17, 127))
ONEHOT_MFMA_BATCHES = (1, 8, 48)                                                                  # 4 / 8 / 16 conv rows per workgroup
RANDOM_SHAPES = ((2, 127, 127), (33, 127, 127), (1, 126, 125), (130, 31, 29))
RANDOM_SCALES = (1.0, 120.0)
LAYOUTS = (False, True)                                                                          # nhwc


# ================================================================================================================= non-finite pixels
NONFINITE_SHAPES = ((2, 17, 13), (128, 17, 13))                                                   # 1-row and 4-row strips (two strips), an odd width


def nonfinite_positions(B, H, W):
    """(name, image, input channel, row, column): row 0 (which rows outside the image re-read), the last row, column W - 2 (the clamped pair's first
    float), column W - 1 of an odd W (the `sh` lane) and an interior pixel."""
    assert W % 2 == 1 and H >= 9 and W >= 9
    b = B // 2
    return (("row 0", b, 0, 0, 5), ("row 0", B - 1, 1, 0, 0), ("last row", b, 1, H - 1, 6), ("column W-2", b, 0, 8, W - 2),
            ("column W-1", b, 1, 7, W - 1), ("column W-1", 0, 0, 0, W - 1), ("interior", b, 0, 8, 6))


def field(B, H, W, b, iy, ix):
    """bool [B,1,Hp,Wp]: the outputs whose receptive field (through the pool) holds input pixel (iy, ix) of image b - every channel sees both planes."""
    ind = torch.zeros(B, 1, H, W, dtype=torch.float64)
    ind[b, 0, iy, ix] = 1.0
    conv = F.conv2d(ind, torch.ones(1, 1, KS, KS, dtype=torch.float64), stride=2, padding=3)
    return F.max_pool2d(conv, 3, 2, 1) > 0


def poisoned(x, value, b, ci, iy, ix):
    x = x.clone()
    x[b, ci, iy, ix] = value
    return x


# ================================================================================================================= the lane arithmetic, restated
MUTANTS = ("kx", "sh", "pool", "mul")


def _shift(v, d, axis):
    """Lane l <- lane l - d along `axis`, 0 shifted in (the wave shifts of from_prev_lane / from_next_lane)."""
    out = np.zeros_like(v)
    src = [slice(None)] * v.ndim
    dst = [slice(None)] * v.ndim
    src[axis], dst[axis] = (slice(0, -1), slice(1, None)) if d == 1 else (slice(1, None), slice(0, -1))
    out[tuple(dst)] = v[tuple(src)]
    return out


def lane_model(x, w, bias, mutant=None):
    """trunk_stem_kernel's arithmetic per lane in float64 numpy: x [B,2,H,W], w [64,2,7,7], bias [64] -> [B,64,Hp,Wp].  mutant: None, or one of
    'kx' (tap kx reads the element of tap kx + 1: one column off), 'sh' (the clamped pair is not shifted), 'pool' (the right neighbour of the pool
    comes from the left), 'mul' (a row outside the image is the re-read row 0 times 0 instead of a selected 0)."""
    assert mutant is None or mutant in MUTANTS
    x, w, bias = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(bias, np.float64)
    B, _, H, W = x.shape
    Hc, Wc, Hp, Wp = dims(H, W)
    lane = np.arange(WAVE)
    ok0, ok1 = 2 * lane < W, 2 * lane + 1 < W
    ix0 = np.minimum(2 * lane, max(W - 2, 0))
    sh = (2 * lane == W - 1) & (mutant != "sh")
    r = np.arange(-1, 2 * Hp)                                                                      # conv rows 2p - 1 .. 2p + 1 of every pooled row
    acc = np.zeros((B, r.size, WAVE, CO))
    with np.errstate(all="ignore"):
        for ci in range(2):
            for ky in range(KS):
                iy = 2 * r - 3 + ky
                rok = (iy >= 0) & (iy < H)
                rows = x[:, ci, np.where(rok, iy, 0), :]                                           # rows outside the image re-read row 0
                vx, vy = rows[:, :, ix0], rows[:, :, ix0 + 1]
                first = np.where(sh, vy, vx)
                if mutant == "mul":
                    k = rok[None, :, None].astype(np.float64)
                    own_x, own_y = np.where(ok0, first, 0.0) * k, np.where(ok1, vy, 0.0) * k
                else:
                    own_x, own_y = np.where(ok0 & rok[None, :, None], first, 0.0), np.where(ok1 & rok[None, :, None], vy, 0.0)
                p_x, p_y = _shift(own_x, 1, 2), _shift(own_y, 1, 2)
                taps = [_shift(p_y, 1, 2), p_x, p_y, own_x, own_y, _shift(own_x, -1, 2), _shift(own_y, -1, 2)]
                for kx in range(KS):
                    v = taps[min(kx + 1, KS - 1)] if mutant == "kx" else taps[kx]
                    acc += v[..., None] * w[None, None, None, :, ci, ky, kx]
        keep = ((lane < Wc)[None, None, :, None]) & ((r >= 0) & (r < Hc))[None, :, None, None]
        act = np.where(keep, np.fmax(acc + bias, 0.0), 0.0)                                        # fmaxf: a NaN becomes 0
        out = np.empty((B, CO, Hp, Wp))
        for p in range(Hp):
            m = np.fmax(np.fmax(act[:, 2 * p], act[:, 2 * p + 1]), act[:, 2 * p + 2])              # r[2p] = conv row 2p - 1
            right = _shift(m, 1, 1) if mutant == "pool" else _shift(m, -1, 1)
            res = np.fmax(np.fmax(_shift(m, 1, 1), m), right)
            out[:, :, p, :] = res[:, 0:2 * Wp:2, :].transpose(0, 2, 1)
    return torch.from_numpy(out)


# ================================================================================================================= on the device
def _lib():
    from hdn_amd import _lib as L
    return L


def same_bits(view, host):
    return torch.equal(view.cpu().contiguous().reshape(-1).view(torch.int32), host.contiguous().reshape(-1).view(torch.int32))


class Inputs:
    """x at float offset xoff inside margins of NaN (a read beyond the tensor would poison a result), wT = w as [ci][ky][kx][co] and bias aligned, as
    FusedStem passes them."""

    def __init__(self, x, w, bias, dev, xoff=0):
        self.x, self.wT, self.b = x.float().contiguous(), w.float().permute(1, 2, 3, 0).contiguous(), bias.float().contiguous()
        self.dev, self.shape = dev, tuple(x.shape)
        self.xd = at_offset(self.x, xoff, dev, margin=PAD, fill=float("nan"))[0]
        self.wd, self.bd = self.wT.to(dev), self.b.to(dev)

    def unchanged(self):
        return same_bits(self.xd, self.x) and same_bits(self.wd, self.wT) and same_bits(self.bd, self.b)


def run_stem(inp, nhwc, ooff=0):
    """One raw call of hdn_trunk_stem_f32; the output starts as NaN at float offset ooff inside margins of 0xA5:
    -> (out as an NCHW view [B,64,Hp,Wp] on the CPU, nothing outside the result written?)."""
    L = _lib()
    B, _, H, W = inp.shape
    _, _, Hp, Wp = dims(H, W)
    n = B * CO * Hp * Wp
    view, buf = at_offset(n, ooff, inp.dev, margin=PAD, fill=FILL)
    L.check(L.load().hdn_trunk_stem_f32(L.ptr(inp.xd), L.ptr(inp.wd), L.ptr(inp.bd), L.ptr(view), B, H, W, 1 if nhwc else 0, L.stream_ptr(inp.dev)),
            "hdn_trunk_stem_f32")
    torch.cuda.synchronize(inp.dev)
    got = view.cpu()
    got = got.view(B, Hp, Wp, CO).permute(0, 3, 1, 2) if nhwc else got.view(B, CO, Hp, Wp)
    return got, untouched(buf.cpu(), PAD + ooff, PAD + ooff + n)


@functools.lru_cache(maxsize=None)
def random_weights():
    """A folded first convolution's scale: w ~ N(0, 0.05^2), bias ~ U(-0.5, 0.5)."""
    rng = np.random.default_rng(SEED + 77)
    return (torch.from_numpy((0.05 * rng.standard_normal((CO, 2, KS, KS))).astype(np.float32)),
            torch.from_numpy(rng.uniform(-0.5, 0.5, CO).astype(np.float32)))


@functools.lru_cache(maxsize=1)
def random_case(B, H, W, scale):
    """(x = scale N(0, 1), w, bias, truth float64, PyTorch's CPU fp32 result)."""
    rng = np.random.default_rng(SEED + 31 * B + 7 * H + W)
    x = torch.from_numpy((scale * rng.standard_normal((B, 2, H, W))).astype(np.float32))
    w, b = random_weights()
    with torch.no_grad():
        ref32 = F.max_pool2d(torch.relu(F.conv2d(x, w, b, stride=2, padding=3)), 3, 2, 1)
    return x, w, b, truth64(x, w, b), ref32
