"""Shared by tests/test_head_batch_host.py and tests/test_gpu_head_batch.py: the shapes that reach every tile and edge situation of
hdn_head_conv3x3_batch_f32 (csrc/head_conv.hip), its documented output offset as a Python function, the integer-indexed expectation of the exact
addressing test and the float64 convolutions.  Nothing here launches a kernel."""
import torch
import torch.nn.functional as F

E_NULL, E_SHAPE, E_LIMIT, E_ALIAS = -1, -2, -3, -4

# (Hi, Wi, n, B, CO, groups, nhwc): 64-pixel tiles of 32 channels, one workgroup per (tile, channel block, level x image)
CASES = [
    (7, 7, 3, 1, 512, 2, False),      # the template, one partial tile
    (7, 7, 3, 2, 512, 2, True),
    (7, 7, 1, 3, 64, 2, False),       # odd batch
    (7, 7, 2, 5, 64, 1, True),
    (15, 15, 3, 2, 512, 2, True),     # log-polar template, 169 px = 2 full tiles + 1 partial
    (3, 3, 4, 3, 64, 2, False),       # one output pixel
    (9, 14, 1, 2, 64, 2, True),       # not square
    (31, 31, 1, 2, 64, 2, False),     # conv_search at B > 1, 14 tiles
    (33, 20, 2, 3, 128, 1, False),
]


def case_id(c):
    return "-".join(str(int(v)) for v in c)


def out_offset(i, co, b, B, groups, CO, P):
    """include/hdn_hip.h: element offset of the first pixel of output channel `co` of level `i`, image `b` in the one buffer
    [n][groups][B][CO / groups][P]."""
    cg = CO // groups
    return (((i * groups + co // cg) * B + b) * cg + co % cg) * P


def scatter_by_offset(ref, groups):
    """ref [n, B, CO, P] -> the flat buffer with every (level, image, channel) row written at out_offset."""
    n, B, CO, P = ref.shape
    flat = torch.full((n * B * CO * P,), float("nan"), dtype=ref.dtype)
    for i in range(n):
        for b in range(B):
            for co in range(CO):
                o = out_offset(i, co, b, B, groups, CO, P)
                flat[o:o + P] = ref[i, b, co]
    return flat


def conv_relu(x, w, b):
    """relu(conv3x3 / stride 1 / no padding + bias) in the dtype of its arguments."""
    return F.conv2d(x, w, b).relu()


def _codes(shape, k=0):
    """Integers in [0, 15] spread over the linear index of `shape` (int64), another sequence per k."""
    n = 1
    for s in shape:
        n *= s
    return ((((torch.arange(n, dtype=torch.int64) + 7919 * k) * 2654435761) % 4194301) % 16).reshape(shape)


def onehot(CO, level):
    """(w [CO, 256, 3, 3] with one 1.0 per output channel, src [CO], ky [CO], kx [CO]): input channel (5 co + 3 + 31 level) mod 256 and tap
    (co + 4 level) mod 9 - another code per level, so a wrong level pointer shows."""
    co = torch.arange(CO)
    src, tap = (5 * co + 3 + 31 * level) % 256, (co + 4 * level) % 9
    w = torch.zeros(CO, 256, 3, 3)
    w[co, src, tap // 3, tap % 3] = 1.0
    return w, src, tap // 3, tap % 3


def exact_case(Hi, Wi, n, B, CO):
    """xs: n int64 [B, 256, Hi, Wi] in [0, 15]; ws: n one-hot [CO, 256, 3, 3]; bs: int64 [n, CO] in [-10, 10];
    want: int64 [n, B, CO, Ho, Wo] = relu(x_l[b, src(co), y + ky(co), x + kx(co)] + b_l[co]), by indexing."""
    Ho, Wo = Hi - 2, Wi - 2
    xs, ws, bs, want = [], [], [], []
    for l in range(n):
        x = _codes((B, 256, Hi, Wi), k=l)
        w, src, ky, kx = onehot(CO, l)
        b = (torch.arange(CO, dtype=torch.int64) * 37 + 53 * l) % 21 - 10
        o = torch.empty(B, CO, Ho, Wo, dtype=torch.int64)
        for co in range(CO):
            y0, x0 = int(ky[co]), int(kx[co])
            o[:, co] = x[:, int(src[co]), y0:y0 + Ho, x0:x0 + Wo]
        xs.append(x)
        ws.append(w)
        bs.append(b)
        want.append(torch.relu(o + b.view(1, CO, 1, 1)))
    return xs, ws, torch.stack(bs), torch.stack(want)


def first_difference(got, want, names="(level, image, channel, y, x)"):
    """None if torch.equal, else a message naming the first wrong element."""
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)}, wanted {tuple(want.shape)}"
    if torch.equal(got, want):
        return None
    bad = (got != want).nonzero()
    i = tuple(bad[0].tolist())
    return f"{bad.shape[0]} of {got.numel()} outputs differ; first {names} = {i}: got {float(got[i])!r}, want {float(want[i])!r}"


def random_case(Hi, Wi, n, B, CO, seed):
    """test_head_conv_search_one_launch_vs_float64's data at batch B: post-ReLU inputs x 2, weights x 0.03, random bias."""
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(B, 256, Hi, Wi, generator=g).relu_() * 2.0 for _ in range(n)]
    ws = [torch.randn(CO, 256, 3, 3, generator=g) * 0.03 for _ in range(n)]
    bs = [torch.randn(CO, generator=g) for _ in range(n)]
    return xs, ws, bs


def seeded_head(cls_name, seed=3):
    """hdn_amd.heads.MultiBAN / MultiCircBAN([256] * 3, 2, weighted=True) in eval mode with non-trivial BatchNorm running statistics, affine
    weights, level weights and loc_scale."""
    from hdn_amd import heads
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    m = getattr(heads, cls_name)([256] * 3, 2, weighted=True).eval()
    u = lambda n, lo, hi: torch.rand(n, generator=g) * (hi - lo) + lo
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            n = mod.num_features
            mod.weight.data, mod.bias.data = u(n, 0.5, 1.5), u(n, -0.3, 0.3)
            mod.running_mean.copy_(u(n, -0.5, 0.5))
            mod.running_var.copy_(u(n, 0.5, 2.0))
    m.cls_weight.data, m.loc_weight.data, m.loc_scale.data = torch.randn(3, generator=g), torch.randn(3, generator=g), u(3, 0.5, 1.5)
    return m


def head_inputs(circular, B, seed):
    """(z_fs, x_fs): 3 x [B, 256, 7, 7] and 3 x [B, 256, 15, 15]; 9 x 9 both for the circular head."""
    g = torch.Generator().manual_seed(seed)
    zs, xs = (9, 9) if circular else (7, 15)
    return ([torch.randn(B, 256, zs, zs, generator=g) for _ in range(3)], [torch.randn(B, 256, xs, xs, generator=g) for _ in range(3)])


# ------------------------------------------------------------------------------------------------- the module-layout predicates' cases
def small_head(levels=1, hidden=32, cin=256):
    """A MultiBAN of `levels` levels with cin -> hidden branches (the constructor's own are cin -> cin), eval mode: the smallest the predicates accept."""
    from hdn_amd import heads
    torch.manual_seed(9)
    m = heads.MultiBAN([cin] * levels, 2, weighted=True)
    for i in range(levels):
        setattr(m, "box" + str(i + 2), heads.DepthwiseBAN(cin, hidden, 2))
    return m.eval()


def _reconv(stage, **kw):
    c = stage[0]
    stage[0] = torch.nn.Conv2d(c.in_channels, c.out_channels, 3, **{"bias": False, **kw})


def _weight(stage, v):
    stage[0].weight.data[3, 5, 1, 1] = v


# one mutation of box2.cls's 3x3 stage each (a Sequential(Conv2d, BatchNorm2d, ReLU))
STAGE_MUTATIONS = {
    "bias": lambda st: _reconv(st, bias=True),
    "stride2": lambda st: _reconv(st, stride=2),
    "padding1": lambda st: _reconv(st, padding=1),
    "dilation2": lambda st: _reconv(st, dilation=2),
    "groups2": lambda st: _reconv(st, groups=2),
    "bn_training": lambda st: st[1].train(),
    "bn_not_affine": lambda st: st.__setitem__(1, torch.nn.BatchNorm2d(st[1].num_features, affine=False).eval()),
    "bn_no_running_stats": lambda st: st.__setitem__(1, torch.nn.BatchNorm2d(st[1].num_features, track_running_stats=False).eval()),
    "identity": lambda st: st.__setitem__(2, torch.nn.Identity()),
    "length4": lambda st: st.append(torch.nn.Identity()),
    "weight7e4": lambda st: _weight(st, 7e4),
}
# ... and whole heads: (levels, hidden, input channels, input side per level; None: the caller's)
HEAD_VARIANTS = {
    "reference": (1, 32, 256, [None]),
    "hidden48": (1, 48, 256, [None]),
    "cin128": (1, 32, 128, [None]),
    "two_shapes": (2, 32, 256, [None, 9]),
    "five_levels": (5, 32, 256, [None] * 5),
    "side17": (1, 32, 256, [17]),
    "side50": (1, 32, 256, [50]),
}
STAGE_CASES = list(HEAD_VARIANTS) + list(STAGE_MUTATIONS)


def stage_case(name, side, B=1, S=5, dev="cpu"):
    """Case `name` applied to `side` (conv_kernel / conv_search) -> (head, its boxes, the levels' inputs [B, C, S, S] of zeros), on `dev`."""
    levels, hidden, cin, sides = HEAD_VARIANTS.get(name, HEAD_VARIANTS["reference"])
    m = small_head(levels, hidden, cin)
    if name in STAGE_MUTATIONS:
        STAGE_MUTATIONS[name](getattr(m.box2.cls, side))
    m = m.to(dev)
    return m, [getattr(m, "box" + str(i + 2)) for i in range(levels)], [torch.zeros(B, cin, s or S, s or S, device=dev) for s in sides]
