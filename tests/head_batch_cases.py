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
