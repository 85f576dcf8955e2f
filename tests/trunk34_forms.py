"""Shared by tests/test_gpu_trunk34_forms.py and tests/test_trunk34_forms_host.py: the batch lists that reach every launch form of the ResNet-34
trunk's 3x3 kernels (csrc/conv3x3.hip, csrc/conv3x3s2.hip), the host queries that prove it, and the integer-indexed expectations of the exact
addressing tests.  Nothing here launches a kernel; the expectations are plain torch on int64 and are checked against float64 convolutions by the
host test, independently of any kernel."""
import torch
import torch.nn.functional as F

from test_gpu_trunk50_forms import _codes

# ----------------------------------------------------------------------------------------------------------------- the cases
# (S, C) -> the FIRST batch of every K-slice form (k_slices<Cf>(B), 200 workgroups; csrc/conv3x3.hip) and the z of that form.  Where a tile holds
# several images ((4, 512): 8, (4, 256) stride 2: 4) every batch is = 1 modulo that count: the last tile holds one image.
S1_CASES = {(32, 64): [1, 13, 25, 32, 50], (16, 128): [1, 13, 25, 50], (8, 256): [1, 13, 25, 50], (4, 512): [1, 9, 25, 49, 97, 193]}
S1_FORMS = {(32, 64): [4, 2, 1, 2, 1], (16, 128): [8, 4, 2, 1], (8, 256): [8, 4, 2, 1], (4, 512): [32, 16, 8, 4, 2, 1]}
S1_EXTRA = {(32, 64): [31]}                     # the last batch of CV_L1 (128-pixel tiles) beside 32, the first of CV_L1B (256-pixel tiles)
S1_TILE_IMAGES = {(4, 512): 8}
# hdn_conv3x3s2_ds_f32, (S, CI): output side and INPUT channels (2 CI out)
S2_CASES = {(16, 64): [1, 13, 25], (8, 128): [1, 13, 25, 50], (4, 256): [1, 13, 25, 49, 97]}
S2_FORMS = {(16, 64): [4, 2, 1], (8, 128): [8, 4, 2, 1], (4, 256): [16, 8, 4, 2, 1]}
S2_TILE_IMAGES = {(4, 256): 4}
QUERY_MAX = 260                                 # the queries are walked over 1 .. QUERY_MAX: past the last switch of every shape (193)
# hdn_conv3x3_v2_f32 (B >= V2_MIN_BATCH = 24): 24, every switch of k_slices_v2 up to 64, and 64
V2_CASES = {(32, 64): [24], (16, 128): [24], (8, 256): [24, 50], (4, 512): [24, 25, 49]}
V2_FORMS = {(32, 64): [1], (16, 128): [1], (8, 256): [2, 1], (4, 512): [4, 2, 1]}
V2_EXTRA = {(32, 64): [25, 64], (16, 128): [25, 64], (8, 256): [25, 64], (4, 512): [64]}
V2_MAX = 64
# hdn_conv3x3s2_v2_f32 takes no workspace and has one form per shape: both sides of nothing, so 24, 25 (a last tile of one image at (4, 256)) and 64
S2V2_CASES = {(16, 64): [24, 25, 64], (8, 128): [24, 25, 64], (4, 256): [24, 25, 64]}
# the chained form (hdn_conv3x3_chain_f32, B <= CHAIN_MAX_BATCH = 16): one batch per distinct hdn_conv3x3_chain_slices
CHAIN1_CASES = {(32, 64): [1, 13], (16, 128): [1, 13], (8, 256): [1, 13], (4, 512): [1, 9]}
CHAIN1_FORMS = {(32, 64): [4, 2], (16, 128): [8, 4], (8, 256): [8, 4], (4, 512): [32, 16]}
CHAIN2_CASES = {(16, 64): [1, 13], (8, 128): [1, 13], (4, 256): [1, 13]}
CHAIN2_FORMS = {(16, 64): [4, 2], (8, 128): [8, 4], (4, 256): [16, 8]}
CHAIN_MAX = 16
CHAIN_SAME_SPLIT_UP_TO = 12                     # the chained and the unchained form split K alike at least up to here (bit-identity is asserted)


def flat(cases, extra=None):
    return [(S, C, B) for (S, C), bs in cases.items() for B in sorted(bs + (extra or {}).get((S, C), []))]


def _lib():
    from hdn_amd import _lib as L
    return L.load()


def _z(n, per, what):
    assert n >= 0 and n % per == 0, (what, n, per)
    return max(1, n // per)                     # no workspace: one slice, the fused epilogue


def z_s1(B, S, C):
    return _z(_lib().hdn_conv3x3_workspace_bytes(B, S, C, 1), B * S * S * C * 4, ("conv3x3", B, S, C))


def z_s2(B, S, CI):
    return _z(_lib().hdn_conv3x3_workspace_bytes(B, S, CI, 2), 2 * B * S * S * 2 * CI * 4, ("conv3x3s2_ds", B, S, CI))   # both outputs


def z_v2(B, S, C):
    return _z(_lib().hdn_conv3x3_v2_workspace_bytes(B, S, C), B * S * S * C * 4, ("conv3x3_v2", B, S, C))


def z_chain(B, S, CI, stride):
    z = _lib().hdn_conv3x3_chain_slices(B, S, CI, stride)
    assert z > 0, (z, B, S, CI, stride)
    return z


def runs(zf, lo, hi):
    """[(first batch, z)] of every run of equal z over lo .. hi."""
    out = []
    for B in range(lo, hi + 1):
        z = zf(B)
        if not out or out[-1][1] != z:
            out.append((B, z))
    return out


def check_coverage(name, cases, forms, zf, lo, hi, extra=None, tile_images=None):
    """The runs of equal z the query shows over lo .. hi are exactly (cases, forms): every form is reached, each listed batch is the first of its
    form, none lies between.  Prints one line per shape."""
    for (S, C), bs in cases.items():
        got = runs(lambda B: zf(B, S, C), lo, hi)
        ex = sorted((extra or {}).get((S, C), []))
        print(f"FORMS coverage {name} (S, C) = ({S}, {C}): " + ", ".join(f"B={B}: z={z}" for B, z in got)
              + ("; also run: " + ", ".join(f"B={B}: z={zf(B, S, C)}" for B in ex) if ex else ""))
        assert got == list(zip(bs, forms[(S, C)])), (f"{name} ({S}, {C}): the query shows the forms (first batch, z) = {got} over B = {lo}..{hi}, the cases are "
                                                     f"{list(zip(bs, forms[(S, C)]))}: re-pick the list (has the slice target moved?)")
        n = (tile_images or {}).get((S, C))
        if n:
            assert all(B % n == 1 for B in bs), (name, S, C, bs, n)


def check_stride1_coverage():
    check_coverage("conv3x3_bias_relu", S1_CASES, S1_FORMS, z_s1, 1, QUERY_MAX, S1_EXTRA, S1_TILE_IMAGES)
    assert z_s1(31, 32, 64) == 1 and z_s1(32, 32, 64) == 2                  # 31 | 32: CV_L1 fused | CV_L1B sliced
    check_coverage("conv3x3_v2", V2_CASES, V2_FORMS, z_v2, 24, V2_MAX, V2_EXTRA)


def check_stride2_coverage():
    check_coverage("conv3x3s2_ds", S2_CASES, S2_FORMS, z_s2, 1, QUERY_MAX, None, S2_TILE_IMAGES)


def check_chain_coverage():
    check_coverage("conv3x3_chain stride 1", CHAIN1_CASES, CHAIN1_FORMS, lambda B, S, C: z_chain(B, S, C, 1), 1, CHAIN_MAX)
    check_coverage("conv3x3_chain stride 2", CHAIN2_CASES, CHAIN2_FORMS, lambda B, S, C: z_chain(B, S, C, 2), 1, CHAIN_MAX)
    # the chained form splits K as the unchained one wherever the bit-identity tests say so
    for (S, C) in CHAIN1_CASES:
        assert all(z_chain(B, S, C, 1) == z_s1(B, S, C) for B in range(1, CHAIN_SAME_SPLIT_UP_TO + 1)), (S, C)
    for (S, CI) in CHAIN2_CASES:
        assert all(z_chain(B, S, CI, 2) == z_s2(B, S, CI) for B in range(1, CHAIN_SAME_SPLIT_UP_TO + 1)), (S, CI)


def check_all_coverage():
    check_stride1_coverage()
    check_stride2_coverage()
    check_chain_coverage()


# ----------------------------------------------------------------------------------------------------------------- integer expectations
def bias_int(C, k=0):
    """Integer bias |b| <= 100, another one per k."""
    return (torch.arange(C, dtype=torch.int64) * 37 + 53 * k) % 201 - 100


def onehot3x3(CO, CI, k=0):
    """(w [CO, CI, 3, 3] with one 1.0 per output channel, src [CO], tap [CO]): input channel (5 co + 3 + 31 k) mod CI, tap (co + 4 k) mod 9."""
    co = torch.arange(CO)
    src, tap = (5 * co + 3 + 31 * k) % CI, (co + 4 * k) % 9
    w = torch.zeros(CO, CI, 3, 3)
    w[co, src, tap // 3, tap % 3] = 1.0
    return w, src, tap


def onehot1x1(CO, CI):
    """The downsample branch: (w [CO, CI, 1, 1], src): input channel (7 co + 1) mod CI."""
    co = torch.arange(CO)
    src = (7 * co + 1) % CI
    w = torch.zeros(CO, CI, 1, 1)
    w[co, src, 0, 0] = 1.0
    return w, src


def pick3x3(xi, src, tap, stride=1, pad=1):
    """The raw convolution with onehot3x3 weights by indexing: xi int64 NHWC [B, H, W, CI] -> int64 NHWC [B, Ho, Wo, CO],
    out[b, oy, ox, co] = xi[b, stride oy + ky - pad, stride ox + kx - pad, src[co]] (zero outside), (ky, kx) = divmod(tap[co], 3)."""
    B, H, W, _ = xi.shape
    Ho, Wo = (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1
    xp = F.pad(xi, (0, 0, pad, pad, pad, pad))
    out = torch.empty(B, Ho, Wo, src.numel(), dtype=torch.int64)
    for t in range(9):
        ky, kx = divmod(t, 3)
        co = (tap == t).nonzero().flatten()
        out[..., co] = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :][..., src[co]]
    return out


def pick1x1s2(xi, src):
    return xi[:, ::2, ::2, :][..., src]


def nchw(t):
    """int64 NHWC -> float32 NCHW view (channels-last in memory)."""
    return t.float().permute(0, 3, 1, 2)


def first_difference(got, want):
    """None if torch.equal, else a message naming the first wrong (image, channel, y, x) of two NCHW tensors."""
    if got.shape == want.shape and torch.equal(got, want):
        return None
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)}, wanted {tuple(want.shape)}"
    bad = (got != want).nonzero()
    i = tuple(bad[0].tolist())
    return f"{bad.shape[0]} of {got.numel()} outputs differ; first (image, channel, y, x) = {i}: got {float(got[i])!r}, want {float(want[i])!r}"


# the trunk's first stage: conv 7x7 / 2 / 3 (2 -> 64 channels) + bias + ReLU + max pool 3 / 2 / 1
def stem_onehot():
    """(w [64, 2, 7, 7], ci, ky, kx): the one 1.0 of output channel co at (co mod 2, (co // 2) mod 7, (3 co + 1) mod 7)."""
    co = torch.arange(64)
    ci, ky, kx = co % 2, (co // 2) % 7, (3 * co + 1) % 7
    w = torch.zeros(64, 2, 7, 7)
    w[co, ci, ky, kx] = 1.0
    return w, ci, ky, kx


def stem_expected(xi, ci, ky, kx, bi):
    """xi int64 NCHW [B, 2, H, W] -> int64 NCHW [B, 64, Hp, Wp]: max_pool2d(3, 2, 1) of relu(xi[b, ci, 2 oy + ky - 3, 2 ox + kx - 3] + bias) on integers."""
    B, _, H, W = xi.shape
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = F.pad(xi, (3, 3, 3, 3))
    conv = torch.empty(B, 64, Hc, Wc, dtype=torch.int64)
    for co in range(64):
        y0, x0 = int(ky[co]), int(kx[co])
        conv[:, co] = xp[:, int(ci[co]), y0:y0 + 2 * (Hc - 1) + 1:2, x0:x0 + 2 * (Wc - 1) + 1:2]
    act = torch.relu(conv + bi.view(1, 64, 1, 1))
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    ap = F.pad(act, (1, 1, 1, 1), value=-(1 << 40))                  # the pool's padding never wins
    out = None
    for dy in range(3):
        for dx in range(3):
            v = ap[:, :, dy:dy + 2 * (Hp - 1) + 1:2, dx:dx + 2 * (Wp - 1) + 1:2]
            out = v if out is None else torch.maximum(out, v)
    return out


# hdn_head_conv3x3_f32: n levels of a 3x3 / no padding convolution of 256 channels + bias + ReLU
def head_conv_case(Hi, Wi, n, CO):
    """Per level its own codes, one-hot and bias -> (xs: n int64 [1, 256, Hi, Wi], ws: n [CO, 256, 3, 3], bs: int64 [n, CO],
    want: int64 [n, CO, Hi - 2, Wi - 2] = relu(x_l[src, y + ky, x + kx] + b_l[co]))."""
    xi = _codes((n, Hi, Wi, 256))
    xs, ws, bs, want = [], [], [], []
    for l in range(n):
        w, src, tap = onehot3x3(CO, 256, k=l)
        b = bias_int(CO, k=l)
        xs.append(xi[l].permute(2, 0, 1)[None].contiguous())
        ws.append(w)
        bs.append(b)
        want.append(torch.relu(pick3x3(xi[l:l + 1], src, tap, 1, 0) + b)[0].permute(2, 0, 1))
    return xs, ws, torch.stack(bs), torch.stack(want)


# hdn_head_tail_f32: hid[g] = relu(W1[g] . feats[g] + b1[g]), out[br] = bf[br] + Wf[br] . hid[br]
def head_tail_case(H, P, n, om):
    """feats int64 [2n, H, P] with |x| < 2^17; w1 [2n, H, H] one-hot per hidden row (column (5 h + 3 + 7 g) mod H) with an integer b1 [2n, H, 1];
    wf [2, om, n H] with 8 entries of +-1 per row, integer bf [2, om, 1]; want int64 [2, om, P].  Every partial sum of the second product is an
    integer below 8 (2^17 + 100) < 2^24: exact in fp32 in any order."""
    G = 2 * n
    feats = _codes((G, H, P), mod=262139, off=131069)
    h = torch.arange(H)
    w1 = torch.zeros(G, H, H)
    src = torch.stack([(5 * h + 3 + 7 * g) % H for g in range(G)])           # [G, H]
    for g in range(G):
        w1[g, h, src[g]] = 1.0
    b1 = torch.stack([(37 * h + 11 * g) % 201 - 100 for g in range(G)]).view(G, H, 1)
    hid = torch.relu(torch.gather(feats, 1, src.view(G, H, 1).expand(G, H, P)) + b1).view(2, n * H, P)
    wf = torch.zeros(2, om, n * H)
    bf = torch.empty(2, om, 1, dtype=torch.int64)
    want = torch.empty(2, om, P, dtype=torch.int64)
    for br in range(2):
        for o in range(om):
            cols = [(17 * o + 5 * br + 97 * k) % (n * H) for k in range(8)]
            assert len(set(cols)) == 8
            sign = [1 - 2 * ((k + o + br) % 2) for k in range(8)]
            bf[br, o, 0] = (7 * o + 3 * br) % 41 - 20
            acc = bf[br, o, 0].expand(P).clone()
            for c, s in zip(cols, sign):
                wf[br, o, c] = float(s)
                acc += s * hid[br, c]
            want[br, o] = acc
    assert int(feats.abs().max()) < 1 << 17
    return feats, w1, b1, wf, bf, want


# the chained form: conv -> lazy conv (want_x) -> finish.  Codes of |x| < 2^20, so that every activation that is split again stays below 2^22
def _codes20(shape):
    return _codes(shape, mod=2097143, off=1048571)


def chain1_case(B, S, C):
    """Two stride-1 convolutions, the first with a residual r, the second with the first's output as its residual (a BasicBlock's tail):
    a = relu(conv0(x) + b0 + r), out = relu(conv1(a) + b1 + a); int64 NHWC expectations raw0, a, raw1, out."""
    xi, ri = _codes20((B, S, S, C)), _codes((B, S, S, C), 40503, 2003, 1001)
    (w0, s0, t0), (w1, s1, t1) = onehot3x3(C, C), onehot3x3(C, C, k=1)
    b0, b1 = bias_int(C), bias_int(C, k=1)
    raw0 = pick3x3(xi, s0, t0)
    a = torch.relu(raw0 + b0 + ri)
    raw1 = pick3x3(a, s1, t1)
    out = torch.relu(raw1 + b1 + a)
    assert int(a.max()) < 1 << 22 and int(out.max()) < 1 << 22
    return dict(xi=xi, ri=ri, w=[w0, w1], b=[b0, b1], raw0=raw0, a=a, raw1=raw1, out=out)


def chain2_case(B, S, CI):
    """The first block of a stage behind a stride-1 convolution: a = relu(conv0(x) + b0 + r) at (2S, CI); y = relu(conv_s2(a) + b1) and the raw
    downsample branch d = a[::2, ::2, srcd] at (S, 2 CI); out = relu(conv2(y) + b2 + d); raw3 = conv3(out), the next block's first convolution."""
    CO = 2 * CI
    xi, ri = _codes20((B, 2 * S, 2 * S, CI)), _codes((B, 2 * S, 2 * S, CI), 40503, 2003, 1001)
    (w0, s0, t0), (w1, s1, t1), (w2, s2, t2), (w3, s3, t3) = onehot3x3(CI, CI), onehot3x3(CO, CI, k=1), onehot3x3(CO, CO, k=2), onehot3x3(CO, CO, k=3)
    wd, sd = onehot1x1(CO, CI)
    b0, b1, b2 = bias_int(CI), bias_int(CO, k=1), bias_int(CO, k=2)
    raw0 = pick3x3(xi, s0, t0)
    a = torch.relu(raw0 + b0 + ri)
    raw1, d = pick3x3(a, s1, t1, 2), pick1x1s2(a, sd)
    y = torch.relu(raw1 + b1)
    raw2 = pick3x3(y, s2, t2)
    out = torch.relu(raw2 + b2 + d)
    raw3 = pick3x3(out, s3, t3)
    assert max(int(a.max()), int(y.max()), int(out.max())) < 1 << 22
    return dict(xi=xi, ri=ri, w=[w0, w1, w2, w3], wd=wd, b=[b0, b1, b2], raw0=raw0, a=a, raw1=raw1, d=d, y=y, raw2=raw2, out=out, raw3=raw3)
