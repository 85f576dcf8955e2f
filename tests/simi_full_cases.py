"""What tests/test_simi_full_host.py (CPU) and tests/test_gpu_conv3x3v.py / tests/test_gpu_simi_stem.py (GPU) share: the case lists of
hdn_conv3x3v_f32 and hdn_simi_stem_f32 and the integer problems of the exact tests, with their expectations built by integer indexing.  The CPU file
checks every expectation against a float64 F.conv2d / F.max_pool2d, so the GPU tests' reference depends on no kernel."""
import torch

# ------------------------------------------------------------------------------------------------------------------ hdn_conv3x3v_f32
# (B, S, CI, CO, stride) by the form dispatch() of csrc/conv3x3d.hip gives them (FILL = 256 workgroups, 128-pixel tiles)
V_CASES = {
    "A split": [(2, 3, 32, 32, 2),                # So = 1
                (2, 5, 32, 96, 2),                # So = 2
                (3, 8, 96, 32, 2),                # So = 3, even S: the last input row and column are never read
                (3, 7, 96, 32, 1)],               # So = 5, stride 1
    "B split": [(1, 63, 128, 128, 2), (1, 31, 128, 128, 2), (1, 63, 256, 512, 2), (1, 31, 256, 512, 2),      # the workload: layer2.0 at both crops
                (3, 31, 128, 128, 2)],
    "A": [(3, 123, 32, 96, 2)],                   # M = 11,163: 88 x 3 workgroups
    "B": [(1, 127, 32, 512, 2)],                  # M = 3,969: 32 x 8
    "C": [(1, 127, 32, 1024, 2)],
}
V_ALL = [c for cs in V_CASES.values() for c in cs]
V_EXACT = [(2, 5, 32, 96, 2), (3, 8, 96, 32, 2), (1, 31, 128, 128, 2)]


def v_out_side(S, stride):
    """The entry point's own rule (include/hdn_hip.h)."""
    return (S - 3) // stride + 1


def v_form_name(v):
    """hdn_conv3x3v_form's value -> "A" / "B" / "C" (+ " split")."""
    assert v > 0, v
    cfg = (v & 15, (v >> 4) & 15, (v >> 8) & 15, (v >> 12) & 15)
    return {(1, 1, 4, 1): "A", (1, 2, 4, 1): "B", (2, 2, 2, 2): "C"}[cfg] + (" split" if (v >> 16) > 1 else "")


def v_integer_problem(B, S, CI, CO, stride):
    """(x, w, bias, want) as int64: inputs in [-4, 4], weights in [-2, 2], bias in [-9, 9]; want[b, co, oy, ox] by integer indexing of the nine
    strided views x[:, :, ky + s oy, kx + s ox] (no convolution routine)."""
    g = torch.Generator().manual_seed(5 + S + CI)
    x = torch.randint(-4, 5, (B, CI, S, S), generator=g)
    w = torch.randint(-2, 3, (CO, CI, 3, 3), generator=g)
    b = torch.randint(-9, 10, (CO,), generator=g)
    So = v_out_side(S, stride)
    want = b.view(1, CO, 1, 1).expand(B, CO, So, So).clone()
    for ky in range(3):
        for kx in range(3):
            win = x[:, :, ky:ky + stride * (So - 1) + 1:stride, kx:kx + stride * (So - 1) + 1:stride]           # [B, CI, So, So]
            want += torch.einsum("bcyx,oc->boyx", win, w[:, :, ky, kx])
    return x, w, b, want


# ------------------------------------------------------------------------------------------------------------------ hdn_simi_stem_f32
# S -> (Sc, Sp).  A workgroup is one pooled row (no row tiling); its four waves are the 32-wide tiles of "conv column + 1", so the column tiling
# switches where Sc passes 32 / 64 / 96: S = 68 | 69 (Sc 31 | 32), 132 | 133 (63 | 64), 196 | 197 (95 | 96).
STEM_SIZES = [7, 8, 9, 11, 13, 68, 69, 127, 132, 133, 196, 197, 255]
STEM_TILING_SIZES = [68, 69, 132, 133, 196, 197]
STEM_EXACT_SIZES = [11, 13, 127] + STEM_TILING_SIZES
STEM_MAX_SIDE = 255


def stem_sides(S):
    Sc = (S - 7) // 2 + 1
    return Sc, (Sc - 1) // 2 + 1


def stem_pool_int(conv):
    """maxpool 3 / 2 / 1 of relu(conv) for an int64 [B, C, Sc, Sc] map, by integer indexing (a padded position is skipped: everything is >= 0)."""
    B, C, Sc, _ = conv.shape
    Sp = (Sc - 1) // 2 + 1
    r = conv.clamp_min(0)
    out = torch.zeros(B, C, Sp, Sp, dtype=torch.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ys = [2 * p + dy for p in range(Sp)]
            xs = [2 * p + dx for p in range(Sp)]
            yi = [p for p, y in enumerate(ys) if 0 <= y < Sc]
            xi = [p for p, x in enumerate(xs) if 0 <= x < Sc]
            sub = r[:, :, [ys[p] for p in yi]][:, :, :, [xs[p] for p in xi]]
            cur = out[:, :, yi[0]:yi[-1] + 1, xi[0]:xi[-1] + 1]
            out[:, :, yi[0]:yi[-1] + 1, xi[0]:xi[-1] + 1] = torch.maximum(cur, sub)
    return out


def stem_integer_problem(B, S):
    """(x, w, bias, want) as int64: pixels 0..255, weights in {-1, 0, 1} with a pattern that differs per (co, ci, ky, kx) (no two channels and no two taps alike),
    integer bias; every partial sum stays below 147 x 255 < 2^24.  want by integer indexing of the 147 strided views."""
    g = torch.Generator().manual_seed(77 + S)
    x = torch.randint(0, 256, (B, 3, S, S), generator=g)
    w = torch.randint(-1, 2, (64, 3, 7, 7), generator=torch.Generator().manual_seed(4))       # (seeded: no period in any index; the CPU test checks it)
    b = (torch.arange(64) * 37) % 201 - 100
    Sc, _ = stem_sides(S)
    conv = b.view(1, 64, 1, 1).expand(B, 64, Sc, Sc).clone()
    for c in range(3):
        for y in range(7):
            for xx in range(7):
                win = x[:, c, y:y + 2 * (Sc - 1) + 1:2, xx:xx + 2 * (Sc - 1) + 1:2]                               # [B, Sc, Sc]
                conv += win.unsqueeze(1) * w[:, c, y, xx].view(1, 64, 1, 1)
    return x, w, b, stem_pool_int(conv)


def stem_tap_problem(S=13):
    """All 147 taps in one loop of three launches: one image whose pixel value names its position, x[ci, y, x] = 1 + (ci S + y) S + x, and in launch l
    output channel co carries the single weight 1 at tap t = 64 l + co = (ci 7 + ky) 7 + kx (the channels past tap 146 of the last launch stay zero).
    Returns (x [1,3,S,S], [w_l] x 3, [want_l] x 3), int64:
    conv output (oy, ox) of tap (ci, ky, kx) is x[ci, 2 oy + ky, 2 ox + kx]; the code grows with y and x, so the pool's maximum is the window's last
    in-range conv position: want[p, q] = x[ci, 2 min(2p + 1, Sc - 1) + ky, 2 min(2q + 1, Sc - 1) + kx]."""
    Sc, Sp = stem_sides(S)
    x = (1 + torch.arange(3 * S * S)).view(1, 3, S, S)
    ws, wants = [], []
    for l in range(3):
        w = torch.zeros(64, 3, 7, 7, dtype=torch.int64)
        want = torch.zeros(1, 64, Sp, Sp, dtype=torch.int64)
        for co in range(64):
            t = 64 * l + co
            if t >= 147:
                break
            ci, ky, kx = t // 49, (t // 7) % 7, t % 7
            w[co, ci, ky, kx] = 1
            for p in range(Sp):
                for q in range(Sp):
                    want[0, co, p, q] = x[0, ci, 2 * min(2 * p + 1, Sc - 1) + ky, 2 * min(2 * q + 1, Sc - 1) + kx]
        ws.append(w)
        wants.append(want)
    return x, ws, wants


def stem_reached(S, y0, x0):
    """[Sp, Sp] bool: the pooled outputs whose 3x3 pool window covers a conv output whose 7x7 / stride-2 window covers input pixel (y0, x0)."""
    Sc, Sp = stem_sides(S)
    hit = torch.zeros(Sp, Sp, dtype=torch.bool)
    for oy in range(Sc):
        for ox in range(Sc):
            if 2 * oy <= y0 <= 2 * oy + 6 and 2 * ox <= x0 <= 2 * ox + 6:
                for p in range(Sp):
                    for q in range(Sp):
                        if abs(2 * p - oy) <= 1 and abs(2 * q - ox) <= 1:
                            hit[p, q] = True
    return hit
