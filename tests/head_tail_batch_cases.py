"""Shared by tests/test_head_tail_batch_host.py and tests/test_gpu_head_tail_batch.py: the shapes that reach every tile and edge situation of
hdn_head_tail_batch_f32 (csrc/head_tail.hip), its documented output offset as a Python function, the integer expectation of the exact addressing test,
random data as in test_head_tail_one_launch_vs_float64 and the two products in the dtype of their arguments.  Nothing here launches a kernel."""
import torch

E_NULL, E_SHAPE, E_LIMIT, E_ALIAS = -1, -2, -3, -4

# (H, P, n, oc, ol, B): a workgroup owns 32 pixels of one (image, branch) and walks over the n levels
CASES = [
    (256, 169, 3, 2, 4, 3),           # the log-polar head: 5 full tiles + 9 pixels, oc != ol, odd batch
    (256, 25, 3, 2, 2, 2),            # one partial tile
    (128, 32, 1, 2, 2, 5),            # exactly one tile, one level, H = 128
    (128, 33, 4, 8, 1, 2),            # four levels, 8 rows, one pixel in the second tile
    (256, 64, 2, 1, 8, 1),            # B = 1 through the batched entry
    (256, 625, 3, 2, 2, 2),           # 25 x 25, 20 tiles
    (256, 961, 3, 2, 2, 2),           # 31 x 31
]


def case_id(c):
    return "-".join(str(int(v)) for v in c)


def out_offset(br, b, o, B, oc, ol, P):
    """include/hdn_hip.h: element offset of the first pixel of row `o` of branch `br` (0 cls, 1 loc), image `b` in the one buffer
    [B][oc][P] ++ [B][ol][P]."""
    return (br * B * oc + b * (ol if br else oc) + o) * P


def scatter_by_offset(ref, oc, ol):
    """ref [B, 2, om, P] -> the flat buffer of B (oc + ol) P elements with every written row (o < n_out[br]) at out_offset."""
    B, _, _, P = ref.shape
    flat = torch.full((B * (oc + ol) * P,), float("nan"), dtype=ref.dtype)
    for br, rows in enumerate((oc, ol)):
        for b in range(B):
            for o in range(rows):
                at = out_offset(br, b, o, B, oc, ol, P)
                flat[at:at + P] = ref[b, br, o]
    return flat


def split_views(flat, B, oc, ol, P):
    """The flat buffer -> (cls [B, oc, P], loc [B, ol, P]) as the documentation says it is laid out."""
    return flat[:B * oc * P].view(B, oc, P), flat[B * oc * P:].view(B, ol, P)


def tail(feats, w1, b1, wf, bf):
    """The two products in the dtype of the arguments: feats [2n, B, H, P], w1 [2n, H, H], b1 [2n, H, 1], wf [2, om, n H], bf [2, om, 1]
    -> [B, 2, om, P] (rows o >= n_out[br] are whatever wf / bf hold there)."""
    G, B, H, P = feats.shape
    out = []
    for b in range(B):
        hid = torch.baddbmm(b1, w1, feats[:, b]).relu()
        out.append(torch.baddbmm(bf, wf, hid.view(2, (G // 2) * H, P)))
    return torch.stack(out)


def _codes(shape, mod=262139, off=131069):
    """Integers in [-off, mod - off) spread over the linear index of `shape` (int64): another value per image, group, channel and pixel."""
    n = 1
    for s in shape:
        n *= s
    return (((torch.arange(n, dtype=torch.int64) * 2654435761) % 4194301) % mod - off).reshape(shape)


def exact_case(H, P, n, oc, ol, B):
    """feats int64 [2n, B, H, P] with |x| < 2^17 (other codes per image, group and level); w1 [2n, H, H] one-hot per hidden row (column
    (5 h + 3 + 7 g) mod H: another column per group, so a wrong group pointer shows) with an integer b1 [2n, H, 1]; wf [2, om, n H] with 8 entries
    of +-1 per written row and zero rows above n_out[br]; integer bf [2, om, 1]; want = (cls int64 [B, oc, P], loc int64 [B, ol, P]).  Every
    partial sum of the second product is an integer below 8 (2^17 + 100) + 20 < 2^24: exact in fp32 in any order."""
    G, om = 2 * n, max(oc, ol)
    feats = _codes((G, B, H, P))
    h = torch.arange(H)
    w1 = torch.zeros(G, H, H)
    src = torch.stack([(5 * h + 3 + 7 * g) % H for g in range(G)])           # [G, H]
    for g in range(G):
        w1[g, h, src[g]] = 1.0
    b1 = torch.stack([(37 * h + 11 * g) % 201 - 100 for g in range(G)]).view(G, H, 1)
    hid = torch.relu(torch.gather(feats, 2, src.view(G, 1, H, 1).expand(G, B, H, P)) + b1.view(G, 1, H, 1))      # [G, B, H, P]
    hid = hid.view(2, n, B, H, P).permute(0, 2, 1, 3, 4).reshape(2, B, n * H, P)                                  # [branch, image, level x channel, pixel]
    wf = torch.zeros(2, om, n * H)
    bf = torch.zeros(2, om, 1, dtype=torch.int64)
    want = [torch.empty(B, oc, P, dtype=torch.int64), torch.empty(B, ol, P, dtype=torch.int64)]
    for br, rows in enumerate((oc, ol)):
        for o in range(rows):
            cols = [(17 * o + 5 * br + 97 * k) % (n * H) for k in range(8)]
            assert len(set(cols)) == 8
            bf[br, o, 0] = (7 * o + 3 * br) % 41 - 20
            acc = bf[br, o, 0].expand(B, P).clone()
            for k, c in enumerate(cols):
                s = 1 - 2 * ((k + o + br) % 2)
                wf[br, o, c] = float(s)
                acc += s * hid[br, :, c]
            want[br][:, o] = acc
    assert int(feats.abs().max()) < 1 << 17
    return feats, w1, b1, wf, bf, want


def random_case(H, P, n, oc, ol, B, seed):
    """test_head_tail_one_launch_vs_float64's data at batch B: post-ReLU feats x 3, w1 x 0.06, wf x 0.05 with zero rows above n_out[br]."""
    g = torch.Generator().manual_seed(seed)
    om = max(oc, ol)
    feats = torch.randn(2 * n, B, H, P, generator=g).relu_() * 3.0
    w1 = torch.randn(2 * n, H, H, generator=g) * 0.06
    b1 = torch.randn(2 * n, H, 1, generator=g)
    wf = torch.randn(2, om, n * H, generator=g) * 0.05
    wf[0, oc:] = 0
    wf[1, ol:] = 0
    bf = torch.randn(2, om, 1, generator=g)
    return feats, w1, b1, wf, bf


def first_difference(got, want, names="(image, row, pixel)"):
    """None if torch.equal, else a message naming the first wrong element."""
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)}, wanted {tuple(want.shape)}"
    if torch.equal(got, want):
        return None
    bad = (got != want).nonzero()
    i = tuple(bad[0].tolist())
    return f"{bad.shape[0]} of {got.numel()} outputs differ; first {names} = {i}: got {float(got[i])!r}, want {float(want[i])!r}"
