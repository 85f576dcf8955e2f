"""Shared by tests/test_gpu_buffer_discipline.py and tests/test_buffer_guard_host.py: which cases of the EXISTING case lists the buffer tests run per
entry point, the host queries that prove that they reach every launch form, and the two exact builders the family lacked (hdn_avgpool_fc_f32,
hdn_bias_relu_f32).  Nothing here launches a kernel."""
import functools

import torch
import torch.nn.functional as F

import conv3x3_train_cases as TC
import head_batch_cases as HB
import head_tail_batch_cases as HT
import simi_full_cases as SC
import test_gpu_conv3x3d as D
import test_gpu_trunk50_forms as T50
import trunk34_forms as T

# ----------------------------------------------------------------------------------------------------------------- the cases, all from existing lists
S1 = T.flat(T.S1_CASES, T.S1_EXTRA)              # hdn_conv3x3_bias_relu_f32 (S, C, B): the first batch of every K-split count and the unsplit form
V2 = T.flat(T.V2_CASES, T.V2_EXTRA)              # hdn_conv3x3_v2_f32: B = 24, 25 (a partial pixel tile), every switch of k_slices_v2, 64
S2DS = T.flat(T.S2_CASES)                        # hdn_conv3x3s2_ds_f32 (S, CI, B)
S2V2 = T.flat(T.S2V2_CASES)                      # hdn_conv3x3s2_v2_f32
CHAIN1 = T.flat(T.CHAIN1_CASES)                  # hdn_conv3x3_chain_f32 / hdn_conv3x3_finish_f32, stride 1
CHAIN2 = T.flat(T.CHAIN2_CASES)                  # ... the stride-2 block
C1X1 = list(T50.EXACT_1X1)                       # hdn_conv1x1_f32 (CI, CO, S, stride, B)
S2 = list(T50.S2_FLAT)                           # hdn_conv3x3s2_f32 (S, C, B)
DIL = list(D.CASES)                              # hdn_conv3x3d_f32 (B, S, CI, CO, dilation)
VALID = list(SC.V_ALL)                           # hdn_conv3x3v_f32 (B, S, CI, CO, stride)
DGRAD = [c for cs in TC.DGRAD_CASES.values() for c in cs]       # (B, S, CI, CO)
WGRAD = [c for cs in TC.WGRAD_CASES.values() for c in cs]
SIMI_STEM = [(B, S) for S in [7] + SC.STEM_TILING_SIZES for B in (1, 3)]
TRUNK_STEM = [1, 3]                              # hdn_trunk_stem_mfma_f32: B (H = W = 127 is the only size it takes)
HEAD_CONV = [(9, 14, 2, 64), (33, 20, 4, 96), (31, 31, 3, 512)]  # hdn_head_conv3x3_f32 (Hi, Wi, n, CO): test_gpu_trunk34_forms.py's, each nhwc 0 and 1
HEAD_CONV_BATCH = list(HB.CASES)                 # (Hi, Wi, n, B, CO, groups, nhwc)
HEAD_TAIL = [(128, 7, 2, 8), (256, 33, 1, 4), (256, 169, 3, 4)]  # hdn_head_tail_f32 (H, P, n, om): test_gpu_trunk34_forms.py's
HEAD_TAIL_BATCH = list(HT.CASES)                 # (H, P, n, oc, ol, B)
# hdn_bias_relu_f32 (B, C, HW, nhwc): the vector path (16-byte words: C % 4 == 0 channels-last, HW % 4 == 0 NCHW) and the scalar path in both layouts,
# each at one partial workgroup and at the smallest n that makes the grid-stride loop go round once (2048 x 256 words / 4096 x 256 floats)
BIAS_RELU = [(3, 8, 20, 1), (3, 5, 20, 0), (3, 6, 15, 1), (3, 5, 15, 0),
             (9, 64, 4096, 1), (9, 64, 4096, 0), (3, 6, 59049, 1), (3, 6, 59049, 0)]
BIAS_RELU_GRID = {True: 2048 * 256 * 4, False: 4096 * 256}      # vector?: elements one pass of the grid covers
# hdn_avgpool_fc_f32 (B, C, HW, O, nhwc): HW a power of two (the mean is exact); C below, at and above the 512 threads, no multiple of 512; HW no
# multiple of 16 and the trunk's 16; O = 1 and 16
AVGPOOL_FC = [(1, 512, 16, 8, 1), (3, 100, 8, 1, 0), (3, 100, 8, 16, 1), (2, 700, 4, 16, 0), (2, 700, 2, 1, 1), (5, 520, 1, 16, 1)]


def bias_relu_vector(B, C, HW, nhwc):
    """The path hdn_bias_relu_f32 takes for 16-byte aligned operands (csrc/epilogue.hip)."""
    return C % 4 == 0 if nhwc else HW % 4 == 0


# ----------------------------------------------------------------------------------------------------------------- the two new exact builders
def bias_relu_case(B, C, HW, nhwc):
    """(y, bias, residual, want with residual, want without) as int64 in memory order ([B, HW, C] channels-last, [B, C, HW] otherwise): |y| <= 1000,
    |bias| <= 100, |residual| <= 1001."""
    shape = (B, HW, C) if nhwc else (B, C, HW)
    y = T50._codes(shape, mod=2003, off=1001) + 1
    r = T50._codes(shape, 40503, 2003, 1001)
    b = T.bias_int(C)
    bb = b.view(1, 1, C) if nhwc else b.view(1, C, 1)
    return y, b, r, torch.relu(y + bb + r), torch.relu(y + bb)


def avgpool_fc_case(B, C, HW, O, nhwc):
    """(x in memory order, w [O, C], bias [O], want [B, O] float64): x in [-8, 8], w in [-3, 3], bias in [-9, 9], integers; HW a power of two, so
    every channel mean is a multiple of 1 / HW below 8 and every partial sum of the product a multiple of 1 / HW below 24 C: exact in fp32."""
    assert HW & (HW - 1) == 0 and 24 * C * HW < 1 << 24
    g = torch.Generator().manual_seed(11 * C + HW + O)
    x = torch.randint(-8, 9, (B, C, HW), generator=g)
    w = torch.randint(-3, 4, (O, C), generator=g)
    b = torch.randint(-9, 10, (O,), generator=g)
    sums = x.sum(2)                                                       # int64 [B, C]
    want = (sums @ w.t()).double() / HW + b.double()
    return (x.permute(0, 2, 1).contiguous() if nhwc else x), w, b, want


# ----------------------------------------------------------------------------------------------------------------- integer convolutions, float64 truth
def _randint_problem(seed, B, S, CI, CO):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (B, CI, S, S), generator=g)
    w = torch.randint(-2, 3, (CO, CI, 3, 3), generator=g)
    b = torch.randint(-9, 10, (CO,), generator=g)
    return x, w, b


@functools.lru_cache(maxsize=4)
def dilated_case(B, S, CI, CO, d):
    """The integer problem of test_gpu_conv3x3d.py::test_conv3x3d_addressing_is_exact at any case: (x, w, b int64, want float64 NCHW without ReLU)."""
    x, w, b = _randint_problem(5 + S, B, S, CI, CO)
    return x, w, b, F.conv2d(x.double(), w.double(), b.double(), 1, d, d)


@functools.lru_cache(maxsize=4)
def valid_case(B, S, CI, CO, stride):
    """simi_full_cases.v_integer_problem's data (same generator, same draws) with the truth by a float64 convolution, which is exact on these
    integers and fast at the large cases; the host test holds it against v_integer_problem's integer indexing."""
    x, w, b = _randint_problem(5 + S + CI, B, S, CI, CO)
    return x, w, b, F.conv2d(x.double(), w.double(), b.double(), stride)


@functools.lru_cache(maxsize=4)
def train_case(B, S, CI, CO):
    """conv3x3_train_cases.integer_problem's data with float64 truths: (x, w, dy int64; gx, gw float64).  Held against integer_problem by the host test."""
    g = torch.Generator().manual_seed(7 * S + CI + 3 * CO + B)
    x = torch.randint(-4, 5, (B, CI, S, S), generator=g)
    w = torch.randint(-2, 3, (CO, CI, 3, 3), generator=g)
    dy = torch.randint(-3, 4, (B, CO, S - 2, S - 2), generator=g)
    gx = F.conv_transpose2d(dy.double(), w.double())
    gw = F.conv2d(x.double().transpose(0, 1), dy.double().transpose(0, 1)).transpose(0, 1)
    return x, w, dy, gx, gw


def simi_stem_case(B, S):
    """simi_full_cases.stem_integer_problem; at S = 7 and 8 (a conv map of one pixel, which its index pooling does not take) the same draws with the
    truth by float64 conv2d / max_pool2d, exact on these integers.  The host test holds the two against each other at S = 11."""
    if SC.stem_sides(S)[0] >= 3:
        return SC.stem_integer_problem(B, S)
    return simi_stem_case_f64(B, S)


def simi_stem_case_f64(B, S):
    g = torch.Generator().manual_seed(77 + S)
    x = torch.randint(0, 256, (B, 3, S, S), generator=g)
    w = torch.randint(-1, 2, (64, 3, 7, 7), generator=torch.Generator().manual_seed(4))
    b = (torch.arange(64) * 37) % 201 - 100
    want = F.max_pool2d(torch.relu(F.conv2d(x.double(), w.double(), b.double(), 2)), 3, 2, 1)
    return x, w, b, want.to(torch.int64)


# ----------------------------------------------------------------------------------------------------------------- forms, by the library's own answer
def _lib():
    from hdn_amd import _lib as L
    return L.load()


def form_of(entry, case):
    """The launch form of a case as the library's queries name it (a string for the BUFFERS lines and the failure messages)."""
    if entry in ("hdn_conv3x3_bias_relu_f32",):
        S, C, B = case
        return f"z={T.z_s1(B, S, C)}"
    if entry == "hdn_conv3x3_v2_f32":
        S, C, B = case
        return f"z={T.z_v2(B, S, C)}"
    if entry == "hdn_conv3x3s2_ds_f32":
        S, CI, B = case
        return f"z={T.z_s2(B, S, CI)}"
    if entry == "hdn_conv3x3s2_v2_f32":
        return "v2"
    if entry == "hdn_conv3x3_chain_f32":
        S, CI, B, stride = case
        return f"z={T.z_chain(B, S, CI, stride)}"
    if entry == "hdn_conv1x1_f32":
        CI, CO, S, stride, B = case
        return T50.form_1x1(B, S, CI, CO, stride)
    if entry == "hdn_conv3x3s2_f32":
        S, C, B = case
        return T50.form_s2(B, S, C)
    if entry == "hdn_conv3x3d_f32":
        return D.form_name(*case)
    if entry == "hdn_conv3x3v_f32":
        return SC.v_form_name(_lib().hdn_conv3x3v_form(*case))
    if entry == "hdn_conv3x3v_dgrad_f32":
        return TC.dgrad_form_name(_lib().hdn_conv3x3v_dgrad_form(*case))
    if entry == "hdn_conv3x3v_wgrad_f32":
        return TC.wgrad_form_name(_lib().hdn_conv3x3v_wgrad_form(*case))
    raise KeyError(entry)


def check_coverage():
    """Every form of every entry point that has a *_form, *_slices, workspace or pack-info query is reached by the cases above (host queries only).
    Returns {entry point: sorted forms}."""
    T.check_all_coverage()                                               # S1 / V2 / S2DS / CHAIN1 / CHAIN2 are trunk34_forms' own lists, whole
    assert S1 == T.flat(T.S1_CASES, T.S1_EXTRA) and V2 == T.flat(T.V2_CASES, T.V2_EXTRA) and S2DS == T.flat(T.S2_CASES)
    assert CHAIN1 == T.flat(T.CHAIN1_CASES) and CHAIN2 == T.flat(T.CHAIN2_CASES)
    seen = {}
    seen["hdn_conv3x3_bias_relu_f32"] = {form_of("hdn_conv3x3_bias_relu_f32", c) for c in S1}
    assert seen["hdn_conv3x3_bias_relu_f32"] == {f"z={z}" for zs in T.S1_FORMS.values() for z in zs} and "z=1" in seen["hdn_conv3x3_bias_relu_f32"]
    seen["hdn_conv3x3_v2_f32"] = {form_of("hdn_conv3x3_v2_f32", c) for c in V2}
    assert seen["hdn_conv3x3_v2_f32"] == {"z=1", "z=2", "z=4"}           # the S = 4 workspace form included
    assert any(B == 24 for _, _, B in V2) and any((B * S * S) % 128 for S, _, B in V2)          # B = 24 and a partial pixel tile
    seen["hdn_conv3x3s2_ds_f32"] = {form_of("hdn_conv3x3s2_ds_f32", c) for c in S2DS}
    assert seen["hdn_conv3x3s2_ds_f32"] == {f"z={z}" for zs in T.S2_FORMS.values() for z in zs}
    seen["hdn_conv3x3_chain_f32"] = ({form_of("hdn_conv3x3_chain_f32", c + (1,)) for c in CHAIN1}
                                     | {form_of("hdn_conv3x3_chain_f32", c + (2,)) for c in CHAIN2})
    assert seen["hdn_conv3x3_chain_f32"] == {f"z={z}" for zs in list(T.CHAIN1_FORMS.values()) + list(T.CHAIN2_FORMS.values()) for z in zs}
    seen["hdn_conv1x1_f32"] = {form_of("hdn_conv1x1_f32", c) for c in C1X1}
    assert seen["hdn_conv1x1_f32"] == T50.ALL_1X1_FORMS
    assert any(stride == 2 and S % 2 for _, _, S, stride, _ in C1X1) and any(B * ((S - 1) // stride + 1) ** 2 == 16 for _, _, S, stride, B in C1X1)
    for (S, C), want in T50.S2_FORMS.items():
        assert list(dict.fromkeys(T50.form_s2(B, S, C) for B in T50.S2_CASES[(S, C)])) == want, (S, C)
    seen["hdn_conv3x3s2_f32"] = {form_of("hdn_conv3x3s2_f32", c) for c in S2}
    seen["hdn_conv3x3d_f32"] = {form_of("hdn_conv3x3d_f32", c) for c in DIL}
    assert seen["hdn_conv3x3d_f32"] == D.ALL_FORMS and any(S <= d for _, S, _, _, d in DIL)
    seen["hdn_conv3x3v_f32"] = {form_of("hdn_conv3x3v_f32", c) for c in VALID}
    assert seen["hdn_conv3x3v_f32"] == set(SC.V_CASES) == D.ALL_FORMS
    for name, cs in SC.V_CASES.items():
        assert all(form_of("hdn_conv3x3v_f32", c) == name for c in cs), name
    assert any(stride == 2 and S % 2 == 0 for _, S, _, _, stride in VALID) and any(stride == 1 for *_, stride in VALID)
    for entry, table, cases in (("hdn_conv3x3v_dgrad_f32", TC.DGRAD_CASES, DGRAD), ("hdn_conv3x3v_wgrad_f32", TC.WGRAD_CASES, WGRAD)):
        for name, cs in table.items():
            assert all(form_of(entry, c) == name for c in cs), (entry, name)
        seen[entry] = {form_of(entry, c) for c in cases}
        assert seen[entry] == set(table), entry
    assert set(TC.DGRAD_CASES) == D.ALL_FORMS and set(TC.WGRAD_CASES) == {f"W{w}{s}" for w in (1, 2, 4) for s in ("", " split")}
    assert any(B % 8 for B, *_ in WGRAD)
    # no query, but a path rule of their own
    for c in BIAS_RELU:
        n = c[0] * c[1] * c[2]
        assert n % 256 or n > BIAS_RELU_GRID[bias_relu_vector(*c)], c
    paths = {(bias_relu_vector(*c), c[3], c[0] * c[1] * c[2] > BIAS_RELU_GRID[bias_relu_vector(*c)]) for c in BIAS_RELU}
    assert len(paths) == 8, paths                                        # (vector | scalar) x (NCHW | channels-last) x (one pass | the loop goes round)
    assert all(c[0] * c[1] * c[2] < 2 * BIAS_RELU_GRID[bias_relu_vector(*c)] for c in BIAS_RELU)       # the smallest that loops once
    assert all(C % 512 for _, C, *_ in AVGPOOL_FC[1:]) and any(HW % 16 for _, _, HW, _, _ in AVGPOOL_FC)
    assert {O for _, _, _, O, _ in AVGPOOL_FC} >= {1, 16} and {n for *_, n in AVGPOOL_FC} == {0, 1}
    assert {S for _, S in SIMI_STEM} == {7} | set(SC.STEM_TILING_SIZES) and {B for B, _ in SIMI_STEM} == {1, 3}
    assert {(g, bool(n)) for *_, g, n in HEAD_CONV_BATCH} == {(1, False), (1, True), (2, False), (2, True)}
    assert any(oc != ol for _, _, _, oc, ol, _ in HEAD_TAIL_BATCH) and any(P % 32 for _, P, *_ in HEAD_TAIL_BATCH) and any(P % 32 for _, P, _, _ in HEAD_TAIL)
    return {k: sorted(v) for k, v in seen.items()}
