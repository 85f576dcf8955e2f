"""Host side of tests/test_gpu_trunk_stem.py: everything the GPU tests of the trunk's first stage rely on, proven without a device.  The form rule
restated in tests/trunk_stem_cases.py stands in the sources and the case lists reach every form, width, strip tail and lane it names; the one-hot sets
meet all 98 taps in every 16-channel block and 32-channel tile; every integer expectation equals float64 conv2d / relu / max_pool2d; the exact
fixtures stay below 2^24; and the fixtures reject four wrong kernels, stated on the lane arithmetic (lane_model): a tap one column off, the `sh`
select removed, the pool's right neighbour taken from the left, the re-read row 0 multiplied instead of selected."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import trunk34_forms as T
import trunk_stem_cases as SC


def _same(want_int, ref64):
    assert want_int.dtype == torch.int64 and ref64.dtype == torch.float64 and tuple(want_int.shape) == tuple(ref64.shape)
    assert int(want_int.abs().max()) < 1 << 53
    assert torch.equal(want_int.double(), ref64), T.first_difference(want_int.double(), ref64)


# ------------------------------------------------------------------------------------------------------------------------ the form rule
def test_restated_form_rule_stands_in_the_sources():
    for name, text in SC.SOURCE_FACTS:
        assert text in SC.source(name), (name, text)
    assert SC.dims(127, 127) == (64, 64, 32, 32) and SC.dims(1, 2) == (1, 1, 1, 1) and SC.dims(9, 13) == (5, 7, 3, 4) and SC.dims(128, 128)[1] == 64
    assert not SC.in_range(1, 5, 1) and not SC.in_range(1, 5, 129) and not SC.in_range(65536, 5, 8) and SC.in_range(65535, 1, 128)
    # the tracker's calls: 1-row strips below 32 images at 127 px, 4-row strips from there on
    assert SC.strip_rows(31, 127, 127) == 1 and SC.strip_rows(32, 127, 127) == 4
    assert [SC.mfma_rows(B) for B in (1, 7, 8, 47, 48, 64)] == [4, 4, 8, 8, 16, 16]
    assert [SC.min_batch_of_4row_form(H, 8) for H in (1, 13, 17, 29, 33)] == [256, 256, 128, 128, 86]


def test_case_lists_reach_every_form_width_and_strip_tail():
    every = SC.ALL_WIDTHS + SC.HEIGHTS + SC.STRIP_CASES + SC.OFFSET_WIDTHS + SC.ONEHOT_WIDTHS + SC.ONEHOT_STRIP4 + SC.NONFINITE_SHAPES + SC.RANDOM_SHAPES
    assert all(SC.in_range(*c) for c in every) and set(SC.LAYOUTS) == {False, True}
    # all widths, in the 1-row form, at an odd and an even conv height; every odd W has its sh lane, W = 127 and 128 end in lane 63
    for H in (5, 6):
        ws = [W for B, h, W in SC.ALL_WIDTHS if h == H and SC.strip_rows(B, h, W) == 1]
        assert ws == list(range(2, 129))
    assert SC.dims(5, 2)[0] % 2 == 1 and SC.dims(6, 2)[0] % 2 == 1 and SC.dims(5, 2)[2] == SC.dims(6, 2)[2] == 2
    assert {SC.sh_lane(W) for _, _, W in SC.ALL_WIDTHS if W % 2} == set(range(1, 64)) and SC.sh_lane(127) == 63 and SC.sh_lane(128) is None
    assert SC.dims(5, 127)[1] == SC.dims(5, 128)[1] == 64 and SC.dims(5, 126)[1] == 63
    # heights 1 .. 26 at both widths: every residue of H mod 4 (the parity of Hc and of the last conv row's pooled row), Hc and Hp odd and even
    for W in (7, 64):
        hs = [H for _, H, w in SC.HEIGHTS if w == W]
        assert hs == list(range(1, 27)) and all(SC.strip_rows(2, H, W) == 1 for H in hs)
        assert {SC.dims(H, W)[0] % 2 for H in hs} == {0, 1} and {SC.dims(H, W)[2] for H in hs} == set(range(1, 8))
    # 4-row strips: every Hp mod 4, one / two / three strips, each at the first batch of the form and one image below it
    assert {SC.dims(H, W)[2] % 4 for _, H, W in SC.STRIP4} == {0, 1, 2, 3}
    assert {SC.strips(B, H, W) for B, H, W in SC.STRIP4} == {1, 2, 3}
    for B, H, W in SC.STRIP4:
        assert B == SC.min_batch_of_4row_form(H, W) and SC.strip_rows(B, H, W) == 4 and SC.strip_rows(B - 1, H, W) == 1, (B, H, W)
        assert (B, H, W) in SC.STRIP_CASES and (B - 1, H, W) in SC.STRIP_CASES
    assert {W for _, _, W in SC.STRIP4} >= {2, 3, 127, 128} and any(W % 2 for _, _, W in SC.STRIP4) and any(W % 2 == 0 for _, _, W in SC.STRIP4)
    # offsets: every residue of x and of out in a 16-byte line, on the strip list and on the edge widths
    assert {xo for xo, _ in SC.OFFSETS} == {oo for _, oo in SC.OFFSETS} == {0, 1, 2, 3} and len(SC.OFFSETS) == 16
    assert set(SC.STRIP_OFFSETS) <= set(SC.OFFSETS) and {xo for xo, _ in SC.STRIP_OFFSETS} == {oo for _, oo in SC.STRIP_OFFSETS} == {0, 1, 2, 3}
    assert [W for _, _, W in SC.OFFSET_WIDTHS] == [2, 3, 127, 128] and all(SC.strip_rows(*c) == 1 for c in SC.OFFSET_WIDTHS)
    # one-hot sets: the width edges in the 1-row form, two shapes in the 4-row form (one with two strips), the three matrix-core forms
    assert all(SC.strip_rows(*c) == 1 for c in SC.ONEHOT_WIDTHS) and all(SC.strip_rows(*c) == 4 for c in SC.ONEHOT_STRIP4)
    assert [W for _, _, W in SC.ONEHOT_WIDTHS] == [2, 3, 4, 5, 7, 8, 31, 32, 33, 63, 64, 65, 95, 96, 97, 125, 126, 127, 128]
    assert max(SC.strips(*c) for c in SC.ONEHOT_STRIP4) > 1
    assert [SC.mfma_rows(B) for B in SC.ONEHOT_MFMA_BATCHES] == [4, 8, 16]
    # the vector form at 127 px behind mfma_disabled: both strip forms
    assert {SC.strip_rows(B, 127, 127) for B in SC.ONEHOT_MFMA_BATCHES} == {1, 4}
    # non-finite pixels and random data: both strip forms
    assert {SC.strip_rows(*c) for c in SC.NONFINITE_SHAPES} == {1, 4} and {SC.strip_rows(*c) for c in SC.RANDOM_SHAPES} == {1, 4}
    assert all(SC.strips(*c) > 1 for c in SC.NONFINITE_SHAPES)


# ------------------------------------------------------------------------------------------------------------------------ one-hot sets
def test_onehot_sets_meet_every_tap_in_every_block_and_tile():
    taps = torch.stack([SC.onehot_tap(s) for s in range(SC.N_SETS)])                              # [7, 64]
    for cb in range(SC.CO // SC.CB):
        assert set(taps[:, cb * 16:(cb + 1) * 16].flatten().tolist()) == set(range(98)), cb        # the vector kernel's wave
    for tile in range(2):
        assert set(taps[:, tile * 32:(tile + 1) * 32].flatten().tolist()) == set(range(98)), tile  # the matrix-core kernel's channel half
    assert bool((taps[:, 0::2] != taps[:, 1::2]).all())                                            # a packed pair (2k, 2k + 1): two taps
    for s in range(SC.N_SETS):
        w, ci, ky, kx = SC.onehot_set(s)
        assert bool((w.flatten(1).sum(1) == 1).all()) and bool((w.flatten(1).abs().sum(1) == 1).all())
        assert torch.equal(w.flatten(1).argmax(1), taps[s]) and torch.equal(ci * 49 + ky * 7 + kx, taps[s])
    # the gap this closes: the one set of test_stem_addressing_is_exact meets 14 of the 98 taps, one kernel column per (input channel, kernel row)
    _, ci, ky, kx = T.stem_onehot()
    old = set(zip(ci.tolist(), ky.tolist(), kx.tolist()))
    assert len(old) == 14 and len({(c, y) for c, y, _ in old}) == 14


@pytest.mark.parametrize("B,H,W", [(2, 1, 2), (2, 2, 3), (2, 9, 13), (1, 17, 127), (3, 5, 128)])
def test_onehot_expectations_equal_float64_conv_and_pool(B, H, W):
    for s in range(SC.N_SETS):
        xi, w, _, bi, want = SC.onehot_case(s, B, H, W)
        assert tuple(want.shape) == (B, 64) + SC.dims(H, W)[2:]
        _same(want, SC.truth64(xi, w, bi))
        assert int(xi.abs().max()) < 1 << 21 and int(bi.abs().max()) <= 100                       # one element + bias: exact in fp32 and in two fp16 pieces


# ------------------------------------------------------------------------------------------------------------------------ dense fixture
def test_dense_fixture_is_exact_in_fp32():
    """Integer tables in range, the no-zero table without zeros, |conv| <= 2,372 < 2^24 - and PyTorch's fp32 convolution indeed returns the float64
    truth bit for bit at a few shapes."""
    for nozero in (False, True):
        w, b = SC.dense_weights(nozero)
        assert bool((w == w.round()).all()) and float(w.abs().max()) == SC.W_ABS and bool((b == b.round()).all()) and float(b.abs().max()) <= SC.B_ABS
        assert bool((w == 0).any()) != nozero
        assert set(w.unique().tolist()) == ({-3.0, -2.0, -1.0, 1.0, 2.0, 3.0} | (set() if nozero else {0.0}))
    assert SC.EXACT_BOUND == 2372 and SC.EXACT_BOUND < 1 << 24
    for B, H, W in ((2, 1, 2), (2, 2, 3), (2, 9, 13), (2, 26, 64), (3, 33, 31)):
        for nozero in (False, True):
            x, w, b, truth = SC.dense_case(B, H, W, nozero)
            assert float(x.abs().max()) <= SC.X_MAX and bool((x == x.round()).all())
            conv = F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=3)
            assert float(conv.abs().max()) <= SC.EXACT_BOUND and float(truth.max()) > 0
            ref32 = F.max_pool2d(torch.relu(F.conv2d(x, w, b, stride=2, padding=3)), 3, 2, 1)
            assert torch.equal(ref32.double(), truth)
    # a batch one image smaller is the first images of the larger one (the strip cases share one truth)
    assert torch.equal(SC.dense_image(5, 9, 13)[:4], SC.dense_image(4, 9, 13))


# ------------------------------------------------------------------------------------------------------------------------ the lane arithmetic
def test_lane_model_equals_the_truths():
    """The restated lane arithmetic gives the float64 truth on the dense fixture at every width and height, and the integer expectation on the
    one-hot sets: what it rejects below, it rejects because of the mutation."""
    for B, H, W in SC.ALL_WIDTHS[:127] + SC.HEIGHTS[:26] + ((2, 6, 127), (2, 6, 128), (2, 26, 64)):
        x, w, b, truth = SC.dense_case(B, H, W)
        assert torch.equal(SC.lane_model(x, w, b), truth), (B, H, W)
    for _, H, W in SC.ONEHOT_WIDTHS:
        for s in (0, 3, 6):
            xi, w, _, bi, want = SC.onehot_case(s, 1, H, W)
            assert torch.equal(SC.lane_model(xi, w, bi), want.double()), (s, H, W)


def _rejected(got, want, B, H, W, taps=None):
    text = SC.difference(got, want, B, H, W, False, taps)
    return text


def test_a_tap_one_column_off_is_rejected_by_the_onehot_sets():
    """At every width of the one-hot list some set rejects the kernel whose tap kx reads tap kx + 1's element, and over the list every kx < 6 of both
    input channels is named."""
    named = set()
    for _, H, W in SC.ONEHOT_WIDTHS:
        texts = []
        for s in range(SC.N_SETS):
            xi, w, taps, bi, want = SC.onehot_case(s, 1, H, W)
            bad = SC.lane_model(xi, w, bi, "kx") != want.double()
            if bool(bad.any()):
                texts.append(_rejected(SC.lane_model(xi, w, bi, "kx"), want.double(), 1, H, W, taps))
                for c in bad.any(dim=3).any(dim=2).any(dim=0).nonzero().flatten().tolist():
                    named.add((int(taps[0][c]), int(taps[2][c])))
        assert texts and all("tap (ci, ky, kx)" in t and f"(B, H, W) = (1, {H}, {W})" in t and "lanes" in t for t in texts), (W, texts)
    assert named == {(ci, kx) for ci in range(2) for kx in range(6)}, named                        # (kx = 6 has no tap to its right: unchanged)


def test_a_missing_sh_select_is_rejected_at_every_odd_width():
    for B, H, W in SC.ALL_WIDTHS[:127]:
        x, w, b, truth = SC.dense_case(B, H, W)
        text = _rejected(SC.lane_model(x, w, b, "sh"), truth, B, H, W)
        assert (text is not None) == (W % 2 == 1), (W, text)
        if text:
            assert f"sh lane: {SC.sh_lane(W)}" in text and f"({B}, {H}, {W})" in text


def test_a_pool_neighbour_from_the_wrong_side_is_rejected_at_every_width():
    for B, H, W in SC.ALL_WIDTHS[:127]:
        x, w, b, truth = SC.dense_case(B, H, W)
        text = _rejected(SC.lane_model(x, w, b, "pool"), truth, B, H, W)
        assert (text is not None) == (W >= 3), (W, text)                                           # W = 2: one conv column, no neighbour


# ------------------------------------------------------------------------------------------------------------------------ non-finite pixels
def _bits_equal(a, b):
    return (a == b) | (a.isnan() & b.isnan())


def test_nonfinite_fixture_and_the_multiplied_padding_row():
    """On the 1-row shape: the float64 reference with one +inf holds no NaN (the no-zero table: no 0 x inf), differs from the clean truth only inside
    the pixel's field, and the lane arithmetic equals it everywhere; with one NaN the lane arithmetic leaves every output outside the field
    bit-equal to the clean one.  A padding row that is the re-read row 0 TIMES 0 breaks exactly that for a non-finite pixel in row 0 - and passes every
    finite fixture, which is why this one exists."""
    B, H, W = SC.NONFINITE_SHAPES[0]
    x, w, b, clean = SC.dense_case(B, H, W, True)
    assert torch.equal(SC.lane_model(x, w, b), clean) and torch.equal(SC.lane_model(x, w, b, "mul"), clean)
    names = set()
    for name, bi, ci, iy, ix in SC.nonfinite_positions(B, H, W):
        names.add(name)
        fld = SC.field(B, H, W, bi, iy, ix).expand_as(clean)
        assert bool(fld.any()) and not bool(fld.all())
        ref = SC.truth64(SC.poisoned(x, float("inf"), bi, ci, iy, ix), w, b)
        assert not bool(ref.isnan().any()) and torch.equal(ref[~fld], clean[~fld]) and bool((ref != clean).any()) and bool(ref.isinf().any())
        assert torch.equal(SC.lane_model(SC.poisoned(x, float("inf"), bi, ci, iy, ix), w, b), ref), name
        for value in (float("nan"), float("inf")):
            xp = SC.poisoned(x, value, bi, ci, iy, ix)
            assert torch.equal(SC.lane_model(xp, w, b)[~fld], clean[~fld]), (name, value)
            spread = not bool(_bits_equal(SC.lane_model(xp, w, b, "mul"), clean)[~fld].all())
            assert spread == (iy == 0), (name, value)                                              # only row 0 is re-read for the rows outside
    assert names == {"row 0", "last row", "column W-2", "column W-1", "interior"}
    # PyTorch gives NaN inside the field of a NaN pixel where the kernel's fmaxf gives 0 behind the ReLU (docs/PARITY.md): no value is asserted there
    name, bi, ci, iy, ix = SC.nonfinite_positions(B, H, W)[-1]
    xp = SC.poisoned(x, float("nan"), bi, ci, iy, ix)
    fld = SC.field(B, H, W, bi, iy, ix).expand_as(clean)
    assert bool(SC.truth64(xp, w, b)[fld].isnan().all()) and not bool(SC.lane_model(xp, w, b).isnan().any())


def test_field_is_the_receptive_field_through_the_pool():
    """field() against the definition: output (p, q) sees conv rows 2p-1 .. 2p+1 and conv row r sees input rows 2r-3 .. 2r+3."""
    B, H, W = 1, 17, 13
    Hc, Wc, Hp, Wp = SC.dims(H, W)
    for iy, ix in ((0, 5), (16, 6), (8, 11), (7, 12), (8, 6)):
        want = torch.zeros(Hp, Wp, dtype=torch.bool)
        for p in range(Hp):
            for q in range(Wp):
                rows = [r for r in (2 * p - 1, 2 * p, 2 * p + 1) if 0 <= r < Hc and abs(iy - 2 * r) <= 3]
                cols = [c for c in (2 * q - 1, 2 * q, 2 * q + 1) if 0 <= c < Wc and abs(ix - 2 * c) <= 3]
                want[p, q] = bool(rows and cols)
        assert torch.equal(SC.field(B, H, W, 0, iy, ix)[0, 0], want), (iy, ix)


def test_random_fixture_has_a_yardstick():
    """The random fixture's bound is check_per_image's 4 e_ref + 1e-5 scale: PyTorch's fp32 result is a real yardstick (e_ref > 0, far below scale)."""
    x, w, b, truth, ref32 = SC.random_case(*SC.RANDOM_SHAPES[3], SC.RANDOM_SCALES[1])
    e_ref, scale = float((ref32.double() - truth).abs().max()), float(truth.abs().max())
    print(f"FORMS trunk stem random fixture {SC.RANDOM_SHAPES[3]} x{SC.RANDOM_SCALES[1]:g}: e_ref {e_ref:.3e}, scale {scale:.3f}")
    assert 0 < e_ref < 1e-5 * scale and np.isfinite(scale)
