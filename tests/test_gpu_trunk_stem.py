"""GPU tests of the trunk's first stage, conv 7x7 / 2 / 3 + bias + ReLU + max pool 3 / 2 / 1, exactly: hdn_trunk_stem_f32 (csrc/trunk_stem.hip, the vector
pipe) through the raw C ABI in its four instantiations - NCHW / channels-last x 1-row / 4-row strips - at every width 2 .. 128, every height 1 .. 26 and
every strip tail, and hdn_trunk_stem_mfma_f32 (csrc/trunk_stem_mfma.hip, the matrix cores) through FusedStem with one-hot weights that meet all 98 taps.

The fixtures, truths, case lists and the runner live in tests/trunk_stem_cases.py; tests/test_trunk_stem_host.py proves without a device that the lists
reach every form, that the expectations equal float64 conv2d / relu / max_pool2d and that the fixtures reject a tap one column off, a missing `sh`
select, a pool neighbour from the wrong side and a multiplied padding row.  Every exact comparison is a torch.equal; a failure names the form, layout,
shape, image, channel, pooled row and column and the wave (cb, strip) that owns the element.  Random data runs under check_per_image's existing bound."""
import pytest
import torch

import trunk_stem_cases as SC
from test_gpu_trunk50_forms import check_per_image

pytestmark = pytest.mark.gpu

CL = torch.channels_last


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _exact_run(inp, nhwc, want, ooff=0, taps=None, what=""):
    """Two raw calls from NaN inside 0xA5 margins: the result torch.equal to `want`, nothing written outside it, both calls bit-equal."""
    B, _, H, W = inp.shape
    got, clean = SC.run_stem(inp, nhwc, ooff)
    if not torch.equal(got, want.float()) or not torch.equal(want.float().double(), want.double()):
        raise AssertionError(f"{what}: {SC.difference(got.double(), want.double(), B, H, W, nhwc, taps)}")
    assert clean, f"{what}: bytes outside the result were written ({SC.where(B, H, W, nhwc, (0, 0, 0, 0))})"
    again, clean2 = SC.run_stem(inp, nhwc, ooff)
    assert clean2 and torch.equal(again.contiguous().view(torch.int32), got.contiguous().view(torch.int32)), f"{what}: two calls differ"
    return got


# ----------------------------------------------------------------------------------------------------------------- 3.1 dense fixture
@pytest.mark.parametrize("nhwc", SC.LAYOUTS)
@pytest.mark.parametrize("H", [5, 6])
def test_dense_fixture_every_width(dev, H, nhwc):
    """W = 2 .. 128 in the 1-row form: every lane count, every `sh` lane, both parities of the last pooled column."""
    for B, h, W in SC.ALL_WIDTHS:
        if h != H:
            continue
        x, w, b, truth = SC.dense_case(B, H, W)
        inp = SC.Inputs(x, w, b, dev)
        _exact_run(inp, nhwc, truth, what=f"dense W={W}")
        assert inp.unchanged(), (B, H, W)


@pytest.mark.parametrize("nhwc", SC.LAYOUTS)
@pytest.mark.parametrize("W", [7, 64])
def test_dense_fixture_every_height(dev, W, nhwc):
    """H = 1 .. 26: conv row -1, the last conv row and the parity of Hc in every residue; Hp = 1 .. 7 one-row strips."""
    for B, H, w_ in SC.HEIGHTS:
        if w_ != W:
            continue
        x, w, b, truth = SC.dense_case(B, H, W)
        inp = SC.Inputs(x, w, b, dev)
        _exact_run(inp, nhwc, truth, what=f"dense H={H}")
        assert inp.unchanged(), (B, H, W)


@pytest.mark.parametrize("nhwc", SC.LAYOUTS)
@pytest.mark.parametrize("B4,H,W", SC.STRIP4)
def test_dense_fixture_strip_forms_at_every_offset(dev, B4, H, W, nhwc):
    """The first batch of the 4-row form (every Hp mod 4, one to three strips) and one image fewer (the 1-row form), with x and out at every float
    offset of a 16-byte line (each side alone and three mixed pairs)."""
    x4, w, b, truth4 = SC.dense_case(B4, H, W)
    for B in (B4, B4 - 1):
        x, truth = x4[:B], truth4[:B]
        for xo in range(4):
            inp = SC.Inputs(x, w, b, dev, xo)
            for oo in [o for a, o in SC.STRIP_OFFSETS if a == xo]:
                _exact_run(inp, nhwc, truth, oo, what=f"dense offsets (x, out) = ({xo}, {oo})")
            assert inp.unchanged(), (B, H, W, xo)


@pytest.mark.parametrize("nhwc", SC.LAYOUTS)
@pytest.mark.parametrize("B,H,W", SC.OFFSET_WIDTHS)
def test_dense_fixture_edge_widths_at_every_offset(dev, B, H, W, nhwc):
    x, w, b, truth = SC.dense_case(B, H, W)
    for xo, oo in SC.OFFSETS:
        inp = SC.Inputs(x, w, b, dev, xo)
        _exact_run(inp, nhwc, truth, oo, what=f"dense offsets (x, out) = ({xo}, {oo})")
        assert inp.unchanged(), (B, H, W, xo)


# ----------------------------------------------------------------------------------------------------------------- 3.2 one-hot sets
@pytest.mark.parametrize("s", range(SC.N_SETS))
def test_onehot_sets_at_the_width_edges(dev, s):
    """Set s of seven (together: all 98 taps in every 16-channel block, the two channels of a packed pair on different taps) in the 1-row form at the
    widths either side of every 32 conv columns and at both ends of the range, both layouts."""
    for B, H, W in SC.ONEHOT_WIDTHS:
        xi, w, taps, bi, want = SC.onehot_case(s, B, H, W)
        inp = SC.Inputs(xi.float(), w, bi.float(), dev)
        for nhwc in SC.LAYOUTS:
            _exact_run(inp, nhwc, want.double(), taps=taps, what=f"one-hot set {s}")
        assert inp.unchanged(), (s, W)


@pytest.mark.parametrize("s", range(SC.N_SETS))
@pytest.mark.parametrize("B,H,W", SC.ONEHOT_STRIP4)
def test_onehot_sets_in_the_4_row_form(dev, B, H, W, s):
    xi, w, taps, bi, want = SC.onehot_case(s, B, H, W)
    inp = SC.Inputs(xi.float(), w, bi.float(), dev)
    for nhwc in SC.LAYOUTS:
        _exact_run(inp, nhwc, want.double(), taps=taps, what=f"one-hot set {s}")
    assert inp.unchanged(), (s, B, H, W)


@pytest.mark.parametrize("s", range(SC.N_SETS))
@pytest.mark.parametrize("B", SC.ONEHOT_MFMA_BATCHES)
def test_onehot_sets_through_fused_stem_at_127(dev, B, s):
    """FusedStem(conv, True, out_domain) at 127 x 127: the matrix-core form with 4 / 8 / 16 conv rows per workgroup, out_domain 0 and 1 (x 2^8 back:
    exact), and with mfma_disabled the vector form at 127 px behind out_domain 1's mul_ (1-row strips at B = 1 and 8, 4-row at 48)."""
    from hdn_amd import trunk
    S = SC.MFMA_SIDE
    xi, w, taps, bi, want = SC.onehot_case(s, B, S, S)
    conv = torch.nn.Conv2d(2, 64, 7, 2, 3)
    conv.weight.data, conv.bias.data = w.clone(), bi.float()
    assert B >= trunk.STEM_MFMA_MIN_BATCH
    xd = xi.float().to(dev)
    un = 2.0 ** trunk.ACT_SCALE_LOG2
    for disabled in (False, True):
        for dom, k in ((0, 1.0), (1, un)):
            st = trunk.FusedStem(conv, True, out_domain=dom).to(dev)
            st.mfma_disabled = disabled
            y = st(xd)
            assert y.is_contiguous(memory_format=CL)
            form = f"vector form, {SC.strip_rows(B, S, S)}-row strips" if disabled else f"matrix-core form, {SC.mfma_rows(B)} conv rows per workgroup"
            msg = SC.difference((y * k).cpu().double(), want.double(), B, S, S, True, taps)
            assert msg is None, f"FusedStem {form}, out_domain {dom}, one-hot set {s}: {msg}"
    assert torch.equal(xd.cpu(), xi.float())


# ----------------------------------------------------------------------------------------------------------------- 3.3 non-finite pixels
def _eq_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("nhwc", SC.LAYOUTS)
@pytest.mark.parametrize("B,H,W", SC.NONFINITE_SHAPES)
def test_nonfinite_pixels_do_not_spread(dev, B, H, W, nhwc):
    """One NaN, then one +inf, in row 0 (which the rows outside the image re-read), the last row, column W - 2 and W - 1 of an odd width (the clamped
    pair) and inside; weights without zeros.  Every output whose receptive field does not hold the pixel is bit-equal to the clean run: padding is
    selected, never multiplied in.  +inf inside the field: the float64 reference exactly (+inf, or a maximum it does not reach).  NaN inside the field:
    no assertion - PyTorch gives NaN, the kernel's fmaxf gives 0 behind the ReLU and drops a NaN in the pool (docs/PARITY.md)."""
    x, w, b, truth = SC.dense_case(B, H, W, True)
    clean = _exact_run(SC.Inputs(x, w, b, dev), nhwc, truth, what="clean run, weights without zeros")
    for name, bi, ci, iy, ix in SC.nonfinite_positions(B, H, W):
        fld = SC.field(B, H, W, bi, iy, ix).expand_as(truth)
        for value in (float("nan"), float("inf")):
            xp = SC.poisoned(x, value, bi, ci, iy, ix)
            inp = SC.Inputs(xp, w, b, dev)
            got, ok = SC.run_stem(inp, nhwc)
            what = f"{value} at {name} = (image {bi}, channel {ci}, row {iy}, column {ix})"
            assert ok and inp.unchanged(), what
            outside = torch.where(fld, torch.zeros_like(got), got)
            outside_clean = torch.where(fld, torch.zeros_like(clean), clean)
            if not _eq_bits(outside, outside_clean):
                i = (outside.contiguous().view(torch.int32) != outside_clean.contiguous().view(torch.int32)).nonzero()[0].tolist()
                raise AssertionError(f"{what} reached an output outside its receptive field: got {float(got[tuple(i)])!r}, clean {float(clean[tuple(i)])!r} "
                                     f"[{SC.where(B, H, W, nhwc, i)}]")
            if value == float("inf"):
                msg = SC.difference(got.double(), SC.truth64(xp, w, b), B, H, W, nhwc)
                assert msg is None, f"{what}: {msg}"


# ----------------------------------------------------------------------------------------------------------------- 3.4 random data
@pytest.mark.parametrize("scale", SC.RANDOM_SCALES)
@pytest.mark.parametrize("B,H,W", SC.RANDOM_SHAPES)
def test_random_data_vs_float64(dev, B, H, W, scale):
    """N(0, 1) x 1 and x 120 (the tracker's crops) against float64 on every image, both layouts, under the project's per-image bound
    4 e_ref + 1e-5 scale (check_per_image: e_ref = the error of PyTorch's CPU fp32 result)."""
    x, w, b, truth, ref32 = SC.random_case(B, H, W, scale)
    inp = SC.Inputs(x, w, b, dev)
    for nhwc in SC.LAYOUTS:
        got, clean = SC.run_stem(inp, nhwc)
        assert clean
        check_per_image(f"trunk stem {SC.strip_rows(B, H, W)}-row {'NHWC' if nhwc else 'NCHW'} ({B}, {H}, {W}) x{scale:g}", got, truth, ref32)
    assert inp.unchanged()


# ----------------------------------------------------------------------------------------------------------------- 3.5 return codes
def test_refusals_launch_nothing(dev):
    """NULL pointers, W = 1, W = 129, B = 65536 and out == x: the code, and the output still NaN."""
    from hdn_amd import _lib as L
    lib = L.load()
    x, w, b, _ = SC.dense_case(2, 5, 8)
    inp = SC.Inputs(x, w, b, dev)
    out = torch.full((4096,), float("nan"), device=dev)
    p, st = L.ptr, L.stream_ptr(dev)
    args = [p(inp.xd), p(inp.wd), p(inp.bd), p(out)]
    for i in range(4):
        a = list(args)
        a[i] = None
        assert lib.hdn_trunk_stem_f32(*a, 2, 5, 8, 0, st) == SC.E_NULL, i
    for (B, H, W), code in (((2, 5, 1), SC.E_LIMIT), ((2, 5, 129), SC.E_LIMIT), ((65536, 5, 8), SC.E_LIMIT), ((0, 5, 8), SC.E_SHAPE)):
        assert not SC.in_range(B, H, W)
        for nhwc in (0, 1):
            assert lib.hdn_trunk_stem_f32(*args, B, H, W, nhwc, st) == code, (B, H, W)
    assert lib.hdn_trunk_stem_f32(args[0], args[1], args[2], args[0], 2, 5, 8, 0, st) == SC.E_ALIAS
    torch.cuda.synchronize(dev)
    assert bool(out.isnan().all()) and inp.unchanged()
    assert lib.hdn_trunk_stem_f32(*args, 2, 5, 8, 0, st) == 0                                      # the same arguments, in range: it runs
    torch.cuda.synchronize(dev)
    n = 2 * 64 * 2 * 2
    assert torch.equal(out[:n].cpu().view(2, 64, 2, 2).double(), SC.dense_case(2, 5, 8)[3]) and bool(out[n:].isnan().all())
