"""PreShareFeature on the device (csrc/share_feature.hip: share_feature_rows_kernel for W <= 128, share_feature_kernel on 4 x 128 LDS tiles beyond) in
every strip height, at every end of a strip and every tile edge, BIT-equal to a float64 chain on the exact fixture of tests/share_feature_cases.py (the
host side, tests/test_share_feature_host.py, proves that the fixture is exact and that the tables reach every form); one bright pixel; canaries around
the buffers; real parameters against float64 with the fp32 PyTorch chain's own error as the yardstick."""
import json
import os
import subprocess
import sys

import pytest
import torch

import share_feature_cases as SC

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT_S = 240      # a child imports torch, opens the GPU and runs 348 small launches with their float64 references: seconds


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def where(b, r, c, B, H, W, n=None):
    """Which strip of how many rows and which row inside it (rows kernel), or which tile (LDS kernel), an output (image b, row r, column c) belongs to."""
    if W <= SC.ROWS_MAX_W:
        n = n or SC.strip_rows(B, H)
        ra, rb = SC.strips(n, H)[r // n]
        return f"strip_rows = {n}: strip {r // n} = rows [{ra}, {rb}), row {r - ra} of it, lane {c // 2} half {c % 2}"
    return f"tile (row {r // SC.TILE_ROWS}, column {c // SC.TILE_COLS}), at ({r % SC.TILE_ROWS}, {c % SC.TILE_COLS}) inside it"


def explain(d, B, H, W):
    """The message of a mismatch: how many, the first (image, row, column) and where() of it."""
    count, (b, r, c), got, want = d
    return (f"{count} of {B * H * W} outputs differ at (B, H, W) = ({B}, {H}, {W}); first (image, row, column) = ({b}, {r}, {c}): got {got!r}, "
            f"want {want!r}; " + where(b, r, c, B, H, W))


def _id(case):
    return "B%d_%dx%d" % case


@pytest.mark.parametrize("case", SC.PROD + SC.N16, ids=_id)
def test_production_strip_heights_are_exact(dev, case):
    """hdn_amd.share_feature.share_feature at the batches that make launch_sf_rows pick 1, 1, 2, 2, 4, 8 rows per wave on 127 x 127 images, 16 rows
    and the n >= H stop on tiny ones: torch.equal to the float64 chain."""
    from hdn_amd import share_feature as SF
    B, H, W = case
    params = SC.exact_params()
    x = SC.exact_image(B, H, W)
    want = SC.reference64(x, params).float()
    got = SF.share_feature(x.to(dev), params[3].to(dev)).cpu()
    d = SC.first_difference(got, want)
    assert d is None, explain(d, B, H, W)


_child_fault = []          # a child that died of a signal or ran into its time limit: nothing more is started on the device by this test


@pytest.mark.parametrize("n", SC.FORCED_N)
def test_forced_strip_height_sweep_is_exact(dev, n):
    """HDN_SF_STRIP = n (read once per process: one fresh child per n, one after another) over every sweep size, (1 .. 26, 33, 34, 35) x (1, 2, 3,
    31 .. 33, 63 .. 65, 126 .. 128) at 3 images: the child compares every size with the float64 chain, from an output buffer that held NaN, and prints
    the failing (H, W, image, row, column)."""
    if _child_fault:
        pytest.fail(f"not started: {_child_fault[0]}")
    cmd = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "share_feature_cases.py")]
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S, env=dict(os.environ, HDN_SF_STRIP=str(n)))
    except subprocess.TimeoutExpired as e:
        _child_fault.append(f"the child with HDN_SF_STRIP={n} did not end within {CHILD_TIMEOUT_S} s")
        pytest.fail(_child_fault[0] + ": " + str(e.stderr)[-1500:])
    tail = res.stdout[-1500:] + res.stderr[-1500:]
    if res.returncode < 0:
        _child_fault.append(f"the child with HDN_SF_STRIP={n} ended with signal {-res.returncode}")
        pytest.fail(_child_fault[0] + ": " + tail)
    assert res.returncode == 0, tail
    answer = json.loads(res.stdout.strip().splitlines()[-1])
    assert answer["strip"] == str(n) and answer["sizes"] == len(SC.sweep_sizes()), answer
    bad = answer["failures"]
    assert bad == [], (f"{len(bad)} of {answer['sizes']} sizes differ at {n} rows per wave; (H, W, image, row, column) of each size's first: {bad[:40]}; "
                       f"the first: " + where(*bad[0][2:], SC.SWEEP_B, bad[0][0], bad[0][1], n))


@pytest.mark.parametrize("case", SC.TILE, ids=_id)
def test_lds_tile_kernel_edges_are_exact(dev, case):
    """The W > 128 kernel on both sides of its 128-column and 4-row tile edges, from an output buffer that held NaN."""
    B, H, W = case
    params = SC.exact_params()
    x = SC.exact_image(B, H, W)
    d = SC.first_difference(SC.run_poisoned(x, params[3].to(dev), dev), SC.reference64(x, params).float())
    assert d is None, explain(d, B, H, W)


@pytest.mark.parametrize("H,W", SC.BRIGHT_SIZES)
def test_one_bright_pixel_reaches_its_7x7_neighbourhood(dev, H, W):
    """All-ones weights, scale 1, shift 0: one pixel of 1 at the corners, the edge midpoints, 4- and 8-row boundaries and lane-boundary columns lights
    exactly its clipped 7 x 7 box, with the float64 path counts (every layer zero-pads its own input); the second image of the batch stays zero."""
    params = SC.ones_params()
    folded = params[3].to(dev)
    for r, c in SC.bright_pixels(H, W):
        x = torch.zeros(2, 1, H, W)
        x[0, 0, r, c] = 1.0
        got = SC.run_poisoned(x, folded, dev)
        box = torch.zeros(H, W, dtype=torch.bool)
        box[max(r - 3, 0):r + 4, max(c - 3, 0):c + 4] = True
        assert torch.equal(got[0, 0] != 0, box), f"pixel ({r}, {c}) of {H} x {W}: support " + str(((got[0, 0] != 0) != box).nonzero()[:8].tolist())
        assert not got[1].any(), f"pixel ({r}, {c}) of {H} x {W}: the next image holds {got[1].count_nonzero()} non-zeros"
        d = SC.first_difference(got, SC.reference64(x, params).float())
        assert d is None, f"pixel ({r}, {c}): " + explain(d, 2, H, W)


CANARY = -12345.678


@pytest.mark.parametrize("B,H,W,img_off,out_off", [(3, 5, 127, 256, 256), (3, 5, 128, 256, 256), (2, 5, 131, 256, 256),
                                                   (3, 5, 127, 255, 256),        # img 4-byte, not 8-byte aligned
                                                   (3, 5, 127, 257, 253)])       # both
def test_no_stray_writes_and_inputs_untouched(dev, B, H, W, img_off, out_off):
    """hdn_share_feature_f32 on slices in the middle of larger buffers: the canaries on both sides of the output and of the image and the image itself
    are bit-unchanged afterwards, and the slice is exact."""
    params = SC.exact_params()
    x = SC.exact_image(B, H, W)
    n = B * H * W
    img_host = torch.full((img_off + n + 256,), CANARY)
    img_host[img_off:img_off + n] = x.flatten()
    img_big, out_big = img_host.to(dev), torch.full((out_off + n + 256,), CANARY, device=dev)
    img, out = img_big[img_off:img_off + n].view(B, 1, H, W), out_big[out_off:out_off + n].view(B, 1, H, W)
    assert img.data_ptr() % 8 == (4 if img_off % 2 else 0) and out.data_ptr() % 8 == (4 if out_off % 2 else 0)
    SC.launch(img, params[3].to(dev), out)
    torch.cuda.synchronize()
    bits = lambda t: t.cpu().view(torch.int32)
    assert torch.equal(bits(img_big), bits(img_host)), "the input buffer changed"
    got = out_big.cpu()
    canary = torch.full((1,), CANARY)
    for name, part in (("before", got[:out_off]), ("behind", got[out_off + n:])):
        wrong = (bits(part) != bits(canary)).nonzero().flatten()
        assert wrong.numel() == 0, f"{wrong.numel()} canaries {name} the output were overwritten, first at {int(wrong[0])} of {part.numel()}"
    d = SC.first_difference(got[out_off:out_off + n].view(B, 1, H, W), SC.reference64(x, params).float())
    assert d is None, explain(d, B, H, W)


@pytest.mark.parametrize("shape", [(9, 1, 127, 127), (128, 1, 127, 127), (3, 1, 26, 127), (2, 1, 9, 257)], ids=lambda s: "B%d_%dx%d" % (s[0], s[2], s[3]))
def test_real_parameters_vs_float64(dev, shape):
    """N(0, 1) images and randomised BatchNorm statistics as test_share_feature_shapes_vs_oracle, at 2 and 8 rows per wave, a sweep size and a tiled
    one: against the float64 chain the kernel's largest error is at most twice that of the fp32 PyTorch chain (oracle.hdn_oracle.share_feature) on the
    same input, plus 1e-6 (the bound of check_xcorr in tests/test_gpu_parity.py), and the two fp32 results are within 1e-4 + 1e-5 max |ref|."""
    import hdn_amd
    from oracle import hdn_oracle as O
    torch.manual_seed(sum(shape))
    m = hdn_amd.PreShareFeature().eval()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.uniform_(-0.5, 0.5)
            mod.running_var.uniform_(0.5, 2.0)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.uniform_(-0.3, 0.3)
    x = torch.randn(shape)
    sd = {"ShareFeature." + k: v.detach().clone() for k, v in m.ShareFeature.state_dict().items()}
    ws, alphas, betas = [], [], []
    for conv, bn in ((0, 1), (3, 4), (6, 7)):                                 # eval-mode BatchNorm as a scale and a shift, in float64
        p = lambda name: sd[f"ShareFeature.{bn}.{name}"].double()
        a = p("weight") / torch.sqrt(p("running_var") + hdn_amd.share_feature.BN_EPS)
        ws.append(sd[f"ShareFeature.{conv}.weight"].double())
        alphas.append(a)
        betas.append(p("bias") - p("running_mean") * a)
    truth = SC.chain(x, ws, torch.cat(alphas), torch.cat(betas))
    ref = O.share_feature(x, sd)
    y = m.to(dev)(x.to(dev)).cpu()
    assert y.shape == ref.shape == truth.shape
    e_hip, e_ref, d = float((y.double() - truth).abs().max()), float((ref.double() - truth).abs().max()), float((y - ref).abs().max())
    print(f"SHARE_FEATURE real parameters {shape}: strip_rows {SC.strip_rows(shape[0], shape[2])}, hip err {e_hip:.3e}, fp32 reference err {e_ref:.3e} "
          f"against float64, max|hip - ref| {d:.3e}, max|ref| {float(ref.abs().max()):.3f}")
    assert d <= 1e-4 + 1e-5 * float(ref.abs().max())
    assert e_hip <= 2 * e_ref + 1e-6, f"hip err {e_hip:.3e} vs reference err {e_ref:.3e} against float64"
