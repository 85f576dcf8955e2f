"""GPU tests (-m gpu) of the device-resident frame handling (hdn_amd.frame) through the C ABI: bit-exact against the
fixtures the reference's own get_subwindow* / get_search_info produced (tests/golden/frame.npz) for the pinned arithmetic,
and bit-exact against oracle/frame_oracle.py for the restated OpenCV pieces.  Those pieces are also held, per pixel and at
the tracker's sizes (720p frames, 127 / 255 / 303 crops), to tests/cv_semantics.py: an independent float64 statement of
each OpenCV call's conventions, with the bars of tests/test_opencv_semantics.py.  Bit-exactness to OpenCV itself stays
unpinned (tests/test_cv2_pin.py, when an image has cv2)."""
import math

import numpy as np
import pytest
import torch

import cv_semantics as S
from conftest import load_golden
from oracle import frame_oracle as F
from oracle import hdn_oracle as O
from test_cv2_pin import HOMOGRAPHIES, ROTATIONS, _frame
from test_opencv_semantics import HORIZON

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


from hdn_amd import frame as FR  # noqa: E402


def test_get_subwindow_golden_config5_crop_size(dev):
    """hdn_subwindow_f32 at model_sz = 303 (the search crop of BASELINE configs[4]) against the reference's own get_subwindow /
    get_subwindow_for_homo (tests/golden/frame303.npz): crop position, every padding side, uint8(avg) fill — bit-exact."""
    g = load_golden("frame303")
    fr = FR.upload(g["im"])
    for i, (pos, sz) in enumerate(zip(g["pos"], g["sz"])):
        sz = int(sz)
        assert sz == 303
        a = FR.get_subwindow(fr, pos, sz, sz, g["avg"])
        assert a.shape == (1, 3, 303, 303)
        np.testing.assert_array_equal(a.cpu().numpy()[0].astype(np.uint8), g[f"crop{i}"][0], err_msg=f"case {i}")
        _, pts = FR.get_subwindow_for_homo(fr, pos, sz, sz, g["avg"])
        np.testing.assert_array_equal(np.array(pts, np.float64), g[f"pts{i}"])
    # with the resize in front (s_x != 303), against the oracle's restated cv2.resize (parity-unpinned)
    for pos, osz in (((208.0, 165.0), 380.0), ((20.3, 300.7), 251.0)):
        np.testing.assert_array_equal(FR.get_subwindow(fr, pos, 303, osz, g["avg"]).cpu().numpy(), F.get_subwindow(g["im"], pos, 303, osz, g["avg"]))


def test_get_subwindow_golden(dev):
    g = load_golden("frame")
    fr = FR.upload(g["im"])
    for i, (pos, sz) in enumerate(zip(g["pos"], g["sz"])):
        sz = int(sz)
        a = FR.get_subwindow(fr, pos, sz, sz, g["avg"])
        assert a.shape == (1, 3, sz, sz) and a.dtype == torch.float32
        np.testing.assert_array_equal(a.cpu().numpy()[0].astype(np.uint8), g[f"crop{i}"][0], err_msg=f"case {i}")
        b, pts = FR.get_subwindow_for_homo(fr, pos, sz, sz, g["avg"])
        assert torch.equal(a, b)
        np.testing.assert_array_equal(np.array(pts, np.float64), g[f"pts{i}"])
    s = FR.get_search_info(fr, [66.0, 48.0], 127, g["avg"])
    assert s.shape == (1, 1, 127, 127)
    np.testing.assert_allclose(s.cpu().numpy()[0], g["search_info"].astype(np.float32), rtol=0, atol=1e-6)
    # parameters that already live on the device
    p = torch.tensor([66.0, 48.0, 127.0, *g["avg"]], dtype=torch.float64, device=dev)
    assert torch.equal(FR.get_search_info(fr, None, None, None, params=p), s)


def test_subwindow_with_resize_vs_oracle(dev):
    r = np.random.default_rng(5)
    im = r.integers(0, 256, (360, 640, 3)).astype(np.uint8)
    fr = FR.upload(im)
    avg = np.mean(im, axis=(0, 1))
    for pos, osz, msz in (((320.0, 180.0), 253.0, 255), ((10.5, 350.2), 311.0, 255), ((600.0, 20.0), 95.0, 127), ((300.3, 200.7), 57.6, 127),
                          ((100.0, 100.0), 127.0, 127), ((333.0, 111.0), 510.0, 255), ((5.0, 5.0), 30.0, 127)):
        want = F.get_subwindow(im, pos, msz, osz, avg)
        got = FR.get_subwindow(fr, pos, msz, osz, avg)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=str((pos, osz, msz)))
        gray = FR.get_search_info(fr, pos, osz, avg, model_sz=msz)
        np.testing.assert_allclose(gray.cpu().numpy()[0], F.search_info(want[0]).astype(np.float32), rtol=0, atol=1e-6)


def test_frame_warps_vs_oracle(dev):
    r = np.random.default_rng(6)
    im = r.integers(0, 256, (180, 320, 3)).astype(np.uint8)
    fr = FR.upload(im)
    assert torch.equal(FR.warp_perspective(fr, np.eye(3)), fr)
    assert torch.equal(FR.rot_around_center(fr, 100.0, 80.0, 0.0), fr)
    Hs = [np.array([[1.02, 0.03, -4.2], [-0.02, 0.97, 6.1], [1e-5, -2e-5, 1.0]]),
          np.array([[0.9, 0.2, 30.0], [-0.15, 1.1, -12.0], [3e-4, 1e-4, 1.0]]),
          np.array([[1, 0, 500.0], [0, 1, -400.0], [0, 0, 1.0]])]
    for M in Hs:
        got = FR.warp_perspective(fr, M).cpu().numpy()
        np.testing.assert_array_equal(got, F.warp_perspective_u8(im, M))
    Md = torch.tensor(Hs[0].reshape(-1), dtype=torch.float64, device=dev)
    assert torch.equal(FR.warp_perspective(fr, Md), FR.warp_perspective(fr, Hs[0]))
    for (cx, cy, rot) in ((160.0, 90.0, 0.3), (10.0, 170.0, -1.2), (400.0, -20.0, 3.0)):
        got = FR.rot_around_center(fr, cx, cy, rot).cpu().numpy()
        np.testing.assert_array_equal(got, F.warp_affine_cubic_u8(im, F.rot_matrix_2x3(cx, cy, rot)))
    # sizes whose pixel count is not a multiple of 4 (the last pixels leave as bytes, the rest as packed 4-byte stores), images narrower
    # than the 4-tap window, a single pixel; and 1- / 4-channel frames (byte path throughout)
    for (h, w) in ((7, 5), (33, 31), (1, 1), (2, 3), (5, 127), (257, 3)):
        im2 = r.integers(0, 256, (h, w, 3)).astype(np.uint8)
        f2 = FR.upload(im2)
        M = np.array([[0.97, 0.05, 0.7], [-0.04, 1.03, -0.4], [1e-4, -2e-4, 1.0]])
        np.testing.assert_array_equal(FR.warp_perspective(f2, M).cpu().numpy(), F.warp_perspective_u8(im2, M), err_msg=str((h, w)))
        A = F.rot_matrix_2x3(w / 2.0, h / 3.0, 0.4)
        np.testing.assert_array_equal(FR.warp_affine_cubic(f2, A).cpu().numpy(), F.warp_affine_cubic_u8(im2, A), err_msg=str((h, w)))
    for c in (1, 4):
        im2 = r.integers(0, 256, (21, 19, c)).astype(np.uint8)
        f2 = FR.upload(im2)
        M = np.array([[1.01, 0.02, -1.3], [0.03, 0.98, 2.2], [0, 0, 1.0]])
        np.testing.assert_array_equal(FR.warp_perspective(f2, M).cpu().numpy(), F.warp_perspective_u8(im2, M))
        A = F.rot_matrix_2x3(9.0, 11.0, -0.2)
        np.testing.assert_array_equal(FR.warp_affine_cubic(f2, A).cpu().numpy(), F.warp_affine_cubic_u8(im2, A))
    with pytest.raises(Exception):
        FR.get_subwindow(torch.zeros(4, 4, 3, dtype=torch.uint8), [1, 1], 3, 3, [0, 0, 0])


def test_log_polar_vs_oracle(dev):
    """get_polar_img / get_subwindow(islog=1) (restated cv2.logPolar, parity-unpinned) bit-exact against the oracle's restatement."""
    r = np.random.default_rng(11)
    for S, C in ((127, 3), (31, 1), (64, 2)):
        img = r.integers(0, 256, (S, S, C), dtype=np.uint8)
        patch = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))[None].astype(np.float32)).to(dev)
        got = FR.get_polar_img(patch)
        assert got.shape == patch.shape and got.dtype == torch.float32
        np.testing.assert_array_equal(got.cpu().numpy()[0].transpose(1, 2, 0).astype(np.uint8), F.get_polar_img(img), err_msg=f"S={S}")
        assert torch.equal(got, got.round())                                       # uint8-valued
    o = (40.2, 71.6)
    patch = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))[None].astype(np.float32)).to(dev)
    np.testing.assert_array_equal(FR.get_polar_img(patch, original=o).cpu().numpy()[0].transpose(1, 2, 0).astype(np.uint8),
                                  F.get_polar_img(img, original=o))
    # the 6-channel template crop of the tracker: np.concatenate((im_patch, getPolarImg(im_patch)), 2)
    g = load_golden("frame")
    fr = FR.upload(g["im"])
    six = FR.get_subwindow(fr, g["pos"][0], 127, int(g["sz"][0]), g["avg"], islog=1)
    assert six.shape == (1, 6, 127, 127)
    three = FR.get_subwindow(fr, g["pos"][0], 127, int(g["sz"][0]), g["avg"])
    assert torch.equal(six[:, :3], three)
    ref = F.get_polar_img(three.cpu().numpy()[0].transpose(1, 2, 0).astype(np.uint8))
    np.testing.assert_array_equal(six[0, 3:].cpu().numpy().transpose(1, 2, 0).astype(np.uint8), ref)
    with pytest.raises(ValueError):
        FR.get_polar_img(patch[0])


# ------------------------------------------------------------------------------- kernels against the independent reference
def _within(got, ref, bar, what):
    bad = S.violations(got, ref, bar)
    d = np.abs(np.asarray(got, np.float64) - ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} values outside the bar, worst excess {float((d - bar).max()):.4g}"


def test_warp_perspective_720p_vs_reference(dev):
    """hdn_frame_warp_perspective_batch_u8 on 720p frames: every pixel within 0.5 + L/32 of cv_semantics.warp_perspective
    (HOMOGRAPHIES of test_cv2_pin plus a matrix whose w = 0 line crosses the frame); then the batch entry, B = 3, each
    frame with its own matrix passed as the column slice [:, :9] of a float64 [3, 16] device array."""
    im = _frame(2)
    fr = FR.upload(im)
    for M in HOMOGRAPHIES + [HORIZON]:
        ref, L = S.warp_perspective(im, M)
        _within(FR.warp_perspective(fr, M).cpu().numpy(), ref, S.bar_bilinear_u8(L), str(M))
    ims = np.stack([_frame(s) for s in (12, 13, 14)])
    Ms = [HOMOGRAPHIES[2], HORIZON, HOMOGRAPHIES[4]]
    rec = torch.zeros(3, 16, dtype=torch.float64)
    for b, M in enumerate(Ms):
        rec[b, :9] = torch.from_numpy(M.reshape(-1))
        rec[b, 9:] = -1e30                                   # the rest of the record must not be read
    rec = rec.to(dev)
    got = FR.warp_perspective(torch.from_numpy(ims).to(dev), rec[:, :9]).cpu().numpy()
    for b, M in enumerate(Ms):
        ref, L = S.warp_perspective(ims[b], M)
        _within(got[b], ref, S.bar_bilinear_u8(L), f"batch {b}")


def test_warp_affine_cubic_720p_vs_reference(dev):
    """hdn_frame_warp_affine_cubic_batch_u8 (rot_around_center and warp_affine_cubic) on a 720p frame, ROTATIONS of
    test_cv2_pin: every pixel within 1 + L/32 of cv_semantics.warp_affine_cubic (Keys a = -0.75, replicate, saturated);
    then the batch form, B = 3 frames with [3, 6] matrices."""
    im = _frame(4)
    fr = FR.upload(im)
    for cx, cy, rot in ROTATIONS:
        A = F.rot_matrix_2x3(cx, cy, rot)
        ref, L = S.warp_affine_cubic(im, A)
        _within(FR.rot_around_center(fr, cx, cy, rot).cpu().numpy(), ref, S.bar_cubic_u8(L), str((cx, cy, rot)))
        _within(FR.warp_affine_cubic(fr, A).cpu().numpy(), ref, S.bar_cubic_u8(L), str((cx, cy, rot)))
    ims = np.stack([_frame(s) for s in (15, 16, 17)])
    rots = ROTATIONS[1:4]
    As = np.stack([F.rot_matrix_2x3(*r).reshape(-1) for r in rots])
    got = FR.warp_affine_cubic(torch.from_numpy(ims).to(dev), torch.from_numpy(As).to(dev)).cpu().numpy()
    for b, r in enumerate(rots):
        ref, L = S.warp_affine_cubic(ims[b], F.rot_matrix_2x3(*r))
        _within(got[b], ref, S.bar_cubic_u8(L), f"batch {b} {r}")


SUBWINDOW_RESIZES = [((640.0, 360.0), 380.0, 303), ((5.0, 5.0), 380.0, 303), ((1275.0, 715.0), 510.0, 255),
                     ((333.0, 111.0), 510.0, 255), ((640.0, 360.0), 253.0, 255), ((100.0, 700.0), 253.0, 255),
                     ((300.3, 200.7), 57.6, 127), ((1200.0, 30.0), 57.6, 127), ((2.0, 718.0), 57.6, 127)]


def test_subwindow_resize_vs_reference(dev):
    """hdn_subwindow_batch_f32 with its resize (303 from 380, 255 from 510 and from 253, 127 from 57.6) at 720p, crops
    overhanging every edge (and, on a small frame, all four at once).  The crop / padding is fixture-pinned
    (F.subwindow_patch); the resize that follows must be within 1 + L/256 of cv_semantics.resize_linear."""
    cases = [(_frame(9), SUBWINDOW_RESIZES), (_frame(10, 200, 300), [((150.0, 100.0), 510.0, 255), ((150.0, 100.0), 253.0, 255)])]
    for im, crops in cases:
        fr = FR.upload(im)
        avg = np.mean(im, axis=(0, 1))
        for pos, osz, msz in crops:
            patch = F.subwindow_patch(im, pos, osz, avg)
            assert patch.shape[0] != msz
            ref, L = S.resize_linear(patch, msz, msz)
            got = FR.get_subwindow(fr, pos, msz, osz, avg).cpu().numpy()[0].transpose(1, 2, 0)
            _within(got, ref, S.bar_resize_u8(L), str((im.shape, pos, osz, msz)))


def test_polar_vs_reference(dev):
    """hdn_remap_linear_f32 through get_polar_img at 127 and 255 (centre S // 2, and an off-centre `original`) and the
    six-channel islog=1 template crop: every value within 0.5 + L/32 of cv_semantics.log_polar (radius exp(rho / M) - 1,
    taps outside = 0)."""
    im = _frame(7)
    for S_, original in ((127, None), (255, None), (127, (40.2, 71.6)), (255, (200.4, 31.5))):
        img = np.ascontiguousarray(im[100:100 + S_, 300:300 + S_])
        patch = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))[None].astype(np.float32)).to(dev)
        c = (S_ // 2, S_ // 2) if original is None else tuple(float(v) for v in np.round(original))
        ref, L = S.log_polar(img, c, S_ / math.log(S_ / 2))
        got = FR.get_polar_img(patch, original=original).cpu().numpy()[0].transpose(1, 2, 0)
        _within(got, ref, S.bar_bilinear_u8(L), f"S={S_} original={original}")
    fr = FR.upload(im)
    avg = np.mean(im, axis=(0, 1))
    for sz in (127, 255):
        six = FR.get_subwindow(fr, (700.0, 400.0), sz, 180.0, avg, islog=1).cpu().numpy()[0].transpose(1, 2, 0)
        assert six.shape == (sz, sz, 6)
        ref, L = S.log_polar(six[:, :, :3], (sz // 2, sz // 2), sz / math.log(sz / 2))
        _within(six[:, :, 3:], ref, S.bar_bilinear_u8(L), f"islog=1 {sz}")


def test_refine_warp_vs_reference(dev):
    """hdn_refine_warp_f32, B = 4, 127 x 127 float, against the float64 bilinear-replicate reference within
    cv_semantics.bar_float.  The matrix the kernel samples through (refine_warp.hip's header, and
    hdn_oracle.refine_step / warp_perspective_replicate): H_hm = fp32(fp32(inv(H)) / fp32(inv(H))[2, 2]) and
    M = fp32(inv(H_hm)) is what cv2.warpPerspective is handed, so the crop is src(M^-1 . (x, y, 1))."""
    from hdn_amd.refine import refine_warp
    r = np.random.default_rng(31)
    img = np.stack([r.standard_normal((127, 127)), r.uniform(0, 1, (127, 127)),
                    _frame(18, 127, 127, 1)[:, :, 0] / 255.0, r.standard_normal((127, 127)) * 3]).astype(np.float32)
    Hm = np.stack([np.eye(3), np.array([[1.01, 0.02, -1.3], [0.03, 0.98, 2.2], [1e-4, -1e-4, 1.0]]),
                   np.array([[0.95, -0.1, 9.0], [0.12, 1.04, -7.5], [-3e-4, 2e-4, 1.0]]),
                   np.array([[1.2, 0.3, -30.0], [-0.25, 0.9, 20.0], [1e-3, -8e-4, 1.0]])]).astype(np.float32)
    got = refine_warp(torch.from_numpy(Hm).to(dev), torch.from_numpy(img)[:, None].to(dev)).cpu().numpy()[:, 0]
    for b in range(4):
        t = np.linalg.inv(Hm[b].astype(np.float64)).astype(np.float32)
        H_hm = (t.astype(np.float64) * (1.0 / np.float64(t[2, 2]))).astype(np.float32)
        M = np.linalg.inv(H_hm.astype(np.float64)).astype(np.float32)
        ref, L = S.warp_perspective(img[b], M.astype(np.float64), ring=1)
        _within(got[b], ref, S.bar_float(ref, L), f"sample {b}")


def test_matrix_forms_at_batch_one(dev):
    """warp_perspective / warp_affine_cubic take the matrix of one frame as a host array or as a float64 device tensor of
    any shape holding its 9 (6) values: [3, 3], [9], [1, 9], a column slice of a wider array; [2, 3], [6], [1, 6].  Each
    gives the host call's output exactly."""
    im = _frame(19, 45, 67)
    fr = FR.upload(im)
    M = np.array([[0.97, 0.05, 0.7], [-0.04, 1.03, -0.4], [1e-4, -2e-4, 1.0]])
    want = FR.warp_perspective(fr, M)
    wide = torch.full((1, 16), -1e30, dtype=torch.float64)
    wide[0, 4:13] = torch.from_numpy(M.reshape(-1))
    d = torch.from_numpy(M).to(dev)
    for name, t in (("[3,3]", d), ("[9]", d.reshape(-1)), ("[1,9]", d.reshape(1, 9)), ("slice", wide.to(dev)[:, 4:13]),
                    ("[3,3] transposed back", d.t().contiguous().t())):
        assert torch.equal(FR.warp_perspective(fr, t), want), name
    A = F.rot_matrix_2x3(30.0, 20.0, 0.4)
    want = FR.warp_affine_cubic(fr, A)
    wide = torch.full((1, 10), -1e30, dtype=torch.float64)
    wide[0, 2:8] = torch.from_numpy(A.reshape(-1))
    a = torch.from_numpy(A).to(dev)
    for name, t in (("[2,3]", a), ("[6]", a.reshape(-1)), ("[1,6]", a.reshape(1, 6)), ("slice", wide.to(dev)[:, 2:8])):
        assert torch.equal(FR.warp_affine_cubic(fr, t), want), name
    for bad in (d[:2], torch.zeros(2, 9, dtype=torch.float64, device=dev)):
        with pytest.raises(ValueError):
            FR.warp_perspective(fr, bad)

