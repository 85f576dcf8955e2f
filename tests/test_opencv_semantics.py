"""CPU tests: the oracle's restatements of the six OpenCV entry points against tests/cv_semantics.py, an independent
float64 statement of what each call computes.

The oracle (oracle/frame_oracle.py, oracle/hdn_oracle.py:warp_perspective_replicate, oracle/tracker_oracle.py:
perspective_transform) restates OpenCV's fixed-point internals, and the kernels are held to it bit for bit
(tests/test_gpu_frame.py); nothing here is bit-exact to OpenCV itself (tests/test_cv2_pin.py is, when cv2 exists).  What
this file pins is the conventions: every output value must lie within a per-value bar of the continuous-coordinate
reference, the bars being what the fixed-point quantisation can explain (cv_semantics' bar_* functions give the
derivations).  No share of violations is tolerated.

The mutation tests show that the bars bite: each changes one convention of the *reference* (a sub-pixel shift, the cubic's
a, the half-pixel centre, the log-polar radius, ...) and requires the unchanged oracle to violate the bar on at least a
stated share of the values.
"""
import math

import numpy as np
import pytest

import cv_semantics as S
from oracle import frame_oracle as F
from oracle import hdn_oracle as O
from oracle import tracker_oracle as TO
from test_cv2_pin import HOMOGRAPHIES, _frame


def _t(dx, dy):
    return np.array([[1, 0, dx], [0, 1, dy], [0, 0, 1.0]])


def _rot_about(cx, cy, rad):
    c, s = math.cos(rad), math.sin(rad)
    return _t(cx, cy) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ _t(-cx, -cy)


# w = 0 on the destination row y = 180 (inside both a 360p and a 720p frame): the sampled point runs off to infinity there
HORIZON = np.linalg.inv(np.array([[1, 0.05, 0], [0.02, 1, 0], [0, -1 / 180, 1.0]]))
ROT45_360P = _rot_about(320, 180, math.pi / 4)
WARPS_360P = HOMOGRAPHIES + [HORIZON, ROT45_360P]
ROTATIONS_360P = [(320.0, 180.0, 0.3), (10.0, 350.0, -1.2), (700.0, -20.0, 3.0)]
RESIZES = [(380, 303), (57, 127), (253, 255)]


def _frame360(seed=2):
    return _frame(seed, 360, 640)


def _square(seed, n):
    return np.ascontiguousarray(_frame(seed, 400, 400)[:n, :n])


def _assert_within(got, ref, bar, what):
    bad = S.violations(got, ref, bar)
    d = np.abs(np.asarray(got, np.float64) - ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} values outside the bar, worst excess {float((d - bar).max()):.4g}"


# ----------------------------------------------------------------------------------------------- the reference itself
def test_reference_conventions_by_hand():
    """A few values of cv_semantics worked out by hand, so that the reference does not need the oracle to be believed."""
    img = np.arange(12, dtype=np.float64).reshape(3, 4) * 10
    # warpPerspective by a +0.25 px translation samples src(x - 0.25): between x - 1 and x, 3/4 of the way to x
    v, L = S.warp_perspective(img, _t(0.25, 0))
    np.testing.assert_allclose(v[1, 1:], 0.25 * img[1, :-1] + 0.75 * img[1, 1:])
    assert np.all(v[:, 0] == img[:, 0]) and np.all(L[1, 1:] == 40)             # replicate at the left edge; vertical step 40
    # Keys' weights at a half-pixel offset with a = -0.75: (-3/32, 19/32, 19/32, -3/32)
    step = np.zeros((1, 8))
    step[0, 3] = 32.0
    v, _ = S.warp_affine_cubic(np.repeat(step, 4, axis=0), np.array([[1, 0, 0.5], [0, 1, 0.0]]))
    np.testing.assert_allclose(v[1, 2:6], [0.0, 19.0, 19.0, 0.0])                   # -3 saturates to 0
    # resize 2 -> 4: source coordinates -0.25, 0.25, 0.75, 1.25 clamped to [0, 1]
    np.testing.assert_allclose(S.resize_source_coords(2, 4), [0.0, 0.25, 0.75, 1.0])
    # logPolar: column rho samples radius exp(rho / M) - 1, so column 0 is the centre pixel itself
    img = np.random.default_rng(0).uniform(0, 255, (31, 31))
    v, _ = S.log_polar(img, (15, 15), 31 / math.log(15.5))
    assert np.all(v[:, 0] == img[15, 15])
    # perspectiveTransform: true division; 0 once |w| <= DBL_EPSILON
    H = np.array([[2.0, 0, 1], [0, 3, 0], [0, 0, 0.5]])
    np.testing.assert_array_equal(S.perspective_transform([[1.0, 2.0]], H), [[6.0, 12.0]])
    np.testing.assert_array_equal(S.perspective_transform([[1.0, 2.0]], np.diag([1.0, 1.0, S.DBL_EPSILON])), [[0.0, 0.0]])


# ------------------------------------------------------------------------------------------------------- the bars hold
@pytest.mark.parametrize("M", WARPS_360P, ids=[f"H{i}" for i in range(len(WARPS_360P))])
def test_warp_perspective_u8_meets_reference(M):
    """cv2.warpPerspective(frame, M, BORDER_REPLICATE) restated (frame_oracle.warp_perspective_u8): |o - ref| <= 0.5 + L/32
    on every value; HORIZON's w = 0 row crosses the frame."""
    im = _frame360()
    ref, L = S.warp_perspective(im, M)
    _assert_within(F.warp_perspective_u8(im, M), ref, S.bar_bilinear_u8(L), str(M))


def test_warp_perspective_u8_meets_reference_720p():
    """The one 720p case: the tracker's frame size, the most distorting homography and the horizon crossing."""
    im = _frame(2)
    for M in (HOMOGRAPHIES[2], HORIZON):
        ref, L = S.warp_perspective(im, M)
        _assert_within(F.warp_perspective_u8(im, M), ref, S.bar_bilinear_u8(L), str(M))


@pytest.mark.parametrize("rot", ROTATIONS_360P, ids=str)
def test_warp_affine_cubic_u8_meets_reference(rot):
    """cv2.warpAffine(INTER_CUBIC, BORDER_REPLICATE) restated (frame_oracle.warp_affine_cubic_u8): |o - ref| <= 1 + L/32."""
    im = _frame360()
    A = F.rot_matrix_2x3(*rot)
    ref, L = S.warp_affine_cubic(im, A)
    _assert_within(F.warp_affine_cubic_u8(im, A), ref, S.bar_cubic_u8(L), str(rot))


@pytest.mark.parametrize("src,dst", RESIZES)
def test_resize_u8_meets_reference(src, dst):
    """cv2.resize(INTER_LINEAR) restated (frame_oracle.resize_linear_u8): |o - ref| <= 1 + L/256."""
    p = _square(1, src)
    ref, L = S.resize_linear(p, dst, dst)
    _assert_within(F.resize_linear_u8(p, dst, dst), ref, S.bar_resize_u8(L), f"{src}->{dst}")


@pytest.mark.parametrize("size,original", [(127, None), (255, None), (127, (40.2, 71.6))], ids=["127", "255", "127-offcentre"])
def test_log_polar_u8_meets_reference(size, original):
    """getPolarImg's cv2.logPolar restated (frame_oracle.get_polar_img): centre (S // 2, S // 2) or round(original),
    M = S / log(S / 2); |o - ref| <= 0.5 + L/32."""
    img = _square(6, size)
    ref, L = S.log_polar(img, _polar_center(size, original), size / math.log(size / 2))
    _assert_within(F.get_polar_img(img, original=original), ref, S.bar_bilinear_u8(L), f"S={size} original={original}")


def _polar_center(size, original):
    return (size // 2, size // 2) if original is None else tuple(float(v) for v in np.round(original))


F32_AFFINES = [np.array([[1, 0, 0], [0, 1, 0.0]]), np.array([[0.9, 0.1, 3.5], [-0.1, 0.9, 8.25]]), F.rot_matrix_2x3(63.0, 63.0, 0.7),
               F.rot_matrix_2x3(10.0, 100.0, -2.0), np.array([[1.3, 0.2, -20.0], [0.1, 0.7, 15.0]])]
F32_WARPS = [np.eye(3), np.array([[1.01, 0.02, -1.3], [0.03, 0.98, 2.2], [1e-4, -1e-4, 1.0]]),
             np.array([[0.95, -0.1, 9.0], [0.12, 1.04, -7.5], [-3e-4, 2e-4, 1.0]]), np.array([[1, 0, 0], [0, 1, 0], [0, -1 / 60, 1.0]])]


@pytest.mark.parametrize("kind", ["uniform", "normal"])
def test_float_warps_meet_reference(kind):
    """The float32 paths: get_mask_window's cv2.warpAffine (frame_oracle.warp_affine_linear_f32, BORDER_CONSTANT 0) and the
    refinement crop's cv2.warpPerspective (hdn_oracle.warp_perspective_replicate), 127 x 127, against cv_semantics.bar_float
    ((17/16) L/32 with L over the window plus one ring, plus float32 rounding)."""
    r = np.random.default_rng(5)
    img = (r.uniform(0, 1, (127, 127)) if kind == "uniform" else r.standard_normal((127, 127))).astype(np.float32)
    for A in F32_AFFINES:
        ref, L = S.warp_affine_linear_f32(img, A, 127, 127, ring=1)
        _assert_within(F.warp_affine_linear_f32(img, A, 127, 127), ref, S.bar_float(ref, L), str(A))
    for M in F32_WARPS:
        ref, L = S.warp_perspective(img, M, ring=1)
        _assert_within(O.warp_perspective_replicate(img, M), ref, S.bar_float(ref, L), str(M))


def _ulp_diff(got, want64):
    want = want64.astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(want), np.float32(1e-30)).astype(np.float32))
    return np.abs(np.asarray(got, np.float32).astype(np.float64) - want.astype(np.float64)) / ulp.astype(np.float64)


def test_perspective_transform_within_one_ulp():
    """cv2.perspectiveTransform restated (tracker_oracle.perspective_transform, float32 points, float64 matrix): <= 1 float32
    ulp of the float64 division, including points whose w is ~1e-3 .. 1e-15, below DBL_EPSILON and exactly 0."""
    r = np.random.default_rng(8)
    pts = r.uniform(-50, 1330, (64, 2)).astype(np.float32)
    for M in HOMOGRAPHIES + [HORIZON]:
        assert _ulp_diff(TO.perspective_transform(pts, M), S.perspective_transform(pts, M)).max() <= 1.0
    p = pts[:1].astype(np.float64)
    for w in (1e-3, 1e-8, 1e-12, 1e-15, 4e-16, 2e-16, 1e-17, 0.0, -3e-14):
        M = np.array([[0.9, 0.2, 30.0], [-0.15, 1.1, -12.0], [3e-4, 1e-4, 0.0]])
        M[2, 2] = w - (p[0, 0] * M[2, 0] + p[0, 1] * M[2, 1])
        want = S.perspective_transform(pts[:1], M)
        assert _ulp_diff(TO.perspective_transform(pts[:1], M), want).max() <= 1.0, w
        assert (want == 0).all() == (abs(p[0, 0] * M[2, 0] + p[0, 1] * M[2, 1] + M[2, 2]) <= S.DBL_EPSILON)


# ---------------------------------------------------------------------------------------- the bars fail on a wrong convention
def _case_warp(M, ref_M=None, **kw):
    im = _frame360()
    ref, L = S.warp_perspective(im, M if ref_M is None else ref_M, **kw)
    return F.warp_perspective_u8(im, M), ref, S.bar_bilinear_u8(L)


def _case_cubic(rot, shift=0.0, **kw):
    im = _frame360()
    A = F.rot_matrix_2x3(*rot)
    A_ref = (np.vstack([A, [0, 0, 1]]) @ _t(-shift, 0))[:2]      # samples src(A^-1 p + (shift, 0))
    ref, L = S.warp_affine_cubic(im, A_ref, **kw)
    return F.warp_affine_cubic_u8(im, A), ref, S.bar_cubic_u8(L)


def _case_resize(src, dst, **kw):
    p = _square(1, src)
    ref, L = S.resize_linear(p, dst, dst, **kw)
    return F.resize_linear_u8(p, dst, dst), ref, S.bar_resize_u8(L)


def _case_polar(size, original=None, swap=False, **kw):
    img = _square(6, size)
    c = _polar_center(size, original)
    ref, L = S.log_polar(img, c[::-1] if swap else c, size / math.log(size / 2), **kw)
    return F.get_polar_img(img, original=original), ref, S.bar_bilinear_u8(L)


def _shifted(M, dx, dy):
    """The matrix whose inverse map samples M^-1 p + (dx, dy): a sub-pixel error in the sampling position."""
    return M @ np.linalg.inv(_t(dx, dy))


H1, H4 = HOMOGRAPHIES[1], HOMOGRAPHIES[4]
MUTATIONS = {
    # name: (case builder, least share of values outside the bar); the shares measured on this data are in the comments
    "warp-shift-1/16px-H1": (lambda: _case_warp(H1, _shifted(H1, 1 / 16, 0)), 0.16),                     # 17 %
    "warp-shift-1/16px-rot45": (lambda: _case_warp(ROT45_360P, _shifted(ROT45_360P, 1 / 16, 0)), 0.16),   # 23 %
    "warp-shift-1/2px-H1": (lambda: _case_warp(H1, _shifted(H1, 0.5, 0.5)), 0.80),                        # 89 %
    "warp-shift-1/2px-rot45": (lambda: _case_warp(ROT45_360P, _shifted(ROT45_360P, 0.5, 0.5)), 0.80),     # 90 %
    "warp-forward-map": (lambda: _case_warp(HOMOGRAPHIES[2], np.linalg.inv(HOMOGRAPHIES[2])), 0.90),      # 99 %
    "warp-border-constant": (lambda: _case_warp(H4, border="constant"), 0.75),                            # 81 %
    "cubic-a=-0.5-rot0.3": (lambda: _case_cubic(ROTATIONS_360P[0], a=-0.5), 0.008),                       # 1.9 %
    "cubic-a=-0.5-rot-1.2": (lambda: _case_cubic(ROTATIONS_360P[1], a=-0.5), 0.008),                      # 0.83 %
    "cubic-shift-1/16px-rot0.3": (lambda: _case_cubic(ROTATIONS_360P[0], shift=1 / 16), 0.05),            # 6.4 %
    "cubic-shift-1/16px-rot-1.2": (lambda: _case_cubic(ROTATIONS_360P[1], shift=1 / 16), 0.05),           # 12 %
    "resize-corner-aligned-380-303": (lambda: _case_resize(380, 303, half_pixel=False), 0.65),            # 65.7 %
    "resize-corner-aligned-57-127": (lambda: _case_resize(57, 127, half_pixel=False), 0.80),              # 83 %
    "polar-radius-without-minus-1": (lambda: _case_polar(255, radius_offset=0.0), 0.90),                  # 90.4 %
    "polar-angle-flipped": (lambda: _case_polar(127, angle_sign=-1.0), 0.80),                             # 82 %
    "polar-cx-cy-swapped": (lambda: _case_polar(127, original=(40.2, 71.6), swap=True), 0.90),            # 98 %
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_bar_fails_on_wrong_convention(name):
    build, least = MUTATIONS[name]
    got, ref, bar = build()
    share = float(S.violations(got, ref, bar).mean())
    assert share >= least, f"{name}: only {share:.2%} of the values violate the bar (expected >= {least:.2%})"
