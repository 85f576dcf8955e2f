"""TEST INFRASTRUCTURE ONLY: the six OpenCV entry points of the tracker loop stated from their documented mathematical
definitions, in float64 with continuous coordinates.

This module is the independent side of tests/test_opencv_semantics.py and of the reference-level checks in
tests/test_gpu_frame.py.  It deliberately shares nothing with oracle/frame_oracle.py, oracle/hdn_oracle.py or hdn_amd:
no fixed-point weights, no 1/32-px tables, no block walks, matrix inverses by np.linalg.inv.  A convention error common to
the oracle and the kernels (half-pixel centres, the cubic's `a`, the log-polar radius, ...) therefore shows up as a
per-pixel violation of the bars below instead of passing unseen.

Every sampler returns (value, L).  L is the local tap range: the largest absolute difference between two horizontally or
vertically neighbouring taps of the interpolation window (2 x 2 bilinear, 4 x 4 cubic), per output value.  The fixed-point
implementations quantise the source coordinate to 1/32 px, i.e. move it by at most 1/64 px per axis; inside one cell the
interpolant's slope along an axis is at most L, so that quantisation moves the value by at most 2 * L / 64 = L / 32.  The
tests' bars are built on that.  `ring` widens the window used for L by that many taps on every side (the value is
unchanged); a bound that has to cover a quantised coordinate falling into the neighbouring cell uses ring=1.

Keyword arguments spell out the conventions; their defaults are OpenCV's.  The tests change them only to show that a
wrong convention breaks the bars.
"""
from __future__ import annotations

import numpy as np

DBL_EPSILON = float(np.finfo(np.float64).eps)


def _as_hwc(img):
    a = np.asarray(img, np.float64)
    return (a[:, :, None], True) if a.ndim == 2 else (a, False)


def _keys(s, a):
    """Keys' cubic convolution kernel with parameter a at signed distance s."""
    s = np.abs(s)
    near = ((a + 2) * s - (a + 3)) * s * s + 1
    far = ((a * s - 5 * a) * s + 8 * a) * s - 4 * a
    return np.where(s <= 1, near, np.where(s < 2, far, 0.0))


def _sample(img, X, Y, *, cubic=False, a=-0.75, border="replicate", ring=0):
    """Interpolate HxWxC float64 `img` at float64 source coordinates (X, Y) (pixel centres at integers).
    -> (value [..., C], L [..., C])."""
    if border not in ("replicate", "constant"):
        raise ValueError(border)
    H, W = img.shape[:2]
    # coordinates far outside the image give the same taps as coordinates a few pixels outside: keep them finite
    X = np.clip(X, -8.0 - ring, W + 7.0 + ring)
    Y = np.clip(Y, -8.0 - ring, H + 7.0 + ring)
    x0, y0 = np.floor(X), np.floor(Y)
    fx, fy = X - x0, Y - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    lo, hi = (-1, 2) if cubic else (0, 1)
    if cubic:
        wx = {k: _keys(k - fx, a) for k in range(lo, hi + 1)}
        wy = {k: _keys(k - fy, a) for k in range(lo, hi + 1)}
    else:
        wx, wy = {0: 1.0 - fx, 1: fx}, {0: 1.0 - fy, 1: fy}
    val = np.zeros(X.shape + (img.shape[2],))
    L = np.zeros_like(val)
    prev = None
    for dy in range(lo - ring, hi + ring + 1):
        yy = y0 + dy
        row = []
        for dx in range(lo - ring, hi + ring + 1):
            xx = x0 + dx
            t = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
            if border == "constant":
                t = t * ((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W))[..., None]
            if lo <= dy <= hi and lo <= dx <= hi:
                val += (wy[dy] * wx[dx])[..., None] * t
            if row:
                np.maximum(L, np.abs(t - row[-1]), out=L)
            if prev is not None:
                np.maximum(L, np.abs(t - prev[len(row)]), out=L)
            row.append(t)
        prev = row
    return val, L


def _out(v, L, flat):
    return (v[:, :, 0], L[:, :, 0]) if flat else (v, L)


def _apply(Minv, w_out, h_out):
    """Destination pixel centres (x, y) -> source (X, Y) = Minv . (x, y, 1) after the perspective divide; w == 0 -> (0, 0)."""
    y, x = np.mgrid[0:h_out, 0:w_out].astype(np.float64)
    w = Minv[2, 0] * x + Minv[2, 1] * y + Minv[2, 2]
    safe = np.where(w != 0.0, w, 1.0)
    X = np.where(w != 0.0, (Minv[0, 0] * x + Minv[0, 1] * y + Minv[0, 2]) / safe, 0.0)
    Y = np.where(w != 0.0, (Minv[1, 0] * x + Minv[1, 1] * y + Minv[1, 2]) / safe, 0.0)
    return X, Y


def _affine3(A):
    return np.vstack([np.asarray(A, np.float64).reshape(2, 3), [0.0, 0.0, 1.0]])


def warp_perspective(img, M, *, border="replicate", ring=0):
    """cv2.warpPerspective(img, M, (W, H), INTER_LINEAR, borderMode=BORDER_REPLICATE), output the size of the input.
    dst(x, y) = src(M^-1 . (x, y, 1)) after the perspective divide (M is the forward map and is inverted).
    Pixel centres are the integer coordinates.
    Bilinear interpolation on the 2 x 2 taps around the source point.
    BORDER_REPLICATE: taps outside the image take the nearest edge pixel (border="constant": they count as 0).
    A destination pixel whose w is exactly 0 samples source (0, 0), as OpenCV's `W ? 1/W : 0` does.
    No rounding or saturation: the value is the ideal one."""
    a, flat = _as_hwc(img)
    X, Y = _apply(np.linalg.inv(np.asarray(M, np.float64).reshape(3, 3)), a.shape[1], a.shape[0])
    return _out(*_sample(a, X, Y, border=border, ring=ring), flat)


def warp_affine_cubic(img, A, *, a=-0.75, border="replicate"):
    """cv2.warpAffine(img, A, (W, H), flags=INTER_CUBIC, borderMode=BORDER_REPLICATE) for uint8 images.
    A (2 x 3) is the forward map and is inverted: dst(x, y) = src(A^-1 . (x, y, 1)).
    Pixel centres are the integer coordinates.
    Keys' cubic convolution kernel with a = -0.75 (OpenCV's value; Keys' own paper and most libraries use -0.5).
    4 x 4 taps at floor(X) - 1 .. floor(X) + 2 per axis, separable weights.
    BORDER_REPLICATE: taps outside the image take the nearest edge pixel.
    The value is saturated to [0, 255] (not rounded)."""
    im, flat = _as_hwc(img)
    X, Y = _apply(np.linalg.inv(_affine3(A)), im.shape[1], im.shape[0])
    v, L = _sample(im, X, Y, cubic=True, a=a, border=border)
    return _out(np.clip(v, 0.0, 255.0), L, flat)


def warp_affine_linear_f32(img, A, dw, dh, *, border="constant", ring=0):
    """cv2.warpAffine(img, A, (dw, dh)) with the default flags, for a float image.
    A (2 x 3) is the forward map and is inverted: dst(x, y) = src(A^-1 . (x, y, 1)).
    Pixel centres are the integer coordinates.
    Bilinear interpolation on the 2 x 2 taps around the source point.
    BORDER_CONSTANT with value 0: taps outside the image count as 0."""
    im, flat = _as_hwc(img)
    X, Y = _apply(np.linalg.inv(_affine3(A)), int(dw), int(dh))
    return _out(*_sample(im, X, Y, border=border, ring=ring), flat)


def resize_source_coords(n_src, n_dst, *, half_pixel=True):
    """Source coordinate of every destination index d along one axis of cv2.resize(INTER_LINEAR):
    (d + 0.5) * n_src / n_dst - 0.5 (pixel centres aligned; half_pixel=False: d * n_src / n_dst, corners aligned),
    clamped to [0, n_src - 1]."""
    d = np.arange(int(n_dst), dtype=np.float64)
    s = n_src / float(n_dst)
    f = (d + 0.5) * s - 0.5 if half_pixel else d * s
    return np.clip(f, 0.0, n_src - 1.0)


def resize_linear(img, dw, dh, *, half_pixel=True):
    """cv2.resize(img, (dw, dh)) with INTER_LINEAR.
    Source coordinate per axis: (d + 0.5) * s / d' - 0.5 for destination index d, source size s, destination size d'.
    That coordinate is clamped to [0, n - 1] per axis (n = source size along the axis).
    Bilinear interpolation on the 2 x 2 taps around the source point (separable)."""
    im, flat = _as_hwc(img)
    xs = resize_source_coords(im.shape[1], dw, half_pixel=half_pixel)
    ys = resize_source_coords(im.shape[0], dh, half_pixel=half_pixel)
    X, Y = np.broadcast_to(xs[None, :], (int(dh), int(dw))), np.broadcast_to(ys[:, None], (int(dh), int(dw)))
    return _out(*_sample(im, X, Y, border="replicate"), flat)


def log_polar(img, center, M, *, radius_offset=1.0, angle_sign=1.0):
    """cv2.logPolar(img, center, M, INTER_LINEAR + WARP_FILL_OUTLIERS), output the size of the input (H rows, W columns).
    Column rho -> radius r = exp(rho / M) - 1.
    The "- 1" is OpenCV's implementation (warpPolar, OpenCV >= 3.4.2); the published formula rho = M * log(r) omits it.
    Row phi -> angle 2 pi * phi / H, turning from +x towards +y (row H / 4 looks along +y, i.e. down the image).
    Source point x = cx + r cos(angle), y = cy + r sin(angle), center = (cx, cy).
    Bilinear interpolation on the 2 x 2 taps around the source point.
    Taps outside the image count as 0 (WARP_FILL_OUTLIERS with a constant border 0)."""
    im, flat = _as_hwc(img)
    H, W = im.shape[:2]
    r = np.exp(np.arange(W, dtype=np.float64) / float(M)) - radius_offset
    ang = angle_sign * 2.0 * np.pi * np.arange(H, dtype=np.float64) / H
    X = float(center[0]) + r[None, :] * np.cos(ang)[:, None]
    Y = float(center[1]) + r[None, :] * np.sin(ang)[:, None]
    return _out(*_sample(im, X, Y, border="constant"), flat)


def perspective_transform(pts, H):
    """cv2.perspectiveTransform(pts, H) for float points [N, 2] -> float64 [N, 2].
    (x', y') = (H0 . p, H1 . p) / (H2 . p) with p = (x, y, 1), all in float64, a true division.
    The result is (0, 0) when |H2 . p| <= DBL_EPSILON."""
    H = np.asarray(H, np.float64).reshape(3, 3)
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    w = p[:, 0] * H[2, 0] + p[:, 1] * H[2, 1] + H[2, 2]
    ok = np.abs(w) > DBL_EPSILON
    safe = np.where(ok, w, 1.0)
    x = (p[:, 0] * H[0, 0] + p[:, 1] * H[0, 1] + H[0, 2]) / safe
    y = (p[:, 0] * H[1, 0] + p[:, 1] * H[1, 1] + H[1, 2]) / safe
    return np.stack([np.where(ok, x, 0.0), np.where(ok, y, 0.0)], 1)


# --------------------------------------------------------------------------------------------------------------- bars
def bar_bilinear_u8(L):
    """uint8 bilinear through 1/32-px coordinates (warpPerspective, logPolar): L / 32 from the coordinate, 0.5 from
    rounding the result to an integer."""
    return 0.5 + L / 32.0


def bar_cubic_u8(L):
    """uint8 bicubic through 1/32-px coordinates (warpAffine INTER_CUBIC): L / 32 from the coordinate; 0.5 from rounding
    plus 0.5 for the 15-bit weight table, whose entries are rounded and then forced to sum to 1."""
    return 1.0 + L / 32.0


def bar_resize_u8(L):
    """uint8 INTER_LINEAR resize: 11-bit weights (L / 2048 per axis, with margin L / 256) and the two truncating shifts
    of the vertical pass plus the final rounding (at most 1)."""
    return 1.0 + L / 256.0


def bar_float(ref, L):
    """float32 bilinear through 1/32-px coordinates (the f32 warpAffine and warpPerspective), with L taken with ring=1.
    Coordinate: the 1/32-px rounding moves it by <= 1/64 px per axis; warpAffine's 1/1024-px walk adds two roundings of
    <= 1/2048 px each, so <= 1/64 + 1/1024 = 17/1024 px per axis (warpPerspective, <= 1/64, is covered too).  The
    interpolant is piecewise bilinear with slope <= L per axis over the cells the moved coordinate can reach (ring=1:
    the quantised point may fall into a neighbouring cell), so the value moves by <= 2 * 17/1024 * L = (17/16) L / 32.
    float32 rounding: four float32 weight products, four tap products and three additions, each a relative error of
    at most 2^-24 on terms bounded by the largest tap; every tap lies within 2 L of the ideal value (two neighbour
    steps across a 2 x 2 window), so <= 11 * 2^-24 * (|ref| + 2 L); 16 * 2^-24 is used."""
    return (17.0 / 16.0) * L / 32.0 + 16.0 * 2.0 ** -24 * (np.abs(ref) + 2.0 * L)


def violations(got, ref, bar):
    """Boolean mask of the values of `got` farther from the reference `ref` than their per-value bar."""
    return np.abs(np.asarray(got, np.float64) - ref) > bar

