"""Device-resident frame handling for the tracker loop.

The reference handles every frame on the host (numpy + OpenCV) and uploads three crops per frame
(hdn/tracker/base_tracker.py:134-135,211-212); here the uint8 frame is uploaded ONCE and the crops / warps are kernels:

    upload(img)                                            np.uint8 [H,W,3] (BGR) -> device tensor
    get_subwindow(frame, pos, model_sz, original_sz, avg)  <- SiameseTracker.get_subwindow, base_tracker.py:61-136
    get_subwindow_for_homo(...)                            <- base_tracker.py:138-213 (also returns the crop points)
    get_search_info(frame, pos, original_sz, avg)          <- get_subwindow_for_homo + get_search_info (get_img_info.py:42-70), fused
    warp_perspective(frame, M)                             <- cv2.warpPerspective(img, M, BORDER_REPLICATE), hdn_tracker_proj_e2e.py:154
    rot_around_center(frame, cx, cy, rot)                  <- img_rot_around_center, hdn/utils/transform.py:69-100
    get_polar_img(patch) / get_subwindow(..., islog=1)     <- getPolarImg (cv2.logPolar), hdn/models/logpolar.py:11-29, base_tracker.py:119-126
    FrameArena(n, Hmax, Wmax)                              n slots holding frames of DIFFERENT sizes (the videos of a dataset, tools/test.py:91-103,
                                                           fed through the lock-step tracker): the crops / warps take it where they take [B,H,W,C]

Same argument meaning and return shapes as the reference's functions; `pos` / `original_sz` / matrices may be host numbers
(packed into a small device array without synchronising) or float64 device tensors (nothing leaves the device).  The parts
that are OpenCV in the reference are restatements (parity-unpinned, see include/hdn_hip.h).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib


def upload(img) -> torch.Tensor:
    """np.uint8 [H,W,C] (as cv2.imread returns it) -> contiguous uint8 device tensor; the one host->device copy of a frame."""
    if isinstance(img, torch.Tensor):
        t = img
    else:
        a = np.ascontiguousarray(img)
        if a.dtype != np.uint8 or a.ndim != 3:
            raise TypeError(f"expected a uint8 [H,W,C] frame, got {a.dtype} {a.shape}")
        t = torch.from_numpy(a)
    if t.dtype != torch.uint8 or t.dim() != 3:
        raise TypeError("expected a uint8 [H,W,C] frame")
    if not torch.cuda.is_available():
        raise _lib.HdnHipError("hdn_amd runs on the GPU only; there is no CPU fallback")
    return t.contiguous().cuda(non_blocking=True) if not t.is_cuda else t.contiguous()


def _check_frame(frame):
    """-> (H, W, C) of a frame [H,W,C], or of every frame of a batch [B,H,W,C] (B sequences in lock step: hdn_amd.batched_tracker)."""
    if not isinstance(frame, torch.Tensor) or frame.dtype != torch.uint8 or frame.dim() not in (3, 4) or not frame.is_cuda:
        raise _lib.HdnHipError("frame must be a uint8 [H,W,C] (or [B,H,W,C]) tensor on the GPU (hdn_amd.frame.upload); there is no CPU fallback")
    if not frame.is_contiguous():
        raise ValueError("frame must be contiguous")
    return frame.shape[-3:]


class FrameArena:
    """n slots of uint8 frames of different sizes in one device buffer: slot b holds a dense [H_b, W_b, C] frame at its start, the slots are
    `slot_stride` = Hmax * Wmax * C bytes apart, and `dims` is the DEVICE int32 [n, 2] table of (H_b, W_b) the ragged kernels read
    (hdn_*_ragged_*, include/hdn_hip.h).  Sizes therefore are data, not launch arguments: a captured hipGraph keeps replaying while set()
    changes a slot's frame size.  A slot that was never set has dims (0, 0) and is skipped by every kernel.

        set(b, img) / set_all(imgs)   np.uint8 [H,W,C] (or a uint8 tensor) -> slot b / every slot, through one pinned staging arena; a frame
                                      above the capacity raises before anything is written
        frame(b)                      the dense [H_b, W_b, C] view of slot b
        like()                        an empty arena of the same geometry sharing THIS `dims` tensor: what the warps return
    """

    def __init__(self, n: int, Hmax: int, Wmax: int, C: int = 3, device=None, _like=None):
        n, Hmax, Wmax, C = int(n), int(Hmax), int(Wmax), int(C)
        if n < 1 or Hmax < 1 or Wmax < 1 or C < 1:
            raise ValueError("FrameArena takes n, Hmax, Wmax, C >= 1")
        self.n, self.Hmax, self.Wmax, self.C = n, Hmax, Wmax, C
        self.slot_stride = Hmax * Wmax * C
        # (a host arena holds frames and checks sizes like a device one - what the host tests use - but no kernel takes it: there is no CPU fallback)
        self.device = _like.device if _like is not None else torch.device(device if device is not None else "cuda")
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.data = torch.empty((n, self.slot_stride), dtype=torch.uint8, device=self.device)
        if _like is None:
            self.dims = torch.zeros((n, 2), dtype=torch.int32, device=self.device)
            self._sizes = [(0, 0)] * n            # the host's copy of `dims` (shared with like(): one table, one copy)
        else:
            self.dims, self._sizes = _like.dims, _like._sizes
        self._staging = self._dims_staging = self._copy_done = None

    def like(self) -> "FrameArena":
        return FrameArena(self.n, self.Hmax, self.Wmax, self.C, _like=self)

    def size(self, b: int):
        """(H_b, W_b) of slot b as last set(); (0, 0): empty."""
        return self._sizes[b]

    def frame(self, b: int) -> torch.Tensor:
        H, W = self._sizes[b]
        if H < 1:
            raise ValueError(f"slot {b} of the arena holds no frame")
        return self.data[b, :H * W * self.C].view(H, W, self.C)

    def _checked(self, b, img):
        """-> (flat uint8 tensor, H, W) of a frame that fits slot b; raises before anything is written."""
        if not 0 <= b < self.n:
            raise IndexError(f"slot {b} of an arena of {self.n}")
        if not isinstance(img, torch.Tensor):
            img = np.asarray(img)
            if img.dtype != np.uint8:
                raise TypeError(f"slot {b}: expected a uint8 [H,W,{self.C}] frame, got {img.dtype} {img.shape}")
            img = torch.from_numpy(np.ascontiguousarray(img))
        t = img
        if t.dtype != torch.uint8 or t.dim() != 3:
            raise TypeError(f"slot {b}: expected a uint8 [H,W,{self.C}] frame, got {t.dtype} {tuple(t.shape)}")
        H, W, C = t.shape
        if C != self.C or H < 1 or W < 1 or H > self.Hmax or W > self.Wmax:
            raise ValueError(f"slot {b}: a frame of {H} x {W} x {C} does not fit the arena's capacity {self.Hmax} x {self.Wmax} x {self.C}")
        return t.contiguous().reshape(-1), H, W

    def _put(self, b, t, H, W):
        nb, pinned = H * W * self.C, self.data.is_cuda and not t.is_cuda
        if pinned and self._staging is None:
            self._staging = torch.empty((self.n, self.slot_stride), dtype=torch.uint8).pin_memory()
            self._dims_staging = torch.zeros((self.n, 2), dtype=torch.int32).pin_memory()
        if pinned:
            self._staging[b, :nb].copy_(t)
            t = self._staging[b, :nb]
        self.data[b, :nb].copy_(t, non_blocking=True)
        if self._sizes[b] != (H, W):
            rec = self._dims_staging[b] if self._dims_staging is not None else torch.empty(2, dtype=torch.int32)
            rec[0], rec[1] = H, W
            self.dims[b].copy_(rec, non_blocking=self._dims_staging is not None)
            self._sizes[b] = (H, W)

    def _wait(self):
        if self._copy_done is not None:
            self._copy_done.synchronize()          # the previous copies have left the staging arena
            self._copy_done = None

    def _guard(self):
        return _lib.device_guard(self.device) if self.data.is_cuda else _lib._NO_GUARD

    def _mark(self):
        if self._staging is not None:
            self._copy_done = torch.cuda.Event()
            self._copy_done.record()

    def set(self, b: int, img):
        """One frame -> slot b (and its dims record when the size changed)."""
        t, H, W = self._checked(b, img)
        self._wait()
        with self._guard():
            self._put(b, t, H, W)
            self._mark()

    def set_all(self, imgs):
        """n frames -> the n slots: every frame is checked before the first byte is written."""
        if len(imgs) != self.n:
            raise ValueError(f"this arena has {self.n} slots, got {len(imgs)} frames")
        checked = [self._checked(b, im) for b, im in enumerate(imgs)]
        self._wait()
        with self._guard():
            for b, (t, H, W) in enumerate(checked):
                self._put(b, t, H, W)
            self._mark()


def _arena_on_gpu(frame):
    if not frame.data.is_cuda:
        raise _lib.HdnHipError("the arena must be on the GPU; there is no CPU fallback")


def _batch(frame):
    """Number of frames a call works on: B of [B,H,W,C], n of an arena, 1 for a single frame."""
    if isinstance(frame, FrameArena):
        return frame.n
    return frame.shape[0] if frame.dim() == 4 else 1


def is_batched(frame) -> bool:
    """An arena or a [B,H,W,C] tensor (results carry a leading batch dimension) as opposed to one [H,W,C] frame."""
    return isinstance(frame, FrameArena) or frame.dim() == 4


def _arena_out(frame, out):
    if out is None:
        return frame.like()
    if (not isinstance(out, FrameArena) or (out.n, out.Hmax, out.Wmax, out.C) != (frame.n, frame.Hmax, frame.Wmax, frame.C)
            or out.dims is not frame.dims or out.device != frame.device):
        raise ValueError("out must be an arena made by like() of the input arena")
    return out


def _records(t, B, width, what):
    """A float64 device array of B parameter records of `width` doubles -> (tensor to keep alive, pointer, stride in doubles).  The records
    may be a column slice of a wider per-sequence array (state[:, 8:14]): only the rows' stride has to be uniform."""
    if t.dtype != torch.float64 or not t.is_cuda:
        raise TypeError(f"{what} must be a float64 GPU tensor")
    if t.dim() == 1 and B == 1:
        t = t.reshape(1, -1)
    if t.dim() != 2 or t.shape[0] != B or t.shape[1] != width or t.stride(1) != 1 or (B > 1 and t.stride(0) < width):
        raise ValueError(f"{what} must be [{B}, {width}] with unit column stride, got {tuple(t.shape)} strides {tuple(t.stride())}")
    return t, t.data_ptr(), (t.stride(0) if B > 1 else width)


def _dev_f64(values, dev) -> torch.Tensor:
    """Host numbers -> a small float64 device array (pinned-free async copy); device tensors pass through."""
    if isinstance(values, torch.Tensor):
        if values.dtype != torch.float64 or not values.is_cuda:
            raise TypeError("device-side parameters must be float64 GPU tensors")
        return values.contiguous().reshape(-1)
    return torch.tensor([float(v) for v in values], dtype=torch.float64).to(dev, non_blocking=True)


def crop_points(pos, original_sz, im_h, im_w):
    """(context_xmin, context_ymin, context_xmax + 1, context_ymax + 1) in the padded frame, as
    get_subwindow_for_homo returns them (base_tracker.py:150-167,213): host arithmetic on host numbers."""
    sz = float(original_sz)
    c = (sz - 1) / 2
    xmin = math.floor(pos[0] - c + 0.5)
    ymin = math.floor(pos[1] - c + 0.5)
    xmax, ymax = xmin + sz - 1, ymin + sz - 1
    left, top = int(max(0., -xmin)), int(max(0., -ymin))
    return (xmin + left, ymin + top, xmax + left + 1, ymax + top + 1)


def _subwindow(frame, pos, model_sz, original_sz, avg_chans, mode, params=None):
    if isinstance(frame, FrameArena):
        if params is None:
            raise ValueError("an arena of frames takes its crop parameters as a float64 device tensor [n, 3 + C] (`params`)")
        _arena_on_gpu(frame)
        B, C, dev, m = frame.n, frame.C, frame.device, int(model_sz)
        keep, pp, stride = _records(params, B, 3 + C, "params")
        out = torch.empty((B, 1 if mode else C, m, m), dtype=torch.float32, device=dev)
        _lib.launch("get_subwindow", dev, _lib.load().hdn_subwindow_ragged_f32, _lib.ptr(frame.data), frame.slot_stride, _lib.ptr(frame.dims), pp, stride,
                    _lib.ptr(out), B, frame.Hmax, frame.Wmax, C, m, mode)
        return out
    H, W, C = _check_frame(frame)
    dev = frame.device
    B = frame.shape[0] if frame.dim() == 4 else 1
    if params is None:
        if B != 1:
            raise ValueError("a batch of frames takes its crop parameters as a float64 device tensor [B, 3 + C] (`params`)")
        params = _dev_f64([pos[0], pos[1], original_sz] + [float(a) for a in np.asarray(avg_chans).reshape(-1)], dev)
    if B == 1 and params.numel() != 3 + C:
        raise ValueError(f"params must be [cx, cy, original_sz, avg x {C}]")
    keep, pp, stride = _records(params, B, 3 + C, "params")
    m = int(model_sz)
    out = torch.empty((B, 1 if mode else C, m, m), dtype=torch.float32, device=dev)
    _lib.launch("get_subwindow", dev, _lib.load().hdn_subwindow_batch_f32, _lib.ptr(frame), pp, stride, _lib.ptr(out), B, H, W, C, m, mode)
    return out


def get_subwindow(frame, pos, model_sz, original_sz, avg_chans, params=None, islog: int = 0):
    """-> float32 [1, C, model_sz, model_sz] (uint8-valued), on the device; islog=1 appends the C log-polar channels
    (np.concatenate((im_patch, getPolarImg(im_patch)), 2), base_tracker.py:119-126) -> [1, 2C, model_sz, model_sz].
    A batch of frames [B,H,W,C] (or a FrameArena of n frames of different sizes) with `params` [B, 3 + C] gives [B, ...]: one launch,
    frame b cut with record b."""
    out = _subwindow(frame, pos, model_sz, original_sz, avg_chans, 0, params)
    if islog == 1:
        return torch.cat([out, get_polar_img(out)], dim=1)
    if islog:
        raise NotImplementedError("islog=2 (cv2.linearPolar) is not used by the shipped tracker configuration")
    return out


def log_polar_maps(w: int, h: int, center, M: float):
    """(mapx, mapy) float32 [h, w] of cv2.logPolar(src, center, M, flags) = cv::warpPolar(src, size(src), center, exp(w / M),
    flags | WARP_POLAR_LOG) as OpenCV >= 3.4.2 / 4.x builds them (imgwarp.cpp): rho along x, angle along y, all in double,
    stored as float."""
    max_radius = math.exp(w / M) if M > 0 else 1.0
    kangle = 2.0 * math.pi / h
    kmag = math.log(max_radius) / w
    rhos = (np.exp(np.arange(w, dtype=np.float64) * kmag) - 1.0).astype(np.float32).astype(np.float64)
    ang = kangle * np.arange(h, dtype=np.float64)
    mx = (rhos[None, :] * np.cos(ang)[:, None] + float(center[0])).astype(np.float32)
    my = (rhos[None, :] * np.sin(ang)[:, None] + float(center[1])).astype(np.float32)
    return mx, my


_polar_maps = {}


def get_polar_img(patch: torch.Tensor, original=None) -> torch.Tensor:
    """getPolarImg (hdn/models/logpolar.py:11-29) on a device crop [1, C, S, S] (uint8-valued float32): cv2.logPolar about
    (S // 2, S // 2) (or round(original)) with M = S / log(S / 2), INTER_LINEAR, outliers filled with 0.  Restated OpenCV."""
    if patch.dim() != 4 or patch.dtype != torch.float32:
        raise ValueError("get_polar_img takes a float32 [B, C, H, W] crop")
    dev = _lib.require_device(patch)
    Bp, C, H, W = patch.shape
    C = Bp * C          # the maps are the same for every plane: a batch of crops is just more planes
    center = (float(np.round(original[0])), float(np.round(original[1]))) if original is not None else (float(H // 2), float(W // 2))
    key = (dev, H, W, center)
    if key not in _polar_maps:
        mx, my = log_polar_maps(W, H, center, W / math.log(W / 2))
        _polar_maps[key] = (torch.from_numpy(mx).to(dev), torch.from_numpy(my).to(dev))
    mx, my = _polar_maps[key]
    src = patch.detach().contiguous()
    out = torch.empty_like(src)
    _lib.launch("get_polar_img", dev, _lib.load().hdn_remap_linear_f32, _lib.ptr(src), _lib.ptr(mx), _lib.ptr(my), _lib.ptr(out), C, H, W, H, W)
    return out


def get_subwindow_for_homo(frame, pos, model_sz, original_sz, avg_chans, islog: int = 0):
    H, W, _ = _check_frame(frame)
    return get_subwindow(frame, pos, model_sz, original_sz, avg_chans, islog=islog), crop_points(pos, original_sz, H, W)


def get_search_info(frame, pos, original_sz, avg_chans, model_sz: int = 127, params=None):
    """The normalised gray crop the homography head consumes, [1, 1, 127, 127] float32 on the device: get_subwindow_for_homo
    followed by get_search_info's (x - mean) / std, channel mean (float64), in one kernel."""
    return _subwindow(frame, pos, model_sz, original_sz, avg_chans, 1, params)


def _matrices(frame, M, width, what):
    """M -> (B, keep, pointer, stride).  At B = 1 a device tensor may have any shape holding `width` values ([3, 3], [9],
    [2, 3], ...); a [1, width] row, possibly a column slice of a wider per-sequence array, is passed with its own stride."""
    B = _batch(frame)
    if isinstance(M, torch.Tensor):
        m = M
        if B == 1:
            if M.numel() != width:
                raise ValueError(f"M must be {what}")
            if not (M.dim() == 2 and M.shape[0] == 1):
                m = M.contiguous().reshape(1, width)
    else:
        a = np.asarray(M, np.float64)
        if a.size != B * width:
            raise ValueError(f"M must be {what}" + (f" per frame ({B} frames)" if B > 1 else ""))
        m = _dev_f64(a.reshape(-1), frame.device).reshape(B, width)
    return (B,) + _records(m, B, width, "M")


def _warp_ragged(frame, M, width, what, entry, name, out):
    _arena_on_gpu(frame)
    B, keep, mp, stride = _matrices(frame, M, width, what)
    out = _arena_out(frame, out)
    _lib.launch(name, frame.device, getattr(_lib.load(), entry), _lib.ptr(frame.data), frame.slot_stride, _lib.ptr(frame.dims), mp, stride, _lib.ptr(out.data),
                B, frame.Hmax, frame.Wmax, frame.C)
    return out


def warp_perspective(frame, M, out=None):
    """cv2.warpPerspective(frame, M, (W, H), borderMode=cv2.BORDER_REPLICATE); M: 3x3 (host array or float64 device tensor).
    A batch [B,H,W,C] takes B matrices [B, 9] (rows of a wider float64 device array are fine) and is one launch.
    A FrameArena takes n matrices the same way, every slot warped at its own size, and returns an arena (`out`, or frame.like())."""
    if isinstance(frame, FrameArena):
        return _warp_ragged(frame, M, 9, "3x3", "hdn_frame_warp_perspective_ragged_u8", "warp_perspective", out)
    if out is not None:
        raise ValueError("`out` is for arenas")
    H, W, C = _check_frame(frame)
    B, keep, mp, stride = _matrices(frame, M, 9, "3x3")
    out = torch.empty_like(frame)
    _lib.launch("warp_perspective", frame.device, _lib.load().hdn_frame_warp_perspective_batch_u8, _lib.ptr(frame), mp, stride, _lib.ptr(out), B, H, W, C)
    return out


def warp_affine_cubic(frame, M, out=None):
    """cv2.warpAffine(frame, M, (W, H), flags=cv2.INTER_CUBIC, borderMode=cv2.BORDER_REPLICATE); M: 2x3 (a batch or an arena: [B, 6])."""
    if isinstance(frame, FrameArena):
        return _warp_ragged(frame, M, 6, "2x3", "hdn_frame_warp_affine_cubic_ragged_u8", "warp_affine_cubic", out)
    if out is not None:
        raise ValueError("`out` is for arenas")
    H, W, C = _check_frame(frame)
    B, keep, mp, stride = _matrices(frame, M, 6, "2x3")
    out = torch.empty_like(frame)
    _lib.launch("warp_affine_cubic", frame.device, _lib.load().hdn_frame_warp_affine_cubic_batch_u8, _lib.ptr(frame), mp, stride, _lib.ptr(out), B, H, W, C)
    return out


def rot_around_center(frame, cx, cy, rot):
    """img_rot_around_center(img, cx, cy, w, h, rot) (hdn/utils/transform.py:69-100): rotation about (cx, cy), bicubic."""
    cc, ss = math.cos(rot), math.sin(rot)
    return warp_affine_cubic(frame, [cc, -ss, cx - cx * cc + cy * ss, ss, cc, cy - cy * cc - cx * ss])
