"""What the tracker loops share on the host side of a launch (hdn_amd.tracker, .batched_tracker, .simi_tracker, .graph): hipGraph capture with
its eager fallback, the set-up of a reference ModelBuilder for the Device* classes, the per-step frame upload, and the decoding of the device
records into the reference's result dictionaries.  Plain functions and one small class; nothing here launches a kernel of its own."""
from __future__ import annotations

import contextlib
import os
import warnings

import numpy as np
import torch

from . import _lib


# ------------------------------------------------------------------------------------------------------ capture
def capture_graph(body, restore=(), label: str = "per-frame", hook=None, fallback: bool = True, warmup: int = 3):
    """body() captured as one hipGraph -> (graph, what body returned inside the capture).  `warmup` runs on a side stream first (MIOpen
    find, lazy initialisations); the tensors in `restore`, which those runs and the capture advance, are put back afterwards.  hook(body),
    when given, runs in place of body() inside the capture.  Stream capture reports what it cannot hold (e.g. a model whose forward makes
    host round trips) as a RuntimeError: with `fallback` that is a warning and -> None, and the caller launches the same kernels one by one.
    Anything else is a real error and propagates."""
    snap = [t.clone() for t in restore]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    try:
        with torch.cuda.stream(side):
            for _ in range(warmup):
                body()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = body() if hook is None else hook(body)
        return graph, out
    except RuntimeError as e:
        if not fallback:
            raise
        warnings.warn(f"hdn_amd: the {label} body could not be captured as a hipGraph ({type(e).__name__}: {e}); running it eagerly")
        return None
    finally:
        torch.cuda.current_stream().wait_stream(side)
        for live, s in zip(restore, snap):
            live.copy_(s)


# ------------------------------------------------------------------------------------------------------ device model set-up
def env_flag(name: str, default: str = "1") -> bool:
    """An on / off switch of the environment: unset -> `default`; "" and "0" are off, anything else is on."""
    return os.environ.get(name, default) not in ("", "0")


def reference_config():
    """-> (TrackerConfig, the reference's cfg node or None): from hdn.core.config.cfg after tools/test.py merged the YAML (incl.
    cfg.BAN.KWARGS.cls_out_channels: 2 = softmax, 1 = sigmoid decode); the defaults where the reference is not importable or lacks a field."""
    from .similarity import TrackerConfig
    try:
        from hdn.core.config import cfg as ref_cfg
        return TrackerConfig.from_reference(ref_cfg), ref_cfg
    except (ImportError, AttributeError):
        return TrackerConfig(), None


@contextlib.contextmanager
def only_benchmark():
    # torch.backends.cudnn.flags() sets EVERY flag (the ones not named fall to its defaults: deterministic=False, allow_tf32=True), which
    # would override a user's settings for the backbone's convolutions and bake them into the captured graph.  Only `benchmark` is touched.
    before = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = True
    try:
        yield
    finally:
        torch.backends.cudnn.benchmark = before


def find_mode(enabled: bool):
    """MIOpen find mode (torch.backends.cudnn.benchmark) around a tracker's own calls, or nothing.  The flag is process-global in torch, so it
    is raised only there (init / track_new / reinit, incl. the graph capture) and put back afterwards: other models keep their setting."""
    return only_benchmark() if enabled else contextlib.nullcontext()


def prepare_model(model, fold_backbone=None):
    """model.eval(), then -> (miopen_find, folded).  The backbone's convolutions are PyTorch-ROCm's and their shapes are fixed for a whole
    sequence, so MIOpen searches for its kernels once (find_mode; 2.9 against 4.5 ms per frame with the production-shaped model; the
    reference's scripts leave torch's default, off, and HDN_MIOPEN_FIND=0 does too).  Their BatchNorm / ReLU / add launches (a third of the
    B = 1 frame) are folded away (hdn_amd.backbone; fold_backbone=False or HDN_FOLD_BACKBONE=0: left as they are)."""
    from . import backbone as BB
    model.eval()
    miopen_find = env_flag("HDN_MIOPEN_FIND") and next(model.parameters()).is_cuda
    folded = BB.optimize_similarity_model(model) if (BB.enabled() if fold_backbone is None else fold_backbone) else []
    return miopen_find, folded


def device_setup(model, cfg, graph, fold_backbone):
    """What the Device* constructors do first -> (cfg, the reference's cfg node or None, graph, miopen_find, folded): cfg None = the reference's
    configuration (the node is looked up only then), graph None = HDN_TRACKER_GRAPH, then prepare_model."""
    ref_cfg = None
    if cfg is None:
        cfg, ref_cfg = reference_config()
    if graph is None:
        graph = env_flag("HDN_TRACKER_GRAPH")
    return (cfg, ref_cfg, graph) + prepare_model(model, fold_backbone)


def validate_frame_capacity(frame_capacity):
    """None, or (Hmax, Wmax) as a pair of ints >= 1."""
    if frame_capacity is None:
        return None
    cap = (int(frame_capacity[0]), int(frame_capacity[1]))
    if min(cap) < 1:
        raise ValueError("frame_capacity must be (Hmax, Wmax) >= 1")
    return cap


# ------------------------------------------------------------------------------------------------------ frames: one upload per step
class FrameUploader:
    """The n frames of a step -> ONE uint8 device tensor [n,H,W,3].  A list of numpy frames goes through one pinned staging buffer (kept
    from step to step) and one asynchronous copy; a stacked uint8 tensor (pageable, pinned or already on the device) is copied / used as it is."""

    def __init__(self, n: int):
        self.n, self._staging, self._copy_done = int(n), None, None

    def __call__(self, imgs, dev, into=None):
        """-> the frames on `dev`, or copied into `into` (the static input of a captured graph).  Every check comes before the first CUDA call."""
        n, t = self.n, imgs
        if isinstance(imgs, torch.Tensor):
            if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[0] != n:
                raise TypeError(f"expected a uint8 [{n},H,W,C] tensor of frames, got {t.dtype} {tuple(t.shape)}")
        else:
            if len(imgs) != n:
                raise ValueError(f"this tracker advances {n} sequences per step, got {len(imgs)} frames")
            frames = [np.asarray(im) for im in imgs]
            a0 = frames[0]
            if a0.dtype != np.uint8 or a0.ndim != 3:
                raise TypeError(f"expected uint8 [H,W,C] frames, got {a0.dtype} {a0.shape}")
            for b, im in enumerate(frames):
                if im.shape != a0.shape or im.dtype != np.uint8:
                    raise ValueError(f"all frames of a step must be uint8 {a0.shape} (they share one buffer); frame {b} is {im.dtype} {im.shape}")
        if not torch.cuda.is_available():
            raise _lib.HdnHipError("hdn_amd runs on the GPU only; there is no CPU fallback")
        if not isinstance(imgs, torch.Tensor):
            if self._staging is None or tuple(self._staging.shape) != (n,) + a0.shape:
                self._staging = torch.empty((n,) + a0.shape, dtype=torch.uint8).pin_memory()
                self._copy_done = None
            if self._copy_done is not None:
                self._copy_done.synchronize()          # the previous step's copy has left the staging buffer
            host = self._staging.numpy()
            for b, im in enumerate(frames):
                host[b] = im
            t = self._staging
        if into is not None:
            if tuple(t.shape) != tuple(into.shape):
                raise ValueError(f"graph mode was captured for uint8 frames of shape {tuple(into.shape)}, got {tuple(t.shape)}")
            into.copy_(t, non_blocking=True)
            dst = into
        else:
            dst = t.contiguous() if t.is_cuda else t.contiguous().to(dev, non_blocking=True)
        if t is self._staging:
            self._copy_done = torch.cuda.Event()
            self._copy_done.record()
        return dst


def upload_arena(arena, imgs, same_size: bool):
    """A list of n frames -> the slots of `arena` (hdn_amd.frame.FrameArena); same_size: every frame must have its slot's current size (a step of
    running sequences).  Every frame is checked before the first byte is written."""
    n = arena.n
    if isinstance(imgs, torch.Tensor) or len(imgs) != n:
        raise ValueError(f"this tracker advances {n} sequences per step and takes a list of {n} frames (each of its slot's size)")
    if same_size:
        for b, im in enumerate(imgs):
            if tuple(im.shape[:2]) != arena.size(b):
                raise ValueError(f"slot {b} runs a sequence of {arena.size(b)} frames, got a frame of {tuple(im.shape[:2])}; "
                                 "a slot changes its frame size in reinit() only")
    arena.set_all(imgs)
    return arena


# ------------------------------------------------------------------------------------------------------ device records -> result dictionaries
def homography_result(row, n_points: int) -> dict:
    """hdnTrackerHomo.track_new's dictionary from one host row of `out` (float32 [2 * points + 1]: the corners (x, y), then best_score)."""
    pn, best_score = row[:2 * n_points].reshape(n_points, 2), row[2 * n_points]
    mx, mn = pn.max(0), pn.min(0)
    bbox = [mn[0], mn[1], mx[0] - mn[0], mx[1] - mn[1]]
    return {"bbox_aligned": bbox, "best_score": best_score, "polygon": pn, "points": pn, "bbox": bbox}


def similarity_result(h) -> dict:
    """hdnTracker.track_new's dictionary (hdn_tracker.py:295-301) from one host row of hdn_simi_track_update_f64's `out` (float64 [20])."""
    return {"bbox": list(h[0:4]), "bbox_aligned": list(h[4:8]), "best_score": np.float32(h[8]), "rot": h[9], "polygon": h[10:18].reshape(4, 2).copy()}


def track_state_row(t) -> dict:
    """One host row of the similarity tracker's `track` record as the attributes the reference keeps on the host (center_pos, size, rot, ...)."""
    return {"center_pos": t[0:2].copy(), "size": t[2:4].copy(), "rot": float(t[4]), "lp_shift": [0, float(t[5])], "scale": float(t[6]), "v": float(t[7]),
            "window_scale_factor": float(t[8]), "lost_count": int(t[9]), "last_lost": bool(t[10]), "rot_is_float32": bool(t[11]),
            "lp_shift_is_float32": bool(t[12]), "frames": int(t[13])}
