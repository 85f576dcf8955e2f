"""TRACKS['hdnTracker'] on the device: the similarity-only tracker with a per-frame template refresh.

    SimiTracker.init(img, bbox, poly, first_point)          <- hdnTracker.init,            hdn/tracker/hdn_tracker.py:109-154
    SimiTracker.track_new(fr_idx, img, gt_box, gt_poly)     <- hdnTracker.track_new,       hdn_tracker.py:174-301
    (inside track_new)                                       <- hdnTracker.update_template, hdn_tracker.py:156-162
    DeviceTrackerSimi(model)                                 <- the class hdn/tracker/tracker_builder.py:13 registers as TRACKS['hdnTracker']
                                                               (cfg.TRACK.TYPE's default, hdn/core/config.py:517; experiments/siamban_r50_l234_pot)

What the reference's loop does per frame: a search crop about the CURRENT centre with a side that follows the current size
(:176-192), ModelBuilder.track_new, numpy decode, a second crop about the moved centre, track_new_lp, numpy decode, the size / rotation /
scale recurrences and the result polygon in numpy (:213-281) — then update_template: the FIRST frame rotated by the accumulated
rotation (cv2.warpAffine, bicubic, full frame), cropped (+ cv2.logPolar channels) and pushed through ModelBuilder.template again
(two more backbone passes).  Four .cpu().numpy() reads, three crop uploads and a full-frame host warp per frame.

Here: one upload of the uint8 frame, the crops / the rotation of the resident first frame as kernels (hdn_amd.frame), the two decodes
(hdn_similarity_*_f32, given THIS frame's centre / s_z / s_x record), ONE one-lane kernel for everything between the second decode and
the next frame's first crop (hdn_simi_track_update_f64: recurrences, clamps, polygon, update_template's matrix, next s_z / s_x), and one
host read of 20 doubles — or none (`sync=False`).  The networks are the model's own (PyTorch-ROCm backbone / necks, the packed heads
around the HIP correlations).  Template features live in static buffers that the refresh overwrites in place, so a frame replays as one
hipGraph (`graph=True`) and the heads' template cache sees the change through the tensors' version counters.

BatchedSimiTracker runs n sequences in lock step; with frame_capacity=(Hmax, Wmax) every slot has its own frame size (the update kernel's
clamps read it from device memory: hdn_simi_track_update_ragged_f64), reinit(slot, ...) starts a new video in a slot in place, and
hdn_amd.track_videos streams a dataset through the slots under one captured hipGraph.

Signatures: the reference's launchers call `init(img, bbox, poly, gt_points, first_point)` / `track_new(idx, img, bbox, poly, gt_points)`
(tools/test.py:130,153) — one argument more than hdnTracker's own methods take; both spellings are accepted here.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import frame as FR
from ._loop import (FrameUploader, capture_graph, device_setup, env_flag, find_mode, similarity_result, track_state_row, upload_arena,
                    validate_frame_capacity)
from .similarity import SEQ_DOUBLES, SimilarityDecoder, TrackerConfig

TRACK_DOUBLES, OUT_DOUBLES = 48, 20     # HDN_SIMI_TRACK_DOUBLES / HDN_SIMI_OUT_DOUBLES


def _center2poly(c):
    """cetner2poly, hdn/utils/bbox.py:40-56."""
    x, y, w, h = c[0], c[1], c[2], c[3]
    return np.array([x - w * 0.5, y - h * 0.5, x + w * 0.5, y - h * 0.5, x + w * 0.5, y + h * 0.5, x - w * 0.5, y + h * 0.5])


def _rot_matrix(cx, cy, rot):
    """getRotMatrix, hdn/utils/bbox.py:58-75."""
    cc, ss = np.cos(rot), np.sin(rot)
    return np.array([[cc, -ss, cx - cx * cc + cy * ss], [ss, cc, cy - cy * cc - cx * ss], [0, 0, 1]])


def _transform_poly(polygon, m):
    """transformPoly, hdn/utils/bbox.py:77-90."""
    polygon = polygon.reshape(-1, 2)
    out = np.ones([polygon.shape[0], 3])
    out[:, 0:2] = polygon
    return (out @ m.transpose(1, 0))[:, 0:2]


def sequence_records(poly, first_point, channel_average, cfg: TrackerConfig):
    """The host arithmetic of hdnTracker.init for ONE sequence (hdn_tracker.py:117-136) -> (track record [48], seq record [8], poly_shift_l, init_s_z)."""
    poly = [float(p) for p in np.asarray(poly, np.float64).reshape(-1)]
    theta = poly[4] if len(poly) > 4 else 0.0
    first_point = np.asarray(first_point, np.float64).reshape(-1)[:2]
    size = np.array([poly[2], poly[3]], np.float64)
    polygon = _transform_poly(_center2poly(poly[:4]), _rot_matrix(poly[0], poly[1], theta))           # :120-125
    fir = (polygon - first_point) ** 2
    shift = int(np.argmin(fir[:, 0] + fir[:, 1]))
    w_z = size[0] + cfg.context_amount * np.sum(size)                                                  # :132-136
    h_z = size[1] + cfg.context_amount * np.sum(size)
    s_z = float(np.floor(np.sqrt(w_z * h_z)))
    s_x = float(np.floor(s_z * float(np.round(cfg.instance_size / cfg.exemplar_size))))
    avg = [float(a) for a in np.asarray(channel_average).reshape(-1)]
    tr = np.zeros(TRACK_DOUBLES, np.float64)
    tr[0:2], tr[2:4], tr[4], tr[6], tr[8] = poly[0:2], size, theta, 1.0, 1.0
    tr[14:16], tr[16], tr[17:19], tr[19], tr[20:23] = size, s_z, poly[0:2], shift, avg
    tr[24:30] = [poly[0], poly[1], s_x] + avg
    tr[32:38] = [1, 0, 0, 0, 1, 0]
    tr[40:46] = [poly[0], poly[1], s_z] + avg
    return tr, np.array([poly[0], poly[1], s_z, s_x, 0.0] + avg, np.float64), shift, s_z


class SimiTracker:
    miopen_find = False        # (DeviceTrackerSimi: MIOpen find mode around the network work of init / reinit / track_new, capture included)
    _label = "per-frame"       # (how the warning of a failed capture names the body)

    def __init__(self, model, cfg: TrackerConfig = None, graph: bool = False, scale_score_thresh: float = 0.5, batch_template: bool = None):
        """model: the reference's ModelBuilder interface (template / track_new / track_new_lp) in eval mode on the GPU.
        scale_score_thresh: cfg.TRACK.SCALE_SCORE_THRESH (0.5 in hdn/core/config.py:527 and every shipped YAML).
        batch_template: refresh the template with one backbone pass over (crop, log-polar crop) instead of template()'s two (checked against
        template() at init; default: HDN_SIMI_BATCH_TEMPLATE, on)."""
        self.model = model
        self.batch_template = env_flag("HDN_SIMI_BATCH_TEMPLATE") if batch_template is None else bool(batch_template)
        self._batched_ok = False
        self.cfg = cfg or TrackerConfig()
        self.use_graph, self._graph = bool(graph), None
        self.scale_score_thresh = float(scale_score_thresh)
        self.host_syncs = 0
        self._zf_static = None
        self._kern_in_graph = True      # (set by _capture: did the heads recompute their template-branch features inside the captured graph?)
        self.n = 1          # sequences advanced per call (BatchedSimiTracker: n > 1)

    # -------------------------------------------------------------------------------------------------- template (init + refresh)
    def _template_features(self, z_crop):
        """(zf, zf_lp) of ModelBuilder.template(z_crop) (model_builder_e2e_unconstrained_v2.py:87-96).  With `batch_template` the crop and its
        log-polar image go through the backbone as ONE batch of 2n instead of two passes of n (the 127-px passes are launch-bound; the necks keep
        their own halves) — used only after _check_batched_template found it equal to the model's own template() on this sequence's first crop."""
        m = self.model
        with torch.no_grad():
            if not self._batched_ok:
                m.template(z_crop)
                return m.zf, m.zf_lp
            n = z_crop.shape[0]
            f = m.feature_extractor(torch.cat((z_crop[:, 0:3], z_crop[:, 3:6]), 0))
            levels = isinstance(f, (list, tuple))
            a, b = ([t[:n] for t in f], [t[n:] for t in f]) if levels else (f[:n], f[n:])
            if hasattr(m, "neck"):                                 # cfg.ADJUST.ADJUST (the attribute exists exactly then, :47-51)
                a, b = m.neck(a), m.neck_lp(b)
        return a, b

    def _check_batched_template(self, z_crop, rtol: float = 1e-4) -> bool:
        """Is the one-pass form this model's template()?  Compared on the sequence's first crop (max difference against the largest magnitude of the
        level: a different convolution algorithm at 2n is rounding, a model whose template() does something else is not); on any doubt the
        model's own method stays."""
        m = self.model
        if not (self.batch_template and hasattr(m, "feature_extractor") and hasattr(m, "neck") == hasattr(m, "neck_lp")):
            return False
        flat = lambda f: list(f) if isinstance(f, (list, tuple)) else [f]
        self._batched_ok = False
        own = [t.detach().clone() for f in self._template_features(z_crop) for t in flat(f)]
        try:
            self._batched_ok = True
            got = [t for f in self._template_features(z_crop) for t in flat(f)]
        except Exception:
            return False
        finally:
            self._batched_ok = False
        if len(got) != len(own) or any(g.shape != o.shape for g, o in zip(got, own)):
            return False
        return all(float((g - o).abs().max()) <= rtol * max(float(o.abs().max()), 1e-30) for g, o in zip(got, own))

    def _template(self, z_crop, first: bool = False):
        """ModelBuilder.template(z_crop) with the resulting features COPIED into buffers that stay where they are: the per-frame refresh
        is then an in-place update (capturable; the heads' template cache keys on the tensors' version counters)."""
        m = self.model
        if first:
            self._batched_ok = False
            self._batched_ok = self._check_batched_template(z_crop)       # (two host reads per level, once per sequence)
        new = list(self._template_features(z_crop))
        if self._zf_static is None:
            self._zf_static = [[t.detach().clone() for t in f] if isinstance(f, (list, tuple)) else f.detach().clone() for f in new]
        else:
            for dst, src in zip(self._zf_static, new):
                if isinstance(dst, list):
                    for d, s in zip(dst, src):
                        d.copy_(s)
                else:
                    dst.copy_(src)
        m.zf, m.zf_lp = self._zf_static

    # -------------------------------------------------------------------------------------------------- init
    def init(self, img, bbox, poly, *rest):
        """img: BGR uint8 [H,W,3]; bbox (x, y, w, h); poly (cx, cy, w, h, theta); then first_point — hdnTracker.init's own signature — or
        gt_points, first_point (what tools/test.py passes); first_point: (x, y) of the first ground-truth corner."""
        if not rest:
            raise TypeError("init(img, bbox, poly, first_point) or init(img, bbox, poly, gt_points, first_point)")
        c = self.cfg
        self.dev = next(self.model.parameters()).device
        self.ratio = float(np.round(c.instance_size / c.exemplar_size))
        frame = FR.upload(img)
        self.init_frame = frame.clone() if isinstance(img, torch.Tensor) and img.is_cuda else frame        # update_template rotates THIS frame, every frame
        self.channel_average = frame.to(torch.float64).mean(dim=(0, 1)).cpu().numpy()                     # :138 (one read per sequence)
        self.host_syncs += 1
        self.frame_hw = (int(frame.shape[0]), int(frame.shape[1]))
        tr, sq, self.poly_shift_l, self.init_s_z = sequence_records(poly, rest[-1], self.channel_average, c)
        self.init_pos, self.init_size = tr[17:19].copy(), tr[14:16].copy()
        self.track = torch.from_numpy(tr).to(self.dev).view(1, -1)
        self.seq = torch.from_numpy(sq).to(self.dev).view(1, -1)
        assert self.seq.shape[1] == SEQ_DOUBLES
        self._dec = SimilarityDecoder(self.dev, c)
        self.state = self._dec.new_state(1)
        self._out = torch.zeros((1, OUT_DOUBLES), dtype=torch.float64, device=self.dev)
        self._zf_static, self._graph = None, None
        z_crop = FR.get_subwindow(frame, None, c.exemplar_size, None, None, params=self.track[:, 40:46], islog=1)    # :140-143
        with find_mode(self.miopen_find):
            self._template(z_crop, first=True)
        return z_crop

    # -------------------------------------------------------------------------------------------------- one frame
    def _body(self, frame):
        """Everything of a frame on the device; no host values, no data-dependent allocations.  -> out float64 [1, 20] (a buffer of this object)."""
        c, m, dec = self.cfg, self.model, self._dec
        x_crop = FR.get_subwindow(frame, None, c.instance_size, None, None, params=self.track[:, 24:30])                 # :189-192
        with torch.no_grad():
            o = m.track_new(x_crop)
        dec.translation(o["cls"], o["loc_c"], self.seq, self.state)                                                   # :193-233
        x_moved = FR.get_subwindow(frame, None, c.instance_size, None, None, params=self.state[:, 8:14])                # :236-238
        with torch.no_grad():
            o = m.track_new_lp(x_moved, [0, 0])
        dec.logpolar(o["cls_lp"], o["loc_lp"], self.seq, self.state)                                                  # :241-246
        self._update()                                                                                                # :213-227, :247-283 and the next :176-188
        rot_img = self._rotated_first()                                                                               # update_template, :156-162
        z_crop = FR.get_subwindow(rot_img, None, c.exemplar_size, None, None, params=self.track[:, 40:46], islog=1)
        self._template(z_crop)
        return self._out

    def _update(self):
        c = self.cfg
        _lib.launch("simi track update", self.dev, _lib.load().hdn_simi_track_update_f64, _lib.ptr(self.state), _lib.ptr(self.track), _lib.ptr(self.seq),
                    _lib.ptr(self._out), self.n, self.frame_hw[1], self.frame_hw[0], self.scale_score_thresh, c.context_amount, self.ratio)

    def _rotated_first(self):
        return FR.warp_affine_cubic(self.init_frame, self.track[:, 32:38])

    def _head_caches(self):
        """The template-branch caches of the model's heads (hdn_amd.heads; None where a head has none)."""
        return [getattr(getattr(self.model, name), "_hdn_template_cache", None) for name in ("head", "head_lp") if hasattr(self.model, name)]

    def _static_input(self, frame_shape):
        frame = torch.empty(frame_shape, dtype=torch.uint8, device=self.dev)
        frame.copy_(self.init_frame)
        return frame

    def _captured_body(self, body):
        before = self._head_caches()
        out = body()
        # (the refresh of the step before changed the template tensors in place, so the heads recomputed their template-branch
        # features INSIDE the capture: they are nodes of the graph and follow the template on every replay)
        self._kern_in_graph = all(b is None or b is not a for a, b in zip(before, self._head_caches()))
        return out

    def _capture(self, frame_shape):
        """One hipGraph for the whole body.  The warm-up / capture runs advance the recurrences and refresh the template: everything they
        touched is put back afterwards (track record, seq, state, template features).  A body that cannot be captured: use_graph goes False."""
        self._static_frame = self._static_input(frame_shape)
        live = [self.track, self.seq, self.state] + [t for f in self._zf_static for t in (f if isinstance(f, list) else [f])]
        got = capture_graph(lambda: self._body(self._static_frame), live, self._label, hook=self._captured_body)
        self.use_graph = got is not None
        if got is not None:
            self._graph, self._g_out = got

    def _frames(self, img, into=None):
        """This step's frame on the device, or copied into `into` (the static input of the captured graph)."""
        if into is None:
            return FR.upload(img)
        return into.copy_(img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img)), non_blocking=True)

    def _step(self, imgs, frame_shape):
        """Capture on first use; the frames into the static input and one replay, or the body eagerly.  -> out (a buffer the next step overwrites)."""
        with find_mode(self.miopen_find):
            if self.use_graph and self._graph is None:
                self._capture(frame_shape)                        # (may switch use_graph off)
            if self.use_graph:
                self._frames(imgs, into=self._static_frame)
                self._graph.replay()
                return self._g_out
            return self._body(self._frames(imgs))

    def track_new(self, fr_idx, img, gt_box=None, gt_poly=None, gt_points=None, sync: bool = True):
        """-> {'bbox', 'bbox_aligned', 'best_score', 'rot', 'polygon'} as hdnTracker.track_new (:295-301); sync=False: the float64 device record
        [20] (include/hdn_hip.h: hdn_simi_track_update_f64's `out`) without any host read."""
        if tuple(img.shape[:2]) != self.frame_hw:
            raise ValueError(f"frames of a sequence have one size: init saw {self.frame_hw}, this one is {tuple(img.shape[:2])}")
        out = self._step(img, tuple(img.shape))
        if not sync:
            return {"record": out.clone().view(-1)}
        h = out.view(-1).cpu().numpy()
        self.host_syncs += 1
        return similarity_result(h)

    def track(self, img):
        return self.track_new(None, img)

    def track_state(self) -> dict:
        """The recurrence state the reference keeps as host attributes (center_pos, size, rot, lp_shift, scale, v, lost_count, ...), read back on
        demand (one device->host read, counted)."""
        t = self.track.view(-1).cpu().numpy()
        self.host_syncs += 1
        return track_state_row(t)


class BatchedSimiTracker(SimiTracker):
    """n independent sequences of the similarity-only tracker in lock step on ONE GPU (what hdn_amd.batched_tracker is for the homography tracker; the
    reference: several videos at once by hand-split ranges, tools/test.py:91-103).  Every kernel of the frame body already takes a batch — the crops and
    the rotation of the resident first frames (blockIdx.y = sequence, per-sequence records read out of the [n, 48] arrays), the two decodes, the update
    kernel — and the model's own forward code is batch-general (n templates, refreshed in place every step).  One step = one upload of [n,H,W,3], one
    hipGraph replay, one host read of [n, 20].  Sequence b of a batch runs exactly the code it runs alone: tests/test_gpu_simi_tracker.py holds every
    sequence to its own B = 1 run and to the CPU loop.

    frame_capacity=(Hmax, Wmax): arena mode, as in hdn_amd.batched_tracker.  The frames live in a hdn_amd.frame.FrameArena, every slot at its own
    size, and so do the resident first frames (a second arena sharing the size table: a slot's video has one size); the crops, the rotation and
    the update kernel's clamps (hdn_simi_track_update_ragged_f64) read each slot's size from device memory, so the captured hipGraph goes on
    replaying while reinit(slot, ...) hands a slot a new video of another size.  track_videos(tracker, videos) schedules a dataset through
    the slots.  init / track_new then take LISTS of n frames."""

    _label = "batched per-frame"

    def __init__(self, model, n: int, cfg: TrackerConfig = None, graph: bool = False, scale_score_thresh: float = 0.5, batch_template: bool = None,
                 frame_capacity=None):
        super().__init__(model, cfg=cfg, graph=graph, scale_score_thresh=scale_score_thresh, batch_template=batch_template)
        if n < 1:
            raise ValueError("n must be >= 1")
        self.frame_capacity = validate_frame_capacity(frame_capacity)
        self._arena = self._first = self._rotated = None      # arena mode: this step's frames, the first frames, their rotation
        self.n = int(n)
        self._upload = FrameUploader(self.n)      # (one pinned staging buffer, one asynchronous copy per step)

    def init(self, imgs, bboxes, polys, *rest):
        """imgs n x BGR uint8 [H,W,3] (one size); bboxes, polys (cx, cy, w, h, theta) and first_points per sequence (hdnTracker.init's arguments; the
        launchers' extra gt_points list is accepted in front of first_points)."""
        if not rest:
            raise TypeError("init(imgs, bboxes, polys, first_points) or init(imgs, bboxes, polys, gt_points, first_points)")
        first_points, c, n = rest[-1], self.cfg, self.n
        if not (len(bboxes) == len(polys) == len(first_points) == n):
            raise ValueError(f"init takes {n} bboxes / polys / first_points")
        self.dev = next(self.model.parameters()).device
        self.ratio = float(np.round(c.instance_size / c.exemplar_size))
        if self.frame_capacity is not None:      # arena mode: first frames of different sizes
            for b, fp in enumerate(first_points):
                if fp is None:
                    raise ValueError(f"slot {b}: the similarity tracker needs the sequence's first_point (the first ground-truth corner)")
            if not torch.cuda.is_available():
                raise _lib.HdnHipError("hdn_amd runs on the GPU only; there is no CPU fallback")
            arena = FR.FrameArena(n, self.frame_capacity[0], self.frame_capacity[1], 3, device=self.dev)
            frames = self._arena = upload_arena(arena, imgs, same_size=False)    # (replaced only once every frame was accepted)
            self._first = arena.like()                                # update_template rotates THESE frames, every step
            self._rotated = arena.like()
            for b in range(n):
                self._first.frame(b).copy_(arena.frame(b))
            self.channel_average = torch.stack([arena.frame(b).to(torch.float64).mean(dim=(0, 1)) for b in range(n)]).cpu().numpy()
            self.frame_hw = [arena.size(b) for b in range(n)]         # per slot
        else:
            frames = self._upload(imgs, self.dev)
            self.init_frame = frames.clone()                              # update_template rotates THESE frames, every step
            self.channel_average = frames.to(torch.float64).mean(dim=(1, 2)).cpu().numpy()
            self.frame_hw = (int(frames.shape[1]), int(frames.shape[2]))
        self.host_syncs += 1
        recs = [sequence_records(polys[b], first_points[b], self.channel_average[b], c) for b in range(n)]
        self.track = torch.from_numpy(np.stack([r[0] for r in recs])).to(self.dev).contiguous()
        self.seq = torch.from_numpy(np.stack([r[1] for r in recs])).to(self.dev).contiguous()
        self.poly_shift_l, self.init_s_z = [r[2] for r in recs], [r[3] for r in recs]
        self._dec = SimilarityDecoder(self.dev, c)
        self.state = self._dec.new_state(n)
        self._out = torch.zeros((n, OUT_DOUBLES), dtype=torch.float64, device=self.dev)
        self._zf_static, self._graph = None, None
        z_crop = FR.get_subwindow(frames, None, c.exemplar_size, None, None, params=self.track[:, 40:46], islog=1)
        with find_mode(self.miopen_find):
            self._template(z_crop, first=True)
        return z_crop

    # -------------------------------------------------------------------------------------------------- arena mode: the parts of a step that see frame sizes
    def _update(self):
        if self._arena is None:
            return super()._update()
        c, a = self.cfg, self._arena
        _lib.launch("simi track update (ragged)", self.dev, _lib.load().hdn_simi_track_update_ragged_f64, _lib.ptr(self.state), _lib.ptr(self.track),
                    _lib.ptr(self.seq), _lib.ptr(self._out), _lib.ptr(a.dims), self.n, a.Hmax, a.Wmax, self.scale_score_thresh, c.context_amount, self.ratio)

    def _rotated_first(self):
        if self._arena is None:
            return super()._rotated_first()
        return FR.warp_affine_cubic(self._first, self.track[:, 32:38], out=self._rotated)

    def _static_input(self, frame_shape):
        # (arena mode: the arena IS the static input - its slots hold the sequences' latest frames, their sizes are device data; the first frames
        # are not copied over them)
        return self._arena if self._arena is not None else super()._static_input(frame_shape)

    def _frames(self, imgs, into=None):
        return self._arena if self._arena is not None else self._upload(imgs, self.dev, into=into)

    def reinit(self, slot: int, img, bbox, poly, gt_points, first_point=None):
        """What init does for ONE sequence, written in place into row `slot` of track / seq / state / the result buffer, of every level of the
        static template buffers (model.zf / zf_lp) and of both arenas: the slot starts a new video (of any frame size up to the capacity) while the
        other slots keep going.  No other row is touched, no tensor is replaced and the captured hipGraph is kept.  Arena mode only.  One host read
        (the first frame's channel average).  The slot's template is computed at batch 1 by the form init chose for this model (one backbone pass
        over both crops, or the model's own template())."""
        from . import heads as HD
        if self._arena is None:
            raise RuntimeError("reinit() needs arena mode (frame_capacity=(Hmax, Wmax)) and an init() before it")
        if not 0 <= slot < self.n:
            raise IndexError(f"slot {slot} of {self.n}")
        if first_point is None:
            raise ValueError(f"slot {slot}: the similarity tracker needs the sequence's first_point (the first ground-truth corner)")
        c, m = self.cfg, self.model
        self._arena.set(slot, img)                   # (raises for a frame above the capacity, before anything is written)
        frame = self._arena.frame(slot)
        self._first.frame(slot).copy_(frame)         # (the size table is shared)
        avg = frame.to(torch.float64).mean(dim=(0, 1)).cpu().numpy()
        self.host_syncs += 1
        tr, sq, self.poly_shift_l[slot], self.init_s_z[slot] = sequence_records(poly, first_point, avg, c)
        self.channel_average[slot], self.frame_hw[slot] = avg, self._arena.size(slot)
        self.track[slot].copy_(torch.from_numpy(tr))
        self.seq[slot].copy_(torch.from_numpy(sq))
        self.state[slot].zero_()
        self._out[slot].zero_()
        z_crop = FR.get_subwindow(frame, None, c.exemplar_size, None, None, params=self.track[slot:slot + 1, 40:46], islog=1)
        # the model's own template() reassigns zf / zf_lp and, behind install(), drops what the heads cached: a replayed graph reads both by address
        heads = [getattr(m, name) for name in ("head", "head_lp") if hasattr(m, name)]
        kept = [HD.template_cache_state(h) for h in heads]
        with find_mode(self.miopen_find):
            try:
                new = self._template_features(z_crop)
                for dst, src in zip(self._zf_static, new):
                    for d, t in zip(*((dst, src) if isinstance(dst, list) else ([dst], [src]))):
                        d[slot:slot + 1].copy_(t)
            finally:
                m.zf, m.zf_lp = self._zf_static
                for h, k in zip(heads, kept):
                    HD.restore_template_cache_state(h, k)
            if self._graph is not None and not self._kern_in_graph:
                # (the capture found the heads' template-branch features cached, outside the graph: a replay reads those buffers, so bring the row up to date)
                for h, z in zip(heads, self._zf_static):
                    HD.refresh_template_cache(h, z if isinstance(z, list) else [z], slot)
        return z_crop

    def track_new(self, fr_idx, imgs, gt_box=None, gt_poly=None, gt_points=None, sync: bool = True):
        """One frame of every sequence -> n result dictionaries with hdnTracker.track_new's keys (sync=True: one host read for all), or the float64 device
        records [n, 20] (sync=False).  Arena mode: a list of n frames, each of its slot's current size."""
        if self.frame_capacity is not None:
            if self._arena is None:
                raise RuntimeError("track_new() before init()")
            if not isinstance(imgs, torch.Tensor):
                imgs = [im if isinstance(im, torch.Tensor) else np.asarray(im) for im in imgs]
            upload_arena(self._arena, imgs, same_size=True)   # (before a first capture too: a refused step leaves nothing half done)
            shape = None
        else:
            shape = tuple(imgs.shape) if isinstance(imgs, torch.Tensor) else (len(imgs),) + tuple(np.asarray(imgs[0]).shape)
            if shape[0] != self.n or tuple(shape[1:3]) != self.frame_hw:
                raise ValueError(f"a step takes {self.n} frames of {self.frame_hw}, got {shape}")
        out = self._step(imgs, shape)
        if not sync:
            return {"record": out.clone()}
        h = out.cpu().numpy()
        self.host_syncs += 1
        return [similarity_result(h[b]) for b in range(self.n)]

    def track_state(self) -> list:
        t = self.track.cpu().numpy()
        self.host_syncs += 1
        return [track_state_row(r) for r in t]


class DeviceTrackerSimi(SimiTracker):
    """Drop-in for hdnTracker behind build_tracker(model) (hdn/tracker/tracker_builder.py:18-19).  One hipGraph per frame, BatchNorm-folded
    backbone / necks and MIOpen find mode around this tracker's calls, exactly as hdn_amd.tracker.DeviceTrackerHomo."""

    def __init__(self, model, graph: bool = None, cfg: TrackerConfig = None, fold_backbone: bool = None, batch_template: bool = None):
        cfg, ref_cfg, graph, self.miopen_find, self.folded = device_setup(model, cfg, graph, fold_backbone)
        thresh = float(getattr(getattr(ref_cfg, "TRACK", None), "SCALE_SCORE_THRESH", 0.5))      # (0.5 too when a cfg was handed in: no node is read then)
        super().__init__(model, cfg=cfg, graph=graph, scale_score_thresh=thresh, batch_template=batch_template)
