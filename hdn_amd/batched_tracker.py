"""N independent sequences advancing in lock step on ONE GPU: the per-frame tracker loop of hdn_amd.tracker at batch N.

    BatchedHomoTracker(hm_net, n, ...)       N x HomoTracker        <- hdnTrackerHomo, hdn/tracker/hdn_tracker_proj_e2e.py:60-285
    BatchedDeviceTracker(model, n)           N x DeviceTrackerHomo  (the reference's ModelBuilder interface; BN-folded backbone, MIOpen find mode)

BatchedHomoTracker derives from HomoTracker and inherits its _body, _capture and _step: the frame body exists once.  Here are only the parts that
see n frames - init / reinit (row b of every per-sequence buffer), _static_input / _frames (one [N,H,W,3] tensor through the pinned uploader, or
the arena) and track_new's list of results - and the class attribute that asks for per-sequence scores.

Why.  The reference's only inference-time parallelism is "several videos at once": tools/test.py pins one GPU (:49) and its authors
split the video list by hand across processes (:91-103).  One sequence is a B = 1 latency problem — 2.9 ms per frame on an MI355X of
which 2.1 ms are a ResNet-50 at batch 1 using < 5 % of the chip (profiles/round5_bench_line.json `sequence`) — and the H_total
recurrence forbids batching ALONG a sequence.  ACROSS sequences nothing is shared, so N of them run as one batch: every kernel of the
frame body already takes a batch dimension (the similarity decode, hdn_track_prepare / accumulate_f64, the correlation heads, the
homography estimator), the three frame kernels got one (hdn_*_batch_*, blockIdx.y = sequence, per-sequence parameter records read
straight out of the [N, 48] similarity state), and the two L1 scores — which the reference takes from sample 0 only (`[0][0]`,
model_builder_e2e_unconstrained_v2.py:213-216) — are computed per sequence (hdn_l1_score2_batch_f32) so that each has its own gate.
One frame of all N sequences = ONE upload of [N,H,W,3], ONE hipGraph replay, ONE host read of [N, 2 * points + 1].

Parity.  Every kernel computes sequence b of a batch exactly as it computes it alone (same code, blockIdx.y / the batch index only
selects the data); what may differ from N separate B = 1 runs is the rounding of the PyTorch-ROCm convolutions (MIOpen picks other
algorithms at another batch size) and of the B = 1-only packed head / chained trunk forms.  tests/test_gpu_tracker.py holds every
sequence of a batch to its own B = 1 run (<= 1e-4 px on the corners with the stand-in networks; bit-exact frame kernels) and to the CPU
restatement of the loop.

Frames of all sequences of a step must have one size (they share the [N,H,W,3] buffer) - unless the tracker is given a
`frame_capacity=(Hmax, Wmax)`: the frames then live in a hdn_amd.frame.FrameArena, every slot at its own size, the three frame kernels read
each slot's size from device memory (hdn_*_ragged_*), and the same captured hipGraph goes on replaying while `reinit(slot, ...)` hands a
slot a new video of another size.  Sequences of different lengths, or more videos than slots: track_videos(tracker, videos) below feeds a
list of videos through the n slots (a finished slot takes the next video; with none left it is fed its last frame again and its results
are dropped).
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import _lib
from . import frame as FR
from ._loop import FrameUploader, device_setup, find_mode, homography_result, upload_arena, validate_frame_capacity
from .similarity import DeviceSimilarity, TrackerConfig
from .tracker import HomoTracker, _const_row, _geometry, attach_hip_trunk


class BatchedHomoTracker(HomoTracker):
    _label = "batched per-frame"
    _per_sample = True           # every sequence its own gate (at n = 1 too: hdn_l1_score2_batch_f32)

    def __init__(self, hm_net, n: int, iterations: int = 1, similarity=None, score_gate: float = 2.5, graph: bool = False, cfg: TrackerConfig = None,
                 frame_capacity=None):
        """hm_net: hdn_amd.HomoModelBuilder (or the reference's, after install()) in eval mode on the GPU; n: sequences per step.
        similarity: None (identity) or a DeviceSimilarity (its model then holds n templates).  graph: one hipGraph per step.
        frame_capacity: None (all frames of a step have one size), or (Hmax, Wmax): arena mode - every slot has its own frame size up to
        that capacity, and reinit() is available."""
        if n < 1:
            raise ValueError("n must be >= 1")
        self.frame_capacity = validate_frame_capacity(frame_capacity)
        super().__init__(hm_net, iterations=iterations, similarity=similarity, score_gate=score_gate, graph=graph, cfg=cfg)
        self._arena = None
        self.n = int(n)
        self._upload = FrameUploader(self.n)      # (one pinned staging buffer, one asynchronous copy per step)

    # -------------------------------------------------------------------------------------------------- init
    def init(self, imgs, bboxes, polys, gt_points, first_points=None):
        """Per sequence what hdnTrackerHomo.init takes (hdn_tracker_proj_e2e.py:60): imgs n x BGR uint8 [H,W,3]; bboxes n x (x, y, w, h);
        polys n x (cx, cy, w, h, theta); gt_points n x the initial corners (the same number of points for every sequence)."""
        c, n = self.cfg, self.n
        if not (len(bboxes) == len(polys) == len(gt_points) == n):
            raise ValueError(f"init takes {n} bboxes / polys / gt_points")
        self.dev = next(self.net.parameters()).device
        geo = [_geometry(p, c) for p in polys]
        self.init_pos, self.size = np.stack([g[0] for g in geo]), np.stack([g[1] for g in geo])
        self.init_s_z, self.init_s_z_sm = np.array([g[2] for g in geo], np.float64), np.array([g[3] for g in geo], np.float64)
        if self.frame_capacity is not None:      # arena mode: first frames of different sizes
            if not torch.cuda.is_available():
                raise _lib.HdnHipError("hdn_amd runs on the GPU only; there is no CPU fallback")
            self._arena = FR.FrameArena(n, self.frame_capacity[0], self.frame_capacity[1], 3, device=self.dev)
            frames = upload_arena(self._arena, imgs, same_size=False)
            self.channel_average = torch.stack([frames.frame(b).to(torch.float64).mean(dim=(0, 1)) for b in range(n)]).cpu().numpy()
            sizes = [frames.size(b) for b in range(n)]
        else:
            frames = self._upload(imgs, self.dev)
            # np.mean(img, axis=(0, 1)) of every first frame: one reduction on the device, read once
            self.channel_average = frames.to(torch.float64).mean(dim=(1, 2)).cpu().numpy()
            sizes = [tuple(frames.shape[1:3])] * n
        self.host_syncs += 1
        self.z_crop_points_sm = [FR.crop_points(self.init_pos[b], self.init_s_z_sm[b], sizes[b][0], sizes[b][1]) for b in range(n)]
        # get_template_info(get_subwindow_for_homo(...)[:, 0:3]): the normalised gray templates, constant for the sequences
        self._const_params = torch.from_numpy(np.concatenate([self.init_pos, self.init_s_z_sm[:, None], self.channel_average], axis=1)).to(self.dev)
        self.init_homo_tmp = FR.get_search_info(frames, None, None, None, model_sz=c.exemplar_size, params=self._const_params)
        with find_mode(self.miopen_find):
            with torch.no_grad():
                self.init_patch_1 = self.net.ShareFeature(self.init_homo_tmp).detach()
            if self.similarity is not None:
                self.similarity.init(frames, self.init_pos, self.init_s_z, self.init_s_z_sm, self.channel_average)
        pts = [np.asarray(g, np.float64).reshape(-1, 2) for g in gt_points]
        if any(p.shape != pts[0].shape for p in pts):
            raise ValueError("every sequence must have the same number of initial points")
        self.n_points = pts[0].shape[0]
        self.init_points = torch.from_numpy(np.stack(pts)).to(self.dev).contiguous()
        self.H_total = torch.eye(3, dtype=torch.float64, device=self.dev).repeat(n, 1, 1).contiguous()
        self._Ht, self._Hinv = (torch.empty((n, 9), dtype=torch.float64, device=self.dev) for _ in range(2))
        self._out = torch.empty((n, 2 * self.n_points + 1), dtype=torch.float32, device=self.dev)
        self._graph = None
        consts = np.stack([_const_row(zp, c.exemplar_size, self.score_gate) for zp in self.z_crop_points_sm])
        self._consts = torch.from_numpy(consts).to(self.dev)

    def reinit(self, slot: int, img, bbox, poly, gt_points, first_point=None):
        """What init does for ONE sequence, written in place into row `slot` of every per-sequence tensor: the slot starts a new video (of any
        frame size up to the capacity) while the other slots keep going.  No other row is touched and no tensor is replaced, so the captured
        hipGraph is not re-captured.  Arena mode only (frame_capacity=...).  gt_points: as many points as init was given.  One host read, the one
        init has (the first frame's channel average).  The similarity branch's template goes through DeviceSimilarity.reinit, which also refreshes
        the heads' cached template-branch features in place - with HDN_HIP_HEADS too: its template pack holds weights only and serves one row."""
        if self._arena is None:
            raise RuntimeError("reinit() needs arena mode (frame_capacity=(Hmax, Wmax)) and an init() before it")
        if not 0 <= slot < self.n:
            raise IndexError(f"slot {slot} of {self.n}")
        pts = np.asarray(gt_points, np.float64).reshape(-1, 2)
        if pts.shape[0] != self.n_points:
            raise ValueError(f"this tracker follows {self.n_points} points per sequence, got {pts.shape[0]}")
        c = self.cfg
        pos, size, s_z, s_z_sm = _geometry(poly, c)
        self._arena.set(slot, img)                   # (raises for a frame above the capacity, before anything is written)
        frame = self._arena.frame(slot)
        avg = frame.to(torch.float64).mean(dim=(0, 1)).cpu().numpy()
        self.host_syncs += 1
        self.init_pos[slot], self.size[slot], self.init_s_z[slot], self.init_s_z_sm[slot], self.channel_average[slot] = pos, size, s_z, s_z_sm, avg
        zp = self.z_crop_points_sm[slot] = FR.crop_points(pos, s_z_sm, frame.shape[0], frame.shape[1])
        self._const_params[slot].copy_(torch.from_numpy(np.concatenate([pos, [s_z_sm], avg])))
        tmp = FR.get_search_info(frame, None, None, None, model_sz=c.exemplar_size, params=self._const_params[slot])
        self.init_homo_tmp[slot:slot + 1].copy_(tmp)
        with find_mode(self.miopen_find):
            with torch.no_grad():
                self.init_patch_1[slot:slot + 1].copy_(self.net.ShareFeature(tmp))
            if self.similarity is not None:
                self.similarity.reinit(slot, frame, pos, s_z, s_z_sm, avg)
        self.init_points[slot].copy_(torch.from_numpy(pts))
        self.H_total[slot].copy_(torch.eye(3, dtype=torch.float64))
        self._consts[slot].copy_(torch.from_numpy(_const_row(zp, c.exemplar_size, self.score_gate)))

    # -------------------------------------------------------------------------------------------------- one step = one frame of every sequence
    def _static_input(self, imgs):
        # (arena mode: the arena IS the static input - its slots hold the sequences' latest frames, their sizes are device data)
        if self._arena is not None:
            return self._arena
        shape = tuple(imgs.shape) if isinstance(imgs, torch.Tensor) else (self.n,) + tuple(np.asarray(imgs[0]).shape)
        return torch.empty(shape, dtype=torch.uint8, device=self.dev)

    def _frames(self, imgs, into=None):
        return self._arena if self._arena is not None else self._upload(imgs, self.dev, into=into)

    _static_frames = property(lambda self: self._static_frame)      # (the static input of the captured graph, under this class's name for it)

    def track_new(self, fr_idx, imgs, sync: bool = True):
        """One frame of every sequence.  -> list of n result dictionaries with hdnTrackerHomo.track_new's keys (sync=True; one host read
        for all of them), or device views {'points' [n, P, 2], 'best_score' [n]} (sync=False)."""
        n, P = self.n, self.n_points
        if self._arena is not None:
            imgs = [np.asarray(im) if not isinstance(im, torch.Tensor) else im for im in imgs] if not isinstance(imgs, torch.Tensor) else imgs
            upload_arena(self._arena, imgs, same_size=True)   # (before a first capture too: a refused step leaves nothing half done)
        out, self.last_score = self._step(imgs, sync)
        self.last_points = out[:, :2 * P].view(n, P, 2)
        if not sync:
            return {"points": self.last_points, "polygon": self.last_points, "best_score": out[:, 2 * P]}
        host = out.cpu().numpy()
        self.host_syncs += 1
        return [homography_result(host[b], P) for b in range(n)]

    def track(self, imgs):
        return self.track_new(None, imgs)

    def similarity_state(self):
        raise NotImplementedError("similarity_state() decodes ONE sequence's record; the lock-step tracker's records are similarity.state [n, 48]")


class BatchedDeviceTracker(BatchedHomoTracker):
    """n x DeviceTrackerHomo in lock step: `model` is the reference's ModelBuilder (hm_net = the homography estimator; template /
    track_new / track_new_lp = the similarity branch, called at batch n — the reference's own forward code is batch-general, its heads
    correlate sample b with template b).  Backbone / necks BatchNorm-folded, MIOpen find mode around this tracker's calls, one hipGraph
    per step (graph=False or HDN_TRACKER_GRAPH=0: eager), exactly as DeviceTrackerHomo does for one sequence; `hip_trunk` as there."""

    def __init__(self, model, n: int, graph: bool = None, iterations: int = 1, cfg: TrackerConfig = None, fold_backbone: bool = None,
                 hip_trunk: bool = None, frame_capacity=None):
        self.model = model
        cfg, _, graph, self.miopen_find, self.folded = device_setup(model, cfg, graph, fold_backbone)
        self.hip_trunk = attach_hip_trunk(model, hip_trunk)
        super().__init__(model.hm_net, n, iterations=iterations, similarity=DeviceSimilarity(model, cfg), graph=graph, cfg=cfg,
                         frame_capacity=frame_capacity)


@dataclasses.dataclass
class _Slot:
    """What track_videos knows of one slot of the tracker."""
    video: object        # index of the video the slot runs; None: idle (its results are dropped)
    frames: object       # iterator over the video's remaining frames
    last: object         # the last frame fed (fed again while the slot idles)
    fed: int             # frames fed after the first
    init: dict           # the video's init dictionary


def track_videos(tracker, videos, on_result=None):
    """Feed a list of videos (any lengths; in arena mode any frame sizes up to the capacity) through the tracker's n slots - what the reference's
    users do by splitting the dataset by hand across processes (tools/test.py:91-103).

    videos: iterable of (frames, init) - frames an iterable of BGR uint8 [H,W,3] whose first frame initialises the sequence, init a dict with
    'bbox', 'poly', 'gt_points' and optionally 'first_point'.  The first n videos fill the slots (init); every step advances all slots
    (track_new: one host read); a slot whose video ended is handed the next one (reinit), and with none left it is fed its last frame again,
    its results dropped.  Fewer videos than slots: the spare slots run copies of the last video, dropped as well.
    -> list, in input order, of per-video lists of track_new's dictionaries (one per frame after the first); with on_result, that is called as
    on_result(video_index, frame_index, result) instead and the lists stay empty.
    Plain scheduling over tracker.n / init / track_new / reinit (and tracker.frame_capacity where it has one: a video whose first frame is
    above it raises before anything is launched).  So it serves the similarity-only hdn_amd.simi_tracker.BatchedSimiTracker(model, n,
    frame_capacity=...) as well, whose init reads the last list as the first_points: every video's init then needs its 'first_point'."""
    n = tracker.n
    cap = getattr(tracker, "frame_capacity", None)
    queue = []
    for k, (frames, init) in enumerate(videos):
        it = iter(frames)
        try:
            first = next(it)
        except StopIteration:
            raise ValueError(f"video {k} has no frames") from None
        if cap is not None and (first.shape[0] > cap[0] or first.shape[1] > cap[1]):
            raise ValueError(f"video {k}: frames of {tuple(first.shape[:2])} are above the tracker's frame capacity {tuple(cap)}")
        queue.append((k, first, it, init))
    results = [[] for _ in queue]
    if not queue:
        return results
    queue.reverse()                                  # pop() from the end = input order
    slots = []
    for b in range(n):
        if queue:
            k, first, it, init = queue.pop()
            slots.append(_Slot(k, it, first, 0, init))
        else:                                        # fewer videos than slots: an idle copy of the last one
            slots.append(_Slot(None, iter(()), slots[-1].last, 0, slots[-1].init))
    tracker.init([s.last for s in slots], [s.init["bbox"] for s in slots], [s.init["poly"] for s in slots], [s.init["gt_points"] for s in slots],
                 [s.init.get("first_point") for s in slots])
    while True:
        # a slot whose video has no further frame takes the next video, or goes idle
        for b, s in enumerate(slots):
            while s.video is not None:
                nxt = next(s.frames, None)
                if nxt is not None:
                    s.last, s.fed = nxt, s.fed + 1
                    break
                if not queue:
                    s.video = None
                    break
                k, first, it, init = queue.pop()
                tracker.reinit(b, first, init["bbox"], init["poly"], init["gt_points"], init.get("first_point"))
                s.video, s.frames, s.last, s.fed, s.init = k, it, first, 0, init
        if all(s.video is None for s in slots):
            return results
        res = tracker.track_new(None, [s.last for s in slots])
        for b, s in enumerate(slots):
            if s.video is not None:
                if on_result is not None:
                    on_result(s.video, s.fed, res[b])
                else:
                    results[s.video].append(res[b])
