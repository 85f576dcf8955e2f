"""The per-frame tracker loop, device-resident (BASELINE config 4).

    HomoTracker.init(img, bbox, poly, gt_points, first_point)        <- hdnTrackerHomo.init,      hdn/tracker/hdn_tracker_proj_e2e.py:60-120
    HomoTracker.track_new(fr_idx, img, gt_box, gt_poly, gt_points)   <- hdnTrackerHomo.track_new, hdn_tracker_proj_e2e.py:141-285
    DeviceTrackerHomo(model)                                         <- the class hdn/tracker/tracker_builder.py:12-19 registers as
                                                                        TRACKS['hdnTrackerHomoProje2e'] (hdn_amd.install.install(tracker=True))

Same call signatures and the same result dictionary ('bbox_aligned', 'best_score', 'polygon', 'points', 'bbox') as the
reference's tracker.  Per frame: undo the accumulated motion (full-frame warp by inv(H_total), :150-155); the similarity
estimate on the stabilised frame (:157-214: search crop, ModelBuilder.track_new, decode, moved crop, track_new_lp, decode, H_sim —
hdn_amd.similarity); rotate back and cut the 127-px homography crop (:223-239); the refinement loop around
ModelBuilder.track_proj (:242-250); un-scale / un-shift the residual (:251-258), gate it (`homo_score > 2.5`, :261-264),
accumulate H_total and project the initial corners (:266-272).

The networks of the similarity branch (ResNet-50 backbone, necks, the 3x3 / 1x1 convolutions of the heads) are PyTorch-ROCm's, as
north_star assigns them; they are reached through `similarity` (hdn_amd.similarity.DeviceSimilarity around an object with the
reference's ModelBuilder interface).  Without one the similarity estimate is the identity.

What the reference does on the host per frame — cv2 warps of the full frame, numpy crops, three crop uploads, numpy decodes of the
head maps and six .cpu().numpy() syncs — is here ONE upload of the uint8 frame, kernels (hdn_amd.frame, .similarity, .refine) and
two one-lane kernels for the 3x3 float64 bookkeeping (hdn_track_prepare_f64 / hdn_track_accumulate_f64); the only host read is the 4 projected corners + best_score the caller asks for
(`sync=True`).  Nothing in the body depends on host values, so it replays as one hipGraph (`graph=True`) with or without the
similarity branch.  Sequences are independent: N GPUs run N sequences (replicas only, no collective).

HomoTracker is written for n sequences per call with n = 1: its _body, _capture and _step take n from the object and never look at a buffer's
shape, so hdn_amd.batched_tracker.BatchedHomoTracker inherits the three and overrides only init / reinit, the frame upload and track_new's results.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import frame as FR
from ._loop import capture_graph, device_setup, env_flag, find_mode, homography_result
from .refine import homo_refine
from .similarity import DeviceSimilarity, TrackerConfig

TRACK_CONST_DOUBLES = 40     # HDN_TRACK_CONST_DOUBLES


def _geometry(poly, cfg):
    """(init_pos [2], size [2], init_s_z, init_s_z_sm) of one sequence from its poly (cx, cy, w, h, ...) (hdn_tracker_proj_e2e.py:66-84)."""
    p = np.asarray(poly, np.float64).reshape(-1)[:4]
    pos, size = p[0:2].copy(), p[2:4].copy()
    ctx = cfg.context_amount * size.sum()
    return pos, size, np.floor(np.sqrt((size[0] + ctx) * (size[1] + ctx))), np.floor(np.sqrt(size[0] * size[1]))


def _const_row(zp, exemplar_size, score_gate):
    """One sequence's row of _consts: the un-scale / un-shift of the residual (:251-258) - four matrices that are constants of the sequence
    (float32 as the reference builds them, their inverses float32 by numpy's dtype rule) - handed to hdn_track_accumulate_f64 with the gate."""
    E, row = exemplar_size, np.zeros(TRACK_CONST_DOUBLES, np.float64)
    S = np.diag([E / (zp[2] - zp[0] + 1), E / (zp[3] - zp[1] + 1), 1.0]).astype(np.float32)
    Sh = np.array([[1, 0, -zp[0]], [0, 1, -zp[1]], [0, 0, 1]], np.float32)
    row[0:9], row[9:18] = np.linalg.inv(S).astype(np.float64).reshape(-1), S.astype(np.float64).reshape(-1)
    row[18:27], row[27:36] = np.linalg.inv(Sh).astype(np.float64).reshape(-1), Sh.astype(np.float64).reshape(-1)
    row[36] = score_gate
    return row


class HomoTracker:
    miopen_find = False          # (the Device* classes: MIOpen find mode around the network work of init / reinit / track_new, capture included)
    _label = "per-frame"         # (how the warning of a failed capture names the body)
    _per_sample = False          # the score that gates: sample 0's (hdn_l1_score2_f32) / every sample's own (hdn_l1_score2_batch_f32)

    def __init__(self, hm_net, iterations: int = 1, similarity=None, score_gate: float = 2.5, graph: bool = False, cfg: TrackerConfig = None):
        """hm_net: hdn_amd.HomoModelBuilder (or the reference's, after install()) in eval mode on the GPU.
        iterations: trip count of the refinement loop (1 in the shipped tracker, :242; 2 in BASELINE config 5).
        similarity: None (identity) or a DeviceSimilarity: `.init(frame, init_pos, init_s_z, init_s_z_sm, avg)` once per
        sequence, `(stabilised_frame) -> views into its device state record` per frame (no host values).
        graph: replay the whole per-frame body as ONE hipGraph (several hundred launches at B = 1 are launch-latency bound)."""
        self.net, self.n = hm_net, 1       # n: sequences advanced per call
        self.cfg = cfg or (similarity.cfg if similarity is not None and hasattr(similarity, "cfg") else TrackerConfig())
        self.use_graph = bool(graph)
        self._graph = None
        self.iterations = int(iterations)
        self.similarity = similarity
        self.score_gate = float(score_gate)
        self.host_syncs = 0  # device->host reads this object has caused (the reference: six per frame)

    # -------------------------------------------------------------------------------------------------- init
    def init(self, img, bbox, poly, gt_points, first_point=None):
        """img: BGR uint8 [H,W,3]; bbox (x, y, w, h); poly (cx, cy, w, h, theta); gt_points: the 4 corners."""
        c = self.cfg
        self.dev = next(self.net.parameters()).device
        self.init_pos, self.size, s_z, s_z_sm = _geometry(poly, c)
        self.center_pos, self.init_s_z, self.init_s_z_sm = self.init_pos.copy(), float(s_z), float(s_z_sm)
        frame = FR.upload(img)
        # np.mean(img, axis=(0, 1)) of the first frame: one reduction on the device, read once per sequence
        self.channel_average = frame.to(torch.float64).mean(dim=(0, 1)).cpu().numpy()
        self.host_syncs += 1
        H, W, _ = frame.shape
        self.z_crop_points_sm = FR.crop_points(self.center_pos, self.init_s_z_sm, H, W)
        # get_template_info(get_subwindow_for_homo(...)[:, 0:3]) : the normalised gray template, constant for the sequence
        self.init_homo_tmp = FR.get_search_info(frame, self.center_pos, self.init_s_z_sm, self.channel_average, model_sz=c.exemplar_size)
        with find_mode(self.miopen_find):
            with torch.no_grad():   # ShareFeature(template): constant for the sequence, so not part of the per-frame work
                self.init_patch_1 = self.net.ShareFeature(self.init_homo_tmp).detach()
            if self.similarity is not None:
                self.similarity.init(frame, self.init_pos, self.init_s_z, self.init_s_z_sm, self.channel_average)   # model.template(z_crop), :99-107
        self.init_points = torch.tensor(np.asarray(gt_points, np.float64).reshape(1, -1, 2), dtype=torch.float64, device=self.dev).contiguous()
        self.n_points = self.init_points.shape[1]      # any number of initial points (cv2.perspectiveTransform takes any; POT gives 4)
        self.H_total = torch.eye(3, dtype=torch.float64, device=self.dev)
        self._Ht, self._Hinv = (torch.empty((3, 3), dtype=torch.float64, device=self.dev) for _ in range(2))
        self._out = torch.empty((1, 2 * self.n_points + 1), dtype=torch.float32, device=self.dev)
        self._const_params = FR._dev_f64([self.init_pos[0], self.init_pos[1], self.init_s_z_sm] + [float(a) for a in self.channel_average], self.dev)
        self._graph = None
        self._consts = torch.from_numpy(_const_row(self.z_crop_points_sm, c.exemplar_size, self.score_gate)).to(self.dev)

    # -------------------------------------------------------------------------------------------------- one frame (of each of the n sequences)
    def _body(self, frames):
        """Everything of a frame that runs on the device, from the uploaded frame(s) - [H,W,3], [n,H,W,3] or an arena - to the projected corners; no
        host reads, no allocations that depend on data: capturable in a hipGraph when the frames are a static buffer.  H_total ([3,3] / [n,3,3]
        float64, a buffer of this object) advances in place.
        -> (out float32 [n, 2 * points + 1] = corners (x, y) + best_score per sequence (a buffer of this object), the gating score)."""
        lib, n = _lib.load(), self.n
        # :150-155  undo the accumulated motion (a singular H_total is reset to the identity, as the reference does).
        # hdn_frame_warp_perspective_u8 inverts its matrix itself (cv2 semantics), so it is handed inv(H_total), every sequence its own.
        _lib.launch("track prepare", self.dev, lib.hdn_track_prepare_f64, _lib.ptr(self.H_total), _lib.ptr(self._Ht), _lib.ptr(self._Hinv), n)
        frames = FR.warp_perspective(frames, self._Hinv.view(n, 9))
        sim_state = None
        if self.similarity is not None:
            # :157-214 on the STABILISED frame; :223 rotate back by -rot_delta about the new centre (bicubic; rot 0 = identity)
            sim = self.similarity(frames)
            sim_state, params = self.similarity.state, sim["params_homo"]
            rot_img = FR.warp_affine_cubic(frames, sim["rot_matrix"])
        else:
            params, rot_img = self._const_params, frames
        # :224-239  cut the homography crop, normalise
        search = FR.get_search_info(rot_img, None, None, None, model_sz=self.cfg.exemplar_size, params=params)
        # :242-250  refinement loop around track_proj
        H_comp, homo_score, _ = homo_refine(self.net, self.init_homo_tmp, search, iterations=self.iterations, patch_1=self.init_patch_1,
                                            per_sample=self._per_sample)
        # :251-272  un-scale, un-shift, gate, accumulate, project the initial corners
        score = homo_score.detach().reshape(-1).to(torch.float32).contiguous()
        _lib.launch("track accumulate", self.dev, lib.hdn_track_accumulate_f64, _lib.ptr(self._Ht), _lib.opt(sim_state), _lib.ptr(H_comp), _lib.ptr(score),
                    _lib.ptr(self._consts), _lib.ptr(self.init_points), self.n_points,
                    _lib.ptr(self.H_total), _lib.ptr(self._out), n)     # (in place: the kernel reads Ht, the copy hdn_track_prepare_f64 made)
        return self._out, (score if self._per_sample else homo_score)

    def _static_input(self, img):
        return torch.empty(tuple(np.shape(img)), dtype=torch.uint8, device=self.dev)

    def _frames(self, img, into=None):
        """This step's frame on the device, or copied into `into` (the static input of the captured graph)."""
        if into is None:
            return FR.upload(img)
        t = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
        if tuple(t.shape) != tuple(into.shape) or t.dtype != torch.uint8:
            raise ValueError(f"graph mode was captured for uint8 frames of shape {tuple(into.shape)}, got {t.dtype} {tuple(t.shape)}")
        return into.copy_(t, non_blocking=True)

    def _capture(self, imgs):
        """hipGraph of the whole per-frame body.  The frames land in a static device buffer; H_total is carried in a static tensor updated
        in place by the graph itself (the recurrence lives inside the graph; the warm-up's advance of it is put back); the similarity state
        record is a static tensor of the DeviceSimilarity.  A body that cannot be captured: use_graph goes False, eager from here on."""
        self._static_frame = self._static_input(imgs)
        got = capture_graph(lambda: self._body(self._static_frame), [self.H_total], self._label)
        self.use_graph = got is not None
        if got is not None:
            self._graph, (self._g_out, self._g_score) = got

    def _step(self, imgs, sync):
        """Capture on first use; the frames into the static input and one replay, or the body eagerly.  -> (out, score) that a later step leaves alone
        (sync: the caller reads `out` to the host before that, so the graph's own buffer will do)."""
        with find_mode(self.miopen_find):
            if self.use_graph and self._graph is None:
                self._capture(imgs)                    # (may switch use_graph off)
            if self.use_graph:
                self._frames(imgs, into=self._static_frame)
                self._graph.replay()
                out, score = self._g_out, self._g_score
                if not sync:  # the graph's static outputs are overwritten by the next replay: hand out copies
                    out, score = out.clone(), score.clone()
            else:
                out, score = self._body(self._frames(imgs))
                out = out.clone()
        return out, score

    def track_new(self, fr_idx, img, gt_box=None, gt_poly=None, gt_points=None, sync: bool = True):
        out, self.last_score = self._step(img, sync)
        P = self.n_points
        pts = self.last_points = out[0, :2 * P].view(P, 2)
        if not sync:
            return {"points": pts, "polygon": pts, "best_score": out[0, 2 * P]}
        host = out.cpu().numpy()
        self.host_syncs += 1
        return homography_result(host[0], P)

    def track(self, img):
        """BaseTracker.track (hdn/tracker/base_tracker.py:28-37, abstract there): the next frame, nothing else known."""
        return self.track_new(None, img)

    def similarity_state(self) -> dict:
        """The last frame's similarity record read back to the host (one extra device->host read, counted): centre, deltas,
        scale / rotation increments, scores.  The reference keeps `center_pos`, `rot`, `scale` as host attributes updated every
        frame (hdn_tracker_proj_e2e.py:185,215-216); nothing outside the tracker reads them and here they live on the device
        only, so they are produced on demand instead of costing every frame a synchronisation."""
        if self.similarity is None or self.similarity.state is None:
            return {}
        from .similarity import state_fields
        row = self.similarity.state.view(-1).cpu()
        self.host_syncs += 1
        f = {k: v.numpy().copy() for k, v in state_fields(row).items()}
        self.center_pos = f["center"].astype(np.float64).copy()
        return f


def hip_trunk_enabled() -> bool:
    """HDN_HIP_TRUNK (default 0): do the device trackers attach the folded HIP trunk to model.hm_net when `hip_trunk` is not given?"""
    return env_flag("HDN_HIP_TRUNK", "0")


def attach_hip_trunk(model, hip_trunk) -> bool:
    """optimize_trunk(model.hm_net, channels_last=True) when `hip_trunk` (None: HDN_HIP_TRUNK) is on and the model is on a GPU; was it attached?"""
    if not (hip_trunk_enabled() if hip_trunk is None else hip_trunk) or not next(model.hm_net.parameters()).is_cuda:
        return False
    from .homo_model import optimize_trunk
    optimize_trunk(model.hm_net, channels_last=True)
    return True


class DeviceTrackerHomo(HomoTracker):
    """Drop-in for hdnTrackerHomo (hdn_tracker_proj_e2e.py:22-285) behind build_tracker(model)
    (hdn/tracker/tracker_builder.py:18-19): same constructor argument, same init / track_new signatures and result keys.
    `model` is the reference's ModelBuilder (hm_net = the homography estimator, template / track_new / track_new_lp = the
    similarity branch).  Each frame is replayed as ONE hipGraph, captured at a sequence's first frame (2.9 against 5.3 ms per frame with the
    production-shaped model: at B = 1 the loop is launch-bound; a body that cannot be captured falls back to eager launches with a warning;
    graph=False or HDN_TRACKER_GRAPH=0: eager).  The model's backbone and necks are switched to their
    BatchNorm-folded, epilogue-fused form (hdn_amd.backbone; fold_backbone=False or HDN_FOLD_BACKBONE=0: left as they are).
    hip_trunk=True (None: HDN_HIP_TRUNK, default 0): model.hm_net's homography trunk (cfg.BACKBONE_HOMO.TYPE resnet34 or resnet50) gets its
    BatchNorm-folded HIP form attached (hdn_amd.homo_model.optimize_trunk(model.hm_net, channels_last=True); enable=False there undoes it)."""

    def __init__(self, model, graph: bool = None, iterations: int = 1, cfg: TrackerConfig = None, fold_backbone: bool = None, hip_trunk: bool = None):
        self.model = model
        cfg, _, graph, self.miopen_find, self.folded = device_setup(model, cfg, graph, fold_backbone)
        self.hip_trunk = attach_hip_trunk(model, hip_trunk)
        super().__init__(model.hm_net, iterations=iterations, similarity=DeviceSimilarity(model, cfg), graph=graph, cfg=cfg)
        if (self.folded or self.miopen_find or self.hip_trunk) and not DeviceTrackerHomo._announced:
            import sys
            DeviceTrackerHomo._announced = True      # once per process
            print("hdn_amd: DeviceTrackerHomo" +
                  (" switched %s of the model it was given to their BatchNorm-folded form (parameters / state_dict unchanged; "
                   "hdn_amd.backbone.restore_similarity_model(model) or HDN_FOLD_BACKBONE=0 undoes it)" % " / ".join(self.folded) if self.folded else "") +
                  ((" and" if self.folded else "") + " attached the folded HIP homography trunk to model.hm_net (hip_trunk / HDN_HIP_TRUNK; "
                   "hdn_amd.homo_model.optimize_trunk(model.hm_net, enable=False) undoes it)" if self.hip_trunk else "") +
                  (" and" if (self.folded or self.hip_trunk) and self.miopen_find else "") +
                  (" runs its networks under MIOpen find mode (torch.backends.cudnn.benchmark, raised around this tracker's calls only; "
                   "HDN_MIOPEN_FIND=0: torch's setting as it is)" if self.miopen_find else ""), file=sys.stderr)

    _announced = False
