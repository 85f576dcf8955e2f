"""The stand-in model, the batches and the CPU twin that tests/test_gpu_simi_training_forward.py shares between its host and its GPU parts for
hdn_amd.simi_training_forward (hdn_amd/simi_train.py).  Nothing here touches the device.

The model has the reference's attribute names around small networks, so that the glue is what is tested: a two-convolution backbone (127 -> 15,
255 -> 31, stride 8 as the reference's), 1 x 1 necks (the template neck crops to 7 x 7 as AdjustLayer does), heads made of 3 x 3 convolutions, one
depthwise correlation (`xcorr`: hdn_amd.xcorr_depthwise on the device, xcorr_ref in the twin) and 1 x 1 convolutions, hdn_amd.STN_PolarTrain, and
hdn_amd.HomoModelBuilder with a two-convolution regressor in place of the ResNet.  The model is in eval() mode with ShareFeature.hip_train = True:
BatchNorm on seeded running statistics, differentiable, and nothing is updated by a forward, so a replayed graph and an eager call see one state.

Each head adds a fixed `prior` to its class map: +-6 on the two logits at one cell per sample.  It gives the argmax of :377 and :390 a margin that
no rounding can cross (the host part asserts it against the fp32 twin's own error), so an index flip cannot be mistaken for a rounding difference.

The twin is ModelBuilder.forward (model_builder_e2e_unconstrained_v2.py:361-563) and HomoModelBuilder.forward (homo_model_builder.py:154-215) written
from stock PyTorch and the restatements of tests/*_cases.py (logpolar_rs, stn_rs, dlt_rs, transformer_rs, the r_* geometry, ref_a .. ref_d, the corner
supervision of corner_loss_cases.Case.evaluate), with the index sets from nonzero() as the reference forms them, at float64 (the truth) and at
fp32 (d_ref).  One difference is carried over on purpose: with no selected sample the homography estimator's feature_loss is 0, not 0 / 0.

The chain bound of the project: a value or gradient of the device may deviate from float64 by max(4 d_ref, 1e-5), d_ref the fp32 CPU twin's own
deviation (max abs over the tensor).
"""
import copy
import functools

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import corner_loss_cases as CC
import simi_geometry_cases as SG
import sup_loss_cases as SL
from affine_stn_cases import stn_rs
from geometry_bwd_cases import dlt_rs, logpolar_rs, transformer_rs

SEED = 20261021
B = 5
FLAGS = {"mixed": ([1, 0, 1, 0, 1], [0, 0, 1, 1, 0]),            # (sup,pos) (sup,neg) (unsup,pos) (unsup,neg) (sup,pos)
         "no_unsup_pos": ([1, 0, 1, 0, 1], [0, 0, 0, 1, 0]),     # the only unsupervised sample is a negative: n_unsup_pos = 0, n_unsup = 1
         "no_neg": ([1, 1, 1, 1, 1], [0, 1, 1, 0, 0])}           # no negative: rule 1 sums every sample and divides by n_sel = 2
PRIOR = 6.0
CELLS = ((12, 13), (11, 12), (13, 11), (12, 12), (14, 13))       # (row, col) of the prior in the 25 x 25 map, one per sample
CELLS_LP = ((6, 7), (5, 6), (7, 6), (6, 6), (6, 5))              # and in the 13 x 13 map
OUTPUT_KEYS = ("cls_loss_sup", "loc_loss_sup", "cls_loss_lp_sup", "loc_loss_lp_sup", "sim_cent_loss", "sim_loss", "cor_err_aug", "cor_err_sim",
               "cor_err", "cor_loss", "cor_pos_loss", "cor_neg_loss", "homo_unsup_loss", "total_loss")


def bound(d_ref):
    return max(4.0 * d_ref, 1e-5)


def xcorr_ref(x, k):
    """out[b,c,i,j] = sum_uv x[b,c,i+u,j+v] k[b,c,u,v] on stock PyTorch"""
    b, c, h, w = k.shape
    out = F.conv2d(x.reshape(1, b * c, x.shape[2], x.shape[3]), k.reshape(b * c, 1, h, w), groups=b * c)
    return out.reshape(b, c, out.shape[2], out.shape[3])


# ------------------------------------------------------------------------------------------------------------------------------------ the model
class Backbone(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1, self.conv2 = nn.Conv2d(3, 6, 7, stride=4), nn.Conv2d(6, 8, 3, stride=2)

    def forward(self, x):
        return torch.tanh(self.conv2(torch.tanh(self.conv1(x))))


class Neck(nn.Module):
    def __init__(self, crop):
        super().__init__()
        self.conv, self.crop = nn.Conv2d(8, 8, 1), crop

    def forward(self, x):
        x = self.conv(x)
        if self.crop and x.shape[3] < 20:                        # AdjustLayer: the template's 15 x 15 map is cut to its central 7 x 7
            x = x[:, :, 4:11, 4:11]
        return x


class Head(nn.Module):
    """3 x 3 convolutions on both branches, one depthwise correlation, 1 x 1 convolutions: 7 / 31 -> 5 (x) 29 -> 25 for the head,
    15 / 15 -> central 3 of 13 (x) 15 -> 13 for the log-polar head."""

    def __init__(self, loc_channels, cells, S, lp):
        super().__init__()
        self.lp = lp
        self.k, self.s = nn.Conv2d(8, 8, 3), nn.Conv2d(8, 8, 3, padding=1 if lp else 0)
        self.cls, self.loc = nn.Conv2d(8, 2, 1), nn.Conv2d(8, loc_channels, 1)
        prior = torch.zeros(len(cells), 2, S, S)
        for b, (r, c) in enumerate(cells):
            prior[b, 0, r, c], prior[b, 1, r, c] = -PRIOR, PRIOR
        self.register_buffer("prior", prior)
        self.xcorr = xcorr_ref

    def forward(self, z, x):
        k, s = self.k(z), self.s(x)
        if self.lp:
            k = k[:, :, 5:8, 5:8]
        f = self.xcorr(s.contiguous(), k.contiguous())
        return self.cls(f) + self.prior, self.loc(f)


class StandIn(nn.Module):
    def __init__(self):
        super().__init__()
        import hdn_amd
        self.feature_extractor = Backbone()
        self.neck, self.neck_lp = Neck(True), Neck(False)
        self.head, self.head_lp = Head(2, CELLS, 25, False), Head(4, CELLS_LP, 13, True)
        self.logpolar_instance = hdn_amd.STN_PolarTrain(255)
        self.hm_net = hdn_amd.HomoModelBuilder()
        self.hm_net.backbone = nn.Sequential(nn.Conv2d(2, 8, 5, stride=4), nn.Tanh(), nn.Conv2d(8, 16, 3, stride=2), nn.Tanh())
        self.hm_net.fc = nn.Linear(16, 8)
        self.hm_net.ShareFeature.hip_train = True


def make_model():
    """The seeded stand-in on the CPU, in eval() mode."""
    torch.manual_seed(SEED)
    m = StandIn()
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        for head in (m.head, m.head_lp):
            head.cls.weight.mul_(0.3)
            head.loc.weight.mul_(0.3)
            head.loc.bias.mul_(0.3)
        m.hm_net.fc.bias.copy_(3.0 * (2 * torch.rand(8, generator=g) - 1))           # a warp of a few pixels
        for mod in m.hm_net.ShareFeature.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.copy_(0.2 * (2 * torch.rand(mod.num_features, generator=g) - 1))
                mod.running_var.copy_(0.8 + 0.4 * torch.rand(mod.num_features, generator=g))
                mod.weight.copy_(0.8 + 0.4 * torch.rand(mod.num_features, generator=g))
                mod.bias.copy_(0.1 * (2 * torch.rand(mod.num_features, generator=g) - 1))
    return m.eval()


def on_device(model, dev):
    """A copy of the model on the device with the package's correlation in its heads."""
    import hdn_amd
    m = copy.deepcopy(model).to(dev)
    m.head.xcorr = m.head_lp.xcorr = hdn_amd.xcorr_depthwise
    return m


# ---------------------------------------------------------------------------------------------------------------------------------- the batches
def _smooth(g, b, c, size):
    """an image without pixel noise: 1/8-resolution normal values, interpolated"""
    low = torch.randn(b, c, size // 8 + 2, size // 8 + 2, generator=g)
    return F.interpolate(low, size=(size, size), mode="bilinear", align_corners=False).contiguous()


@functools.lru_cache(maxsize=None)
def make_batch(flags="mixed", seed=0):
    g = torch.Generator().manual_seed(SEED + 100 + seed)
    rng = np.random.default_rng(SEED + 100 + seed)
    d = {"template": _smooth(g, B, 3, 127), "template_lp": _smooth(g, B, 3, 127), "search": _smooth(g, B, 3, 255),
         "template_hm": _smooth(g, B, 3, 127), "search_hm": _smooth(g, B, 3, 255)}
    label_cls = torch.zeros(B, 25, 25)
    label_cls_lp = torch.zeros(B, 13, 13, dtype=torch.int64)
    for b in range(B):
        r, c = CELLS[b]
        label_cls[b, r - 1:r + 2, c - 1:c + 2] = 1.0
        label_cls[b, 0, b] = -1.0                                # an ignored cell
        r, c = CELLS_LP[b]
        label_cls_lp[b, r - 1:r + 2, c - 1:c + 2] = 1
        label_cls_lp[b, 12, b] = -1
    d["label_cls"], d["label_cls_lp"] = label_cls, label_cls_lp
    d["label_loc_c"] = torch.from_numpy(rng.uniform(-1.5, 1.5, (B, 2, 25, 25)).astype(np.float32))
    d["label_loc_lp"] = torch.from_numpy(rng.uniform(-1.5, 1.5, (B, 4, 13, 13)).astype(np.float32))
    tp = CC._quads(rng, B)
    d["template_poly"] = torch.from_numpy(tp.astype(np.float32))
    d["search_poly"] = torch.from_numpy((64.0 + tp + rng.uniform(-6, 6, (B, 4, 2))).astype(np.float32))       # the quad inside the 255 crop
    d["temp_cx"] = torch.from_numpy((63.5 + rng.uniform(-8, 8, B)).astype(np.float32))
    d["temp_cy"] = torch.from_numpy((63.5 + rng.uniform(-8, 8, B)).astype(np.float32))
    pos, un = FLAGS[flags]
    d["if_pos"], d["if_unsup"] = torch.tensor(pos, dtype=torch.float32), torch.tensor(un, dtype=torch.float32)
    return d


# ------------------------------------------------------------------------------------------------------------------------------------- the twin
def _triplet_rows(a, p, n):
    return torch.triplet_margin_loss(a, p, n, 1.0, 1.0, 1e-6, False, 0)


def twin_homo(hm, data, dtype):
    """HomoModelBuilder.forward (homo_model_builder.py:154-215) -> feature_loss [1], homo_neg_loss, x, H_mat"""
    sf = hm.ShareFeature.ShareFeature                            # the stock layers, on the running statistics
    org, inp, h4p = data["org_imgs"], data["input_tensors"], data["h4p"]
    n = org.shape[0]
    p1, p2 = sf(inp[:, :1]), sf(inp[:, 1:])
    x = hm.backbone(torch.cat((p1, p2), 1))
    x = hm.fc(hm.avgpool(x).view(n, -1))
    H = dlt_rs(h4p, x, dtype).reshape(n, 3, 3)
    M = torch.tensor([[63.5, 0.0, 63.5], [0.0, 63.5, 63.5], [0.0, 0.0, 1.0]], dtype=dtype)
    Hn = torch.matmul(torch.matmul(torch.inverse(M).expand(n, 3, 3), H), M.expand(n, 3, 3))
    pred = transformer_rs(org[:, :1], Hn.reshape(n, 9), dtype).permute(0, 3, 1, 2)
    pf = sf(pred)
    if_pos, if_unsup = data["if_pos"], data["if_unsup"]
    neg_ids = if_pos.eq(0).nonzero().squeeze(1)
    pos_ids = (if_pos * if_unsup).eq(1).nonzero().squeeze(1)
    homo_neg_loss = torch.zeros((), dtype=dtype)
    a, p, ng = p2, pf, p1
    if neg_ids.shape[0] != 0:
        a, p, ng = a[pos_ids], p[pos_ids], ng[pos_ids]
        homo_neg_loss = torch.sum(torch.norm(x[neg_ids, :], p=2, dim=1)) / neg_ids.shape[0]
    if pos_ids.shape[0] == 0:
        feature_loss = torch.zeros(1, dtype=dtype)               # the package's statement; the reference divides by zero here
    else:
        feature_loss = (torch.sum(_triplet_rows(a, p, ng)) / pos_ids.shape[0] / (127 * 127)).reshape(1)
    return {"feature_loss": feature_loss, "homo_neg_loss": homo_neg_loss, "x": x, "H_mat": H}


def twin_forward(model, data, dtype):
    """ModelBuilder.forward (:361-563) on the CPU at `dtype` -> (the fourteen outputs, intermediates)"""
    A = SG.TorchA(dtype)
    T = lambda t: t.to(dtype) if t.is_floating_point() else t
    d = {k: T(v) for k, v in data.items()}
    n, ar = B, torch.arange(B)
    if_pos, if_unsup = d["if_pos"], d["if_unsup"]
    zf, zf_lp, xf = (model.feature_extractor(d[k]) for k in ("template", "template_lp", "search"))
    zf, xf = model.neck(zf), model.neck(xf)
    cls, loc = model.head(zf, xf)
    table = torch.as_tensor(SG.analytic_points(8, 25), dtype=dtype)
    best = torch.argmax(cls.detach().reshape(n, 2, -1)[:, 1], 1)                      # :377
    flat = (loc * 8).reshape(n, 2, -1)
    polar = torch.stack(SG.r_polar(A, table[best, 0], table[best, 1], flat[ar, 0, best], flat[ar, 1, best], 1.0), 1)
    tabs = model.logpolar_instance._tables(torch.device("cpu"), 0.0)
    x_lp = logpolar_rs(d["search"], polar, tabs, dtype)                               # :379
    xf_lp = model.neck_lp(model.feature_extractor(x_lp))
    zf_lp = model.neck_lp(zf_lp)
    cls_lp, loc_lp = model.head_lp(zf_lp, xf_lp)
    table_lp = torch.as_tensor(SG.analytic_points(8, 13), dtype=dtype)
    best_lp = torch.argmax(cls_lp.detach().reshape(n, 2, -1).permute(0, 2, 1).softmax(2)[:, :, 1], 1)   # :390
    flat_lp = loc_lp.reshape(n, 4, -1)
    scale, rot = SG.r_lp(A, table_lp[best_lp, 0], table_lp[best_lp, 1], flat_lp[ar, 0, best_lp], flat_lp[ar, 2, best_lp], 8)
    one, zero, half = torch.ones_like(scale), torch.zeros_like(scale), 127 / 2
    p0, p1 = polar[:, 0], polar[:, 1]
    mats = [SG.r_rows(A, SG.r_operands(A, 0, half, half, p0, p1, scale, True, 255, 127), rot),
            SG.r_rows(A, SG.r_operands(A, 1, half, half, p0, p1, 1 / scale, False, 255, 127), -rot),
            SG.r_rows(A, SG.r_operands(A, 0, d["temp_cx"], d["temp_cy"], zero, zero, one, True, 255, 127), zero),
            SG.r_rows(A, SG.r_operands(A, 1, d["temp_cx"], d["temp_cy"], zero, zero, one, False, 255, 127), zero)]
    affine_m, affine_m_lt0, affine_m_c_aug, affine_m_lt0_aug = (A.stack(v, (2, 3)) for v in mats)
    hmg = torch.cat([d["search_poly"].permute(0, 2, 1), torch.ones(n, 1, 4, dtype=dtype)], 1)
    last = torch.tensor([0, 0, 1], dtype=dtype).repeat(n, 1, 1)
    pred_points = torch.bmm(torch.cat([affine_m_lt0, last], 1), hmg)
    aug_sear_points = torch.bmm(torch.cat([affine_m_lt0_aug, last], 1), hmg)
    size = (n, 1, 127, 127)
    warped_search_ori = stn_rs(d["search_hm"], affine_m, size, dtype)                 # :407-408
    search_hm_simi_ori = stn_rs(d["search_hm"], affine_m_c_aug, size, dtype)
    template_mean = d["template_hm"].mean(1, keepdim=True)
    sf = model.hm_net.ShareFeature.ShareFeature
    tmp_f, sear_f = sf(template_mean), sf(search_hm_simi_ori.mean(1, keepdim=True))
    warped_mean = warped_search_ori.mean(1, keepdim=True)
    pre_sear_f = sf(warped_mean)
    ids = CC.set_ids(if_pos.numpy(), if_unsup.numpy())
    up = torch.from_numpy(ids["unsup_pos"])
    out = {k: torch.zeros((), dtype=dtype) for k in OUTPUT_KEYS}
    if len(up):                                                                       # :433-440
        out["sim_loss"] = torch.sum(_triplet_rows(tmp_f[up], pre_sear_f[up], sear_f[up])) / (127 * 127) / len(up)
    org = torch.cat([template_mean, warped_mean], 1)
    h4p = torch.tensor([0, 0, 0, 127, 127, 127, 127, 0], dtype=dtype).repeat(n, 1)
    batch_out = twin_homo(model.hm_net, {"org_imgs": org, "input_tensors": org, "h4p": h4p, "if_pos": if_pos, "if_unsup": if_unsup}, dtype)
    if len(ids["unsup"]):
        out["homo_unsup_loss"] = batch_out["feature_loss"].mean()
    sup = torch.from_numpy(ids["sup"])
    if len(sup):                                                                      # :457-478
        p = F.softmax(cls[sup].permute(0, 2, 3, 1), dim=3)
        logp = F.log_softmax(cls_lp[sup].permute(0, 2, 3, 1), dim=3)
        out["cls_loss_sup"] = SL.ref_a(p, d["label_cls"][sup], 100)[0]
        out["loc_loss_sup"] = SL.ref_b(loc[sup], d["label_loc_c"][sup], d["label_cls"][sup])[0]
        out["cls_loss_lp_sup"] = SL.ref_c(logp, d["label_cls_lp"][sup])
        out["loc_loss_lp_sup"] = SL.ref_d(loc_lp[sup], d["label_loc_lp"][sup], d["label_cls_lp"][sup])
        out["sim_cent_loss"] = 1.0 * (out["cls_loss_lp_sup"] + out["cls_loss_sup"]) + 1.0 * (out["loc_loss_sup"] + out["loc_loss_lp_sup"])
    cc = object.__new__(CC.Case)                                                       # :441-444, :481-523, :552-556
    cc.B, cc.ids, cc.template_poly, cc.w = n, ids, data["template_poly"].numpy(), np.ones(6, dtype=np.float32)
    leaves = {"H_mat": batch_out["H_mat"], "pred_points": pred_points, "aug_sear_points": aug_sear_points, "template_poly": d["template_poly"],
              "x": batch_out["x"]}
    cor = cc.evaluate(CC.TA(dtype), leaves=leaves)
    for k in CC.KEYS:
        out[k] = cor[k]
    out["total_loss"] = out["sim_cent_loss"] * 100 + out["homo_unsup_loss"] + out["cor_neg_loss"] + out["cor_err"] / 4
    mid = {"cls": cls.detach(), "cls_lp": cls_lp.detach(), "best": best, "best_lp": best_lp, "polar": polar.detach(), "scale": scale.detach(),
           "rot": rot.detach(), "counts": cor["counts"]}
    return out, mid


@functools.lru_cache(maxsize=None)
def twin(flags="mixed", seed=0):
    """Computed once and left unchanged: {dtype: (outputs, parameter gradients of total_loss, intermediates)} for float64 and fp32."""
    res = {}
    for dtype in (torch.float64, torch.float32):
        m = copy.deepcopy(make_model()).to(dtype)
        out, mid = twin_forward(m, make_batch(flags, seed), dtype)
        out["total_loss"].backward()
        grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}
        res[dtype] = ({k: v.detach() for k, v in out.items()}, grads, mid)
    return res


def deviation(a, b):
    return float((a.double() - b.double()).abs().max())
