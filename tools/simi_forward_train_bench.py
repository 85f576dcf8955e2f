"""Forward + backward of the similarity model's whole training forward around small stand-in networks, so that the glue is what is timed:
hdn_amd.simi_training_forward against the same lines written with `ids=` and their nonzero() reads: profiles/simi_forward_train.json and one JSON line.

    python tools/simi_forward_train_bench.py [--rounds 7] [--seconds 1.0] [--out profiles/simi_forward_train.json]

A step = model_builder_e2e_unconstrained_v2.py:361-563 and total_loss.backward() at TRAIN.BATCH_SIZE 32 with 24 supervised samples, one sample in
five negative.  The networks are stand-ins with the reference's attribute names (a two-convolution backbone 127 -> 15 / 255 -> 31, 1 x 1 necks,
heads of 3 x 3 convolutions + hdn_amd.xcorr_depthwise + 1 x 1 convolutions, hdn_amd.STN_PolarTrain, hdn_amd.HomoModelBuilder with a two-convolution
regressor, eval() mode with ShareFeature.hip_train): next to the real ResNets the glue measured here is a small part of a step.  In the same process,
on the same inputs and parameters:
  ids      what a user can write today from INTEGRATION.md: the same operators, sim_loss as triplet_l1(..., ids=unsup_pos_ids) behind
           (if_pos * if_unsup).eq(1).nonzero() and a shape read, hm_net.training_forward(homo_data) with its two nonzero() reads, its
           torch.tensor(M) upload and torch.inverse.  The baseline.
  eager    hdn_amd.simi_training_forward: no host read, no upload
  graph    simi_training_forward and total_loss.backward() captured once in a graph and replayed
Before timing, the three forms' fourteen outputs and parameter gradients are compared (1e-4 of the largest element; the bounds against float64 are
the business of tests/test_gpu_simi_training_forward.py).  All forms are warmed up (one untimed window each), then alternate --rounds times; a window
repeats whole steps until at least --seconds have passed on the host clock and is timed by device events around it.  Reported per form: median,
min and max ms per step over the windows, and the spread (max - min) / median.  Nothing is switched by the result and no threshold is fixed in
advance; this tool promises no speed-up.

There is no CPU fallback: without a GPU this tool fails."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

B, N_SUP = 32, 24
PRIOR = 6.0


# ---- the stand-in networks
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
        return x[:, :, 4:11, 4:11] if self.crop and x.shape[3] < 20 else x


class Head(nn.Module):
    """7 / 31 -> 5 (x) 29 -> 25 for the head, 15 / 15 -> central 3 of 13 (x) 15 -> 13 for the log-polar head; `prior` fixes the argmax per sample"""

    def __init__(self, loc_channels, S, lp):
        super().__init__()
        import hdn_amd
        self.lp, self.xcorr = lp, hdn_amd.xcorr_depthwise
        self.k, self.s = nn.Conv2d(8, 8, 3), nn.Conv2d(8, 8, 3, padding=1 if lp else 0)
        self.cls, self.loc = nn.Conv2d(8, 2, 1), nn.Conv2d(8, loc_channels, 1)
        prior = torch.zeros(B, 2, S, S)
        for b in range(B):
            r, c = S // 2 - 1 + b % 3, S // 2 - 1 + (b // 3) % 3
            prior[b, 0, r, c], prior[b, 1, r, c] = -PRIOR, PRIOR
        self.register_buffer("prior", prior)

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
        self.head, self.head_lp = Head(2, 25, False), Head(4, 13, True)
        self.logpolar_instance = hdn_amd.STN_PolarTrain(255)
        self.hm_net = hdn_amd.HomoModelBuilder()
        self.hm_net.backbone = nn.Sequential(nn.Conv2d(2, 8, 5, stride=4), nn.Tanh(), nn.Conv2d(8, 16, 3, stride=2), nn.Tanh())
        self.hm_net.fc = nn.Linear(16, 8)
        self.hm_net.ShareFeature.hip_train = True


def make_model(dev):
    torch.manual_seed(20261021)
    m = StandIn()
    with torch.no_grad():
        for head in (m.head, m.head_lp):
            for p in (head.cls.weight, head.loc.weight, head.loc.bias):
                p.mul_(0.3)
        m.hm_net.fc.bias.uniform_(-3.0, 3.0)
    return m.eval().to(dev)


def make_inputs(dev):
    gen = torch.Generator().manual_seed(20261022)
    un = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=gen)
    img = lambda size: F.interpolate(torch.randn(B, 3, size // 8 + 2, size // 8 + 2, generator=gen), size=(size, size), mode="bilinear")
    d = {k: img(s) for k, s in (("template", 127), ("template_lp", 127), ("search", 255), ("template_hm", 127), ("search_hm", 255))}
    d["label_cls"] = torch.zeros(B, 25, 25)
    d["label_cls"][:, 11:14, 11:14] = 1.0
    d["label_cls_lp"] = torch.zeros(B, 13, 13, dtype=torch.int64)
    d["label_cls_lp"][:, 5:8, 5:8] = 1
    d["label_loc_c"], d["label_loc_lp"] = un(-1.5, 1.5, B, 2, 25, 25), un(-1.5, 1.5, B, 4, 13, 13)
    far = torch.tensor([[0, 0], [0, 1], [1, 1], [1, 0]], dtype=torch.float32)
    near = un(5, 40, B, 4, 2)
    d["template_poly"] = torch.where(far.bool(), 127 - near, near)                         # quads inside 127 x 127, sides >= 47 px
    d["search_poly"] = 64.0 + d["template_poly"] + un(-6, 6, B, 4, 2)
    d["temp_cx"], d["temp_cy"] = 63.5 + un(-8, 8, B), 63.5 + un(-8, 8, B)
    d["if_unsup"] = (torch.arange(B) >= N_SUP).float()
    d["if_pos"] = (torch.arange(B) % 5 != 4).float()
    return {k: v.contiguous().to(dev) for k, v in d.items()}


# ---- the baseline: the same operators with ids= and the host reads that go with them
def ids_forward(model, data):
    import hdn_amd
    from hdn_amd.simi_train import homo_constants
    if_pos, if_unsup = data["if_pos"], data["if_unsup"]
    n = data["search"].shape[0]
    zf, zf_lp, xf = (model.feature_extractor(data[k]) for k in ("template", "template_lp", "search"))
    zf, xf = model.neck(zf), model.neck(xf)
    cls, loc = model.head(zf, xf)
    polar = hdn_amd.polar_pick(cls.detach(), loc, stride=8)
    x_lp, _ = model.logpolar_instance(data["search"], polar)
    zf_lp, xf_lp = model.neck_lp(zf_lp), model.neck_lp(model.feature_extractor(x_lp))
    cls_lp, loc_lp = model.head_lp(zf_lp, xf_lp)
    g = hdn_amd.similarity_warps(cls_lp.detach(), loc_lp, polar, data["temp_cx"], data["temp_cy"], data["search_poly"])
    size = (n, 1, 127, 127)
    warped = hdn_amd.affine_sample(data["search_hm"], g["affine_m"], size, differentiable=True)
    simi = hdn_amd.affine_sample(data["search_hm"], g["affine_m_c_aug"], size, differentiable=True)
    template_mean, warped_mean = data["template_hm"].mean(1, keepdim=True), warped.mean(1, keepdim=True)
    sf = model.hm_net.ShareFeature
    tmp_f, sear_f, pre_sear_f = sf(template_mean), sf(simi.mean(1, keepdim=True)), sf(warped_mean)
    unsup_pos_ids = (if_pos * if_unsup).eq(1).nonzero().squeeze(1)                         # a host read: the shape
    sim_loss = torch.zeros((), device=if_pos.device)
    if unsup_pos_ids.shape[0] != 0:
        mat = hdn_amd.triplet_l1(tmp_f, pre_sear_f, sear_f, ids=unsup_pos_ids, differentiable=True)
        sim_loss = torch.sum(mat) / (127 * 127) / unsup_pos_ids.shape[0]
    h4p, patch_indices = homo_constants(n, if_pos.device)
    org = torch.cat([template_mean, warped_mean], 1)
    batch_out = model.hm_net.training_forward({"org_imgs": org, "input_tensors": org, "h4p": h4p, "patch_indices": patch_indices,
                                               "if_pos": if_pos, "if_unsup": if_unsup})  # two nonzero() reads, an upload, torch.inverse
    head = hdn_amd.supervised_losses(cls, loc, cls_lp, loc_lp, data["label_cls"], data["label_loc_c"], data["label_cls_lp"], data["label_loc_lp"],
                                     if_unsup=if_unsup)
    cor = hdn_amd.corner_losses(batch_out["H_mat"], g["pred_points"], data["template_poly"], batch_out["x"], if_pos, if_unsup,
                                aug_sear_points=g["aug_sear_points"])
    return hdn_amd.training_outputs(head, cor, sim_loss, batch_out["feature_loss"].mean(), 1.0, 1.0)


def make_step(fn, model, data):
    params = [p for p in model.parameters()]

    def step():
        for p in params:
            p.grad = None
        out = fn(model, data)
        out["total_loss"].backward()
        return out
    return step


def snapshot(out, model):
    return {k: v.detach().clone() for k, v in out.items()}, {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def make_graph_step(model, data):
    import hdn_amd
    step = make_step(hdn_amd.simi_training_forward, model, data)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for p in model.parameters():
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hdn_amd.simi_training_forward(model, data)
        out["total_loss"].backward()
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    return graph.replay, out, grads


def window(step, seconds):
    """Whole steps until `seconds` have passed on the host, device events around them -> (ms per step, steps)."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0, steps = time.perf_counter(), 0
    e0.record()
    while True:
        step()
        steps += 1
        if steps % 4 == 0:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= seconds:
                break
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, steps


def summary(ms):
    med = statistics.median(ms)
    return {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4)}


def worst(a, b):
    return max(float((a[k] - b[k]).abs().max() / b[k].abs().max().clamp_min(1e-6)) for k in b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simi_forward_train.json"))
    args = ap.parse_args()
    if args.rounds < 5 or args.seconds < 0.5:
        ap.error("at least five alternations, each window at least half a second")
    if not torch.cuda.is_available():
        raise SystemExit("tools/simi_forward_train_bench.py measures on a GPU; there is none here")
    import hdn_amd
    dev = torch.device("cuda:0")
    model, data = make_model(dev), make_inputs(dev)
    replay, g_out, g_grads = make_graph_step(model, data)                                # captured first: the eager steps below replace .grad
    replay()
    torch.cuda.synchronize()
    graph_out, graph_grads = {k: v.detach().clone() for k, v in g_out.items()}, {k: v.detach().clone() for k, v in g_grads.items()}
    steps = {"ids": make_step(ids_forward, model, data), "eager": make_step(hdn_amd.simi_training_forward, model, data)}
    ids_out, ids_grads = snapshot(steps["ids"](), model)
    eager_out, eager_grads = snapshot(steps["eager"](), model)
    assert set(ids_out) == set(eager_out) == set(graph_out) and set(ids_grads) == set(eager_grads) == set(graph_grads)
    agreement = {"eager_against_ids_outputs": float("%.3g" % worst(eager_out, ids_out)),
                 "eager_against_ids_gradients": float("%.3g" % worst(eager_grads, ids_grads)),
                 "graph_against_eager_outputs": float("%.3g" % worst(graph_out, eager_out)),
                 "graph_against_eager_gradients": float("%.3g" % worst(graph_grads, eager_grads))}
    assert max(agreement.values()) <= 1e-4, f"the three forms disagree: {agreement}"
    steps["graph"] = replay
    names = ("eager", "ids", "graph")
    for name in names:
        window(steps[name], args.seconds)
        print(f"[simi_forward_train_bench] {name}: warm", file=sys.stderr, flush=True)
    ms, counts = {name: [] for name in names}, {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            v, n = window(steps[name], args.seconds)
            ms[name].append(v)
            counts[name].append(n)
            print(f"[simi_forward_train_bench] {name}: {v:.4f} ms per step over {n} steps", file=sys.stderr, flush=True)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "B": B, "n_sup": N_SUP,
           "parameters": sum(p.numel() for p in model.parameters()), "rounds": args.rounds, "window_seconds": args.seconds,
           "steps_per_window": counts, "agreement": agreement, "outputs": {k: float(v) for k, v in eager_out.items()}}
    for name in names:
        res[name] = summary(ms[name])
    res["ids_over_eager"] = round(res["ids"]["median"] / res["eager"]["median"], 3)
    res["eager_over_graph"] = round(res["eager"]["median"] / res["graph"]["median"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
