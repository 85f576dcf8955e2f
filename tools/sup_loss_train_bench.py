"""Forward + backward of the training step's supervised head losses, hdn_amd.losses (csrc/sup_losses.hip) against the reference's formulation on
PyTorch-ROCm: profiles/sup_loss_train.json and one JSON line.

    python tools/sup_loss_train_bench.py [--rounds 7] [--seconds 1.0] [--out profiles/sup_loss_train.json]

A step = what model_builder_e2e_unconstrained_v2.py:457-478 does at TRAIN.BATCH_SIZE 32 with 24 supervised samples (WEIGHTED_MAP_LP: False): the raw
head maps cls, loc [32,2,25,25], cls_lp [32,2,13,13], loc_lp [32,4,13,13] require grad; the four losses are formed, added, and one backward delivers
the four gradients.  In the same process, on the same inputs:
  reference          the reference's formulation restated in PyTorch: if_unsup.eq(0).nonzero(), eight x[sup_ids] gathers, softmax / log_softmax over
                     the permuted maps, and the four loss functions with their nonzero().squeeze() / index_select / topk / reductions
  drop_ins           the same lines with the five hdn_amd.losses drop-ins in place of the four functions: what install(train=True) gives the
                     reference while SUP_LOSS_TRAIN_BOUND
  supervised_losses  hdn_amd.supervised_losses on the raw maps with the mask: one launch forward, one backward, no nonzero()
Before timing, the three sides' losses are compared (1e-5 relative) and their gradients (1e-2 of the largest element: a coarse check that the
sides compute the same thing - the gradient of -log(1 - p) moves by 0.2 % per ulp of p at 1 - p = 3e-5, and softmax's backward forms 1 - p a
second time; the bounds against float64 are the business of tests/test_gpu_sup_loss.py).  All sides are warmed up (one
untimed window each), then alternate --rounds times; a window repeats whole steps until at least --seconds have passed on the host clock and is
timed by device events around it.  Reported per side: median, min and max ms per step over the windows.
`ahead`: is the drop_ins median below the reference median by more than the larger of the two sides' (max - min)?  It decides
hdn_amd.install.SUP_LOSS_TRAIN_BOUND.  This tool promises no speed-up.

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
import torch.nn.functional as F  # noqa: E402

B, N_SUP, S, S_LP = 32, 24, 25, 13
MAPS = ("cls", "loc", "cls_lp", "loc_lp")


def make_inputs(dev):
    gen = torch.Generator().manual_seed(20261021)
    rn = lambda *s: torch.randn(*s, generator=gen)
    t = {"cls": 2 * rn(B, 2, S, S), "loc": rn(B, 2, S, S), "cls_lp": 2 * rn(B, 2, S_LP, S_LP), "loc_lp": rn(B, 4, S_LP, S_LP),
         "label_loc_c": rn(B, 2, S, S), "label_loc_lp": rn(B, 4, S_LP, S_LP)}
    r = torch.rand(B, S, S, generator=gen)
    t["label_cls"] = torch.where(r < 0.6, torch.zeros(()), torch.where(r < 0.9, 0.3 + 0.7 * torch.rand(B, S, S, generator=gen), -torch.ones(())))
    r = torch.rand(B, S_LP, S_LP, generator=gen)
    t["label_cls_lp"] = torch.where(r < 0.5, 0, torch.where(r < 0.8, 1, -1)).long()
    t["if_unsup"] = torch.tensor([1.0 if i % 4 == 1 else 0.0 for i in range(B)])
    t = {k: v.to(dev) for k, v in t.items()}
    for k in MAPS:
        t[k].requires_grad_(True)
    return t


# ---- the reference's formulation (hdn/models/loss.py), restated: every nonzero() below is a host synchronisation
def _hits(mask):
    return mask.nonzero().squeeze()


def _empty(idx):
    return idx.dim() == 0 or idx.numel() == 0


def _smooth(d):
    a = d.abs()
    near = a.lt(1).float()
    return near * (0.5 * d ** 2) + (1 - near) * (a - 0.5)


def ref_top_k(pred, label):
    n = label.shape[0]
    label, pred = label.reshape(-1), pred.view(-1, 2)
    neg, pos = _hits(label.eq(0)), _hits(label.gt(0))
    zero = torch.tensor(0.0).to(pred.device)
    pos_loss = zero
    if not _empty(pos):
        ap = (label[pos] - torch.index_select(pred, 0, pos)[:, 1]).abs()
        pos_loss = ap.sum() / (ap.shape[0] + 1)
    neg_loss = zero
    if not _empty(neg):
        pn = torch.index_select(pred, 0, neg)[:, 1].clamp(min=0.000001, max=0.9999999)
        top = torch.topk(-torch.log(1 - pn), n * 100).values
        neg_loss = top.sum() / (top.shape[0] + 1)
    return pos_loss + neg_loss


def ref_l1_c(pred, target, label):
    label = label.reshape(-1)
    pos = _hits(label.gt(label.max() - 0.2))
    if _empty(pos):
        return torch.tensor(0.0).to(pred.device)
    pred, target = (torch.index_select(x.permute(0, 2, 3, 1).reshape(-1, 2), 0, pos) for x in (pred, target))
    return _smooth(pred - target).sum() / (target.shape[0] * target.shape[1] + 1)


def ref_cross_entropy(pred, label):
    pred, label = pred.view(-1, 2), label.view(-1)

    def term(idx):
        return 0 if _empty(idx) else F.nll_loss(torch.index_select(pred, 0, idx), torch.index_select(label, 0, idx))
    return term(_hits(label.eq(1))) * 0.5 + term(_hits(label.eq(0))) * 0.5


def ref_kalyo(output, target):
    return _smooth(target - output).sum() / (output.shape[0] * output.shape[1] + 1)


def ref_l1(pred, target, label):
    pos = _hits(label.reshape(-1).gt(0))
    pred, target = (torch.index_select(x.permute(0, 2, 3, 1).reshape(-1, 4), 0, pos) for x in (pred, target))
    return ref_kalyo(pred, target)


def make_step(kind, t):
    if kind == "reference":
        fa, fb, fc, fd = ref_top_k, ref_l1_c, ref_cross_entropy, ref_l1
    else:
        import hdn_amd
        fa, fb, fc, fd = (hdn_amd.select_xr_focal_fuse_smooth_l1_loss_top_k, hdn_amd.select_l1_loss_c, hdn_amd.select_cross_entropy_loss,
                          hdn_amd.select_l1_loss)

    def step():
        for k in MAPS:
            t[k].grad = None
        if kind == "supervised_losses":
            d = hdn_amd.supervised_losses(t["cls"], t["loc"], t["cls_lp"], t["loc_lp"], t["label_cls"], t["label_loc_c"], t["label_cls_lp"],
                                          t["label_loc_lp"], if_unsup=t["if_unsup"])
            losses = [d[k] for k in hdn_amd.losses.KEYS]
        else:
            ids = t["if_unsup"].eq(0).nonzero().squeeze(1)
            losses = [0, 0, 0, 0]
            if len(ids) > 0:
                g = {k: t[k][ids] for k in t if k != "if_unsup"}
                p = F.softmax(g["cls"].permute(0, 2, 3, 1).contiguous(), dim=3)
                logp = F.log_softmax(g["cls_lp"].permute(0, 2, 3, 1).contiguous(), dim=3)
                losses = [fa(p, g["label_cls"]), fb(g["loc"], g["label_loc_c"], g["label_cls"]), fc(logp, g["label_cls_lp"]),
                          fd(g["loc_lp"], g["label_loc_lp"], g["label_cls_lp"])]
        (losses[0] + losses[1] + losses[2] + losses[3]).backward()
        return torch.stack([x.detach() for x in losses]), [t[k].grad.clone() for k in MAPS]
    return step


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sup_loss_train.json"))
    args = ap.parse_args()
    if args.rounds < 5 or args.seconds < 0.5:
        ap.error("at least five alternations, each window at least half a second")
    if not torch.cuda.is_available():
        raise SystemExit("tools/sup_loss_train_bench.py measures on a GPU; there is none here")
    dev = torch.device("cuda:0")
    t = make_inputs(dev)
    names = ("drop_ins", "reference", "supervised_losses")
    steps = {name: make_step(name, t) for name in names}
    ref_losses, ref_grads = steps["reference"]()
    agreement = {}
    for name in ("drop_ins", "supervised_losses"):
        losses, grads = steps[name]()
        dl = float(((losses - ref_losses).abs() / ref_losses.abs().clamp_min(1e-6)).max())
        dg = max(float((g - r).abs().max() / r.abs().max()) for g, r in zip(grads, ref_grads))
        agreement[name] = {"worst_relative_loss_difference": float("%.3g" % dl), "worst_gradient_difference_over_largest": float("%.3g" % dg)}
        assert dl <= 1e-5 and dg <= 1e-2, f"{name} disagrees with the reference's formulation: {agreement}"
    for name in names:
        window(steps[name], args.seconds)
        print(f"[sup_loss_train_bench] {name}: warm", file=sys.stderr, flush=True)
    ms, counts = {name: [] for name in names}, {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            v, n = window(steps[name], args.seconds)
            ms[name].append(v)
            counts[name].append(n)
            print(f"[sup_loss_train_bench] {name}: {v:.4f} ms per step over {n} steps", file=sys.stderr, flush=True)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "B": B, "n_sup": N_SUP, "S": S, "S_lp": S_LP,
           "rounds": args.rounds, "window_seconds": args.seconds, "steps_per_window": counts, "against_reference_formulation": agreement,
           "losses": [float(x) for x in ref_losses]}
    for name in names:
        res[name] = summary(ms[name])
    res["reference_over_drop_ins"] = round(res["reference"]["median"] / res["drop_ins"]["median"], 3)
    res["reference_over_supervised_losses"] = round(res["reference"]["median"] / res["supervised_losses"]["median"], 3)
    spread_ms = max(res[n]["max"] - res[n]["min"] for n in ("drop_ins", "reference"))
    res["ahead"] = bool(res["reference"]["median"] - res["drop_ins"]["median"] > spread_ms)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
