"""Forward + backward of the training step's corner supervision and output dictionary, hdn_amd.corner (csrc/corner_losses.hip) against the same lines
formulated on PyTorch-ROCm: profiles/corner_loss_train.json and one JSON line.

    python tools/corner_loss_train_bench.py [--rounds 7] [--seconds 1.0] [--out profiles/corner_loss_train.json]

A step = what model_builder_e2e_unconstrained_v2.py:441-444, :481-523 and :526-562 do at TRAIN.BATCH_SIZE 32 with 24 supervised samples, one sample in
five negative: H_mat [32,3,3], pred_points [32,3,4] and x [32,8] require grad; the corner errors, the two kalyo_l1_loss terms and the fourteen-key
dictionary are formed (the head losses, sim_loss and loss_feature are constants here), and total_loss + cor_loss is backpropagated.  In the same
process, on the same inputs:
  reference       the lines restated in PyTorch with what they cost there: six nonzero() / len() host reads, the index gathers, torch.inverse inside
                  the DLT of every sample, the search-corner constant and the thirteen torch.tensor(0.0).to(device) uploads
  corner_losses   hdn_amd.corner_losses + hdn_amd.training_outputs: one launch forward, one backward, torch.where on the counts, no host read
  graph           corner_losses, training_outputs and the explicit corner_losses_backward captured once in a graph and replayed: the device's own
                  time for the same work, which tells whether the eager windows are bound by the host
Before timing, the two eager sides' dictionaries are compared (2e-3 relative: the reference's fp32 inverse is 1.4e-4 off on general quads) and their
gradients (1e-2 of the largest element); the bounds against float64 are the business of tests/test_gpu_corner_loss.py.  All sides are warmed up
(one untimed window each), then alternate --rounds times; a window repeats whole steps until at least --seconds have passed on the host clock and
is timed by device events around it.  Reported per side: median, min and max ms per step over the windows.  `host_bound`: is the eager
corner_losses median more than twice the graph's?  Nothing is switched by the result (these lines are statements of the forward: nothing is
rebound), and this tool promises no speed-up.

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

B, N_SUP = 32, 24
CLS_WEIGHT, LOC_WEIGHT = 1.0, 1.2
LEAVES = ("H_mat", "pred_points", "x")
HEAD = ("cls_loss_sup", "loc_loss_sup", "cls_loss_lp_sup", "loc_loss_lp_sup")


def make_inputs(dev):
    gen = torch.Generator().manual_seed(20261021)
    un = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=gen)
    far = torch.tensor([[0, 0], [0, 1], [1, 1], [1, 0]], dtype=torch.float32)
    near = un(5, 40, B, 4, 2)
    tp = torch.where(far.bool(), 127 - near, near)                                       # quads inside 127 x 127, sides >= 47 px
    ones = torch.ones(B, 1, 4)
    H = torch.eye(3).repeat(B, 1, 1)
    H[:, :2, :2] += un(-0.05, 0.05, B, 2, 2)
    H[:, :2, 2] += un(-4, 4, B, 2)
    H[:, 2, :2] += un(-1e-3, 1e-3, B, 2)
    t = {"H_mat": H, "template_poly": tp, "pred_points": torch.cat([(tp + un(-16, 16, B, 4, 2)).permute(0, 2, 1), ones], 1),
         "aug_sear_points": torch.cat([(tp + un(-16, 16, B, 4, 2)).permute(0, 2, 1), ones], 1), "x": un(-20, 20, B, 8),
         "if_unsup": (torch.arange(B) >= N_SUP).float(), "if_pos": (torch.arange(B) % 5 != 4).float()}
    t = {k: v.contiguous().to(dev) for k, v in t.items()}
    for k in LEAVES:
        t[k].requires_grad_(True)
    t["head"] = {k: torch.tensor(0.1 * (i + 1), device=dev) for i, k in enumerate(HEAD)}
    t["sim_loss"], t["loss_feature"] = torch.tensor(0.7, device=dev), torch.tensor(0.9, device=dev)
    return t


# ---- the reference's formulation, restated: every nonzero() / len() below is a host synchronisation
def _kalyo(output, target):
    d = target - output
    a = d.abs()
    near = a.lt(1).float()
    return (near * (0.5 * d ** 2) + (1 - near) * (a - 0.5)).sum() / (output.shape[0] * output.shape[1] + 1)


def _dlt(src, off):
    """the 4-point DLT with torch.inverse over every sample of the batch: src, off [B,4,2] -> H [B,3,3] (rows (x, y, 1, 0, 0, 0, -u x, -u y | u) and
    (0, 0, 0, x, y, 1, -v x, -v y | v) per point, (u, v) = src + off)"""
    n, dev = src.shape[0], src.device
    dst = src + off
    point = torch.cat([src, torch.ones(n, 4, 1).to(dev)], 2)                               # [n,4,3]
    blank = torch.zeros(n, 4, 3).to(dev)
    left = torch.stack([torch.cat([point, blank], 2), torch.cat([blank, point], 2)], 2)    # [n,4,2,6]
    right = -dst.unsqueeze(3) * src.unsqueeze(2)                                           # [n,4,2,2]
    A = torch.cat([left, right], 3).reshape(n, 8, 8)
    h8 = torch.matmul(torch.inverse(A), dst.reshape(n, 8, 1)).reshape(n, 8)
    return torch.cat([h8, torch.ones(n, 1).to(dev)], 1).reshape(n, 3, 3)


def reference_outputs(t):
    dev = t["x"].device
    if_pos, if_unsup, H_mat, pred_points, template_poly, x = (t[k] for k in ("if_pos", "if_unsup", "H_mat", "pred_points", "template_poly", "x"))
    if_neg, if_sup = if_pos.eq(0), if_unsup.eq(0)
    unsup_pos_ids = (if_pos * if_unsup).eq(1).nonzero().squeeze(1)
    unsup_ids = if_unsup.eq(1).nonzero().squeeze(1)
    if unsup_pos_ids.shape[0] != 0:
        simi = pred_points.permute(0, 2, 1)[:, :, :-1][unsup_pos_ids]
        cor_err_sim = torch.sum(torch.abs(simi - template_poly[unsup_pos_ids])) / unsup_pos_ids.shape[0] / 4
    sup_ids = if_unsup.eq(0).nonzero().squeeze(1)
    sup_pos_ids = (if_sup * if_pos).eq(1).nonzero().squeeze(1)
    sup_neg_ids = (if_sup * if_neg).eq(1).nonzero().squeeze(1)
    if len(sup_pos_ids) > 0:
        pts = torch.bmm(H_mat, pred_points).permute(0, 2, 1)
        pts = (pts / pts[:, :, 2].unsqueeze(2))[:, :, :-1]
        poly_pos = template_poly[sup_pos_ids]
        cor_err = torch.sum(torch.abs(pts[sup_pos_ids] - poly_pos)) / sup_pos_ids.shape[0] / 4
        cor_err_aug = torch.sum(torch.abs(t["aug_sear_points"].permute(0, 2, 1)[:, :, :-1][sup_pos_ids] - poly_pos)) / sup_pos_ids.shape[0] / 4
        homo = pred_points.permute(0, 2, 1)
        homo = (homo / homo[:, :, 2].unsqueeze(2))[:, :, :-1]
        H_gt = _dlt(template_poly, homo - template_poly)[sup_pos_ids]
        corner = torch.tensor([[0, 0], [0, 127], [127, 127], [127, 0]]).float().unsqueeze(0).repeat((H_gt.shape[0], 1, 1)).to(dev)
        hmg = torch.cat([corner.permute(0, 2, 1), torch.ones([H_gt.shape[0], 1, 4]).to(dev)], 1)
        warped = torch.bmm(H_gt, hmg).permute(0, 2, 1)
        warped = (warped / warped[:, :, 2].unsqueeze(2))[:, :, :-1]
        pos_loss = _kalyo(x[sup_pos_ids], (warped - corner).reshape(-1, 8))
    neg_ids = if_neg.eq(1).nonzero().squeeze(1)
    if len(neg_ids):
        neg = x[neg_ids]
        neg_loss = _kalyo(neg, torch.zeros_like(neg).to(dev))
    out = {k: torch.tensor(0.0).to(dev) for k in HEAD + ("sim_cent_loss", "sim_loss", "cor_err_aug", "cor_err_sim", "cor_err", "cor_loss",
                                                          "cor_pos_loss", "cor_neg_loss", "homo_unsup_loss")}
    if len(sup_ids) > 0:
        h = t["head"]
        out.update(h)
        out["sim_cent_loss"] = CLS_WEIGHT * (h["cls_loss_lp_sup"] + h["cls_loss_sup"]) + LOC_WEIGHT * (h["loc_loss_sup"] + h["loc_loss_lp_sup"])
    if len(sup_pos_ids) > 0:
        out["cor_err_aug"], out["cor_err"], out["cor_pos_loss"] = cor_err_aug, cor_err, pos_loss
        out["cor_loss"] = out["cor_loss"] + pos_loss
    if len(sup_neg_ids) > 0:
        out["cor_loss"] = out["cor_loss"] + neg_loss
        out["cor_neg_loss"] = neg_loss
    if len(unsup_ids) > 0:
        out["homo_unsup_loss"] = t["loss_feature"]
    if len(unsup_pos_ids) > 0:
        out["sim_loss"], out["cor_err_sim"] = t["sim_loss"], cor_err_sim
    out["total_loss"] = out["sim_cent_loss"] * 100 + out["homo_unsup_loss"] + out["cor_neg_loss"] + out["cor_err"] / 4
    return out


def hip_outputs(t):
    import hdn_amd
    d = hdn_amd.corner_losses(t["H_mat"], t["pred_points"], t["template_poly"], t["x"], t["if_pos"], t["if_unsup"],
                              aug_sear_points=t["aug_sear_points"])
    return hdn_amd.training_outputs(t["head"], d, t["sim_loss"], t["loss_feature"], CLS_WEIGHT, LOC_WEIGHT)


def make_step(kind, t):
    fn = reference_outputs if kind == "reference" else hip_outputs

    def step():
        for k in LEAVES:
            t[k].grad = None
        out = fn(t)
        (out["total_loss"] + out["cor_loss"]).backward()
        return {k: v.detach() for k, v in out.items()}, [t[k].grad.clone() for k in LEAVES]
    return step


def make_graph_step(t, dev):
    """the same work without autograd's bookkeeping, captured once: forward, dictionary, explicit backward for d (total_loss + cor_loss)"""
    import hdn_amd
    d = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in t.items()}
    g = torch.tensor([0.25, 0, 0, 0, 1, 1], device=dev)

    def body():
        c = hdn_amd.corner_losses(d["H_mat"], d["pred_points"], d["template_poly"], d["x"], d["if_pos"], d["if_unsup"],
                                  aug_sear_points=d["aug_sear_points"])
        out = hdn_amd.training_outputs(d["head"], c, d["sim_loss"], d["loss_feature"], CLS_WEIGHT, LOC_WEIGHT)
        gr = hdn_amd.corner_losses_backward(d["H_mat"], d["pred_points"], d["template_poly"], d["x"], d["if_pos"], d["if_unsup"], g,
                                            aug_sear_points=d["aug_sear_points"], need=(True, True, False, True))
        return out, gr, c["counts"]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kept = body()
    return graph.replay, kept


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corner_loss_train.json"))
    args = ap.parse_args()
    if args.rounds < 5 or args.seconds < 0.5:
        ap.error("at least five alternations, each window at least half a second")
    if not torch.cuda.is_available():
        raise SystemExit("tools/corner_loss_train_bench.py measures on a GPU; there is none here")
    dev = torch.device("cuda:0")
    t = make_inputs(dev)
    steps = {name: make_step(name, t) for name in ("reference", "corner_losses")}
    ref_out, ref_grads = steps["reference"]()
    out, grads = steps["corner_losses"]()
    assert set(out) == set(ref_out)
    dl = max(float((out[k] - ref_out[k]).abs() / ref_out[k].abs().clamp_min(1e-6)) for k in ref_out)
    dg = max(float((g - r).abs().max() / r.abs().max()) for g, r in zip(grads, ref_grads))
    agreement = {"worst_relative_output_difference": float("%.3g" % dl), "worst_gradient_difference_over_largest": float("%.3g" % dg)}
    assert dl <= 2e-3 and dg <= 1e-2, f"corner_losses disagrees with the reference's formulation: {agreement}"
    replay, kept = make_graph_step(t, dev)
    replay()
    torch.cuda.synchronize()
    assert all(torch.equal(kept[0][k], out[k]) for k in out), "the replayed graph differs from the eager call"
    steps["graph"] = replay
    names = ("corner_losses", "reference", "graph")
    for name in names:
        window(steps[name], args.seconds)
        print(f"[corner_loss_train_bench] {name}: warm", file=sys.stderr, flush=True)
    ms, counts = {name: [] for name in names}, {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            v, n = window(steps[name], args.seconds)
            ms[name].append(v)
            counts[name].append(n)
            print(f"[corner_loss_train_bench] {name}: {v:.4f} ms per step over {n} steps", file=sys.stderr, flush=True)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "B": B, "n_sup": N_SUP,
           "counts": [int(v) for v in kept[2].cpu()],
           "rounds": args.rounds, "window_seconds": args.seconds, "steps_per_window": counts, "against_reference_formulation": agreement,
           "outputs": {k: float(v) for k, v in ref_out.items()}}
    for name in names:
        res[name] = summary(ms[name])
    res["reference_over_corner_losses"] = round(res["reference"]["median"] / res["corner_losses"]["median"], 3)
    res["corner_losses_over_graph"] = round(res["corner_losses"]["median"] / res["graph"]["median"], 3)
    res["host_bound"] = bool(res["corner_losses"]["median"] > 2 * res["graph"]["median"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
