"""Forward + backward of a training step's two triplet-loss sites, hdn_amd.triplet (csrc/triplet_loss.hip) against x[ids] + nn.TripletMarginLoss on
PyTorch-ROCm: profiles/triplet_train.json and one JSON line.

    python tools/triplet_train_bench.py [--rounds 5] [--seconds 0.5] [--out profiles/triplet_train.json]

A step = what the reference's training forward makes `triplet_loss` do at TRAIN.BATCH_SIZE 32, once per site
(model_builder_e2e_unconstrained_v2.py:428-440, sim_loss_mat; homo_model_builder.py:185-199, feature_loss_mat): three [32,1,127,127] N(0,1) maps that
require grad are gathered with ids that select 24 of the 32 samples, the loss matrix [24,1,127] is formed, sum / n / 127^2 is taken, the two sites'
scalars are added and one backward delivers the six gradients.
  library        x[ids] x 3 + nn.TripletMarginLoss(margin=1.0, p=1, reduction='none')
  hip            the same gathers + hdn_amd.TripletMarginLossL1: what install(train=True) gives the reference while TRIPLET_TRAIN_BOUND
  hip_fused_ids  hdn_amd.triplet_l1(..., ids=ids, differentiable=True): no gathered copies; what HomoModelBuilder.training_forward uses
Before timing every side is checked against float64 on the CPU: each loss row within (D + 3) 2^-24 (margin + d_ap + d_an) + 2 D 2^-24 eps of it
(the bound of tests/triplet_cases.py) and, for the HIP sides, the gradients equal to the float64 ones on every row whose |v| exceeds that bound.
All sides are warmed up (one untimed window each), then alternate (hip, library, hip_fused_ids, hip, ...) --rounds times in one process; a window repeats whole steps until at
least --seconds have passed on the host clock and is timed by device events around it.  Reported: the median ms per step over the windows with the
smallest and the largest beside it, and the spread (largest - smallest) / median.
`ahead`: is the hip median below the library median by more than the larger of the two sides' (largest - smallest)?  This tool sets no threshold;
`ahead` decides hdn_amd.install.TRIPLET_TRAIN_BOUND, i.e. whether install(train=True) rebinds the two `triplet_loss` attributes.

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

B, S, N_SEL, SITES = 32, 127, 24, 2
MARGIN, EPS = 1.0, 1e-6


def make_inputs(dev, dtype=torch.float32):
    """Per site: (sear, pred, tmp) [32,1,127,127] leaves that require grad, and ids selecting 24 of 32 (every fourth sample left out)."""
    gen = torch.Generator().manual_seed(20261020)
    maps = [[torch.randn(B, 1, S, S, generator=gen) for _ in range(3)] for _ in range(SITES)]
    ids = torch.tensor([i for i in range(B) if i % 4 != 1], dtype=torch.long)
    assert ids.numel() == N_SEL
    return [[t.to(dev, dtype).requires_grad_(True) for t in site] for site in maps], ids.to(dev)


def make_step(kind, inputs, ids):
    if kind == "library":
        loss_fn = nn.TripletMarginLoss(margin=MARGIN, p=1, eps=EPS, reduction="none")
    elif kind == "hip":
        from hdn_amd import TripletMarginLossL1
        loss_fn = TripletMarginLossL1(margin=MARGIN, eps=EPS)
    else:
        from hdn_amd import triplet_l1

    def step():
        total, mats = None, []
        for sear, pred, tmp in inputs:
            sear.grad = pred.grad = tmp.grad = None
            if kind == "hip_fused_ids":
                mat = triplet_l1(sear, pred, tmp, margin=MARGIN, eps=EPS, ids=ids, differentiable=True)
            else:
                mat = loss_fn(sear[ids], pred[ids], tmp[ids])
            loss = torch.sum(mat) / ids.shape[0] / (S * S)
            total = loss if total is None else total + loss
            mats.append(mat)
        total.backward()
        return mats
    return step


def check_against_float64(steps, inputs, ids):
    """Worst |loss row - float64| / tol per side, and for the HIP sides the number of gradient elements that differ from float64's on compared rows."""
    in64 = [[t.detach().cpu().double().requires_grad_(True) for t in site] for site in inputs]
    mats64 = make_step("library", in64, ids.cpu())()
    U = 2.0 ** -24
    report = {}
    for name, step in steps.items():
        mats = step()
        worst, differ = 0.0, 0
        for site, site64, mat, mat64 in zip(inputs, in64, mats, mats64):
            sear, pred, tmp = (t.detach()[ids.cpu()] for t in site64)
            d_ap, d_an = ((sear - pred) + EPS).abs().sum(-1), ((sear - tmp) + EPS).abs().sum(-1)
            tol = (S + 3) * U * (MARGIN + d_ap + d_an) + 2 * S * U * EPS
            worst = max(worst, float(((mat.detach().cpu().double() - mat64.detach()).abs() / tol).max()))
            v = (MARGIN + d_ap) - d_an
            compared = torch.zeros(B, 1, S, 1, dtype=torch.bool)
            compared[ids.cpu()] = (v.abs() > tol).unsqueeze(-1)
            unselected = torch.ones(B, dtype=torch.bool)
            unselected[ids.cpu()] = False
            compared[unselected] = True
            for t, t64 in zip(site, site64):
                scale = 1.0 / N_SEL / (S * S)
                # the float64 gradient is (+-1, +-2, 0) / n / 127^2; the fp32 one carries one rounding of that factor
                differ += int((((t.grad.cpu().double() - t64.grad).abs() > 1e-6 * scale) & compared).sum())
        report[name] = {"worst_loss_error_over_tol": float("%.3g" % worst), "gradient_elements_off": differ}
    return report


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
            torch.cuda.synchronize()                   # (the host must not run minutes ahead of the device)
            if time.perf_counter() - t0 >= seconds:
                break
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, steps


def summary(ms):
    med = statistics.median(ms)
    return {"ms_per_step": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triplet_train.json"))
    args = ap.parse_args()
    if args.rounds < 5 or args.seconds < 0.5:
        ap.error("at least five alternations, each window at least half a second")
    if not torch.cuda.is_available():
        raise SystemExit("tools/triplet_train_bench.py measures on a GPU; there is none here")
    dev = torch.device("cuda:0")
    inputs, ids = make_inputs(dev)
    names = ("hip", "library", "hip_fused_ids")
    steps = {name: make_step(name, inputs, ids) for name in names}
    report = check_against_float64(steps, inputs, ids)
    for name in names:
        assert report[name]["worst_loss_error_over_tol"] <= 1.0, f"{name} leaves the bound against float64: {report}"
        assert report[name]["gradient_elements_off"] == 0, f"{name}: gradients differ from float64's: {report}"
    for name in names:                                   # warm-up: first-use costs of all sides, and one untimed window each so that the
        window(steps[name], args.seconds)                # first timed window does not carry the clocks' ramp (a step is half a millisecond)
        print(f"[triplet_train_bench] {name}: warm", file=sys.stderr, flush=True)
    ms = {name: [] for name in names}
    counts = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            t, n = window(steps[name], args.seconds)
            ms[name].append(t)
            counts[name].append(n)
            print(f"[triplet_train_bench] {name}: {t:.4f} ms per step over {n} steps", file=sys.stderr, flush=True)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "batch": B, "selected": N_SEL, "map": [S, S], "sites_per_step": SITES,
           "rounds": args.rounds, "window_seconds": args.seconds, "steps_per_window": counts, "against_float64": report}
    for name in names:
        res[name] = summary(ms[name])
    res["library_over_hip"] = round(res["library"]["ms_per_step"] / res["hip"]["ms_per_step"], 3)
    res["library_over_hip_fused_ids"] = round(res["library"]["ms_per_step"] / res["hip_fused_ids"]["ms_per_step"], 3)
    spread_ms = max(res[n]["max"] - res[n]["min"] for n in ("hip", "library"))
    res["ahead"] = bool(res["library"]["ms_per_step"] - res["hip"]["ms_per_step"] > spread_ms)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
