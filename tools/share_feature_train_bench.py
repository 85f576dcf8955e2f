"""Forward + backward of a training step's six PreShareFeature calls, hdn_amd.PreShareFeatureTrain against the stock nn.Sequential on PyTorch-ROCm:
profiles/share_feature_train.json and one JSON line.

    python tools/share_feature_train_bench.py [--rounds 5] [--seconds 0.5] [--out profiles/share_feature_train.json]

A step = what tools/train.py makes hm_net.ShareFeature do at TRAIN.BATCH_SIZE 32 in train() mode: six calls on [32, 1, 127, 127] through one module,
in two groups of three (model_builder_e2e_unconstrained_v2.py:420-427: template, search, warped search; homo_model_builder.py:154-171: patch 1,
patch 2, pred_I2).  Four inputs are data, the third of each group requires grad; each group carries the triplet-L1 loss of homo_model_builder.py:197
(anchor = the second call, positive = the third, negative = the first), and one backward of the two losses' sum delivers the gradient of all nine
parameters (accumulated over the six calls) and of the two inputs that require it.  The running buffers are updated six times per step.
  hip      hdn_amd.PreShareFeatureTrain (csrc/share_feature_train.hip: batch statistics, the backward, no atomics)
  library  the same module class with hip_train False: its train() mode is the stock nn.Sequential (MIOpen / ATen convolutions and BatchNorm)
Both hold the same parameters, are warmed up, then alternate (hip, library, hip, library, ...) --rounds times in one process; a window repeats whole
steps until at least --seconds have passed on the host clock and is timed by device events around it.  Reported: the median ms per step over the
windows with the smallest and the largest beside it, and the spread (largest - smallest) / median.
`ahead`: is the HIP median below the library median by more than the larger of the two spreads?  This tool sets no threshold; `ahead` decides
hdn_amd.install.SHARE_FEATURE_TRAIN_BOUND, i.e. whether install(train=True) binds PreShareFeatureTrain.

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

B, H, W = 32, 127, 127


def triplet_l1(anchor, positive, negative):
    return F.triplet_margin_loss(anchor, positive, negative, margin=1.0, p=1, reduction="none").sum() / B / (H * W)


def make_inputs(dev):
    gen = torch.Generator().manual_seed(20261019)
    xs = [torch.randn(B, 1, H, W, generator=gen).to(dev) for _ in range(6)]
    xs[2].requires_grad_(True)
    xs[5].requires_grad_(True)
    return xs


def make_step(module, xs):
    params = list(module.parameters())

    def step():
        for t in params + [xs[2], xs[5]]:
            t.grad = None
        f = [module(x) for x in xs]
        (triplet_l1(f[1], f[2], f[0]) + triplet_l1(f[4], f[5], f[3])).backward()
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "share_feature_train.json"))
    args = ap.parse_args()
    if args.rounds < 5 or args.seconds < 0.5:
        ap.error("at least five alternations, each window at least half a second")
    if not torch.cuda.is_available():
        raise SystemExit("tools/share_feature_train_bench.py measures on a GPU; there is none here")
    import hdn_amd
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    mods = {"hip": hdn_amd.PreShareFeatureTrain().to(dev).train(), "library": hdn_amd.PreShareFeature().to(dev).train()}
    mods["library"].load_state_dict(mods["hip"].state_dict())
    xs = make_inputs(dev)
    steps = {name: make_step(m, xs) for name, m in mods.items()}
    # a gross check of what is timed (the bound is checked by tests/test_gpu_share_feature_train.py): the same step through the stock layers in
    # float64 on the device is the yardstick; the HIP side must agree with it, the library's own deviation is recorded beside it
    f64 = hdn_amd.PreShareFeature().to(dev).double().train()
    f64.load_state_dict({k: v.double() for k, v in mods["hip"].state_dict().items()})
    xs64 = [x.detach().double().requires_grad_(x.requires_grad) for x in xs]
    make_step(f64, xs64)()
    truth = [p.grad for p in f64.parameters()] + [xs64[2].grad, xs64[5].grad]
    deviation = {}
    for name in steps:
        steps[name]()
        got = [p.grad for p in mods[name].parameters()] + [xs[2].grad, xs[5].grad]
        deviation[name] = max(float((u.double() - v).abs().max()) / float(v.abs().max()) for u, v in zip(got, truth))
    assert deviation["hip"] <= 1e-2, f"the HIP step disagrees with float64: {deviation}"
    del f64, xs64, truth
    for name in steps:                                   # warm-up: kernel selection of the library, first-use costs of both
        for _ in range(3):
            steps[name]()
        torch.cuda.synchronize()
        print(f"[share_feature_train_bench] {name}: warm", file=sys.stderr, flush=True)
    ms = {"hip": [], "library": []}
    counts = {"hip": [], "library": []}
    for _ in range(args.rounds):
        for name in ("hip", "library"):
            t, n = window(steps[name], args.seconds)
            ms[name].append(t)
            counts[name].append(n)
            print(f"[share_feature_train_bench] {name}: {t:.4f} ms per step over {n} steps", file=sys.stderr, flush=True)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "batch": B, "plane": [H, W], "calls_per_step": 6,
           "calls_with_grad_input": 2, "rounds": args.rounds, "window_seconds": args.seconds, "steps_per_window": counts,
           "max_gradient_deviation_from_float64": {k: float("%.3g" % v) for k, v in deviation.items()},
           "hip": summary(ms["hip"]), "library": summary(ms["library"])}
    res["library_over_hip"] = round(res["library"]["ms_per_step"] / res["hip"]["ms_per_step"], 3)
    spread_ms = max(res[n]["max"] - res[n]["min"] for n in ("hip", "library"))
    res["ahead"] = bool(res["library"]["ms_per_step"] - res["hip"]["ms_per_step"] > spread_ms)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
