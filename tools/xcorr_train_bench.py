"""Forward + backward of a training step's twelve depthwise correlations, the HIP op against PyTorch-ROCm autograd: profiles/xcorr_backward.json and
one JSON line.

    python tools/xcorr_train_bench.py [--rounds 5] [--seconds 0.5] [--out profiles/xcorr_backward.json]

A step = six correlations at (32, 256, 29, 29) (x) 5 x 5 and six circular ones at (32, 256, 13, 13) (x) 13 x 13 (TRAIN.BATCH_SIZE 32, 256 channels,
three levels x {cls, loc} of MultiBAN and of MultiCircBAN), each one a forward and torch.autograd.grad of both inputs for a fixed N(0, 1) grad_out.
  hip      hdn_amd.xcorr_depthwise / xcorr_depthwise_circular (the forward kernels of csrc/xcorr.hip, the backward of csrc/xcorr_bwd.hip)
  library  oracle.hdn_oracle.xcorr_depthwise / xcorr_depthwise_circular on device tensors: a grouped conv2d with B C = 8,192 groups of one channel
           (the reference's formulation, hdn/core/xcorr.py:37-61) and autograd's own data- and weight-gradient; the circular pad is two index_selects
           whose index vectors are built on the device inside the call, as the oracle builds them.
Both are warmed up, then alternate (hip, library, hip, library, ...) --rounds times in one process; a window repeats whole steps until at least
--seconds have passed on the host clock and is timed by device events around it.  Reported: the median ms per step over the windows with the smallest
and the largest beside it, the spread (largest - smallest) / median, and the algorithmic bytes of a step over the median time.
Algorithmic bytes per correlation, 4 bytes each: the forward reads x and k and writes out; the backward reads x, k and g and writes gx and gk:
    4 P ((Hx Wx + Hk Wk + Ho Wo) + (Hx Wx + Hk Wk + Ho Wo + Hx Wx + Hk Wk)),  P = B C planes
`ahead`: is the HIP median below the library median by more than the larger of the two spreads?

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

B, C = 32, 256
SHAPES = ((False, 29, 5, 25), (True, 13, 13, 13))      # circular, Hx = Wx, Hk = Wk, Ho = Wo
PER_SHAPE = 6


def step_bytes():
    total = 0
    for _, hx, hk, ho in SHAPES:
        x, k, o = hx * hx, hk * hk, ho * ho
        total += PER_SHAPE * 4 * B * C * ((x + k + o) + (x + k + o + x + k))
    return total


def make_problems(dev):
    gen = torch.Generator().manual_seed(20261019)
    probs = []
    for circ, hx, hk, ho in SHAPES:
        for _ in range(PER_SHAPE):
            x = torch.randn(B, C, hx, hx, generator=gen).relu_().to(dev).requires_grad_(True)
            k = torch.randn(B, C, hk, hk, generator=gen).relu_().to(dev).requires_grad_(True)
            g = torch.randn(B, C, ho, ho, generator=gen).to(dev)
            probs.append((circ, x, k, g))
    return probs


def make_step(probs, plain, circular):
    def step():
        for circ, x, k, g in probs:
            torch.autograd.grad((circular if circ else plain)(x, k), (x, k), g)
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
    return {"ms_per_step": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4),
            "algorithmic_GBps": round(step_bytes() / (med * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xcorr_backward.json"))
    args = ap.parse_args()
    if args.rounds < 5 or args.seconds < 0.5:
        ap.error("at least five alternations, each window at least half a second")
    if not torch.cuda.is_available():
        raise SystemExit("tools/xcorr_train_bench.py measures on a GPU; there is none here")
    import hdn_amd
    from oracle import hdn_oracle as O
    dev = torch.device("cuda:0")

    def lib_circular(x, k):
        with torch.device(dev):
            return O.xcorr_depthwise_circular(x, k)

    probs = make_problems(dev)
    steps = {"hip": make_step(probs, hdn_amd.xcorr_depthwise, hdn_amd.xcorr_depthwise_circular),
             "library": make_step(probs, O.xcorr_depthwise, lib_circular)}
    # the two compute the same gradients (the project's correlation bound is checked by tests/test_gpu_xcorr_bwd.py; here: a gross check)
    for circ, x, k, g in (probs[0], probs[-1]):
        a = torch.autograd.grad((hdn_amd.xcorr_depthwise_circular if circ else hdn_amd.xcorr_depthwise)(x, k), (x, k), g)
        b = torch.autograd.grad((lib_circular if circ else O.xcorr_depthwise)(x, k), (x, k), g)
        for u, v in zip(a, b):
            assert float((u - v).abs().max()) <= 1e-3 * float(v.abs().max()), "the two sides disagree"
    for name in steps:                                   # warm-up: kernel selection of the library, first-use costs of both
        for _ in range(3):
            steps[name]()
        torch.cuda.synchronize()
        print(f"[xcorr_train_bench] {name}: warm", file=sys.stderr, flush=True)
    torch.cuda.synchronize()
    ms = {"hip": [], "library": []}
    counts = {"hip": [], "library": []}
    for _ in range(args.rounds):
        for name in ("hip", "library"):
            t, n = window(steps[name], args.seconds)
            ms[name].append(t)
            counts[name].append(n)
            print(f"[xcorr_train_bench] {name}: {t:.4f} ms per step over {n} steps", file=sys.stderr, flush=True)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "batch": B, "channels": C,
           "correlations": [{"circular": c, "x": [hx, hx], "k": [hk, hk], "count": PER_SHAPE} for c, hx, hk, _ in SHAPES],
           "rounds": args.rounds, "window_seconds": args.seconds, "steps_per_window": counts, "algorithmic_bytes_per_step": step_bytes(),
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
