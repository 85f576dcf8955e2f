"""Forward + backward of a training step's three stn_with_theta calls, hdn_amd.affine (csrc/affine_stn.hip) against F.affine_grid + F.grid_sample on
PyTorch-ROCm: profiles/affine_stn_train.json and one JSON line.

    python tools/affine_stn_train_bench.py [--rounds 5] [--seconds 0.5] [--out profiles/affine_stn_train.json]

A step = what the reference's training forward makes ModelBuilder.stn_with_theta do at TRAIN.BATCH_SIZE 32
(model_builder_e2e_unconstrained_v2.py:407, :408, :418), grid size [32, 1, 127, 127]:
  search_hm     [32,3,255,255] with affine_m         (requires grad: built from the first head's polar and the log-polar head's scale / rot)
  search_hm     [32,3,255,255] with affine_m_c_aug   (no grad)
  search_window [32,1,255,255] with affine_m
each followed by the channel mean the reference takes (get_simi_data), and one backward per step for a fixed N(0, 1) grad of the results that
carry a graph, which delivers the gradient of affine_m (summed over its two calls).  The thetas are drawn as combine_affine_c0_v2 builds them (scale about one half,
a rotation, a normalised shift).
  hip      hdn_amd.affine.stn_with_theta (one kernel per call forward, one call backward; grad_theta without atomics)
  library  the reference's three lines: theta.view(-1, 2, 3), F.affine_grid, F.grid_sample
Before timing both sides are checked against the same three lines in float64 on the device (the bounds are checked by
tests/test_gpu_affine_stn.py).  Both are warmed up, then alternate (hip, library, hip, library, ...) --rounds times in one process; a window repeats
whole steps until at least --seconds have passed on the host clock and is timed by device events around it.  Reported: the median ms per step over the
windows with the smallest and the largest beside it, and the spread (largest - smallest) / median.
`ahead`: is the HIP median below the library median by more than the larger of the two spreads?  This tool sets no threshold; `ahead` decides
hdn_amd.install.AFFINE_STN_TRAIN_BOUND, i.e. whether install(train=True) rebinds ModelBuilder.stn_with_theta.

There is no CPU fallback: without a GPU this tool fails."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

B, S_IN, S_OUT = 32, 255, 127


def library_stn(x, theta, size):
    """ModelBuilder.stn_with_theta's three lines (PyTorch's defaults written out)."""
    theta = theta.view(-1, 2, 3)
    grid = F.affine_grid(theta, size, align_corners=False)
    return F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def similarity_theta(gen, jitter):
    """[B,2,3] as combine_affine_c0_v2 builds it: sc = out_sz / in_sz * scale, a rotation, a shift normalised by out_sz."""
    sc = S_OUT / S_IN * (1.0 + jitter * (torch.rand(B, generator=gen) - 0.5))
    rot = jitter * (torch.rand(B, generator=gen) - 0.5) * math.pi / 4
    t = jitter * 0.2 * (torch.rand(B, 2, generator=gen) - 0.5)
    a, c = sc * torch.cos(rot), sc * torch.sin(rot)
    return torch.stack([a, -c, t[:, 0], c, a, t[:, 1]], dim=1).reshape(B, 2, 3)


def make_inputs(dev, dtype=torch.float32):
    gen = torch.Generator().manual_seed(20261020)
    hm = torch.randn(B, 3, S_IN, S_IN, generator=gen)
    window = torch.randn(B, 1, S_IN, S_IN, generator=gen)
    affine_m, affine_aug = similarity_theta(gen, 0.5), similarity_theta(gen, 0.1)
    gs = [torch.randn(B, 1, S_OUT, S_OUT, generator=gen) for _ in range(3)]                  # (the second is not used: that call has no backward)
    to = lambda t: t.to(dev, dtype)
    return to(hm), to(window), to(affine_m).requires_grad_(True), to(affine_aug), [to(g) for g in gs]


def make_step(stn, inputs):
    hm, window, affine_m, affine_aug, gs = inputs
    size = torch.Size([B, 1, S_OUT, S_OUT])

    def step():
        affine_m.grad = None
        outs = (stn(hm, affine_m, size).mean(1, keepdim=True), stn(hm, affine_aug, size).mean(1, keepdim=True), stn(window, affine_m, size))
        torch.autograd.backward([outs[0], outs[2]], [gs[0], gs[2]])     # the second call's theta carries no graph: forward only
        return outs
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affine_stn_train.json"))
    args = ap.parse_args()
    if args.rounds < 5 or args.seconds < 0.5:
        ap.error("at least five alternations, each window at least half a second")
    if not torch.cuda.is_available():
        raise SystemExit("tools/affine_stn_train_bench.py measures on a GPU; there is none here")
    from hdn_amd import affine
    dev = torch.device("cuda:0")
    inputs = make_inputs(dev)
    steps = {"hip": make_step(lambda x, t, s: affine.stn_with_theta(None, x, t, s), inputs), "library": make_step(library_stn, inputs)}
    # both sides against the same three lines in float64 on the device: the outputs and the gradient of affine_m, relative to the largest value
    in64 = make_inputs(dev, torch.float64)
    outs64 = make_step(library_stn, in64)()
    truth = [o.detach() for o in outs64] + [in64[2].grad]
    deviation = {}
    for name in steps:
        got = [o.detach() for o in steps[name]()] + [inputs[2].grad]
        deviation[name] = max(float((u.double() - v).abs().max()) / float(v.abs().max()) for u, v in zip(got, truth))
    assert deviation["hip"] <= 1e-3, f"the HIP step disagrees with float64: {deviation}"
    del in64, outs64, truth
    for name in steps:                                   # warm-up: first-use costs of both
        for _ in range(3):
            steps[name]()
        torch.cuda.synchronize()
        print(f"[affine_stn_train_bench] {name}: warm", file=sys.stderr, flush=True)
    ms = {"hip": [], "library": []}
    counts = {"hip": [], "library": []}
    for _ in range(args.rounds):
        for name in ("hip", "library"):
            t, n = window(steps[name], args.seconds)
            ms[name].append(t)
            counts[name].append(n)
            print(f"[affine_stn_train_bench] {name}: {t:.4f} ms per step over {n} steps", file=sys.stderr, flush=True)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "batch": B, "image": [S_IN, S_IN], "output": [S_OUT, S_OUT],
           "calls_per_step": 3, "calls_with_grad_theta": 2, "rounds": args.rounds, "window_seconds": args.seconds, "steps_per_window": counts,
           "max_deviation_from_float64": {k: float("%.3g" % v) for k, v in deviation.items()},
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
