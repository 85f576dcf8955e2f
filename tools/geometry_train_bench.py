"""Forward + backward of the three geometry drop-ins of a training step, the HIP ops against PyTorch-ROCm autograd through the oracle formulation:
profiles/geometry_backward.json and one JSON line.

    python tools/geometry_train_bench.py [--rounds 5] [--seconds 0.5] [--out profiles/geometry_backward.json]

At B = 32 (TRAIN.BATCH_SIZE), each operator a forward and torch.autograd.grad of the input that requires grad in the reference's training step, for a
fixed N(0, 1) grad_out:
  sampler  x [32,3,255,255], polar [32,2] (grad)      hdn_amd.STN_PolarTrain(255)      | oracle.hdn_oracle.logpolar_sample (grid built per call + F.grid_sample)
  dlt      h4p [32,8], offsets [32,8] (grad)          hdn_amd.DLT_solve                | oracle.hdn_oracle.dlt_solve (inverse(A) @ b)
  warp     U [32,1,127,127], theta [32,3,3] (grad)    hdn_amd.transformer              | oracle.hdn_oracle.transformer (gathers + weights in torch ops)
The library side runs the oracle's statements on device tensors (its tensor constructors inside `with torch.device(dev)`).  Both sides are warmed up,
then alternate (hip, library, ...) --rounds times in one process; a window repeats whole steps until at least --seconds have passed on the host clock
and is timed by device events around it.  Reported per operator: the median ms per step over the windows with the smallest and the largest beside it and
the spread (largest - smallest) / median.  `ahead`: is the HIP median below the library median by more than the larger of the two spreads?
No threshold applies: nothing is promised about these kernels' speed.

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

B = 32


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


def make_operators(dev):
    """name -> (hip forward, library forward, the input that requires grad, grad_out); a forward maps that input to the differentiated output."""
    import hdn_amd
    from oracle import hdn_oracle as O
    gen = torch.Generator().manual_seed(20261019)
    ops = {}

    x = torch.randn(B, 3, 255, 255, generator=gen).to(dev)
    polar = (8.0 * torch.randn(B, 2, generator=gen)).to(dev).requires_grad_(True)
    stn = hdn_amd.STN_PolarTrain(255)

    def lib_sampler(p):
        with torch.device(dev):
            return O.logpolar_sample(x, p, image_sz=255)[0]

    ops["sampler"] = (lambda p: stn(x, p)[0], lib_sampler, polar, torch.randn(B, 3, 127, 127, generator=gen).to(dev))

    h4p = torch.tensor([[0.0, 0.0, 0.0, 127.0, 127.0, 127.0, 127.0, 0.0]]).repeat(B, 1).to(dev)
    off = (8.0 * torch.randn(B, 8, generator=gen)).to(dev).requires_grad_(True)

    def lib_dlt(o):
        with torch.device(dev):
            return O.dlt_solve(h4p, o)

    ops["dlt"] = (lambda o: hdn_amd.DLT_solve(h4p, o), lib_dlt, off, torch.randn(B, 1, 3, 3, generator=gen).to(dev))

    U = torch.randn(B, 1, 127, 127, generator=gen).to(dev)
    theta = (torch.eye(3).repeat(B, 1, 1) + 0.02 * torch.randn(B, 3, 3, generator=gen)).to(dev).requires_grad_(True)

    def lib_warp(t):
        with torch.device(dev):
            return O.transformer(U, t, (127, 127))[0]

    ops["warp"] = (lambda t: hdn_amd.transformer(U, t, (127, 127), want_condition=False)[0], lib_warp, theta,
                   torch.randn(B, 127, 127, 1, generator=gen).to(dev))
    return ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_backward.json"))
    args = ap.parse_args()
    if args.rounds < 5 or args.seconds < 0.5:
        ap.error("at least five alternations, each window at least half a second")
    if not torch.cuda.is_available():
        raise SystemExit("tools/geometry_train_bench.py measures on a GPU; there is none here")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "batch": B, "rounds": args.rounds,
           "window_seconds": args.seconds, "operators": {}}
    for name, (hip, lib, inp, g) in make_operators(dev).items():
        steps = {"hip": lambda f=hip: torch.autograd.grad(f(inp), inp, g), "library": lambda f=lib: torch.autograd.grad(f(inp), inp, g)}
        # a gross check that the two sides compute the same gradient (the bounds are checked by tests/test_gpu_geometry_bwd.py)
        (a,), (b,) = steps["hip"](), steps["library"]()
        assert float((a - b).abs().max()) <= 2e-2 * float(b.abs().max()), f"{name}: the two sides disagree"
        for side in steps:
            for _ in range(3):
                steps[side]()
            torch.cuda.synchronize()
        ms, counts = {"hip": [], "library": []}, {"hip": [], "library": []}
        for _ in range(args.rounds):
            for side in ("hip", "library"):
                t, n = window(steps[side], args.seconds)
                ms[side].append(t)
                counts[side].append(n)
                print(f"[geometry_train_bench] {name} {side}: {t:.4f} ms per step over {n} steps", file=sys.stderr, flush=True)
        r = {"hip": summary(ms["hip"]), "library": summary(ms["library"]), "steps_per_window": counts}
        r["library_over_hip"] = round(r["library"]["ms_per_step"] / r["hip"]["ms_per_step"], 3)
        spread_ms = max(r[s]["max"] - r[s]["min"] for s in ("hip", "library"))
        r["ahead"] = bool(r["library"]["ms_per_step"] - r["hip"]["ms_per_step"] > spread_ms)
        res["operators"][name] = r
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
