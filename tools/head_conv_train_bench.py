"""Forward + backward of a training step's 24 head convolutions (Conv2d(256, 256, 3, bias=False) in front of the correlations, ban.py:55-64,
ban_lp.py:17-26), hdn_amd.conv3x3_valid against PyTorch-ROCm autograd through nn.Conv2d: profiles/head_conv_train.json and one JSON line.

    python tools/head_conv_train_bench.py [--windows 7] [--seconds 1.0] [--out profiles/head_conv_train.json]

A step = the four shapes 7 -> 5 (head, kernel), 31 -> 29 (head, search), 15 -> 13 (head_lp, kernel) and 15 -> 13 (head_lp, search), six times each
(3 levels x cls / loc), at B = 32 with 256 channels: forward, then torch.autograd.grad of input and weight for a fixed gradient of a mean loss's size.
  hip          hdn_amd.conv3x3_valid, eager: device packer + hdn_conv3x3v_f32; hdn_grad_scale_f32, device packer + hdn_conv3x3v_dgrad_f32, hdn_conv3x3v_wgrad_f32
  hip_graph    the same step replayed from one hipGraph
  hip_nchw     hdn_amd.conv3x3_valid on CONTIGUOUS tensors (what the reference's necks hand over): the two channels-last copies of x and of the
               gradient are part of the step
  torch_cl     F.conv2d on channels_last tensors (what the parent commit runs when the model is channels_last), autograd's backward
  torch_nchw   the same on contiguous tensors
All five are warmed up, then take turns (--windows rounds in one process); a window repeats whole steps until at least --seconds have passed on the
host clock and is timed by device events around it.  Reported per side: the median ms per step with the smallest and largest window beside it.
`ahead`: is the slowest of the three HIP medians below the faster of the two PyTorch medians by more than the largest min-to-max range of the five?  That
is the rule that sets hdn_amd.install.HEAD_CONV_TRAIN_BOUND.
Per entry point and shape (windows of --seconds / 4, device events, the call alone): ms per call and, for the three matrix-core kernels, the achieved
fraction of the fp16 matrix rate on the three piece products, 3 x 2 M N K flop over the time over 16 x 157.3 TFLOP/s (MI355X: the fp16 MFMA rate is 16 x
the fp32 matrix rate).  The packer's and the scale pass's share of the eager step follow from the same table.

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

B, C = 32, 256
SHAPES = (("head kernel", 7), ("head search", 31), ("head_lp kernel", 15), ("head_lp search", 15))
PER_SHAPE = 6
FP16_MATRIX_TFLOPS = 16 * 157.3
CL = torch.channels_last


def make_problems(dev, cl):
    gen = torch.Generator().manual_seed(20261021)
    probs = []
    for _, S in SHAPES:
        for _ in range(PER_SHAPE):
            x = torch.randn(B, C, S, S, generator=gen).relu_().to(dev)
            g = (torch.randn(B, C, S - 2, S - 2, generator=gen) * 1e-6).to(dev)
            if cl:
                x, g = x.contiguous(memory_format=CL), g.contiguous(memory_format=CL)
            w = (torch.randn(C, C, 3, 3, generator=gen) * (2.0 / (9 * C)) ** 0.5).to(dev)
            probs.append((x.requires_grad_(True), w.requires_grad_(True), g))
    return probs


def make_step(probs, conv):
    def step():
        for x, w, g in probs:
            torch.autograd.grad(conv(x, w), (x, w), g)
    return step


def window(step, seconds, every=4):
    """Whole steps until `seconds` have passed on the host (looked at every `every` steps, after a synchronise: the host must not run minutes ahead of
    the device), device events around them -> (ms per step, steps)."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0, steps = time.perf_counter(), 0
    e0.record()
    while True:
        step()
        steps += 1
        if steps % every == 0:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= seconds:
                break
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, steps


def summary(ms):
    med = statistics.median(ms)
    return {"ms_per_step": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / med, 4)}


def per_kernel(dev, seconds):
    """ms per call of every entry point at each of the three distinct shapes, the call alone."""
    from hdn_amd import conv_train as CT
    table = []
    gen = torch.Generator().manual_seed(3)
    w = (torch.randn(C, C, 3, 3, generator=gen) * (2.0 / (9 * C)) ** 0.5).to(dev)
    for S in sorted({s for _, s in SHAPES}):
        x = torch.randn(B, C, S, S, generator=gen).relu_().to(dev).contiguous(memory_format=CL)
        dy = (torch.randn(B, C, S - 2, S - 2, generator=gen) * 1e-6).to(dev).contiguous(memory_format=CL)
        e = CT.grad_scale(dy)
        gx, gw = torch.empty_like(x), torch.empty_like(w)
        flop = 3 * 2 * B * (S - 2) ** 2 * 9 * C * C        # the three piece products of the valid convolution's M N K (dgrad: zero taps of the halo included below)
        calls = {"pack": (lambda: CT.pack_dev(w, 0), 0), "scale": (lambda: CT.grad_scale(dy, out=e), 0), "forward": (lambda: CT.forward(x, w), flop),
                 "dgrad": (lambda: CT.dgrad(dy, w, e, S, out=gx), 3 * 2 * B * S * S * 9 * C * C), "wgrad": (lambda: CT.wgrad(x, dy, e, out=gw), flop)}
        for name, (fn, fl) in calls.items():
            for _ in range(3):
                fn()
            ms, n = window(fn, seconds, every=64)
            if name in ("forward", "dgrad"):               # these two pack inside: the packer's time is taken off below
                ms_pack = next(r["ms"] for r in table if r["S"] == S and r["call"] == "pack")
                ms -= ms_pack
            row = {"S": S, "call": name, "ms": round(ms, 5), "calls": n}
            if fl:
                row["fp16_matrix_fraction"] = round(fl / (ms * 1e-3) / (FP16_MATRIX_TFLOPS * 1e12), 4)
            table.append(row)
            print(f"[head_conv_train_bench] S {S} {name}: {ms:.4f} ms", file=sys.stderr, flush=True)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_conv_train.json"))
    args = ap.parse_args()
    if args.windows < 5 or args.seconds < 0.5:
        ap.error("at least five windows of at least half a second")
    if not torch.cuda.is_available():
        raise SystemExit("tools/head_conv_train_bench.py measures on a GPU; there is none here")
    import hdn_amd
    dev = torch.device("cuda:0")
    cl, nchw = make_problems(dev, True), make_problems(dev, False)
    steps = {"hip": make_step(cl, hdn_amd.conv3x3_valid), "hip_nchw": make_step(nchw, hdn_amd.conv3x3_valid), "torch_cl": make_step(cl, F.conv2d), "torch_nchw": make_step(nchw, F.conv2d)}
    # the sides compute the same gradients (the bound itself is tests/test_gpu_conv3x3_train.py's; here: a gross check)
    for x, w, g in (cl[0], cl[PER_SHAPE], cl[-1]):
        a = torch.autograd.grad(hdn_amd.conv3x3_valid(x, w), (x, w), g)
        b = torch.autograd.grad(F.conv2d(x, w), (x, w), g)
        for u, v in zip(a, b):
            assert float((u - v).abs().max()) <= 1e-3 * float(v.abs().max()), "the two sides disagree"
    for name in steps:
        for _ in range(3):
            steps[name]()
        torch.cuda.synchronize()
        print(f"[head_conv_train_bench] {name}: warm", file=sys.stderr, flush=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        steps["hip"]()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        steps["hip"]()
    steps["hip_graph"] = graph.replay
    order = ("hip", "hip_graph", "hip_nchw", "torch_cl", "torch_nchw")
    ms, counts = {n: [] for n in order}, {n: [] for n in order}
    for _ in range(args.windows):
        for name in order:
            t, n = window(steps[name], args.seconds)
            ms[name].append(t)
            counts[name].append(n)
            print(f"[head_conv_train_bench] {name}: {t:.4f} ms per step over {n} steps", file=sys.stderr, flush=True)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "batch": B, "channels": C,
           "convolutions": [{"site": s, "side": [S, S - 2], "count": PER_SHAPE} for s, S in SHAPES],
           "windows": args.windows, "window_seconds": args.seconds, "steps_per_window": counts}
    for name in order:
        res[name] = summary(ms[name])
    hip = max(res[n]["ms_per_step"] for n in ("hip", "hip_graph", "hip_nchw"))
    lib = min(res["torch_cl"]["ms_per_step"], res["torch_nchw"]["ms_per_step"])
    rng = max(res[n]["max"] - res[n]["min"] for n in order)
    res["torch_over_hip"] = round(lib / hip, 3)
    res["ahead"] = bool(lib - hip > rng)
    res["per_call"] = per_kernel(dev, args.seconds / 4)
    eager = res["hip"]["ms_per_step"]
    tot = lambda call, k: sum(PER_SHAPE * r["ms"] * (2 if r["S"] == 15 else 1) * k for r in res["per_call"] if r["call"] == call)
    res["packer_share_of_eager_step"] = round(tot("pack", 2) / eager, 4)          # two packs per convolution: forward and dgrad
    res["scale_share_of_eager_step"] = round(tot("scale", 1) / eager, 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
