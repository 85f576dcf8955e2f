"""Forward + backward of a training step's 24 head BatchNorm2d(256) + ReLU sites (between a head branch's 3x3 convolution and its correlation,
ban.py:55-64, ban_lp.py:17-26), hdn_amd.batchnorm_relu_train against what the parent commit runs there: profiles/head_bn_train.json and one JSON line.

    python tools/head_bn_train_bench.py [--windows 7] [--seconds 1.0] [--out profiles/head_bn_train.json]

A step = six sites at 5x5, six at 29x29 and twelve at 13x13, at B = 32 with 256 channels.  Inputs are channels-last, as conv3x3_valid hands them over;
outputs and their gradients are contiguous NCHW, as the correlation takes and returns them.
  stock        the modules' BatchNorm2d (batch statistics) + ReLU(inplace=True) on the channels-last map, the correlation's x.detach().contiguous()
               of its forward (xcorr._prep) and the same copy again in its backward, autograd's backward from the NCHW gradient, and the
               channels-last copy _Conv3x3Valid.backward makes of what arrives (conv_train._cl; no copy where it already is channels-last)
  hip          hdn_amd.batchnorm_relu_train, eager: one forward and one backward entry point per site, no copy
  hip_graph    the same step replayed from one hipGraph
All sides are warmed up, then take turns (--windows rounds in one process); a window repeats whole steps until at least --seconds have passed on the
host clock and is timed by device events around it.  Reported per side: the median ms per step with the smallest and largest window beside it.
`ahead`: is the hip median below the stock median by more than the larger of the two min-to-max ranges?  That is the rule that sets
hdn_amd.install.HEAD_BN_TRAIN_BOUND.
Records, not assertions: per shape and direction (windows of --seconds / 4, the call alone) ms per call, the algorithmic traffic (forward 8 N C bytes,
backward 12 N C) per second, and beside it this tool's own copy rate (hdn_ubench_copy_f32, 8 bytes per element) on a buffer of the map's size; and
`forms`: forward + backward in either launch form (HDN_BN_TRAIN_FUSED_ROWS forces one) as N = 25 B grows, which is where the threshold in
bn_train.hip comes from.

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
SHAPES = (("head kernel", 5, 6), ("head search", 29, 6), ("head_lp kernel / search", 13, 12))
CL = torch.channels_last
FORM_ENV = "HDN_BN_TRAIN_FUSED_ROWS"


def make_sites(dev):
    gen = torch.Generator().manual_seed(20261021)
    sites = []
    for _, S, count in SHAPES:
        for _ in range(count):
            c = (2.0 * torch.randn(B, C, S, S, generator=gen) + 0.5).to(dev).contiguous(memory_format=CL).requires_grad_(True)
            g = (torch.randn(B, C, S, S, generator=gen) * 1e-3).to(dev)
            bn = torch.nn.BatchNorm2d(C).to(dev).train()
            with torch.no_grad():
                bn.weight.uniform_(0.5, 1.5, generator=None)
                bn.bias.normal_()
            sites.append((c, g, bn, torch.nn.ReLU(inplace=True)))
    return sites


def stock_site(c, g, bn, relu):
    from hdn_amd.conv_train import _cl
    y = relu(bn(c))
    y.detach().contiguous()                   # the correlation's forward
    y.detach().contiguous()                   # the correlation's backward
    dc, dgamma, dbeta = torch.autograd.grad(y, (c, bn.weight, bn.bias), g)
    return y, _cl(dc), dgamma, dbeta


def hip_site(c, g, bn, relu):
    import hdn_amd
    y = hdn_amd.batchnorm_relu_train(c, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, relu=True, out_nchw=True)
    bn.num_batches_tracked.add_(1)
    dc, dgamma, dbeta = torch.autograd.grad(y, (c, bn.weight, bn.bias), g)
    return y, dc, dgamma, dbeta


def make_step(sites, fn):
    def step():
        for s in sites:
            fn(*s)
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


def _problem(dev, b, S, gen):
    from hdn_amd import bn_train as BT
    c = (2.0 * torch.randn(b, C, S, S, generator=gen) + 0.5).to(dev).contiguous(memory_format=CL)
    dy = torch.randn(b, C, S, S, generator=gen).to(dev)
    gamma, beta = torch.rand(C, generator=gen).to(dev) + 0.5, torch.randn(C, generator=gen).to(dev)
    y, stats = torch.empty(b, C, S, S, device=dev), torch.empty(2 * C, device=dev)
    fwd = lambda: BT.forward(c, gamma, beta, None, None, 0.1, 1e-5, True, True, out=y, stats=stats)
    bwd = lambda: BT.backward(dy, c, gamma, beta, stats, True, True)
    return fwd, bwd


def per_call(dev, seconds):
    """ms per call of the two entry points at each shape, the call alone, with the algorithmic traffic per second and the copy rate at that size."""
    from hdn_amd import _lib
    lib = _lib.load()
    table, gen = [], torch.Generator().manual_seed(3)
    for _, S, _ in SHAPES:
        n = B * S * S * C
        fwd, bwd = _problem(dev, B, S, gen)
        src, dst = torch.randn(n, device=dev), torch.empty(n, device=dev)
        copy = lambda: _lib.launch("ubench_copy", dev, lib.hdn_ubench_copy_f32, _lib.ptr(src), _lib.ptr(dst), n)
        row = {"side": S, "N": B * S * S, "form": int(lib.hdn_bn_relu_train_form(B, S * S, C))}
        for name, fn, bytes_per in (("forward", fwd, 8), ("backward", bwd, 12), ("copy", copy, 8)):
            for _ in range(3):
                fn()
            ms, calls = window(fn, seconds, every=64)
            row[name] = {"ms": round(ms, 5), "calls": calls, "bytes_per_s": float("%.4g" % (bytes_per * n / (ms * 1e-3)))}
            print(f"[head_bn_train_bench] {S}x{S} {name}: {ms:.5f} ms", file=sys.stderr, flush=True)
        for name in ("forward", "backward"):
            row[name]["over_copy_rate"] = round(row[name]["bytes_per_s"] / row["copy"]["bytes_per_s"], 3)
        table.append(row)
    return table


def forms(dev, seconds):
    """Forward + backward at P = 25 in either launch form as the batch grows: ms per pair."""
    table, gen = [], torch.Generator().manual_seed(4)
    keep = os.environ.get(FORM_ENV)
    try:
        for b in (4, 8, 16, 32, 48, 64, 96, 128, 256):
            fwd, bwd = _problem(dev, b, 5, gen)
            pair = lambda: (fwd(), bwd())
            row = {"N": 25 * b}
            for form, rows in (("one_launch", 1 << 30), ("three_launches", 1)):
                os.environ[FORM_ENV] = str(rows)
                for _ in range(3):
                    pair()
                row[form] = round(window(pair, seconds, every=64)[0], 5)
            table.append(row)
            print(f"[head_bn_train_bench] forms N {row['N']}: one launch {row['one_launch']} ms, three {row['three_launches']} ms", file=sys.stderr, flush=True)
    finally:
        if keep is None:
            os.environ.pop(FORM_ENV, None)
        else:
            os.environ[FORM_ENV] = keep
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_bn_train.json"))
    args = ap.parse_args()
    if args.windows < 5 or args.seconds < 0.5:
        ap.error("at least five windows of at least half a second")
    if not torch.cuda.is_available():
        raise SystemExit("tools/head_bn_train_bench.py measures on a GPU; there is none here")
    import hdn_amd  # noqa: F401
    import hdn_amd.install as hi
    dev = torch.device("cuda:0")
    sites = make_sites(dev)
    # the sides compute the same thing (the bounds are tests/test_gpu_bn_train.py's; here: a gross check)
    for s in (sites[0], sites[6], sites[-1]):
        for u, v in zip((t.detach() for t in hip_site(*s)), (t.detach() for t in stock_site(*s))):
            assert float((u - v).abs().max()) <= 1e-3 * float(v.abs().max()) + 1e-6, "the two sides disagree"
    steps = {"stock": make_step(sites, stock_site), "hip": make_step(sites, hip_site)}
    for name in steps:
        for _ in range(3):
            steps[name]()
        torch.cuda.synchronize()
        print(f"[head_bn_train_bench] {name}: warm", file=sys.stderr, flush=True)
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
    order = ("stock", "hip", "hip_graph")
    ms, counts = {n: [] for n in order}, {n: [] for n in order}
    for _ in range(args.windows):
        for name in order:
            t, n = window(steps[name], args.seconds)
            ms[name].append(t)
            counts[name].append(n)
            print(f"[head_bn_train_bench] {name}: {t:.4f} ms per step over {n} steps", file=sys.stderr, flush=True)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "batch": B, "channels": C,
           "sites": [{"site": s, "side": S, "count": n} for s, S, n in SHAPES],
           "windows": args.windows, "window_seconds": args.seconds, "steps_per_window": counts}
    for name in order:
        res[name] = summary(ms[name])
    rng = max(res[n]["max"] - res[n]["min"] for n in ("stock", "hip"))
    res["stock_over_hip"] = round(res["stock"]["ms_per_step"] / res["hip"]["ms_per_step"], 3)
    res["stock_over_hip_graph"] = round(res["stock"]["ms_per_step"] / res["hip_graph"]["ms_per_step"], 3)
    res["ahead"] = bool(res["stock"]["ms_per_step"] - res["hip"]["ms_per_step"] > rng)
    res["flag_as_shipped"] = bool(hi.HEAD_BN_TRAIN_BOUND)
    res["per_call"] = per_call(dev, args.seconds / 4)
    res["forms"] = forms(dev, args.seconds / 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
