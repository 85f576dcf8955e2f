"""Homography trunk forward time, three ways, on one GPU: one JSON line.

    python tools/trunk_bench.py --backbone resnet34|resnet50 --batch N [--iters 50] [--warmup 10]

(a) "miopen": the trunk as built (BatchNorm unfolded, NCHW, MIOpen); (b) "folded_cl": fold_for_inference(channels_last=True,
fused_epilogue=False), still MIOpen; (c) "hip": fold_for_inference(channels_last=True, fused_stem=True, fused_epilogue=True), the HIP trunk.
ms per trunk forward: warmed, HIP-event timed per forward, median of --iters.  All three in one process, on the same seeded weights and input.
For resnet50 it also lists every hdn_conv1x1_f32 launch of one forward: shape, algorithmic bytes (x + out + residual + packed weights), its own
event-timed median, and its floor = max(bytes / the measured copy rate, MFMA work at the dense fp16 peak x 3 piece products); and the same table
("conv3x3s2") for the three hdn_conv3x3s2_f32 launches (bytes = x + out + packed weights; K-slice workspace traffic is the kernel's own cost, not in the floor).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

MFMA_F16_PEAK = 2.5e15        # dense fp16 FLOP/s (spec)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def copy_rate(dev):
    """Bytes per second of hdn_ubench_copy_f32 (read + write) over 2 x 256 MB."""
    from hdn_amd import _lib
    n = 64 << 20
    src, dst = torch.ones(n, device=dev), torch.empty(n, device=dev)
    lib = _lib.load()
    ms = timed(lambda: _lib.check(lib.hdn_ubench_copy_f32(_lib.ptr(src), _lib.ptr(dst), n, _lib.stream_ptr(dev)), "ubench_copy"), 20, 5)
    return 2 * n * 4 / (ms * 1e-3)


def conv1x1_launches(net, B):
    """(CI, CO, S_in, stride, residual) of every 1x1 convolution of a Bottleneck trunk's forward, in launch order."""
    out, S = [], 32
    for name in ("layer1", "layer2", "layer3", "layer4"):
        for blk in getattr(net, name):
            s = blk.conv2.stride[0]
            CI, P, CO = blk.conv1.in_channels, blk.conv1.out_channels, blk.conv3.out_channels
            out.append((CI, P, S, 1, False))
            if blk.downsample is not None:
                out.append((CI, CO, S, blk.downsample[0].stride[0], False))
            S = (S - 1) // s + 1
            out.append((P, CO, S, 1, True))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", choices=("resnet34", "resnet50"), default="resnet50")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import make_golden as mg
    from hdn_amd import trunk as T

    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = True
    net = mg.seeded_trunk_state_((T.resnet34_homo() if args.backbone == "resnet34" else T.resnet50_homo()).eval()).to(dev)
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((args.batch, 2, 127, 127)).astype(np.float32)).to(dev)
    xcl = x.contiguous(memory_format=torch.channels_last)
    folded = T.fold_for_inference(net, channels_last=True, fused_stem=False, fused_epilogue=False)
    hip = T.fold_for_inference(net, channels_last=True, fused_stem=True, fused_epilogue=True)
    res = {"backbone": args.backbone, "batch": args.batch, "iters": args.iters, "device": torch.cuda.get_device_name(dev)}
    with torch.no_grad():
        ref = net(x)
        err = float((hip(x) - ref).abs().max() / ref.abs().max())
        res["ms"] = {"miopen": timed(lambda: net(x), args.iters, args.warmup),
                     "folded_cl": timed(lambda: folded(xcl), args.iters, args.warmup),
                     "hip": timed(lambda: hip(x), args.iters, args.warmup)}
        res["hip_vs_miopen_rel_err"] = err
        res["speedup_hip_vs_folded_cl"] = res["ms"]["folded_cl"] / res["ms"]["hip"]
        if args.backbone == "resnet50":
            rate = copy_rate(dev)
            res["copy_GBps"] = rate / 1e9
            rows, cl = [], torch.channels_last
            for CI, CO, S, s, has_res in conv1x1_launches(net, args.batch):
                So = (S - 1) // s + 1
                B = args.batch
                xi = torch.rand(B, CI, S, S, device=dev).contiguous(memory_format=cl)
                r = torch.rand(B, CO, So, So, device=dev).contiguous(memory_format=cl) if has_res else None
                wp = T.pack_conv1x1(torch.randn(CO, CI, 1, 1) * 0.05).to(dev)
                bias = torch.zeros(CO, device=dev)
                nbytes = 4 * (B * S * S * CI + B * So * So * CO * (2 if has_res else 1) + CO * CI)
                us = 1e3 * timed(lambda: T.conv1x1(xi, wp, bias, r, stride=s), args.iters, args.warmup)
                floor = max(nbytes / rate, 3 * 2.0 * B * So * So * CI * CO / MFMA_F16_PEAK) * 1e6
                rows.append({"CI": CI, "CO": CO, "S": S, "stride": s, "residual": has_res, "bytes": nbytes, "us": round(us, 2),
                             "floor_us": round(floor, 2), "x_floor": round(us / floor, 2)})
            res["conv1x1"] = rows
            rows = []
            for S, C in ((16, 128), (8, 256), (4, 512)):        # conv2 of the first block of layer2 / 3 / 4
                B = args.batch
                xi = torch.rand(B, C, 2 * S, 2 * S, device=dev).contiguous(memory_format=cl)
                wp = T.pack_conv3x3s2(torch.randn(C, C, 3, 3) * 0.02).to(dev)
                bias = torch.zeros(C, device=dev)
                nbytes = 4 * (B * 4 * S * S * C + B * S * S * C + 9 * C * C)
                us = 1e3 * timed(lambda: T.conv3x3s2(xi, wp, bias), args.iters, args.warmup)
                floor = max(nbytes / rate, 3 * 2.0 * B * S * S * 9 * C * C / MFMA_F16_PEAK) * 1e6
                rows.append({"S": S, "C": C, "bytes": nbytes, "us": round(us, 2), "floor_us": round(floor, 2), "x_floor": round(us / floor, 2)})
            res["conv3x3s2"] = rows
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
