"""Similarity backbone + both necks, forward time four ways, on one GPU: one JSON line.

    python tools/backbone_bench.py --batch N [--iters 30] [--warmup 5]

The production stand-in's ResNet-50 (stride 8, atrous) and its two necks (tests/production_standin.py) on 127- and 255-px crops:
(a) "as_built": the modules' own forward (BatchNorm / ReLU / add launches, MIOpen); (b) "folded": optimize_similarity_model(model), today's default
(MIOpen convolutions + hdn_bias_relu_f32); (c) "hip": optimize_similarity_model(model, hip=True) (hdn_conv1x1_f32 / hdn_conv3x3d_f32); (d) "hip_full":
optimize_similarity_model(model, hip=2) (level 2: also hdn_conv3x3v_f32 and hdn_simi_stem_f32, no library convolution left).
ms per forward: warmed, HIP-event timed per forward, median of --iters with the 10th / 90th percentile beside it.  All four in one process, on the same
seeded weights and inputs.  It also lists every distinct hdn_conv3x3d_f32 launch of one forward per crop: shape, launch form, count per forward,
algorithmic bytes (x + out + packed weights), its own event-timed median, and its floor = max(bytes / the measured copy rate, MFMA work at the dense
fp16 peak x 3 piece products); K-slice workspace traffic is the kernel's own cost, not in the floor.  The same table for level 2's launches: "conv3x3v"
(hdn_conv3x3v_f32) and "simi_stem" (hdn_simi_stem_f32, K = 147 in the floor's MFMA work), the latter beside "level1_stem_us": the event-timed sum of
the four launches it replaces (library convolution, hdn_bias_relu_f32, max pool, NCHW -> channels-last copy), measured the same way.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

MFMA_F16_PEAK = 2.5e15        # dense fp16 FLOP/s (spec)


def timed(fn, iters, warmup):
    """(median, 10th percentile, 90th percentile) ms of fn, one HIP event pair per call."""
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
    ts.sort()
    return statistics.median(ts), ts[len(ts) // 10], ts[(9 * len(ts)) // 10]


def copy_rate(dev):
    """Bytes per second of hdn_ubench_copy_f32 (read + write) over 2 x 256 MB."""
    from hdn_amd import _lib
    n = 64 << 20
    src, dst = torch.ones(n, device=dev), torch.empty(n, device=dev)
    lib = _lib.load()
    ms = timed(lambda: _lib.check(lib.hdn_ubench_copy_f32(_lib.ptr(src), _lib.ptr(dst), n, _lib.stream_ptr(dev)), "ubench_copy"), 20, 5)[0]
    return 2 * n * 4 / (ms * 1e-3)


def conv3x3d_launches(net, crop):
    """{(CI, CO, S, d): count} of the hdn_conv3x3d_f32 launches of one forward at this crop size."""
    from hdn_amd import backbone as BB
    S = ((crop - 7) // 2 + 1 - 1) // 2 + 1                      # 7x7 / 2 without padding, then maxpool 3 / 2 / 1
    out = {}
    for name in ("layer1", "layer2", "layer3", "layer4"):
        for blk in getattr(net, name):
            convs = [blk.conv2] + ([blk.downsample[0]] if blk.downsample is not None else [])
            for c in convs:
                if BB.hip_conv_kind(c) == "conv3x3d":
                    key = (c.in_channels, c.out_channels, S, c.dilation[0])
                    out[key] = out.get(key, 0) + 1
            c2 = blk.conv2
            S = (S + 2 * c2.padding[0] - c2.dilation[0] * 2 - 1) // c2.stride[0] + 1
    return out


def conv3x3v_launches(net, crop):
    """{(CI, CO, S, stride): count} of the hdn_conv3x3v_f32 launches of one level-2 forward at this crop size (S: the INPUT side)."""
    from hdn_amd import backbone as BB
    S = ((crop - 7) // 2 + 1 - 1) // 2 + 1
    out = {}
    for name in ("layer1", "layer2", "layer3", "layer4"):
        for blk in getattr(net, name):
            convs = [blk.conv2] + ([blk.downsample[0]] if blk.downsample is not None else [])
            for c in convs:
                if BB.hip_conv_kind(c, level=2) == "conv3x3v":
                    key = (c.in_channels, c.out_channels, S, c.stride[0])
                    out[key] = out.get(key, 0) + 1
            c2 = blk.conv2
            S = (S + 2 * c2.padding[0] - c2.dilation[0] * 2 - 1) // c2.stride[0] + 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import production_standin as PS
    from hdn_amd import _lib, backbone as BB, trunk as T

    dev = torch.device("cuda:0")
    torch.manual_seed(2)
    model = types.SimpleNamespace(backbone=PS.AtrousResNet50(), neck=PS.Necks(True), neck_lp=PS.Necks(False))
    for i, part in enumerate((model.backbone, model.neck, model.neck_lp)):
        PS._seed(part, 40 + i)
        part.to(dev).eval()
    B = args.batch
    xs = {s: torch.randn(B, 3, s, s, device=dev) * 60 + 110 for s in (127, 255)}

    def forward(x):
        f = model.backbone(x)
        return list(f) + list(model.neck(f)) + list(model.neck_lp(f))

    res = {"batch": B, "iters": args.iters, "device": torch.cuda.get_device_name(dev), "ms": {}, "rel_err_vs_as_built": {}}
    lib = _lib.load()
    with torch.no_grad():
        ref = {s: forward(x) for s, x in xs.items()}
        for form, setup in (("as_built", lambda: BB.restore_similarity_model(model)), ("folded", lambda: BB.optimize_similarity_model(model, hip=False)),
                            ("hip", lambda: BB.optimize_similarity_model(model, hip=True)),
                            ("hip_full", lambda: BB.optimize_similarity_model(model, hip=2))):
            setup()
            for s, x in xs.items():
                got = forward(x)
                res["rel_err_vs_as_built"][f"{form}_{s}"] = max(float((g - w).abs().max() / w.abs().max()) for g, w in zip(got, ref[s]))
                med, lo, hi = timed(lambda: forward(x), args.iters, args.warmup)
                res["ms"][f"{form}_{s}"] = {"median": round(med, 4), "p10": round(lo, 4), "p90": round(hi, 4)}
        BB.restore_similarity_model(model)
        for s in xs:
            res["ms"][f"speedup_hip_vs_folded_{s}"] = round(res["ms"][f"folded_{s}"]["median"] / res["ms"][f"hip_{s}"]["median"], 3)
            res["ms"][f"speedup_hip_full_vs_hip_{s}"] = round(res["ms"][f"hip_{s}"]["median"] / res["ms"][f"hip_full_{s}"]["median"], 3)
        rate = copy_rate(dev)
        res["copy_GBps"] = round(rate / 1e9, 1)
        rows, cl = [], torch.channels_last
        for crop in xs:
            for (CI, CO, S, d), count in conv3x3d_launches(model.backbone, crop).items():
                xi = torch.rand(B, CI, S, S, device=dev).contiguous(memory_format=cl)
                wp = T.pack_conv3x3d(torch.randn(CO, CI, 3, 3) * 0.02).to(dev)
                bias = torch.zeros(CO, device=dev)
                nbytes = 4 * (B * S * S * (CI + CO) + 9 * CI * CO)
                med, lo, hi = timed(lambda: T.conv3x3d(xi, wp, bias, dilation=d), args.iters, args.warmup)
                floor = max(nbytes / rate, 3 * 2.0 * B * S * S * 9 * CI * CO / MFMA_F16_PEAK) * 1e6
                fm = lib.hdn_conv3x3d_form(B, S, CI, CO, d)
                rows.append({"crop": crop, "CI": CI, "CO": CO, "S": S, "d": d, "count": count,
                             "form": f"Cfg<{fm & 15},{(fm >> 4) & 15},{(fm >> 8) & 15},{(fm >> 12) & 15}> x {fm >> 16}", "bytes": nbytes,
                             "us": round(1e3 * med, 2), "us_p10": round(1e3 * lo, 2), "us_p90": round(1e3 * hi, 2), "floor_us": round(floor, 2),
                             "x_floor": round(1e3 * med / floor, 2)})
                del xi, wp
        res["conv3x3d"] = rows
        rows = []
        for crop in xs:
            for (CI, CO, S, st), count in conv3x3v_launches(model.backbone, crop).items():
                So = (S - 3) // st + 1
                xi = torch.rand(B, CI, S, S, device=dev).contiguous(memory_format=cl)
                wp = T.pack_conv3x3d(torch.randn(CO, CI, 3, 3) * 0.02).to(dev)
                bias = torch.zeros(CO, device=dev)
                nbytes = 4 * (B * (S * S * CI + So * So * CO) + 9 * CI * CO)
                med, lo, hi = timed(lambda: T.conv3x3v(xi, wp, bias, stride=st), args.iters, args.warmup)
                floor = max(nbytes / rate, 3 * 2.0 * B * So * So * 9 * CI * CO / MFMA_F16_PEAK) * 1e6
                fm = lib.hdn_conv3x3v_form(B, S, CI, CO, st)
                rows.append({"crop": crop, "CI": CI, "CO": CO, "S": S, "So": So, "stride": st, "count": count,
                             "form": f"Cfg<{fm & 15},{(fm >> 4) & 15},{(fm >> 8) & 15},{(fm >> 12) & 15}> x {fm >> 16}", "bytes": nbytes,
                             "us": round(1e3 * med, 2), "us_p10": round(1e3 * lo, 2), "us_p90": round(1e3 * hi, 2), "floor_us": round(floor, 2),
                             "x_floor": round(1e3 * med / floor, 2)})
                del xi, wp
        res["conv3x3v"] = rows
        rows = []
        BB.optimize_similarity_model(model, hip=True)
        stem1 = vars(model.backbone)["_hdn_fused"]                      # level 1: its stem is the four launches the fused one replaces
        w7, b7 = stem1.c1.weight, stem1.c1.bias
        wp = T.pack_simi_stem(w7).to(dev)
        for crop, x in xs.items():
            Sc = (crop - 7) // 2 + 1
            Sp = (Sc - 1) // 2 + 1
            nbytes = 4 * (B * (3 * crop * crop + Sp * Sp * 64) + 64 * 147)
            med, lo, hi = timed(lambda: T.simi_stem(x, wp, b7), args.iters, args.warmup)
            m1, lo1, hi1 = timed(lambda: stem1.maxpool(stem1.c1.act(x)).contiguous(memory_format=cl), args.iters, args.warmup)
            floor = max(nbytes / rate, 3 * 2.0 * B * Sc * Sc * 147 * 64 / MFMA_F16_PEAK) * 1e6
            rows.append({"crop": crop, "Sc": Sc, "Sp": Sp, "grid": 2 * B * Sp, "bytes": nbytes, "us": round(1e3 * med, 2), "us_p10": round(1e3 * lo, 2),
                         "us_p90": round(1e3 * hi, 2), "floor_us": round(floor, 2), "x_floor": round(1e3 * med / floor, 2),
                         "level1_stem_us": round(1e3 * m1, 2), "level1_stem_us_p10": round(1e3 * lo1, 2), "level1_stem_us_p90": round(1e3 * hi1, 2)})
        BB.restore_similarity_model(model)
        res["simi_stem"] = rows
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
