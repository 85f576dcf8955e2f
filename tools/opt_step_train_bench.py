"""The optimizer stretch of a training iteration (tools/train.py:271-281 of the reference) on the production-shaped parameter list,
hdn_amd.GatedAMSGrad (csrc/opt_step.hip) against the stock formulations on PyTorch-ROCm: profiles/opt_step_train.json and one JSON line.

    python tools/opt_step_train_bench.py [--rounds 7] [--seconds 1.0] [--out profiles/opt_step_train.json]

The parameters are those of tests/production_standin.ProductionStandIn around hdn_amd.HomoModelBuilder, grouped as build_opt_lr (train.py:100-170,
TRAIN.OBJ 'ALL', past BACKBONE.TRAIN_EPOCH) groups them: backbone layers 2-4 at 0.1 BASE_LR, neck_lp, neck, head_lp, head at BASE_LR (2e-4), hm_net
at 2e-5.  Every parameter has a fixed random gradient (no forward or backward is run: the step alone is timed); the loss is a device scalar.  In
the same process, each side on its own copy of the parameters:
  gated_amsgrad     GatedAMSGrad(weight_decay=1e-4, max_norm=10).step(loss), eager: norm, gate and update launches, no host read
  graph             the same step captured once and replayed: the device's own time
  reference         the reference's lines: is_valid_number(loss.item()) - a host read -, clip_grad_norm_(10), Adam(amsgrad=True, weight_decay=1e-4)
                    .step(), everything at its default (foreach on this build)
  stock_capturable  the best stock form that can be captured: clip_grad_norm_(foreach=True) + Adam(amsgrad=True, fused=True, capturable=True),
                    eager and replayed from a graph.  It has NO loss gate (the gate is a host decision in stock PyTorch).  If it does not run on
                    this build the error is recorded instead.
Before timing, one step of gated_amsgrad and of reference from equal parameters is compared (5e-7 absolute: a rounding of parameters of O(1));
the bounds against float64 are the business of tests/test_gpu_opt_step.py.  All sides are warmed up (one untimed window each), then alternate
--rounds times; a window repeats whole steps until at least --seconds have passed on the host clock and is timed by device events around it.
Reported per side: median, min and max ms per step over the windows.  `bandwidth`: the algorithmic traffic of the replayed step (4 bytes per
element for the norm pass, 36 for the update) per second, against this tool's own measured copy rate (hdn_ubench_copy_f32 over a buffer of the
parameters' size, 8 bytes per element).  Nothing is switched by the result, and this tool promises no speed-up.

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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

BASE_LR, HOMO_LR, WEIGHT_DECAY, GRAD_CLIP = 2e-4, 2e-5, 1e-4, 10.0


def make_groups(dev, seed):
    """[{params, lr}] of a fresh production-shaped model on `dev`, every parameter with a fixed gradient"""
    import hdn_amd
    from production_standin import ProductionStandIn
    torch.manual_seed(20261021)
    m = ProductionStandIn(hdn_amd.HomoModelBuilder()).to(dev)
    backbone = [p for layer in ("layer2", "layer3", "layer4") for p in getattr(m.backbone, layer).parameters()]
    groups = [{"params": backbone, "lr": 0.1 * BASE_LR}]
    groups += [{"params": list(part.parameters()), "lr": BASE_LR} for part in (m.neck_lp, m.neck, m.head_lp, m.head)]
    groups += [{"params": list(m.hm_net.parameters()), "lr": HOMO_LR}]
    gen = torch.Generator(device=dev).manual_seed(seed)
    for g in groups:
        for p in g["params"]:
            p.grad = 1e-2 * torch.randn(p.shape, generator=gen, device=dev)
    return groups


def flat(groups):
    return [p for g in groups for p in g["params"]]


def is_valid_number(x):
    return not (math.isnan(x) or math.isinf(x) or x > 1e4)


def captured(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph.replay


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "opt_step_train.json"))
    args = ap.parse_args()
    if args.rounds < 5 or args.seconds < 0.5:
        ap.error("at least five alternations, each window at least half a second")
    if not torch.cuda.is_available():
        raise SystemExit("tools/opt_step_train_bench.py measures on a GPU; there is none here")
    import hdn_amd
    from hdn_amd import _lib
    dev = torch.device("cuda:0")
    loss = torch.tensor(3.5, device=dev)
    steps, notes = {}, {}

    g_ours = make_groups(dev, 1)
    ours = hdn_amd.GatedAMSGrad(g_ours, lr=BASE_LR, weight_decay=WEIGHT_DECAY, max_norm=GRAD_CLIP)
    g_ref = make_groups(dev, 1)
    p_ref = flat(g_ref)
    ref = torch.optim.Adam(g_ref, lr=BASE_LR, amsgrad=True, weight_decay=WEIGHT_DECAY)

    def reference_step():                                       # (clip_grad_norm_ scales in place: from the second step on its coefficient is 1,
        if is_valid_number(loss.item()):
            torch.nn.utils.clip_grad_norm_(p_ref, GRAD_CLIP)    #  and it multiplies by it all the same)
            ref.step()

    ours.step(loss)
    reference_step()
    torch.cuda.synchronize()
    d = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(flat(g_ours), p_ref))
    assert int(ours.report.status) == 0 and d <= 5e-7, f"GatedAMSGrad disagrees with the reference's lines after one step: {d}"
    n_tensors, n_elements = len(p_ref), sum(p.numel() for p in p_ref)
    steps["gated_amsgrad"] = lambda: ours.step(loss)
    steps["reference"] = reference_step

    g_graph = make_groups(dev, 1)
    graphed = hdn_amd.GatedAMSGrad(g_graph, lr=BASE_LR, weight_decay=WEIGHT_DECAY, max_norm=GRAD_CLIP)
    steps["graph"] = captured(lambda: graphed.step(loss))

    try:                                                        # the best stock capturable form; no gate
        g_cap = make_groups(dev, 1)
        p_cap = flat(g_cap)
        cap = torch.optim.Adam(g_cap, lr=BASE_LR, amsgrad=True, weight_decay=WEIGHT_DECAY, fused=True, capturable=True)

        def capturable_step():
            torch.nn.utils.clip_grad_norm_(p_cap, GRAD_CLIP, foreach=True)
            cap.step()
        capturable_step()
        torch.cuda.synchronize()
        steps["stock_capturable"] = capturable_step
        steps["stock_capturable_graph"] = captured(capturable_step)
    except Exception as e:  # noqa: BLE001  (recorded, not hidden: the JSON says what did not run)
        notes["stock_capturable_error"] = f"{type(e).__name__}: {e}"[:400]
        steps.pop("stock_capturable_graph", None)
        torch.cuda.synchronize()

    # this tool's own copy rate, over a buffer of the parameters' size
    n_copy = n_elements // 4 * 4                                # (the copy kernel moves whole 16-byte pieces)
    src, dst = torch.randn(n_copy, device=dev), torch.empty(n_copy, device=dev)
    lib = _lib.load()
    steps["copy"] = lambda: _lib.launch("ubench_copy", dev, lib.hdn_ubench_copy_f32, _lib.ptr(src), _lib.ptr(dst), n_copy)

    names = tuple(steps)
    for name in names:
        window(steps[name], args.seconds)
        print(f"[opt_step_train_bench] {name}: warm", file=sys.stderr, flush=True)
    ms, counts = {name: [] for name in names}, {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            v, n = window(steps[name], args.seconds)
            ms[name].append(v)
            counts[name].append(n)
            print(f"[opt_step_train_bench] {name}: {v:.4f} ms per step over {n} steps", file=sys.stderr, flush=True)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "tensors": n_tensors, "elements": n_elements,
           "groups": [len(g["params"]) for g in g_ref], "tensors_per_launch": hdn_amd.optim.TENSORS_PER_LAUNCH, "chunk": hdn_amd.optim.CHUNK,
           "rounds": args.rounds, "window_seconds": args.seconds, "steps_per_window": counts,
           "worst_parameter_difference_after_one_step": float("%.3g" % d), "grad_norm": float(ours.report.grad_norm),
           "stock_capturable_has_no_gate": True, **notes}
    for name in names:
        res[name] = summary(ms[name])
    copy_rate = 8.0 * n_copy / (res["copy"]["median"] * 1e-3)
    achieved = 40.0 * n_elements / (res["graph"]["median"] * 1e-3)
    res["bandwidth"] = {"copy_bytes_per_s": float("%.4g" % copy_rate), "graph_algorithmic_bytes_per_s": float("%.4g" % achieved),
                        "bytes_per_element": 40, "graph_over_copy_rate": round(achieved / copy_rate, 3)}
    res["reference_over_gated_amsgrad"] = round(res["reference"]["median"] / res["gated_amsgrad"]["median"], 3)
    res["gated_amsgrad_over_graph"] = round(res["gated_amsgrad"]["median"] / res["graph"]["median"], 3)
    res["host_bound"] = bool(res["gated_amsgrad"]["median"] > 2 * res["graph"]["median"])
    if "stock_capturable_graph" in res:
        res["stock_capturable_graph_over_graph"] = round(res["stock_capturable_graph"]["median"] / res["graph"]["median"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
