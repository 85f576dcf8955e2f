"""Both correlation heads at batch B, forward time at HDN_HIP_HEADS levels 0 / 1 / 2, on one GPU: profiles/head_batch.json and one JSON line.

    python tools/head_batch_bench.py [--batches 1,4,16,32] [--rounds 3] [--replays 200] [--out profiles/head_batch.json]

Seeded MultiBAN and MultiCircBAN at 256 channels with the tracker's shapes (7 x 7 template / 31 x 31 search features; 15 x 15 / 15 x 15 log-polar), at
every batch of the lock-step trackers.  A case is ONE forward captured as a hipGraph with the template cache warm, replayed --replays times back to
back between two events: us per forward = elapsed / replays.  The levels alternate within a round (0, 1, 2, 0, 1, 2, ...: --rounds alternations, at
least 3, in one process on one box) and the figure of a (head, batch, level) is the median over the rounds, with the smallest and largest beside it.
Also the number of kernel nodes of each graph (what a frame graph of a lock-step tracker carries per head) and, per (head, batch), level 2's outputs
against level 0's (max |difference| / max |value|).  The level is set through head._hdn_hip_heads, which is what HDN_HIP_HEADS sets for every head.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

SHAPES = {"MultiBAN": (7, 31), "MultiCircBAN": (15, 15)}        # template / search feature side
LEVELS = (0, 1, 2)


def _hip_runtime():
    """The HIP runtime this process already has loaded (the graph handle belongs to it), or None."""
    try:
        with open("/proc/self/maps") as f:
            paths = {line.split()[-1] for line in f if "libamdhip64" in line}
        return ctypes.CDLL(sorted(paths)[0]) if paths else None
    except OSError:
        return None


def kernel_nodes(graph):
    """Number of kernel nodes of a captured torch.cuda.CUDAGraph(keep_graph=True), or None where the handle is not to be had."""
    hip = _hip_runtime()
    if hip is None or not hasattr(graph, "raw_cuda_graph"):
        return None
    handle = ctypes.c_void_p(graph.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    if hip.hipGraphGetNodes(handle, None, ctypes.byref(n)) != 0 or n.value == 0:
        return None
    nodes = (ctypes.c_void_p * n.value)()
    if hip.hipGraphGetNodes(handle, nodes, ctypes.byref(n)) != 0:
        return None
    count = 0
    for node in nodes:
        kind = ctypes.c_int(-1)
        if hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(kind)) != 0:
            return None
        count += kind.value == 0                                 # hipGraphNodeTypeKernel
    return count


class Case:
    """One (head, batch, level): its own module (so its packs and template cache stay warm between rounds), static inputs and the captured forward."""

    def __init__(self, cls_name, B, level, dev):
        import head_batch_cases as HB
        zs, xs = SHAPES[cls_name]
        g = torch.Generator().manual_seed(100 + B)
        self.head = HB.seeded_head(cls_name).to(dev)
        self.head._hdn_hip_heads = level
        self.z = [torch.randn(B, 256, zs, zs, generator=g).to(dev) for _ in range(3)]
        self.x = [torch.randn(B, 256, xs, xs, generator=g).to(dev) for _ in range(3)]
        for _ in range(3):                                        # template cache, packs, library handles
            self.head(self.z, self.x)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.head(self.z, self.x)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        try:
            self.graph = torch.cuda.CUDAGraph(keep_graph=True)
            keep = True
        except TypeError:
            self.graph, keep = torch.cuda.CUDAGraph(), False
        with torch.cuda.graph(self.graph):
            self.out = self.head(self.z, self.x)
        self.nodes = kernel_nodes(self.graph) if keep else None
        if keep:
            self.graph.instantiate()
        self.graph.replay()
        torch.cuda.synchronize()

    def us_per_forward(self, replays):
        for _ in range(10):
            self.graph.replay()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            self.graph.replay()
        b.record()
        b.synchronize()
        return 1e3 * a.elapsed_time(b) / replays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4,16,32")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_batch.json"))
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds: at least three alternations of the levels")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "replays": args.replays, "torch": torch.__version__, "cases": []}
    with torch.no_grad():
        for cls_name in SHAPES:
            for B in (int(b) for b in args.batches.split(",")):
                cases = {lv: Case(cls_name, B, lv, dev) for lv in LEVELS}
                times = {lv: [] for lv in LEVELS}
                for _ in range(args.rounds):                      # the levels alternate: drift of the box lands on all three alike
                    for lv in LEVELS:
                        times[lv].append(cases[lv].us_per_forward(args.replays))
                ref = cases[0].out
                row = {"head": cls_name, "batch": B}
                for lv in LEVELS:
                    t = sorted(times[lv])
                    row[f"level{lv}"] = {"us": round(statistics.median(t), 2), "us_min": round(t[0], 2), "us_max": round(t[-1], 2),
                                         "kernel_nodes": cases[lv].nodes}
                    row[f"level{lv}"]["rel_diff_vs_level0"] = max(float((g - w).abs().max() / w.abs().max()) for g, w in zip(cases[lv].out, ref))
                row["level2_vs_level1"] = round(row["level1"]["us"] / row["level2"]["us"], 3)
                res["cases"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                del cases
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
