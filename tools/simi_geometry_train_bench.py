"""Forward + backward of the training step's similarity geometry, hdn_amd.simi_geometry (csrc/simi_geometry.hip) against the reference's formulation on
PyTorch-ROCm: profiles/simi_geometry_train.json and one JSON line.

    python tools/simi_geometry_train_bench.py [--rounds 7] [--seconds 1.0] [--out profiles/simi_geometry_train.json]

A step = what model_builder_e2e_unconstrained_v2.py:377, :390, :396-404 and :409-415 do at TRAIN.BATCH_SIZE 32: cls, loc [32,2,25,25] give polar,
cls_lp [32,2,13,13] and loc_lp [32,4,13,13] give scale and rot, then the four matrices and the two point sets.  loc and loc_lp require grad; a scalar
is formed from fixed random weights on polar, affine_m, affine_m_lt0 and pred_points, and one backward delivers the two gradients.  In the same
process, on the same inputs:
  reference   the lines restated in PyTorch with their per-step host uploads kept: the point tables from numpy, torch.zeros / ones / tensor(...) made
              on the host and copied to the device, argmax / softmax / expand / gather / stack / permute / cat / bmm as the reference issues them
  drop_ins    the same lines with hdn_amd's get_polar_from_two_para_loc, lp_pick, combine_affine_c0_v2 and combine_affine_lt0 in place: what
              install(train=True) gives the reference while SIMI_GEOMETRY_TRAIN_BOUND (the uploads of :396-398 and :409-410 stay: they are the model's)
  fused       hdn_amd.polar_pick + hdn_amd.similarity_warps: two launches forward, two backward, nothing from the host
Before timing the sides are compared (1e-4 of the largest element of each output and gradient: a coarse check that they compute the same thing; the
bounds against float64 are the business of tests/test_gpu_simi_geometry.py).  All sides are warmed up (one untimed window each), then alternate
--rounds times; a window repeats whole steps until at least --seconds have passed on the host clock and is timed by device events around it.
Reported per side: median, min and max ms per step over the windows.
`ahead`: is the drop_ins median below the reference median by more than the larger of the two sides' (max - min)?  It decides
hdn_amd.install.SIMI_GEOMETRY_TRAIN_BOUND.  This tool promises no speed-up.

There is no CPU fallback: without a GPU this tool fails."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, S, S_LP = 32, 25, 13
STRIDE, STRIDE_LP, MAP_SIZE, IN_SZ, OUT_SZ = 8, 8, 127, 255, 127
OUTS = ("polar", "affine_m", "affine_m_lt0", "pred_points")


def make_inputs(dev):
    gen = torch.Generator().manual_seed(20261021)
    rn = lambda *s: torch.randn(*s, generator=gen)
    t = {"cls": 2 * rn(B, 2, S, S), "loc": rn(B, 2, S, S), "cls_lp": 2 * rn(B, 2, S_LP, S_LP), "loc_lp": 0.5 * rn(B, 4, S_LP, S_LP),
         "temp_cx": 63.5 + 5 * rn(B), "temp_cy": 63.5 + 5 * rn(B), "search_poly": 127 + 40 * rn(B, 4, 2)}
    w = {"polar": rn(B, 2), "affine_m": rn(B, 2, 3), "affine_m_lt0": rn(B, 2, 3), "pred_points": rn(B, 3, 4)}
    t = {k: v.to(dev) for k, v in t.items()}
    t["loc"].requires_grad_(True)
    t["loc_lp"].requires_grad_(True)
    return t, {k: v.to(dev) for k, v in w.items()}


# ---- the reference's formulation, restated; every .to(dev) of a host tensor below is a pageable upload per step
def grid_points(stride, size):
    first = -(size // 2) * stride
    x, y = np.meshgrid([first + stride * i for i in np.arange(0, size)], [first + stride * j for j in np.arange(0, size)])
    pts = np.zeros((size * size, 2), dtype=np.float32)
    pts[:, 0], pts[:, 1] = x.astype(np.float32).flatten(), y.astype(np.float32).flatten()
    return pts


def _gather_best(best, delta, table):
    n = delta.size(0)
    pick = best.unsqueeze(1).unsqueeze(2).expand(n, 1, delta.size(2))
    table = table.expand(n, table.size(0), table.size(1))
    return torch.gather(delta, 1, pick).squeeze(1), torch.gather(table, 1, pick[:, :, 0:2]).squeeze(1)


class RefPolarPick:
    def __init__(self, dev):
        self.points = torch.from_numpy(grid_points(STRIDE, S))
        self.points_dev = self.points.to(dev)

    def get_polar_from_two_para_loc(self, cls, loc):
        n = cls.size(0)
        score = cls.view(n, 2, -1).permute(0, 2, 1)
        best = torch.argmax(score[:, :, 1], 1)
        delta, point = _gather_best(best, loc.view(n, 2, -1).permute(0, 2, 1), self.points_dev)
        out = torch.zeros(n, 2).to(cls.device)
        out[:, 0] = point[:, 0] - delta[:, 0]
        out[:, 1] = point[:, 1] - delta[:, 1]
        return out


def ref_lp_pick(cls, loc, channels, stride, stride_lp, size_lp, map_size):
    n = cls.size(0)
    score = cls.view(n, channels, -1).permute(0, 2, 1)
    best = torch.argmax(score.softmax(2)[:, :, 1], 1)
    table = torch.from_numpy(grid_points(stride, size_lp)).to(cls.device)
    delta, point = _gather_best(best, loc.view(n, 4, -1).permute(0, 2, 1), table)
    scale = point[:, 0] - delta[:, 0] * stride_lp
    rot = (point[:, 1] - delta[:, 2] * stride_lp) * (2 * np.pi / map_size)
    return torch.exp(scale * (np.log(map_size / 2) / map_size)), rot


def ref_c0_v2(cx, cy, shift, scale, rot, scale_h, in_sz, out_sz):
    cc, ss = torch.cos(rot), torch.sin(rot)
    sc = out_sz / in_sz * scale
    a, b, c, d = sc * cc, -sc * ss, sc * ss, sc * cc
    ux, uy = (cx - out_sz / 2) * in_sz / out_sz, (cy - out_sz / 2) * in_sz / out_sz
    t0, t1 = -a * ux - b * uy + shift[:, 0], -c * ux - d * uy + shift[:, 1]
    if scale_h:
        t0, t1 = t0 / out_sz, t1 / out_sz
    return torch.stack([a, b, t0, c, d, t1]).permute(1, 0).reshape([-1, 2, 3]).float()


def ref_lt0(cx, cy, shift, scale, rot, in_sz, o_sz):
    cc, ss = torch.cos(rot), torch.sin(rot)
    o, p, q, l = scale * cc, -scale * ss, scale * ss, scale * cc
    sx, sy = shift[:, 0] + in_sz / 2, shift[:, 1] + in_sz / 2
    return torch.stack([o, p, -o * sx - p * sy + cx, q, l, -q * sx - l * sy + cy]).permute(1, 0).reshape([-1, 2, 3]).float()


def make_step(kind, t, w, dev):
    import hdn_amd
    if kind == "reference":
        picker, lp_pick, c0_v2, lt0 = RefPolarPick(dev), ref_lp_pick, ref_c0_v2, ref_lt0
        get_polar = RefPolarPick.get_polar_from_two_para_loc
    else:
        picker = types.SimpleNamespace(points=torch.from_numpy(grid_points(STRIDE, S)))
        get_polar, lp_pick, c0_v2, lt0 = hdn_amd.get_polar_from_two_para_loc, hdn_amd.lp_pick, hdn_amd.combine_affine_c0_v2, hdn_amd.combine_affine_lt0
    half = OUT_SZ / 2

    def lines():
        polar = get_polar(picker, t["cls"], t["loc"] * STRIDE)
        scale, rot = lp_pick(t["cls_lp"], t["loc_lp"], 2, STRIDE, STRIDE_LP, S_LP, MAP_SIZE)
        ones = torch.ones([B]).float().to(dev)
        zeros = torch.zeros([B]).float().to(dev)
        zeros2 = torch.zeros([B, 2]).float().to(dev)
        m = c0_v2(half, half, polar, scale, rot, True, IN_SZ, OUT_SZ)
        m_lt0 = lt0(half, half, polar, 1 / scale, -rot, IN_SZ, OUT_SZ)
        m_aug = c0_v2(t["temp_cx"], t["temp_cy"], zeros2, ones, zeros, True, IN_SZ, OUT_SZ)
        m_lt0_aug = lt0(t["temp_cx"], t["temp_cy"], zeros2, ones, zeros, IN_SZ, OUT_SZ)
        poly_ones = torch.ones([B, 1, 4]).to(dev)
        last = torch.tensor([0, 0, 1]).float().repeat([B, 1, 1]).to(dev)
        poly_h = torch.cat([t["search_poly"].permute(0, 2, 1), poly_ones], 1)
        aug_points = torch.bmm(torch.cat([m_lt0_aug, last], 1), poly_h)
        points = torch.bmm(torch.cat([m_lt0, last], 1), poly_h)
        return {"polar": polar, "scale": scale, "rot": rot, "affine_m": m, "affine_m_lt0": m_lt0, "affine_m_c_aug": m_aug,
                "affine_m_lt0_aug": m_lt0_aug, "pred_points": points, "aug_sear_points": aug_points}

    def fused():
        polar = hdn_amd.polar_pick(t["cls"], t["loc"], stride=STRIDE)
        out = hdn_amd.similarity_warps(t["cls_lp"], t["loc_lp"], polar, t["temp_cx"], t["temp_cy"], t["search_poly"], stride=STRIDE,
                                       stride_lp=STRIDE_LP, map_size=MAP_SIZE, in_sz=IN_SZ, out_sz=OUT_SZ)
        out["polar"] = polar
        return out

    forward = fused if kind == "fused" else lines

    def step():
        t["loc"].grad = t["loc_lp"].grad = None
        out = forward()
        total = (w["polar"] * out["polar"]).sum()
        for k in OUTS[1:]:
            total = total + (w[k] * out[k]).sum()
        total.backward()
        return {k: v.detach() for k, v in out.items()}, [t["loc"].grad.clone(), t["loc_lp"].grad.clone()]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simi_geometry_train.json"))
    args = ap.parse_args()
    if args.rounds < 7 or args.seconds < 1.0:
        ap.error("at least seven alternations, each window at least one second")
    if not torch.cuda.is_available():
        raise SystemExit("tools/simi_geometry_train_bench.py measures on a GPU; there is none here")
    dev = torch.device("cuda:0")
    t, w = make_inputs(dev)
    names = ("drop_ins", "reference", "fused")
    steps = {name: make_step(name, t, w, dev) for name in names}
    ref_out, ref_grads = steps["reference"]()
    agreement = {}
    for name in ("drop_ins", "fused"):
        out, grads = steps[name]()
        do = max(float((out[k] - ref_out[k]).abs().max() / ref_out[k].abs().max()) for k in ref_out)
        dg = max(float((g - r).abs().max() / r.abs().max()) for g, r in zip(grads, ref_grads))
        agreement[name] = {"worst_output_difference_over_largest": float("%.3g" % do), "worst_gradient_difference_over_largest": float("%.3g" % dg)}
        assert do <= 1e-4 and dg <= 1e-4, f"{name} disagrees with the reference's formulation: {agreement}"
    for name in names:
        window(steps[name], args.seconds)
        print(f"[simi_geometry_train_bench] {name}: warm", file=sys.stderr, flush=True)
    ms, counts = {name: [] for name in names}, {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            v, n = window(steps[name], args.seconds)
            ms[name].append(v)
            counts[name].append(n)
            print(f"[simi_geometry_train_bench] {name}: {v:.4f} ms per step over {n} steps", file=sys.stderr, flush=True)
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "B": B, "S": S, "S_lp": S_LP, "rounds": args.rounds,
           "window_seconds": args.seconds, "steps_per_window": counts, "against_reference_formulation": agreement}
    for name in names:
        res[name] = summary(ms[name])
    res["reference_over_drop_ins"] = round(res["reference"]["median"] / res["drop_ins"]["median"], 3)
    res["reference_over_fused"] = round(res["reference"]["median"] / res["fused"]["median"], 3)
    spread_ms = max(res[n]["max"] - res[n]["min"] for n in ("drop_ins", "reference"))
    res["ahead"] = bool(res["reference"]["median"] - res["drop_ins"]["median"] > spread_ms)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
