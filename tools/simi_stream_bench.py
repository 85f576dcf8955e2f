"""The similarity-only lock-step tracker with and without slots (frame_capacity), frames per second on one GPU: profiles/simi_stream.json and one JSON line.

    python tools/simi_stream_bench.py [--batches 4,16] [--rounds 5] [--seconds 1.0] [--out profiles/simi_stream.json]

The production-shaped stand-in (tests/production_standin.py: ResNet-50 on PyTorch-ROCm, 256-channel heads), 1280 x 720 frames, n sequences per step,
one hipGraph per step.  Two BatchedSimiTracker objects, each around its own copy of the model, are given the SAME frames: `fixed` (the frame size a
launch argument, one dense [n,H,W,3] buffer) and `arena` (frame_capacity=(720, 1280): the frames in a FrameArena, every size read from device
memory).  A step is track_new(list of n host frames) as a user calls it - the upload, one graph replay, one host read.  After a warm-up the two
alternate within a round (fixed, arena, fixed, arena, ...; --rounds rounds in one process on one box); a timed window runs whole steps until at least
--seconds have passed and ends in a synchronise; frames/s = n * steps / elapsed.  Reported per (n, mode): the median over the rounds with the
smallest and the largest beside it.  At equal sizes the ragged grids are those of the batch kernels (sized from the capacity), so the two should
cost the same; the spread over the rounds says what "the same" means on the day.

Then one track_videos run: videos of two frame sizes (1280 x 720 and 960 x 540) and different lengths through n = 4 slots, frames/s over the whole
call (init with the capture of its graph, the re-inits and idle slots included).

There is no CPU fallback: without a GPU this tool fails."""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

CAPACITY = (720, 1280)


def _model(dev, frames, init):
    import production_standin as PS
    from test_gpu_parity import _seeded_net
    twin = PS.ProductionStandIn(_seeded_net())
    twin.calibrate(*PS.calibration_crops(frames, init))
    return twin.to(dev).eval()


def _window(tracker, frames, n, seconds, step0):
    """Whole steps until `seconds` have passed, ended by a synchronise -> (frames/s, steps)."""
    torch.cuda.synchronize()
    t0, steps = time.perf_counter(), 0
    while True:
        tracker.track_new(step0 + steps, [frames[1 + (step0 + steps) % (len(frames) - 1)]] * n)
        steps += 1
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return n * steps / (time.perf_counter() - t0), steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simi_stream.json"))
    args = ap.parse_args()
    if args.rounds < 3 or args.seconds < 1.0:
        ap.error("at least three alternations, each window at least a second")
    if not torch.cuda.is_available():
        raise SystemExit("tools/simi_stream_bench.py measures on a GPU; there is none here")
    from synth_sequence import make_sequence
    from hdn_amd import track_videos
    from hdn_amd.simi_tracker import BatchedSimiTracker
    dev = torch.device("cuda:0")
    frames, _, init = make_sequence(n_frames=5, frame_hw=CAPACITY, target_wh=(300, 200), seed=20260928)
    model = _model(dev, frames, init)
    fp = np.array([init["first_point"]])
    res = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "frame_hw": list(CAPACITY), "rounds": args.rounds,
           "window_seconds": args.seconds, "cases": []}
    for n in (int(b) for b in args.batches.split(",")):
        trackers = {"fixed": BatchedSimiTracker(copy.deepcopy(model), n, graph=True),
                    "arena": BatchedSimiTracker(copy.deepcopy(model), n, graph=True, frame_capacity=CAPACITY)}
        done = {}
        for name, t in trackers.items():
            t.init([frames[0]] * n, [init["bbox"]] * n, [init["poly"]] * n, [fp] * n)
            for i in range(5):                                    # capture, MIOpen find at this batch, pinned staging
                t.track_new(i, [frames[1 + i % (len(frames) - 1)]] * n)
            if t._graph is None:
                raise SystemExit(f"{name}: the step was not captured as a hipGraph")
            done[name] = 5
        fps = {name: [] for name in trackers}
        for _ in range(args.rounds):                              # the two alternate: drift of the box lands on both alike
            for name, t in trackers.items():
                f, steps = _window(t, frames, n, args.seconds, done[name])
                done[name] += steps
                fps[name].append(f)
        row = {"n": n}
        for name in trackers:
            v = sorted(fps[name])
            row[name] = {"frames_per_s": round(statistics.median(v), 1), "min": round(v[0], 1), "max": round(v[-1], 1)}
        row["arena_vs_fixed"] = round(row["arena"]["frames_per_s"] / row["fixed"]["frames_per_s"], 4)
        row["heads_template_branch_in_graph"] = bool(trackers["arena"]._kern_in_graph)
        res["cases"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del trackers
        torch.cuda.empty_cache()
    # a dataset of two frame sizes and different lengths through four slots
    small, _, init_s = make_sequence(n_frames=5, frame_hw=(540, 960), target_wh=(220, 150), seed=20260929)
    lengths, which = [40, 25, 60, 30, 45, 20, 35, 50, 15, 30], [0, 1, 0, 1, 1, 0, 1, 0, 1, 0]
    videos = []
    for T, w in zip(lengths, which):
        fr, ini = (frames, init) if w == 0 else (small, init_s)
        videos.append(([fr[0]] + [fr[1 + i % (len(fr) - 1)] for i in range(T - 1)], ini))
    t = BatchedSimiTracker(copy.deepcopy(model), 4, graph=True, frame_capacity=CAPACITY)
    track_videos(t, videos[:4])                                   # warm-up: MIOpen's choices at this batch, the library's lazy initialisations
    torch.cuda.synchronize()
    s0, t0 = t.host_syncs, time.perf_counter()
    out = track_videos(t, videos)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tracked = sum(len(r) for r in out)
    assert tracked == sum(lengths) - len(lengths)
    res["track_videos"] = {"n": 4, "videos": len(videos), "lengths": lengths, "frame_hw": [list(CAPACITY) if w == 0 else [540, 960] for w in which],
                           "frames_tracked": tracked, "seconds": round(dt, 3), "frames_per_s": round(tracked / dt, 1),
                           "host_reads": t.host_syncs - s0}
    print(json.dumps(res["track_videos"]), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
