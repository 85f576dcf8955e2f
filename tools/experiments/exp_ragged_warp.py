"""What reading (H, W) from device memory costs the perspective warp: hdn_frame_warp_perspective_ragged_u8 against hdn_frame_warp_perspective_batch_u8
at n = 16 frames of 720 x 1280, every slot at full capacity, in one process.  100 launches of each, alternating batch / ragged / batch: the batch entry
is timed twice, so the distance between its two series is the run-to-run spread the ragged series is read against.  Device events around every launch."""
import os, sys
R = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."); sys.path.insert(0, R)
import numpy as np
import torch
from hdn_amd import frame as FR
dev = torch.device("cuda:0")
n, H, W, reps = 16, 720, 1280, 100
g = np.random.default_rng(0)
frames = torch.from_numpy(g.integers(0, 256, (n, H, W, 3), dtype=np.uint8)).to(dev)
arena = FR.FrameArena(n, H, W, device=dev)
arena.set_all([frames[b] for b in range(n)])
Hs = np.tile(np.eye(3), (n, 1, 1))
Hs[:, :2, 2] = g.normal(0, 6, (n, 2)); Hs[:, :2, :2] += g.normal(0, 0.03, (n, 2, 2)); Hs[:, 2, :2] = g.normal(0, 1e-5, (n, 2))
M = torch.from_numpy(Hs.reshape(n, 9)).to(dev)
calls = {"batch (1st series)": lambda: FR.warp_perspective(frames, M), "ragged": lambda: FR.warp_perspective(arena, M),
         "batch (2nd series)": lambda: FR.warp_perspective(frames, M)}
assert torch.equal(calls["ragged"]().data.view(n, H, W, 3), calls["batch (1st series)"]())        # same bytes, before any timing
for _ in range(10):
    for f in calls.values(): f()
torch.cuda.synchronize()
ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for k in calls}
for i in range(reps):
    for k, f in calls.items():
        a, b = ev[k][i]
        a.record(); f(); b.record()
torch.cuda.synchronize()
px = n * H * W
for k in calls:
    t = np.array([a.elapsed_time(b) * 1e3 for a, b in ev[k]])
    print("%-20s median %7.1f us  mean %7.1f us  min %7.1f us  p90 %7.1f us   (%.2f Gpixel/s at the median)" %
          (k, np.median(t), t.mean(), t.min(), np.percentile(t, 90), px / np.median(t) * 1e-3))
