"""Map smoothing timing (tools only): device-event ms per ``smooth_maps`` call (with the per-image maximum and without) at the
MVTec grid test split (78 x 128 px) and at 8 x 1024 px tiles, for sigma 4 and 16, next to ``anomaly_maps`` (ws 11) on the same
images.  Beside each time: the bytes the call must move (the maps read once, written once) and its fp64 operations (3 per tap
plus the centre, in the H pass also for the 2r halo columns of every 128-column tile), as rates, to tell whether the kernel is
bound by memory traffic or by fp64 issue.  --reps N timed calls after one warm-up call."""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from importlib import import_module
M = import_module("anomaly-detection-super-resolution_amd.metrics")

TILE_W = 128                                             # kTileW of kernels_map_smooth.hip


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
args = ap.parse_args()
g = torch.Generator().manual_seed(5)
for tag, n, px in (("grid_78x128px", 78, 128), ("tile_8x1024px", 8, 1024)):
    hr = torch.randint(0, 256, (n, px, px, 1), generator=g, dtype=torch.uint8)
    sr = (hr.int() + torch.randint(-6, 7, (n, px, px, 1), generator=g, dtype=torch.int32)).clamp(0, 255).to(torch.uint8)
    sr, hr = sr.cuda(), hr.cuda()
    ms_maps = timed(lambda: M.anomaly_maps(sr, hr, 11), args.reps)
    maps = M.anomaly_maps(sr, hr, 11)
    print(f"{tag}: pixels={n * px * px}  anomaly_maps(ws=11) {ms_maps:.3f} ms", flush=True)
    for sigma in (4.0, 16.0):
        r = len(M.gaussian_weights(sigma)) - 1
        tiles_x = (px + TILE_W - 1) // TILE_W
        flops = (3 * r + 1) * (n * px * (px + 2 * r * tiles_x) + n * px * px)
        nbytes = 8 * n * px * px
        ms = timed(lambda: M.smooth_maps(maps, sigma), args.reps)
        ms_max = timed(lambda: M.smooth_maps(maps, sigma, with_max=True), args.reps)
        print(f"  sigma={sigma:g} (r={r}): smooth_maps {ms:.4f} ms, with max {ms_max:.4f} ms  "
              f"({nbytes / 1e6:.1f} MB -> {nbytes / ms / 1e6:.0f} GB/s; {flops / 1e9:.2f} G fp64 op -> {flops / ms / 1e9:.2f} T op/s)  "
              f"smooth/maps {ms_max / ms_maps:.2f}", flush=True)
