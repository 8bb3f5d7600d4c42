"""Pixel-level metrics timing (tools only): device-event ms per call of ``anomaly_maps`` (one window size) and of the exact
``pixel_roc_auc`` over all pixels of the split, at the MVTec grid test split (78 x 128 px) and at 8 x 1024 px tiles.
--reps N timed calls after one warm-up call.  Bytes per pixel are the algorithm's: maps = 2 u8 planes read + the five float64
tables written, summed down the columns (read + written twice) and read by the map kernel + fp32 map written; AUC = the keys
(u64) written once, read twice and written once in each of the 3 radix passes, read twice by the final scan, plus the scores and
labels read once."""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from importlib import import_module
M = import_module("anomaly-detection-super-resolution_amd.metrics")

MAP_BYTES_PER_PX = 2 + 40 + 2 * 80 + 40 * 4 + 4     # sr + hr, rows pass, column passes, 4 corners x 5 tables (L2-served), map
AUC_BYTES_PER_PX = 5 + 8 + 3 * 24 + 2 * 8           # scores + labels, keys, 3 passes, final scan (count matrix not counted)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
for tag, n, px in (("grid_78x128px", 78, 128), ("tile_8x1024px", 8, 1024)):
    g = torch.Generator(device="cpu").manual_seed(5)
    hr = torch.randint(0, 256, (n, px, px, 1), generator=g, dtype=torch.uint8).cuda()
    sr = (hr.int() + torch.randint(-6, 7, hr.shape, generator=g).cuda()).clamp(0, 255).to(torch.uint8)
    ws = 11
    maps = M.anomaly_maps(sr, hr, ws)
    labels = (torch.rand(maps.shape, generator=g) < 0.1).to(torch.uint8).cuda()
    M.pixel_roc_auc(maps, labels)
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    for _ in range(args.reps):
        M.anomaly_maps(sr, hr, ws)
    e[1].record()
    # pixel_roc_auc reads its four counts back (a device-to-host copy that synchronises): that is part of the call
    for _ in range(args.reps):
        M.pixel_roc_auc(maps, labels)
    e[2].record()
    torch.cuda.synchronize()
    ms_map, ms_auc = e[0].elapsed_time(e[1]) / args.reps, e[1].elapsed_time(e[2]) / args.reps
    npx = n * px * px
    print(f"{tag}: pixels={npx} anomaly_maps(ws={ws}) {ms_map:.3f} ms ({MAP_BYTES_PER_PX} B/px, "
          f"{MAP_BYTES_PER_PX * npx / ms_map / 1e6:.0f} GB/s)  pixel_roc_auc {ms_auc:.3f} ms ({AUC_BYTES_PER_PX} B/px, "
          f"{AUC_BYTES_PER_PX * npx / ms_auc / 1e6:.0f} GB/s)", flush=True)
