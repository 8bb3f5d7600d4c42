"""Operating-point timing (tools only): device-event ms per call of ``map_threshold`` (the radix select), of ``operating_point``
with masks at ``min_area`` 1 and 4, and - the yardstick, on the same arrays in the same run - of the sort-based
``pixel_roc_auc``, at the two cases of pro_bench.py: the MVTec grid test split (78 x 128 px) and 8 x 1024 px tiles, maps with
~70 % of the pixels exactly 0.0 (one huge tie group).  --reps N timed calls after one warm-up call of each.  Each Python call
reads its counts back (a device-to-host copy that synchronises): that is part of the call, as in pro_bench.py."""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from importlib import import_module
M = import_module("anomaly-detection-super-resolution_amd.metrics")


def blob_case(n, px, g):
    """The case of pro_bench.py: disc masks (a third of the images good), 1/256-quantised maps raised inside the discs, ~70 %
    exact zeros."""
    yy, xx = torch.meshgrid(torch.arange(px), torch.arange(px), indexing="ij")
    masks = torch.zeros(n, px, px, dtype=torch.uint8)
    for i in range(n):
        if i % 3 == 0:
            continue
        for k in range(40):
            cy, cx = torch.randint(0, px, (2,), generator=g).tolist()
            r = px * (0.05 + 0.1 * torch.rand(1, generator=g).item()) if k < 3 else 1 + 3 * torch.rand(1, generator=g).item()
            masks[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    maps = torch.randint(0, 256, (n, px, px), generator=g).float() / 256 + 0.25 * masks.float()
    maps[torch.rand(n, px, px, generator=g) < 0.7] = 0.0
    return maps.cuda(), masks.cuda()


ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rate", type=float, default=0.01)
args = ap.parse_args()
for tag, n, px in (("grid_78x128px", 78, 128), ("tile_8x1024px", 8, 1024)):
    maps, masks = blob_case(n, px, torch.Generator().manual_seed(7))
    t, rate = M.map_threshold(maps, args.rate)
    calls = (("map_threshold", lambda: M.map_threshold(maps, args.rate)),
             ("operating_point min_area=1", lambda: M.operating_point(maps, t, masks, 1)),
             ("operating_point min_area=4", lambda: M.operating_point(maps, t, masks, 4)),
             ("pixel_roc_auc", lambda: M.pixel_roc_auc(maps, masks)))
    for _, f in calls:
        f()
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
    e[0].record()
    for k, (_, f) in enumerate(calls):
        for _ in range(args.reps):
            f()
        e[k + 1].record()
    torch.cuda.synchronize()
    ms = [e[k].elapsed_time(e[k + 1]) / args.reps for k in range(len(calls))]
    counts = M.operating_point(maps, t, masks, 4)[2]
    print(f"{tag}: pixels={n * px * px} threshold={t:g} (rate {args.rate:g}, achieved {rate:.6f}) predicted@4={counts['tp'] + counts['fp']}  "
          + "  ".join(f"{name} {v:.3f} ms" for (name, _), v in zip(calls, ms))
          + f"  select/auc {ms[0] / ms[3]:.2f}", flush=True)
