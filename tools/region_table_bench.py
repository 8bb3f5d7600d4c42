"""Region-table timing (tools only): device-event ms per call of ``region_table`` and, on the same input, of the calls it
follows and shares its labelling with - ``operating_point`` (``min_area`` 1, no masks: threshold and count) and
``mask_regions`` (the labelling, the sizes and the counts) - on three masks at 64 x 256 x 256: blob-like predictions, one
region filling each image, and the stride-2 lattice of single pixels (the most regions a shape holds).  The maps are made so
that ``maps > 0.5`` is the mask, and ``region_table`` is given the mask ``operating_point`` returned.  ``region_table`` is
timed at a capacity that holds every record (one call of the entry point) and at the default capacity (a second call where
more than 4096 regions exist).  Each Python call reads its counts back, which synchronises: that is part of the call.
--repeats blocks of --reps calls after a warm-up call of each; the median block is printed, with the spread."""
import argparse
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from importlib import import_module
M = import_module("anomaly-detection-super-resolution_amd.metrics")


def blob_mask(n, px, g):
    yy, xx = torch.meshgrid(torch.arange(px), torch.arange(px), indexing="ij")
    masks = torch.zeros(n, px, px, dtype=torch.uint8)
    for i in range(n):
        for k in range(30):
            cy, cx = torch.randint(0, px, (2,), generator=g).tolist()
            r = px * (0.04 + 0.08 * torch.rand(1, generator=g).item()) if k < 3 else 1 + 3 * torch.rand(1, generator=g).item()
            masks[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    return masks


def cases(n, px, g):
    full = torch.ones(n, px, px, dtype=torch.uint8)
    lattice = torch.zeros(n, px, px, dtype=torch.uint8)
    lattice[:, ::2, ::2] = 1
    return (("blobs", blob_mask(n, px, g)), ("full", full), ("lattice", lattice))


ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--px", type=int, default=256)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
g = torch.Generator().manual_seed(7)
median = {}
for tag, mask in cases(args.n, args.px, g):
    maps = (torch.randint(0, 128, mask.shape, generator=g).float() / 256 + 0.5 * mask.float() + 1 / 512).cuda()   # ties; > 0.5 on the mask
    pred, _, _ = M.operating_point(maps, 0.5, None, 1)
    assert torch.equal(pred, mask.cuda())
    n_reg = M.region_table(pred, maps)["n_regions"]
    calls = (("region_table", lambda: M.region_table(pred, maps, cap=max(n_reg, 1))),
             ("region_table default cap", lambda: M.region_table(pred, maps)),
             ("operating_point", lambda: M.operating_point(maps, 0.5, None, 1)),
             ("mask_regions", lambda: M.mask_regions(pred)))
    for _, f in calls:
        f()
    torch.cuda.synchronize()
    blocks = [[] for _ in calls]
    for _ in range(args.repeats):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
        e[0].record()
        for k, (_, f) in enumerate(calls):
            for _ in range(args.reps):
                f()
            e[k + 1].record()
        torch.cuda.synchronize()
        for k in range(len(calls)):
            blocks[k].append(e[k].elapsed_time(e[k + 1]) / args.reps)
    median[tag] = statistics.median(blocks[0])
    print(f"{tag}: pixels={mask.numel()} regions={n_reg} member pixels={int(mask.sum())}  "
          + "  ".join(f"{name} {statistics.median(b):.3f} ms [{min(b):.3f}, {max(b):.3f}]" for (name, _), b in zip(calls, blocks)), flush=True)
print(f"region_table, one region per image / blobs: {median['full'] / median['blobs']:.2f}; lattice / blobs: "
      f"{median['lattice'] / median['blobs']:.2f}")
