"""Squared-error map timing (tools only): device-event ms per call of ``error_maps`` / ``error_maps_multi`` and, in the same
process as the yardstick, of ``anomaly_maps`` / ``anomaly_maps_multi`` at the same shape and sizes: the MVTec grid test split
(78 x 128 px) and 8 x 1024 px tiles, gray, at ws 1, ws 11 and [11, 21, 31] mean.  The two sources alternate round by round after
a warm-up of both; the medians over the rounds and their ratio are printed, each squared-error output is compared bit for bit
with the numpy definition on the first image, and each case is set against what its bytes allow at --tbps (HBM, TB/s): the
ws 1 launch moves 2 C + 4 bytes per pixel; the table path writes 8 B of table in the row pass, moves 16 to 32 B in the column
pass and reads 8 B of corners per size (no reflection) before the 4 B store.  --rounds N rounds of --reps calls each."""
import argparse
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from importlib import import_module
M = import_module("anomaly-detection-super-resolution_amd.metrics")


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def definition(sr, hr, sizes):
    """numpy: the mean over ``sizes`` of float32(S * inv) for [1, H, W, C] u8 arrays (fp32 sum in list order)."""
    d = sr.astype(np.int64) - hr.astype(np.int64)
    e = (d * d).sum(-1)
    H, W = e.shape[1:]
    acc = None
    for ws in sizes:
        lo, hi = ws // 2, ws - 1 - ws // 2
        p = np.pad(e, ((0, 0), (lo, hi), (lo, hi)), mode="reflect")
        c = np.zeros((1, p.shape[1] + 1, p.shape[2] + 1), dtype=np.int64)
        c[:, 1:, 1:] = p.cumsum(1).cumsum(2)
        S = c[:, ws:ws + H, ws:ws + W] - c[:, :H, ws:ws + W] - c[:, ws:ws + H, :W] + c[:, :H, :W]
        m = np.float32(S.astype(np.float64) * (1.0 / (sr.shape[-1] * ws * ws * 65025)))
        acc = m if acc is None else acc + m
    return acc * np.float32(1.0 / len(sizes)) if len(sizes) > 1 else acc


def bench(args):
    g = torch.Generator().manual_seed(5)
    for tag, n, px in (("grid_78x128px", 78, 128), ("tile_8x1024px", 8, 1024)):
        C = 1
        hr = torch.randint(0, 256, (n, px, px, C), generator=g, dtype=torch.uint8)
        sr = (hr.int() + torch.randint(-6, 7, (n, px, px, C), generator=g, dtype=torch.int32)).clamp(0, 255).to(torch.uint8)
        first = (sr[:1].numpy(), hr[:1].numpy())
        sr, hr = sr.cuda(), hr.cuda()
        npix = n * px * px
        for name, sizes in (("ws 1", [1]), ("ws 11", [11]), ("11,21,31 mean", [11, 21, 31])):
            if len(sizes) == 1:
                err, ssim = (lambda: M.error_maps(sr, hr, sizes[0])), (lambda: M.anomaly_maps(sr, hr, sizes[0]))
            else:
                err, ssim = (lambda: M.error_maps_multi(sr, hr, sizes, "mean")), (lambda: M.anomaly_maps_multi(sr, hr, sizes, "mean"))
            exact = np.array_equal(err()[:1].cpu().numpy(), definition(*first, sizes))      # also the warm-up of both paths
            ssim()
            torch.cuda.synchronize()
            te, ts = [], []
            for _ in range(args.rounds):
                te.append(timed(err, args.reps))
                ts.append(timed(ssim, args.reps))
            me, ms = statistics.median(te), statistics.median(ts)
            # bytes per pixel: the two u8 reads and the store; on the table path also 8 B of row pass, 32 B of column pass (two
            # launches: these images have more than 32 rows) and 8 B of corners per size
            per_px = 2 * C + 4 if sizes == [1] else 2 * C + 8 + 32 + 8 * len(sizes) + 4
            floor_ms = npix * per_px / (args.tbps * 1e12) * 1e3
            print(f"{tag} {name}: error maps {me:.4f} ms [{min(te):.4f} .. {max(te):.4f}]  SSIM maps {ms:.4f} ms "
                  f"[{min(ts):.4f} .. {max(ts):.4f}]  SSIM / error {ms / me:.2f}  {per_px} B/pixel = {floor_ms:.4f} ms at "
                  f"{args.tbps:g} TB/s ({floor_ms / me:.2f} of what the bytes allow)  equals the definition {exact}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tbps", type=float, default=6.3, help="the HBM rate the byte counts are set against, TB/s (MI355X: 8 peak, 6.3 for a copy)")
    bench(ap.parse_args())
