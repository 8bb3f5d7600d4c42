"""Map-baseline timing (tools only): device-event ms per call of ``map_stats_accumulate``, ``normalize_maps`` (without and
with the per-image maximum) and ``normalize_maps_loo`` and, in the same process as the yardstick, of ``smooth_maps`` at radius 0
with the maximum - a copy through the same maximum machinery - at the MVTec grid test split (78 x 128 px) and 8 x 1024 px maps.
The five alternate round by round after a warm-up of all; each case is set against what its bytes allow at --tbps (HBM, TB/s):
accumulate reads 4 B per map pixel and moves 32 B per plane pixel of sums, apply moves 8 B per map pixel plus 8 B of planes
per plane pixel, leave-one-out 8 B plus 16 B of sums, the copy 8 B.  --processes P runs the measurement in P fresh processes,
one after the other, and prints the median of their medians; --rounds N rounds of --reps calls each."""
import argparse
import json
import os
import statistics
import subprocess
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = (("grid_78x128px", 78, 128), ("tile_8x1024px", 8, 1024))
KERNELS = ("accumulate", "apply", "apply+max", "leave-one-out", "copy+max (smooth_maps r=0)")


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(args):
    """{case: {kernel: median ms}} in this process."""
    import torch
    from importlib import import_module
    M = import_module("anomaly-detection-super-resolution_amd.metrics")
    g = torch.Generator().manual_seed(5)
    out = {}
    for tag, n, px in CASES:
        maps = (0.05 + 0.5 * torch.rand(n, px, px, generator=g)).cuda()
        s1, s2 = M.map_stats_accumulate(maps)
        mean = s1 / n
        sd = ((s2 - s1 * s1 / n).clamp_min(0) / (n - 1)).sqrt().clamp_min(1e-3)
        mu, inv, floor = mean.float(), (1.0 / sd).float(), 1e-3
        dst = torch.empty_like(maps)
        a1, a2 = torch.zeros_like(s1), torch.zeros_like(s2)
        fns = (lambda: M.map_stats_accumulate(maps, a1, a2), lambda: M.normalize_maps(maps, mu, inv, out=dst),
               lambda: M.normalize_maps(maps, mu, inv, with_max=True, out=dst), lambda: M.normalize_maps_loo(maps, s1, s2, n, floor, with_max=True),
               lambda: M.smooth_maps(maps, 0.0, with_max=True))
        for fn in fns:                                        # warm-up of every path
            fn()
        torch.cuda.synchronize()
        t = [[] for _ in fns]
        for _ in range(args.rounds):
            for k, fn in enumerate(fns):
                t[k].append(timed(fn, args.reps))
        out[tag] = {name: statistics.median(v) for name, v in zip(KERNELS, t)}
    return out


def report(args, runs):
    for tag, n, px in CASES:
        npix, plane = n * px * px, px * px
        bytes_of = {"accumulate": 4 * npix + 32 * plane, "apply": 8 * npix + 8 * plane, "apply+max": 8 * npix + 8 * plane,
                    "leave-one-out": 8 * npix + 16 * plane, KERNELS[4]: 8 * npix}
        for name in KERNELS:
            ms = [r[tag][name] for r in runs]
            med = statistics.median(ms)
            floor_ms = bytes_of[name] / (args.tbps * 1e12) * 1e3
            print(f"{tag} {name}: {med:.4f} ms [{min(ms):.4f} .. {max(ms):.4f} over {len(ms)} processes]  "
                  f"{bytes_of[name] / 1e6:.2f} MB = {floor_ms:.4f} ms at {args.tbps:g} TB/s ({floor_ms / med:.2f} of what the bytes allow)", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--processes", type=int, default=3, help="fresh processes the measurement is repeated in")
    ap.add_argument("--tbps", type=float, default=6.3, help="the HBM rate the byte counts are set against, TB/s (MI355X: 8 peak, 6.3 for a copy)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a)))
    else:
        runs = []
        for _ in range(max(1, a.processes)):                  # one at a time: a fresh process each, never two on the GPU at once
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--rounds", str(a.rounds)],
                               check=True, capture_output=True, text=True, timeout=300)
            runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        report(a, runs)
