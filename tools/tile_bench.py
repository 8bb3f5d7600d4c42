"""Tiled-inference timing (tools only; DESIGN.md "Tiled inference").  Case: 8 images of 256 x 256 LR, tile 32, overlap 8, scale 4.

  kernels  ``srad_tile_gather`` and ``srad_tile_blend`` (both modes) on gray and RGB, device events around ``--reps`` launches,
           each next to the time its bytes take at the copy rate DESIGN.md uses (4.5 TB/s): image read + tiles written for the
           gather, tile outputs read + image written for the blend.
  tiled    ``Model.forward`` of the DRCT-L 128 px preset (12 RDG, window 8, split-bf16) with tile 32 / overlap 8 on the batch.
  whole    the same model's whole-image forward of the same batch - all the parent of this feature can do.

The parent process never touches the GPU: every measurement is a fresh child process, and the rounds alternate the three so
that drift on a shared machine falls on all of them.  It prints one JSON line per child and a last one with the medians and
the share of gather + blend in the tiled forward.  Weights are the random initialisation: the times do not depend on them."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, LR, TILE, OVERLAP, SCALE, GRANULE = 8, 256, 32, 8, 4, 8
COPY_RATE = 4.5e12                                             # bytes / s


def event_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def child_kernels(reps):
    import torch
    from srad_amd import ops
    out = {}
    for name, C in (("gray", 1), ("rgb", 3)):
        x = torch.rand(B, C, LR, LR, generator=torch.Generator().manual_seed(1)).cuda()
        tiles = ops.tile_gather(x, TILE, OVERLAP, GRANULE)
        y = torch.rand(tiles.shape[0], C, TILE * SCALE, TILE * SCALE, generator=torch.Generator().manual_seed(2)).cuda()
        dst = torch.empty(B, C, LR * SCALE, LR * SCALE, device="cuda")
        g_bytes, b_bytes = 4 * (x.numel() + tiles.numel()), 4 * (y.numel() + dst.numel())
        out[name] = dict(tiles=tiles.shape[0], gather_ms=event_ms(lambda: ops.tile_gather(x, TILE, OVERLAP, GRANULE), reps),
                         gather_floor_ms=g_bytes / COPY_RATE * 1e3, blend_floor_ms=b_bytes / COPY_RATE * 1e3,
                         **{f"blend_{m}_ms": event_ms(lambda: ops.tile_blend(y, LR, LR, TILE, OVERLAP, GRANULE, SCALE, m, out=dst), reps)
                            for m in ("mean", "feather")})
    return out


def child_forward(tiled, reps):
    import torch
    from srad_amd import options as Opt
    from srad_amd.model import Model
    opt = Opt.build_opt('drct', 'grid', 128, 4, dtype='bf16x3')
    if tiled:
        opt.tile, opt.tile_overlap = TILE, OVERLAP
    m = Model(opt, None).eval()
    x = (torch.rand(B, 1, LR, LR, generator=torch.Generator().manual_seed(1)) * 255).cuda()
    with torch.no_grad():
        ms = event_ms(lambda: m(x), reps)
    return dict(forward_ms=ms, peak_gb=torch.cuda.max_memory_allocated() / 2 ** 30)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="timed calls per child after one warm-up call (kernels: 20 x as many)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", choices=["kernels", "tiled", "whole"], default=None)
    args = ap.parse_args()
    if args.child:
        res = child_kernels(20 * args.reps) if args.child == "kernels" else child_forward(args.child == "tiled", args.reps)
        print(json.dumps(dict(what=args.child, **res)), flush=True)
        return 0
    runs = {"kernels": [], "tiled": [], "whole": []}
    for r in range(args.rounds):
        order = ["kernels", "tiled", "whole"] if r % 2 == 0 else ["whole", "tiled", "kernels"]
        for what in order:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--reps", str(args.reps)], capture_output=True,
                               text=True, timeout=600)
            if p.returncode != 0:                             # nothing more is started on the GPU after a failure
                sys.stderr.write(p.stdout + p.stderr)
                return p.returncode or 1
            line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
            print(line, flush=True)
            runs[what].append(json.loads(line))
    med = lambda rows, *keys: statistics.median([_dig(r, keys) for r in rows])
    summary = dict(what="summary", rounds=args.rounds, tiled_forward_ms=med(runs["tiled"], "forward_ms"),
                   whole_forward_ms=med(runs["whole"], "forward_ms"), tiled_peak_gb=med(runs["tiled"], "peak_gb"),
                   whole_peak_gb=med(runs["whole"], "peak_gb"))
    for name in ("gray", "rgb"):
        for k in ("gather_ms", "gather_floor_ms", "blend_mean_ms", "blend_feather_ms", "blend_floor_ms"):
            summary[f"{name}_{k}"] = med(runs["kernels"], name, k)
    summary["gather_blend_share_of_tiled_forward"] = (summary["gray_gather_ms"] + summary["gray_blend_mean_ms"]) / summary["tiled_forward_ms"]
    print(json.dumps(summary), flush=True)
    return 0


def _dig(row, keys):
    for k in keys:
        row = row[k]
    return row


if __name__ == "__main__":
    sys.exit(main())
