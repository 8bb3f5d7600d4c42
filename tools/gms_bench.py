"""Gradient-magnitude similarity timing (tools only; DESIGN.md "Gradient-magnitude maps and loss"), by the protocol of
tools/error_map_bench.py: device events around --reps calls, the candidates of one comparison alternating round by round after
a warm-up of all of them, the median of --rounds rounds - and then the median over --processes fresh processes, one at a time
(this process only starts them and never opens the GPU itself).

  maps   ``gms_maps`` at levels 1 and 4 on the MVTec grid test split (78 x 128 px) and on 8 x 1024 px tiles, gray, with
         ``anomaly_maps`` and ``error_maps`` at ws 11 on the same stacks as the yardsticks (unchanged code), each set against
         what its bytes allow at --tbps: 2 C read and 4 written per pixel, and at 4 levels 16 B per coarse cell written and
         read back (21/64 of a cell per pixel: 10.5 B)
  loss   forward + backward of the kinds GMS and MSGMS at (8, 1, 128, 128) and (4, 3, 256, 256), the existing SSIM kind at
         the same shapes as the yardstick
  step   the eager DRCT training step (--step-rdg groups, 8 images of 32 -> 128 px) with 0.8*L1+0.2*MSGMS against the same
         step with 0.8*L1+0.2*MSE: what the term costs a step

One JSON line per process (--child), then one line of medians over the processes."""
import argparse
import json
import os
import statistics
import subprocess
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(fns, args):
    """{name: median ms} of the callables, alternating round by round after one warm-up call of each."""
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, args.reps))
    return {k: statistics.median(v) for k, v in times.items()}


def child(args):
    import torch
    from srad_amd import loss as Lo
    from srad_amd import metrics as M
    out = {}
    g = torch.Generator().manual_seed(5)
    for tag, n, px in (("grid_78x128px", 78, 128), ("tile_8x1024px", 8, 1024)):
        hr = torch.randint(0, 256, (n, px, px, 1), generator=g, dtype=torch.uint8)
        sr = (hr.int() + torch.randint(-6, 7, (n, px, px, 1), generator=g, dtype=torch.int32)).clamp(0, 255).to(torch.uint8)
        sr, hr = sr.cuda(), hr.cuda()
        ms = alternate(dict(gms=lambda: M.gms_maps(sr, hr, 1), msgms=lambda: M.gms_maps(sr, hr, 4),
                            ssim_ws11=lambda: M.anomaly_maps(sr, hr, 11), mse_ws11=lambda: M.error_maps(sr, hr, 11)), args)
        for k, v in ms.items():
            out[f"maps/{tag}/{k}_ms"] = v
        npix = n * px * px
        for k, per_px in (("gms", 6.0), ("msgms", 16.5)):
            out[f"maps/{tag}/{k}_share_of_bytes"] = npix * per_px / (args.tbps * 1e12) * 1e3 / ms[k]
    for shape in ((8, 1, 128, 128), (4, 3, 256, 256)):
        hr = torch.rand(shape, generator=g) * 255
        sr = (hr + torch.randn(shape, generator=g) * 12).cuda()
        hr = hr.cuda()
        dsr = torch.empty_like(sr)

        def fb(kind):
            k = Lo.KINDS[kind]

            def run():
                out2, saved = Lo.loss_forward(k, sr, hr, 255.0, shape[0])
                Lo.loss_backward(k, saved, out2, 255.0, shape[0], 1.0, into=dsr)
            return run
        ms = alternate({k: fb(k) for k in ("GMS", "MSGMS", "SSIM")}, args)
        for k, v in ms.items():
            out[f"loss/{'x'.join(map(str, shape))}/{k}_fwd_bwd_ms"] = v
    if args.step_rdg > 0:
        from srad_amd import options as Opt
        from srad_amd.nets import DRCT
        from srad_amd.train import FusedAdam, train_step
        opt = Opt.build_opt('drct', 'grid', 128, 4, dtype='fp32')
        opt.depths, opt.num_heads = (6,) * args.step_rdg, (6,) * args.step_rdg
        x = (torch.rand(8, 1, 32, 32, generator=g) * 255).cuda()
        hr = (torch.rand(8, 1, 128, 128, generator=g) * 255).cuda()
        steps = {}
        for spec in ("0.8*L1+0.2*MSGMS", "0.8*L1+0.2*MSE"):
            torch.manual_seed(1)
            net = DRCT(opt).cuda().train()
            net.enable_training()
            adam = FusedAdam(net, lr=1e-4)
            opt.loss = spec
            lf = Lo.Loss(opt)
            lf.start_log()
            steps[spec] = (lambda net=net, adam=adam, lf=lf: train_step(net, x, hr, adam, None, lf))
        ms = alternate(steps, args)
        for k, v in ms.items():
            out[f"step/drct_{args.step_rdg}rdg_8x32px/{k}_ms"] = v
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--tbps", type=float, default=6.3, help="the HBM rate the byte counts are set against, TB/s (MI355X: 8 peak, 6.3 for a copy)")
    ap.add_argument("--step-rdg", type=int, default=12, help="residual groups of the DRCT of the step comparison; 0 leaves it out")
    ap.add_argument("--child", action="store_true", help="measure in this process and print one JSON line")
    args = ap.parse_args()
    if args.child:
        child(args)
        sys.exit(0)
    runs = []
    for _ in range(args.processes):                           # one process at a time
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--rounds", str(args.rounds),
               "--tbps", str(args.tbps), "--step-rdg", str(args.step_rdg)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit(f"a measuring process failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        runs.append(json.loads(line))
    med = {k: round(statistics.median(r[k] for r in runs), 5) for k in runs[0]}
    print(json.dumps(dict(median_of_processes=len(runs), **med)), flush=True)
