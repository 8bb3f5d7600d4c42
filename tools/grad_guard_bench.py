"""Guarded-step cost (tools only; DESIGN.md "Guarded step").  One graphed DRCT-L x4 training step at the C4 shape
(8 images of 32 x 32 -> 128 x 128 on one GPU, ``GraphedTrainStep``) in three configurations of one process:
guard off, ``--skip-nonfinite`` (the norm pass and the decision, no clipping) and ``--grad-clip 1``.  Every configuration
is timed --rounds times in turn, --reps replays each between two device events; the median and the spread (min .. max over
the rounds) are printed, so the guard's cost can be read against the run-to-run spread.  Then the device time of the three
guard-side launches on a flat buffer of DRCT-L's parameter count, against the plain step's.
Run it on the parent commit with --only-off for the off / off comparison: that path issues the same launches."""
import argparse
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from srad_amd import _lib as L
from srad_amd import options as Opt
from srad_amd.nets import DRCT
from srad_amd.train import FusedAdam, GraphedTrainStep

N_DRCT_L = 27382021                                          # parameters of the 12-RDG preset (tests/test_abi.py)


def wall_ms(fn, reps):
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
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--dtype", default="bf16", choices=["fp32", "bf16"])
ap.add_argument("--only-off", action="store_true", help="time the unguarded step alone (also runs on a commit without the guard)")
ap.add_argument("--skip-kernels", action="store_true")
args = ap.parse_args()

configs = [("off", {})]
if not args.only_off:
    configs += [("skip_nonfinite", dict(skip_nonfinite=True)), ("grad_clip_1", dict(max_grad_norm=1.0))]
g = torch.Generator().manual_seed(1)
opt = Opt.build_opt('drct', 'grid', 128, 4, dtype=args.dtype)
x = (torch.rand(args.batch, 1, 32, 32, generator=g) * 255).cuda()
hr = (torch.rand(args.batch, 1, 128, 128, generator=g) * 255).cuda()
steps = {}
for label, kw in configs:
    torch.manual_seed(1)
    net = DRCT(opt).cuda().train()
    step = GraphedTrainStep(net, FusedAdam(net, lr=1e-4, **kw), warmup=2)
    for _ in range(3):                                       # two eager warm-up steps, then the capture
        step(x, hr)
    assert step._graphs, "the step was not captured"
    steps[label] = (net, step)
times = {label: [] for label, _ in configs}
for _ in range(args.rounds):                                 # interleaved: drift hits every configuration alike
    for label, _ in configs:
        step = steps[label][1]
        times[label].append(wall_ms(lambda: step(x, hr), args.reps))
out = dict(preset="DRCT 12 RDG, 128 px, x4 (C4 shape)", dtype=args.dtype, batch=args.batch, reps=args.reps, rounds=args.rounds)
for label, _ in configs:
    t = times[label]
    out[label] = dict(median_ms=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4))
    if label != "off":
        out[label]["over_off"] = round(statistics.median(t) / statistics.median(times["off"]), 5)
        out[label]["guard_stats"] = steps[label][1].optimizer.guard_stats()
print(json.dumps(out), flush=True)
del steps

if not (args.skip_kernels or args.only_off):
    from srad_amd.train import GradGuard
    n = N_DRCT_L
    p, grad, m = (torch.randn(n, generator=g).cuda() for _ in range(3))
    v = (torch.rand(n, generator=g) * 1e-2).cuda()
    lib, s = L.lib(), L.current_stream_ptr()
    guard = GradGuard([n], "cuda", (0.9, 0.999), 1.0)
    hyper = torch.tensor([1e-4, 0.0, 0.0, 1.0]).cuda()
    dev_hyper = torch.tensor([1e-4, 0.1, 0.03, 1.0]).cuda()

    def plain():
        L.check(lib.srad_adam_step_dev(L.dptr(p), L.dptr(grad), L.dptr(m), L.dptr(v), n, 0.9, 0.999, 1e-8, 0.0, L.dptr(dev_hyper), s), "adam_step_dev")

    def norm_only():
        guard.run([grad], hyper)

    def guarded():
        guard.run([grad], hyper)
        L.check(lib.srad_adam_guarded_step(L.dptr(p), L.dptr(grad), L.dptr(m), L.dptr(v), n, 0.9, 0.999, 1e-8, 0.0, L.dptr(guard.ws), s),
                "adam_guarded_step")

    reps = 20
    a, b, c = wall_ms(plain, reps), wall_ms(norm_only, reps), wall_ms(guarded, reps)
    print(json.dumps(dict(n=n, reps=reps, adam_step_dev_ms=round(a, 4), norm_and_finalize_ms=round(b, 4),
                          norm_gbps=round(4.0 * n / b / 1e6, 1), guarded_three_launches_ms=round(c, 4),
                          guarded_over_plain=round(c / a, 4), byte_model_guarded_over_plain=32.0 / 28.0)), flush=True)
