"""Weight-EMA cost (tools only; DESIGN.md "Weight EMA").  With the library's event profiler (``srad_prof_*``): the device time
of ``srad_adam_ema_step`` against ``srad_adam_step`` on flat buffers of DRCT-L's parameter count (the 12-RDG 128 px preset),
and, with device events around the calls, both against the two-launch alternative - ``srad_adam_step`` followed by a torch
``mul_`` / ``add_`` pair on the average.  The byte model (36 against 28 bytes per element) is printed beside the measured
ratio: an expectation, not a pass mark.  Then one graphed training step of that preset (``GraphedTrainStep``) with and
without the average.  --reps N timed calls after warm-up; --skip-train leaves the training steps out."""
import argparse
import json
import os
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


def prof_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    L.prof_enable(True)
    L.prof_collect()
    for _ in range(reps):
        fn()
    prof = L.prof_collect()
    L.prof_enable(False)
    return prof["optim"]["ms"] / reps, prof["optim"]["bytes"] / reps


ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--dtype", default="bf16", choices=["fp32", "bf16"])
ap.add_argument("--decay", type=float, default=0.999)
ap.add_argument("--skip-train", action="store_true")
args = ap.parse_args()

n, d = N_DRCT_L, args.decay
g = torch.Generator().manual_seed(1)
p, grad, m, ema = (torch.randn(n, generator=g).cuda() for _ in range(4))
v = (torch.rand(n, generator=g) * 1e-2).cuda()
lib, s = L.lib(), L.current_stream_ptr()
count = [0]


def plain():
    count[0] += 1
    L.check(lib.srad_adam_step(L.dptr(p), L.dptr(grad), L.dptr(m), L.dptr(v), n, 1e-4, 0.9, 0.999, 1e-8, 0.0, count[0], 1.0, s), "adam_step")


def fused():
    count[0] += 1
    L.check(lib.srad_adam_ema_step(L.dptr(p), L.dptr(grad), L.dptr(m), L.dptr(v), L.dptr(ema), n, 1e-4, 0.9, 0.999, 1e-8, 0.0, count[0],
                                   1.0, d, s), "adam_ema_step")


def two_launch():
    plain()
    ema.mul_(d).add_(p, alpha=1.0 - d)


plain_ms, plain_bytes = prof_ms(plain, args.reps)
fused_ms, fused_bytes = prof_ms(fused, args.reps)
out = dict(n=n, reps=args.reps, decay=d,
           adam_step_ms=plain_ms, adam_step_gbps=plain_bytes / plain_ms / 1e6,
           adam_ema_step_ms=fused_ms, adam_ema_step_gbps=fused_bytes / fused_ms / 1e6,
           fused_over_plain=fused_ms / plain_ms, byte_model_fused_over_plain=36.0 / 28.0,
           wall_adam_step_ms=wall_ms(plain, args.reps), wall_adam_ema_step_ms=wall_ms(fused, args.reps),
           wall_adam_step_then_mul_add_ms=wall_ms(two_launch, args.reps), byte_model_two_launch_over_plain=(28.0 + 12.0 + 12.0) / 28.0)
print(json.dumps(out), flush=True)
del p, grad, m, v, ema

if not args.skip_train:
    opt = Opt.build_opt('drct', 'grid', 128, 4, dtype=args.dtype)
    x = (torch.rand(args.batch, 1, 32, 32, generator=g) * 255).cuda()
    hr = (torch.rand(args.batch, 1, 128, 128, generator=g) * 255).cuda()
    steps = {}
    for label, kw in (("plain", {}), ("ema", dict(ema_decay=d))):
        torch.manual_seed(1)
        net = DRCT(opt).cuda().train()
        step = GraphedTrainStep(net, FusedAdam(net, lr=1e-4, **kw), warmup=2)
        for _ in range(3):                                   # two eager warm-up steps, then the capture
            step(x, hr)
        assert step._graphs, "the step was not captured"
        steps[label] = wall_ms(lambda: step(x, hr), args.reps)
        del net, step
    print(json.dumps(dict(preset="DRCT 12 RDG, 128 px, x4", dtype=args.dtype, batch=args.batch, reps=args.reps,
                          graphed_step_ms=steps["plain"], graphed_step_ema_ms=steps["ema"],
                          ema_over_plain=steps["ema"] / steps["plain"])), flush=True)
