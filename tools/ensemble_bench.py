"""Self-ensemble timing (tools only): with the library's event profiler (``srad_prof_*``), the device time of the two ensemble
launches (``srad_ensemble_inputs`` on [B,1,32,32], ``srad_ensemble_mean`` on the [8B,1,128,128] output) next to every other
launch of ``Model.forward_x8`` - the stacked DRCT forward of the 128 px / x4 preset (12 RDG, window 8) - at B = 8, per
precision; and the wall time (device events) of ``forward_x8`` against one plain forward of the same B images.  Weights are
the random initialisation: the times do not depend on them.  --reps N profiled calls after one warm-up call."""
import argparse
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from srad_amd import _lib as L
from srad_amd import options as Opt
from srad_amd.model import Model


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
ap.add_argument("--batch", type=int, default=8)
args = ap.parse_args()
for dtype in ("bf16x3", "fp32"):
    opt = Opt.build_opt('drct', 'grid', 128, 4, dtype=dtype)
    opt.use_graph = False                                    # the profiler does not record launches inside a captured graph
    m = Model(opt, None).eval()
    x = (torch.rand(args.batch, 1, 32, 32, generator=torch.Generator().manual_seed(1)) * 255).cuda()
    with torch.no_grad():
        m.forward_x8(x)                                      # warm-up: weights packed, workspaces allocated
        torch.cuda.synchronize()
        L.prof_enable(True)
        L.prof_collect()
        for _ in range(args.reps):
            m.forward_x8(x)
        prof = L.prof_collect()
        L.prof_enable(False)
        ens = prof.pop("ensemble")
        rest_ms = sum(v["ms"] for v in prof.values()) / args.reps
        out = dict(dtype=dtype, batch=args.batch, lr=32, hr=128, reps=args.reps,
                   ensemble_launches_per_call=ens["launches"] / args.reps, ensemble_ms_per_call=ens["ms"] / args.reps,
                   ensemble_bytes_per_call=ens["bytes"] / args.reps, other_launches_ms_per_call=rest_ms,
                   forward_x8_wall_ms=wall_ms(lambda: m.forward_x8(x), args.reps), plain_forward_wall_ms=wall_ms(lambda: m.model(x), args.reps))
    print(json.dumps(out), flush=True)
