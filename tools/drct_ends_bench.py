"""The DRCT body-end launch on its own (tools only): its device time with HIP events (the library's event
profiler, per kernel class) against the launches it replaces, the packing launches of both forms left out.
The batch-8 row is what the one-round rule of srad_drct_ends_supported was decided on.
    python tools/drct_ends_bench.py [reps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srad_amd import _lib as L, ops  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
E, F, D = 180, 64, 308
WORK = ("layout", "layernorm", "gemm_bn64", "gemm_bn32", "gemm_bn16", "body_end")     # everything but pack_weight


def timed(fn, reps):
    """Microseconds per call of the WORK classes' launches (device time between the events around each launch)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    L.prof_enable(True)
    L.prof_collect()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    prof = L.prof_collect()
    L.prof_enable(False)
    return sum(prof[c]["ms"] for c in WORK if c in prof) * 1e3 / reps


def main():
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    ln_g, ln_b = 1 + 0.1 * r(E), 0.1 * r(E)
    w1, b1, w2, b2 = 0.02 * r(E, E, 3, 3), 0.02 * r(E), 0.02 * r(F, E, 3, 3), 0.02 * r(F)
    for B, H, W in ((4, 32, 32), (8, 32, 32), (1, 8, 8), (1, 64, 64)):
        T = B * H * W
        x, feat0 = r(T, D), r(T, E)
        new = timed(lambda: ops.drct_body_end(x, ln_g, ln_b, w1, b1, feat0, w2, b2, B, H, W), REPS)

        def chain():
            body = ops.layernorm(x[:, :E].contiguous(), ln_g, ln_b)
            c1 = ops.gemm(body, w1, b1, B=B, H=H, W=W, residual=feat0, precision="bf16")
            return ops.gemm(c1, w2, b2, B=B, H=H, W=W, act=L.ACT_LRELU, slope=0.01, precision="bf16")
        old = timed(chain, REPS)
        tiles = B * H * ((W + 15) // 16)
        print(f"{B} x {H} x {W} ({tiles} tiles): body end {new:7.1f} us | LayerNorm + two GEMM convs {old:7.1f} us")


if __name__ == "__main__":
    main()
