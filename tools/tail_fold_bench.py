"""The folded DRCT output end on its own (tools only): the one-time cost of building a fold from its fp32 sources
and the device time of the folded launch, both with HIP events, against the chain of launches it replaces (ops.gemm, bf16).
    python tools/tail_fold_bench.py [reps]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srad_amd import _lib as L, ops  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
F = 64


def timed(fn, reps, cls=None):
    """Microseconds per call: of the library's event-profiler class `cls` (device time between the events around its launches),
    or, without a class, of everything between two events on the stream (Python's launch overhead included)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    if cls is not None:
        L.prof_enable(True)
        L.prof_collect()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        prof = L.prof_collect()
        L.prof_enable(False)
        return prof[cls]["ms"] * 1e3 / reps
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    for scale, C in ((4, 1), (4, 3), (2, 1), (2, 3)):
        ups = [(torch.randn(4 * F, F, 3, 3, generator=g).mul_(0.04).to(dev), torch.randn(4 * F, generator=g).mul_(0.04).to(dev))
               for _ in range(1 if scale == 2 else 2)]
        lw, lb = torch.randn(C, F, 3, 3, generator=g).mul_(0.04).to(dev), torch.randn(C, generator=g).mul_(0.04).to(dev)
        upw, upb = [w for w, _ in ups], [b for _, b in ups]
        build_us = timed(lambda: ops.tail_fold_build(upw, upb, lw, lb), 10, "pack_weight")
        print(f"x{scale} C={C}: fold build (four launches, events around them) {build_us:9.1f} us")
        fold = ops.tail_fold_build(upw, upb, lw, lb)
        for B, H, W in ((4, 32, 32), (8, 32, 32), (1, 256, 256)):
            c2 = torch.randn(B * H * W, F, generator=g).to(dev)
            fold_us = timed(lambda: ops.tail_fold(c2, upw, upb, lw, lb, B, H, W, fold=fold), REPS, "tail_fold")

            def chain():
                t, h, w = c2, H, W
                for uw, ub in ups:
                    t = ops.gemm(t, uw, ub, B=B, H=h, W=w, pixel_shuffle=True, precision="bf16")
                    h, w = 2 * h, 2 * w
                return ops.gemm(t, lw, lb, B=B, H=h, W=w, precision="bf16")
            chain_us = timed(chain, max(3, REPS // 5))
            print(f"    {B} x {H} x {W}: folded launch {fold_us:8.1f} us (events around it) | chain through ops.gemm, packing its weights per call, stream time {chain_us:9.1f} us")


if __name__ == "__main__":
    main()
