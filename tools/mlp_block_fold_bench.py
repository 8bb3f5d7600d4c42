"""mlp_block with fc2 folded into the adjust conv against the chain, per block shape of DRCT-L and per tile
height a launch picks: 16 rows at 4096 tokens (the headline step's swin5: the height at which the engine folds), 32 at 8192
(batches of 8 at 32 x 32), 64 at 65536 (the 1024 px tile).  Back-to-back launches, microseconds per launch, three alternating runs of each form; the folded form
counts as faster when its median is below the chain's minimum.

    python tools/mlp_block_fold_bench.py [launches per run] [block dims ...]
"""
import ctypes as C, os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srad_amd import _lib as L
FOLD = 0x40000                                               # bit 18 of srad_bench_mlp_block's dbg word: the folded form
dev = torch.device("cuda:0")
TMAX = 65536
x = torch.randn(TMAX, 320, device=dev); y = torch.empty(TMAX, 320, device=dev)
attn = torch.randn(TMAX, 320, device=dev).to(torch.bfloat16)
w = torch.randn(3 * 320 * 320, device=dev) * 0.05            # every weight of a block is cut from here
scratch = torch.empty(16 << 20, dtype=torch.uint8, device=dev); off = (-scratch.data_ptr()) % 256
sp, sb = C.c_void_p(scratch.data_ptr() + off), C.c_size_t(scratch.numel() - off)
lib = L.lib()
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
only = [int(v) for v in sys.argv[2:]]
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    for d, heads, m, no in [(180, 6, 360, 32), (212, 4, 424, 32), (244, 2, 488, 32), (276, 6, 276, 32), (308, 4, 308, 180)]:
        if only and d not in only:
            continue
        for fm, T in ((16, 4096), (32, 8192), (64, 65536)):
            if not lib.srad_mlp_block_fold_supported(L.PREC_BF16, T, d, m, no):
                print(f"d={d} m={m} no={no} fm={fm} T={T}: no folded instance (the launch keeps the chain)", flush=True)
                continue
            n = max(iters * 4096 // T, 20)
            runs = {False: [], True: []}
            for _ in range(3):
                for folded in (False, True):
                    us = C.c_float()
                    L.check(lib.srad_bench_mlp_block(T, d, m, no, L.dptr(attn), L.dptr(x), L.dptr(y), L.dptr(w), sp, sb, (fm << 8) | (FOLD if folded else 0),
                                                     n, C.byref(us), L.current_stream_ptr()), "bench")
                    runs[folded].append(us.value)
            fmed, umin = statistics.median(runs[True]), min(runs[False])
            print(f"d={d} m={m} no={no} fm={fm} T={T} ({n} launches): folded {' '.join(f'{v:8.2f}' for v in runs[True])} vs chain "
                  f"{' '.join(f'{v:8.2f}' for v in runs[False])} us: {'FASTER' if fmed < umin else 'not faster'} ({umin - fmed:+.2f})", flush=True)
torch.cuda.synchronize()
