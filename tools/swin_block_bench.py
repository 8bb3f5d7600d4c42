"""The one-launch Swin block (swin_block_kernel) against the pair it replaces (qkv_attn + mlp_block<16>), per block shape of
DRCT-L at the benched geometry (B = 4, 32 x 32), shift 0 and 4: back-to-back launches, microseconds per launch, median of 3.
A shape goes into the engine's table (srad_swin_block_wins) only if  block < qkv_attn + mlp_block + BOUNDARY.
Each line ends with the folded second half against the unfolded block, three alternating runs of each."""
import ctypes as C, os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srad_amd import _lib as L
BOUNDARY = 1.45            # us between two dependent launches in a replayed graph
dev = torch.device("cuda:0")
B, H, W = 4, 32, 32
T = B * H * W
x = torch.randn(T, 320, device=dev); y = torch.empty(T, 320, device=dev)
attn = torch.randn(T, 320, device=dev).to(torch.bfloat16)
w = torch.randn(3 * 320 * 320, device=dev) * 0.05        # every weight of a block is cut from here; the largest is qkv.weight [3 d][d]
scratch = torch.empty(16 << 20, dtype=torch.uint8, device=dev); off = (-scratch.data_ptr()) % 256
sp, sb = C.c_void_p(scratch.data_ptr() + off), C.c_size_t(scratch.numel() - off)
lib = L.lib()
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
only = [int(v) for v in sys.argv[2:]]                     # block dims to run (default: all five)
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    for d, heads, m, no in [(180, 6, 360, 32), (212, 4, 424, 32), (244, 2, 488, 32), (276, 6, 276, 32), (308, 4, 308, 180)]:
        if only and d not in only:
            continue
        for shift in (0, 4):
            def med(f):
                v = []
                for _ in range(3):
                    us = C.c_float()
                    L.check(f(us), "bench")
                    v.append(us.value)
                return statistics.median(v)
            qa = med(lambda us: lib.srad_bench_qkv_attn(L.dptr(x), 320, B, H, W, shift, d, heads, L.dptr(w), L.dptr(attn), sp, sb, iters, C.byref(us),
                                                        L.current_stream_ptr()))
            mb = med(lambda us: lib.srad_bench_mlp_block(T, d, m, no, L.dptr(attn), L.dptr(x), L.dptr(y), L.dptr(w), sp, sb, 16 << 8, iters, C.byref(us),
                                                         L.current_stream_ptr()))
            sbk = med(lambda us: lib.srad_bench_swin_block(L.dptr(x), B, H, W, shift, d, heads, m, no, L.dptr(w), L.dptr(y), sp, sb, iters, C.byref(us),
                                                          L.current_stream_ptr()))
            # the folded second half (bit 17 of the shift argument): the three runs of each form alternate, and the
            # folded form counts as faster when its median is below the unfolded minimum
            runs = {False: [], True: []}
            for _ in range(3):
                for folded in (False, True):
                    us = C.c_float()
                    L.check(lib.srad_bench_swin_block(L.dptr(x), B, H, W, shift | (0x20000 if folded else 0), d, heads, m, no, L.dptr(w), L.dptr(y),
                                                      sp, sb, iters, C.byref(us), L.current_stream_ptr()), "bench")
                    runs[folded].append(us.value)
            fmed, umin = statistics.median(runs[True]), min(runs[False])
            pair = qa + mb + BOUNDARY
            print(f"d={d} heads={heads} m={m} no={no} shift={shift}: qkv_attn {qa:6.2f} + mlp_block {mb:6.2f} + {BOUNDARY} = {pair:6.2f} us | "
                  f"swin_block {sbk:6.2f} us | {'WIN' if sbk < pair else 'loss'} ({pair - sbk:+.2f}) | folded "
                  f"{' '.join(f'{v:6.2f}' for v in runs[True])} vs unfolded {' '.join(f'{v:6.2f}' for v in runs[False])} us: "
                  f"{'FASTER' if fmed < umin else 'not faster'} ({umin - fmed:+.2f})", flush=True)
torch.cuda.synchronize()
