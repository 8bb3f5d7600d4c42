"""Every non-diagnostic instance of qkv_attn_kernel, mlp_block_kernel and swin_block_kernel, timed alone: per block shape of
DRCT-L the plain and the query-split grid of qkv_attn, its split-bf16 instance, mlp_block at 16 / 32 / 64 rows per workgroup
and its split-bf16 instances at 16 / 32, and swin_block; shift 0 and 4 where a shift exists.  One line per launch: name,
microseconds per launch (median of 3 x ITERS back-to-back launches).  tools/swin_block_bench.py covers the benched geometry
only; this is the A/B tool for a change that touches the other instances (SRAD_LIB_PATH selects the library).
usage: swin_instances_bench.py [ITERS = 1000] [only: qkv_attn | mlp_block | swin_block ...]"""
import ctypes as C, os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srad_amd import _lib as L
dev = torch.device("cuda:0")
ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
ONLY = sys.argv[2:]
TMAX = 32768
x = torch.randn(TMAX, 320, device=dev); y = torch.empty(TMAX, 320, device=dev)
attn_h = torch.randn(TMAX, 320, device=dev).to(torch.bfloat16)
attn_f = torch.randn(TMAX, 320, device=dev)
w = torch.randn(3 * 320 * 320, device=dev) * 0.05
scratch = torch.empty(32 << 20, dtype=torch.uint8, device=dev); off = (-scratch.data_ptr()) % 256
sp, sb = C.c_void_p(scratch.data_ptr() + off), C.c_size_t(scratch.numel() - off)
lib = L.lib()
SHAPES = [(180, 6, 360, 32), (212, 4, 424, 32), (244, 2, 488, 32), (276, 6, 276, 32), (308, 4, 308, 180)]   # as tools/swin_block_bench.py


def on(kernel):
    return not ONLY or kernel in ONLY


def med(f):
    v = []
    for _ in range(3):
        us = C.c_float()
        L.check(f(us), "bench")
        v.append(us.value)
    return statistics.median(v)


s = torch.cuda.Stream()
with torch.cuda.stream(s):
    st = L.current_stream_ptr()
    for d, heads, m, no in SHAPES:
        for shift in (0, 4):
            # qkv_attn: B = 4 -> the plain grid (query split for 2 heads), B = 2 -> the query split, B = 8 -> plain for 2 heads
            for B in ((4, 2) + ((8,) if heads == 2 else ())) if on("qkv_attn") else ():
                grid = (C.c_int * 2)()
                L.check(lib.srad_qkv_attn_grid(1, B, 32, 32, d, heads, 0, grid), "grid")   # 1 = bf16: what the launch below takes
                kind = "qsplit" if grid[1] == 2 * heads else "plain"
                us = med(lambda u: lib.srad_bench_qkv_attn(L.dptr(x), 320, B, 32, 32, shift, d, heads, L.dptr(w), L.dptr(attn_h), sp, sb, ITERS, C.byref(u), st))
                print(f"qkv_attn d={d} {kind} B={B} shift={shift} {us:.3f}", flush=True)
            if on("qkv_attn"):
                us = med(lambda u: lib.srad_bench_qkv_attn(L.dptr(x), 320, 4, 32, 32, shift | 0x20000, d, heads, L.dptr(w), L.dptr(y), sp, sb, ITERS, C.byref(u), st))
                print(f"qkv_attn d={d} split-bf16 B=4 shift={shift} {us:.3f}", flush=True)
            if on("swin_block"):
                us = med(lambda u: lib.srad_bench_swin_block(L.dptr(x), 4, 32, 32, shift, d, heads, m, no, L.dptr(w), L.dptr(y), sp, sb, ITERS, C.byref(u), st))
                print(f"swin_block d={d} B=4 shift={shift} {us:.3f}", flush=True)
                # the folded second half: bit 17 of the shift argument
                us = med(lambda u: lib.srad_bench_swin_block(L.dptr(x), 4, 32, 32, shift | 0x20000, d, heads, m, no, L.dptr(w), L.dptr(y), sp, sb, ITERS, C.byref(u), st))
                print(f"swin_block d={d} folded B=4 shift={shift} {us:.3f}", flush=True)
        if not on("mlp_block"):
            continue
        for fm, M in ((16, 4096), (32, 8192), (64, 32768)):
            us = med(lambda u: lib.srad_bench_mlp_block(M, d, m, no, L.dptr(attn_h), L.dptr(x), L.dptr(y), L.dptr(w), sp, sb, fm << 8, ITERS, C.byref(u), st))
            print(f"mlp_block d={d} fm={fm} M={M} {us:.3f}", flush=True)
        for fm, M in ((16, 4096), (32, 8192)):
            us = med(lambda u: lib.srad_bench_mlp_block(M, d, m, no, L.dptr(attn_f), L.dptr(x), L.dptr(y), L.dptr(w), sp, sb, (fm << 8) | 0x20000, ITERS, C.byref(u), st))
            print(f"mlp_block d={d} split-bf16 fm={fm} M={M} {us:.3f}", flush=True)
torch.cuda.synchronize()
