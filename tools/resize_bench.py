"""Device resize timing (tools only): with the library's event profiler (``srad_prof_*``), the device time of ``srad_resize_u8``
(both launches inside one profiled scope) for the two LANCZOS resizes of a predict stream - 16 x 1024^2 x 3 -> 128^2 and
16 x 128^2 x 3 -> 32^2 - next to PIL.Image.resize on the host for the same images (one core), the bytes moved (source read
once, the u8 intermediate written and read, the result written) and the share of the HBM peak they amount to.  One JSON line
per case.  --reps N profiled calls after one warm-up call; --peak-tbs: the HBM peak in TB/s the share refers to."""
import argparse
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image
from srad_amd import _lib as L
from srad_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--peak-tbs", type=float, default=8.0)
args = ap.parse_args()
for src, dst in ((1024, 128), (128, 32)):
    x = np.random.RandomState(1).randint(0, 256, (args.batch, src, src, 3)).astype(np.uint8)
    xd = torch.from_numpy(x).cuda()
    out = torch.empty(args.batch, dst, dst, 3, dtype=torch.uint8, device="cuda")
    tmp = torch.empty(args.batch, src, dst, 3, dtype=torch.uint8, device="cuda")
    ops.resize_u8(xd, (dst, dst), out=out, tmp=tmp)          # warm-up: the tables are built and uploaded
    torch.cuda.synchronize()
    L.prof_enable(True)
    L.prof_collect()
    ms = []
    for _ in range(args.reps):
        ops.resize_u8(xd, (dst, dst), out=out, tmp=tmp)
        ms.append(L.prof_collect()["resize"])
    L.prof_enable(False)
    dev_ms = float(np.median([m["ms"] for m in ms]))
    imgs = [Image.fromarray(a) for a in x]
    t0 = time.perf_counter()
    ref = [np.asarray(im.resize((dst, dst), Image.LANCZOS)) for im in imgs]
    pil_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(out.cpu().numpy(), np.stack(ref)), "the device resize differs from PIL"
    nbytes = ms[0]["bytes"]
    print(json.dumps(dict(batch=args.batch, src=src, dst=dst, channels=3, reps=args.reps, device_ms=dev_ms,
                          device_ms_min=float(min(m["ms"] for m in ms)), pil_host_ms=pil_ms, pil_host_ms_per_image=pil_ms / args.batch,
                          bytes=nbytes, gb_per_s=nbytes / dev_ms / 1e6, hbm_peak_share=nbytes / dev_ms / 1e9 / args.peak_tbs)),
          flush=True)
