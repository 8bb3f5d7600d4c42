"""Float32 resize timing (tools only): ``ops.resize_f32`` (bilinear, both launches of ``srad_resize_f32``) next to
``torch.nn.functional.interpolate(mode='bilinear')`` on the same device tensors, for the map resizes of a predict stream -
16 maps of 128 x 128 to 1024 x 1024 and to 700 x 900, and 16 of 32 x 32 to 80 x 96.  interpolate is fp32 arithmetic with other
weights and does not equal Pillow; it is here as the time a framework call takes for the same bytes.  Device events around
``--reps`` calls, the two alternating over ``--rounds`` rounds after a warm-up of each; medians.  Every run also asserts
equality with Pillow's mode-F resize on the first map.  One JSON line per case.  --peak-tbs: the HBM peak the share refers to."""
import argparse
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image
from srad_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--peak-tbs", type=float, default=8.0)
args = ap.parse_args()


def timed(fn):
    """ms per call: device events around ``args.reps`` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / args.reps


for (H, W), (h, w) in (((128, 128), (1024, 1024)), ((128, 128), (700, 900)), ((32, 32), (80, 96))):
    x = np.random.RandomState(1).uniform(0, 1, (args.batch, H, W)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    out = torch.empty(args.batch, h, w, dtype=torch.float32, device="cuda")
    tmp = torch.empty(args.batch, H, w, dtype=torch.float32, device="cuda")
    ours = lambda: ops.resize_f32(xd, (h, w), "bilinear", out=out, tmp=tmp)
    x4 = xd[:, None]
    theirs = lambda: F.interpolate(x4, size=(h, w), mode="bilinear", align_corners=False)
    ours(), theirs()                                         # warm-up: tables built and uploaded, code objects loaded
    timed(ours), timed(theirs)
    ref = np.asarray(Image.fromarray(x[0]).resize((w, h), Image.BILINEAR))
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), ref.view(np.uint32)), "the device resize differs from Pillow"
    t_ours, t_theirs = [], []
    for _ in range(args.rounds):
        t_ours.append(timed(ours))
        t_theirs.append(timed(theirs))
    nbytes = 4.0 * args.batch * (H * W + 2 * H * w + h * w)  # source read, intermediate written and read, result written
    ms = float(np.median(t_ours))
    print(json.dumps(dict(batch=args.batch, src=[H, W], dst=[h, w], reps=args.reps, rounds=args.rounds, resize_f32_ms=ms,
                          resize_f32_ms_min=float(min(t_ours)), resize_f32_ms_max=float(max(t_ours)),
                          interpolate_ms=float(np.median(t_theirs)), interpolate_ms_min=float(min(t_theirs)),
                          interpolate_ms_max=float(max(t_theirs)), bytes=nbytes, gb_per_s=nbytes / ms / 1e6,
                          hbm_peak_share=nbytes / ms / 1e9 / args.peak_tbs)), flush=True)
