"""Writes tests/golden/eval_stage.json: what ``evaluate.evaluate_on_test`` returns and prints, case by case, at world 1 on the
CPU - the returned dictionary with its key order, the printed lines, and what it asked to be saved.  The kernels behind it are
replaced by the CPU stand-ins of tests/helpers.py and the ones below; they need not be right, only deterministic and the same
for the recording and for tests/test_eval_stage_golden.py, which recomputes every case and requires equality.  The recording
is what an earlier evaluator gave, so it is made on a checkout of the commit BEFORE a change to the evaluator (this file and
tests/helpers.py copied in) and never from the code under test:

    python tests/golden/make_eval_stage_golden.py

Everything goes through the public signature of ``evaluate_on_test``, so the script runs unchanged on either side."""
import contextlib
import io
import itertools
import json
import math
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "eval_stage.json")

from tests import helpers as T  # noqa: E402

NAMES = [f"im{i}" for i in range(5)]            # two fewer than images: the last two are named by their index
CALIB = (0, 1, 2, 7)                            # the images that stand for the defect-free validation split


def masks_all():
    """A mask for every image: zeros for the good ones, two rectangles (one at the border) for each bad one."""
    out = []
    for i in range(T.N_IMG):
        m = np.zeros((T.HW, T.HW), np.uint8)
        if T.Y_TRUE[i]:
            m[2 + i:6 + i, 3:3 + i] = 1
            m[T.HW - 3:, T.HW - 2 - i:] = 1
        out.append(m)
    return out


def _pairs(idx):
    """(LR, HR) u8 pairs whose LR pixel carries the image index for the ``super_resolve_u8`` stand-in."""
    return [(np.full((T.HW // 4, T.HW // 4, 1), i, np.uint8), np.zeros((T.HW, T.HW, 1), np.uint8)) for i in idx]


def _super_resolve_u8(model, lr_u8, hr_u8, rgb_range, batch=0):
    return T.stage_images([int(lr.flat[0]) for lr in lr_u8])


def _score_pairs(sr, hr, sizes):
    """A float64 score table from integer sums.  At window size 3 the first bad image looks better than the good ones, so the
    sweep's best size is a later one; one good image has a poor PSNR, so the three AUCs differ."""
    import torch
    d = (sr.long() - hr.long()).reshape(sr.shape[0], -1)
    n = d.shape[1]
    mse = [int(v) / (n * 65025.0) for v in (d * d).sum(1).tolist()]
    l1 = [int(v) / (n * 255.0) for v in d.abs().sum(1).tolist()]
    ssim = [[1.0 - a * (1.0 + 3.0 / ws) + (a if ws == 3 and a == l1[3] else 0.0) for ws in sizes] for a in l1]
    psnr = [-10.0 * math.log10(m) - (20.0 if m == mse[2] else 0.0) for m in mse]
    return (torch.tensor(ssim, dtype=torch.float64), torch.tensor(mse, dtype=torch.float64), torch.tensor(psnr, dtype=torch.float64))


def _pixel_roc_auc(scores, labels):
    from srad_amd import metrics as M
    return M.roc_auc((labels.reshape(-1) != 0).int().numpy(), scores.reshape(-1).double().numpy())


def _aupro(scores, masks, fpr_limit=0.3):
    s, m = scores.double().reshape(-1).tolist(), (masks.reshape(-1) != 0).tolist()
    inside = math.fsum(v for v, d in zip(s, m) if d) / max(1, sum(m))
    return inside / (inside + math.fsum(s) / len(s) + float(fpr_limit))


def _map_threshold(values, rate):
    from srad_amd import metrics as M
    v = np.sort(values.numpy().ravel())
    t = float(v[M.rank_for_rate(len(v), rate)])
    return t, int((v > t).sum()) / len(v)


def _operating_point(maps, threshold, masks=None, min_area=1):
    """A compare and counts; ``min_area`` drops an image's whole prediction when it has fewer pixels than that."""
    import torch
    pred = (maps.double() > float(threshold))
    pred = pred & (pred.sum((1, 2), keepdim=True) >= int(min_area))
    truth = torch.zeros_like(pred) if masks is None else masks != 0
    tp, fp, fn = int((pred & truth).sum()), int((pred & ~truth).sum()), int((~pred & truth).sum())
    regions = int(truth.any(2).any(1).sum())
    num = (tp << 64) // max(1, tp + fn) * regions
    counts = dict(tp=tp, fp=fp, fn=fn, tn=pred.numel() - tp - fp - fn, n_nan=0, n_regions=regions, pro_hi=num >> 64,
                  pro_lo=num & ((1 << 64) - 1))
    return pred.to(torch.uint8), pred.sum((1, 2)).to(torch.int32), counts


def cases():
    """name -> keyword arguments of ``evaluate_on_test`` (``masks``: 'all', 'one_missing' or None)."""
    out = {}
    on = dict(save_maps=True, map_image_score=True, pixel_metrics=True, aupro=True)
    for a, b, c, p in itertools.product((False, True), repeat=4):
        out[f"flags_{int(a)}{int(b)}{int(c)}{int(p)}"] = dict(save_maps=a, map_image_score=b, pixel_metrics=c, aupro=p, masks="all")
    windows = dict(ws0=dict(map_ws=0), ws3=dict(map_ws=3), scales_mean=dict(map_scales=[3, 7], map_reduce="mean"),
                   scales_max=dict(map_scales=[7, 3, 3], map_reduce="max"), sweep=dict(map_scales="sweep"))
    for source, (w, kw) in itertools.product(("ssim", "mse"), windows.items()):
        out[f"{source}_{w}"] = dict(on, map_source=source, masks="all", **kw)
        out[f"{source}_{w}_sigma_fpr"] = dict(on, map_source=source, masks="all", map_sigma=1.5,
                                              operating_point=dict(fpr=0.05, level="pixel", calib=_pairs(CALIB)), **kw)
    points = dict(given=dict(threshold=0.02, min_area=3), fpr_pixel=dict(fpr=0.05, level="pixel", calib=_pairs(CALIB)),
                  fpr_image=dict(fpr=0.3, level="image", calib=_pairs(CALIB)))
    for (p, op), masks in itertools.product(points.items(), ("all", "one_missing", None)):
        out[f"op_{p}_masks_{masks}"] = dict(pixel_metrics=True, aupro=True, masks=masks, operating_point=op)
    out["save_masks"] = dict(on, masks="all", save_images=True, operating_point=dict(threshold=0.02, save_masks=True))
    return out


def run_cases():
    from srad_amd import evaluate as E
    saved, log = [], []
    extra = dict(score_pairs=_score_pairs, pixel_roc_auc=_pixel_roc_auc, aupro=_aupro, map_threshold=_map_threshold,
                 operating_point=_operating_point)
    keep = {k: getattr(E, k) for k in ("super_resolve_u8", "save_masks", "save_sr_image")}
    opt = types.SimpleNamespace(rgb_range=255.0, scale=[4])
    model = types.SimpleNamespace(eval=lambda: None)
    out = {}
    try:
        E.super_resolve_u8 = _super_resolve_u8
        E.save_masks = lambda pred, names, splits, d: log.append(["masks", list(names), list(splits), d, pred.sum((1, 2)).tolist()])
        E.save_sr_image = lambda img, name, split, scale, d: log.append(["sr", name, split, int(scale), d])
        with T.stand_ins(E, saved, **extra):
            for name, kw in cases().items():
                kw = dict(kw)
                which = kw.pop("masks")
                masks = None if which is None else masks_all()
                if which == "one_missing":
                    masks[4] = None
                del saved[:], log[:]
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    res = E.evaluate_on_test(opt, model, _pairs(range(3)), _pairs(range(3, T.N_IMG)), names=NAMES,
                                             output_dir="out", masks=masks, **kw)
                out[name] = dict(result=[[k, v] for k, v in res.items()], lines=buf.getvalue().splitlines(),
                                 saved=[["maps", names, [math.fsum(img.reshape(-1).tolist()) for img in m.double()]] for names, m in saved]
                                 + [list(entry) for entry in log])
    finally:
        for k, fn in keep.items():
            setattr(E, k, fn)
    return json.loads(json.dumps(out, allow_nan=False))       # what the file holds: lists for tuples, floats as they are


def main():
    data = run_cases()
    with open(OUT, "w") as f:
        json.dump(data, f, indent=0, allow_nan=False)
        f.write("\n")
    print(f"{len(data)} cases -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
