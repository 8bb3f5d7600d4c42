"""GPU: the operating point in the evaluator (evaluate_on_test(operating_point=...) and the CLI's --threshold / --threshold-fpr /
--threshold-level / --min-region-area / --save-masks) end to end.  Every new key is recomputed in the test: the same
super_resolve_u8 calls (same lists, same order, so the same batching), then metrics.anomaly_maps / smooth_maps, then numpy -
np.sort for the threshold, boolean arithmetic for the counts, the pure-Python union-find labeller for the area filter and the
regions, Python integers for the overlap sum.  Counts and thresholds are compared exactly, the ratios at 1e-12."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from srad_amd import spec as S
from tests.test_gpu_pixel_eval import _model, _pairs_and_masks, _write_prepared_tree

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IMAGE_KEYS = {"image_tp", "image_fp", "image_fn", "image_tn", "image_tpr", "image_fpr"}
PIXEL_KEYS = {"pixel_tp", "pixel_fp", "pixel_fn", "pixel_tn", "precision", "recall", "f1", "iou", "fpr", "pro_at_threshold"}
FPR_KEYS = {"threshold_fpr", "threshold_level", "calib_images", "calib_rate"}


def _generator():
    spec = importlib.util.spec_from_file_location("make_pro_golden", os.path.join(GOLDEN_DIR, "make_pro_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ratio(a, b):
    return a / b if b else 0.0


def _maps(M, sr, hr, ws, scales, sigma, with_max=False):
    maps = M.anomaly_maps_multi(sr, hr, scales, "mean") if scales else M.anomaly_maps(sr, hr, ws)
    if with_max:
        return M.smooth_maps(maps, sigma, with_max=True)
    return M.smooth_maps(maps, sigma) if sigma > 0 else maps


def _expected(E, M, opt, model, good, bad, calib, masks, ws, threshold=None, fpr=None, level="pixel", min_area=1, sigma=0.0,
              scales=()):
    """The new keys of the result, from the definitions.  masks: a list with a mask for every image, or None."""
    G = _generator()
    pairs = list(good) + list(bad)
    y = np.array([0] * len(good) + [1] * len(bad))
    sr, hr = E.super_resolve_u8(model, [p[0] for p in pairs], [p[1] for p in pairs], float(opt.rgb_range))
    maps = _maps(M, sr, hr, ws, list(scales), sigma).cpu().numpy()
    want = {}
    if fpr is not None:
        csr, chr_ = E.super_resolve_u8(model, [p[0] for p in calib], [p[1] for p in calib], float(opt.rgb_range))
        if level == "image":
            cm, _ = _maps(M, csr, chr_, ws, list(scales), sigma, with_max=True)
            values = cm.cpu().numpy().max((1, 2))
        else:
            values = _maps(M, csr, chr_, ws, list(scales), sigma).cpu().numpy().ravel()
        n = len(values)
        k = n - 1 - min(max(math.floor(fpr * n), 0), n - 1)
        t = float(np.sort(values)[k])
        want.update(threshold=t, threshold_source="fpr", threshold_fpr=fpr, threshold_level=level, calib_images=len(calib),
                    calib_rate=int((values > np.float32(t)).sum()) / n)
        assert want["calib_rate"] <= fpr
    else:
        t = float(threshold)
        want.update(threshold=t, threshold_source="given")
    want["min_region_area"] = min_area
    pred = maps.astype(np.float64) > t
    if min_area > 1:
        pred &= G.uf_sizes(pred)[0] >= min_area
    flagged = pred.any((1, 2))
    itp, ifp, ifn = int((flagged & (y == 1)).sum()), int((flagged & (y == 0)).sum()), int((~flagged & (y == 1)).sum())
    itn = len(y) - itp - ifp - ifn
    want.update(image_tp=itp, image_fp=ifp, image_fn=ifn, image_tn=itn, image_tpr=_ratio(itp, itp + ifn), image_fpr=_ratio(ifp, ifp + itn))
    if masks is not None:
        m = np.stack(masks) != 0
        z, R = G.uf_sizes(m)
        tp, fp, fn = int((pred & m).sum()), int((pred & ~m).sum()), int((~pred & m).sum())
        tn = m.size - tp - fp - fn
        num = sum((1 << 64) // int(v) for v in z[pred & m])
        want.update(pixel_tp=tp, pixel_fp=fp, pixel_fn=fn, pixel_tn=tn, precision=_ratio(tp, tp + fp), recall=_ratio(tp, tp + fn),
                    f1=_ratio(2 * tp, 2 * tp + fp + fn), iou=_ratio(tp, tp + fp + fn), fpr=_ratio(fp, fp + tn),
                    pro_at_threshold=_ratio(num, R << 64))
    return want, pred, maps


def _same(got, want):
    for k, v in want.items():
        if isinstance(v, float) and k not in ("threshold", "threshold_fpr"):
            assert abs(got[k] - v) <= 1e-12, (k, got[k], v)
        else:
            assert got[k] == v and type(got[k]) is type(v), (k, got[k], v)


@pytest.mark.parametrize("model_type", ["drct", "drn-l"])
def test_operating_point_keys_match_the_recomputation(model_type):
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    scale, hr_size = 4, 64
    opt, model, cfg, sd = _model(model_type, hr_size, scale)
    y, good, bad, masks = _pairs_and_masks(6, 8, hr_size, scale, 1)
    _, calib, _, _ = _pairs_and_masks(5, 1, hr_size, scale, 1, seed=21)
    assert len(calib) == 5
    plain = E.evaluate_on_test(opt, model, good, bad)
    off = E.evaluate_on_test(opt, model, good, bad, masks=masks, operating_point=None)
    assert off == plain and list(off) == list(plain)                       # the feature off: today's result, key for key
    ws = plain["best_ws"]
    base_keys = {"threshold", "threshold_source", "min_region_area"} | IMAGE_KEYS | PIXEL_KEYS
    # calibrated at each level
    for level in ("pixel", "image"):
        spec = E.OperatingPoint(fpr=0.05, level=level, calib=calib)
        got = E.evaluate_on_test(opt, model, good, bad, masks=masks, operating_point=spec)
        for k in plain:
            assert got[k] == plain[k], k
        assert set(got) - set(plain) == base_keys | FPR_KEYS | {"map_ws"} and got["map_ws"] == ws
        want, pred, _ = _expected(E, M, opt, model, good, bad, calib, masks, ws, fpr=0.05, level=level)
        _same(got, want)
    assert pred.any()                                                       # the image-level threshold still predicts something
    # a given threshold (no float32), as a dict, with the area filter
    _, _, maps = _expected(E, M, opt, model, good, bad, calib, masks, ws, threshold=0.0)
    t = float(np.quantile(maps.astype(np.float64), 0.9))
    got = E.evaluate_on_test(opt, model, good, bad, masks=masks, operating_point=dict(threshold=t, min_area=3))
    assert set(got) - set(plain) == base_keys | {"map_ws"}
    want, pred, _ = _expected(E, M, opt, model, good, bad, calib, masks, ws, threshold=t, min_area=3)
    _same(got, want)
    unfiltered, _, _ = _expected(E, M, opt, model, good, bad, calib, masks, ws, threshold=t)
    assert want["pixel_tp"] + want["pixel_fp"] < unfiltered["pixel_tp"] + unfiltered["pixel_fp"]      # the filter removed something
    # smoothed maps, and multi-scale maps: the calibration images go the same way
    spec = E.OperatingPoint(fpr=0.05, calib=calib, min_area=2)
    got = E.evaluate_on_test(opt, model, good, bad, masks=masks, operating_point=spec, map_sigma=2.0)
    assert set(got) - set(plain) == base_keys | FPR_KEYS | {"map_ws", "map_sigma"} and got["map_sigma"] == 2.0
    _same(got, _expected(E, M, opt, model, good, bad, calib, masks, ws, fpr=0.05, min_area=2, sigma=2.0)[0])
    spec = E.OperatingPoint(fpr=0.05, level="image", calib=calib)
    got = E.evaluate_on_test(opt, model, good, bad, masks=masks, operating_point=spec, map_sigma=2.0)
    _same(got, _expected(E, M, opt, model, good, bad, calib, masks, ws, fpr=0.05, level="image", sigma=2.0)[0])
    spec = E.OperatingPoint(fpr=0.05, calib=calib)
    got = E.evaluate_on_test(opt, model, good, bad, masks=masks, operating_point=spec, map_scales=[7, 11])
    assert set(got) - set(plain) == base_keys | FPR_KEYS | {"map_scales", "map_reduce"} and got["map_scales"] == [7, 11]
    _same(got, _expected(E, M, opt, model, good, bad, calib, masks, 0, fpr=0.05, scales=[7, 11])[0])
    # a missing mask drops only the pixel-level keys
    holey = list(masks)
    holey[-1] = None
    spec = E.OperatingPoint(fpr=0.05, calib=calib)
    got = E.evaluate_on_test(opt, model, good, bad, masks=holey, operating_point=spec)
    assert set(got) - set(plain) == (base_keys - PIXEL_KEYS) | FPR_KEYS | {"map_ws"}
    _same(got, _expected(E, M, opt, model, good, bad, calib, None, ws, fpr=0.05)[0])
    # beside the other pixel metrics: their numbers do not move
    both = E.evaluate_on_test(opt, model, good, bad, masks=masks, pixel_metrics=True, aupro=True, operating_point=spec)
    alone = E.evaluate_on_test(opt, model, good, bad, masks=masks, pixel_metrics=True, aupro=True)
    for k in alone:
        assert both[k] == alone[k], k
    assert set(both) - set(alone) == base_keys | FPR_KEYS
    # an inconsistent specification is refused before any work
    for bad_spec in (dict(), dict(threshold=0.5, fpr=0.05, calib=calib), dict(fpr=0.05), dict(fpr=1.5, calib=calib),
                     dict(threshold=0.5, min_area=0), dict(threshold=0.5, level="region")):
        with pytest.raises(ValueError):
            E.evaluate_on_test(opt, model, good, bad, masks=masks, operating_point=bad_spec)


def _write_val_good(root, size, scale, n):
    _, calib, _, _ = _pairs_and_masks(n, 1, size, scale, 1, seed=33)
    base = root / "grid" / "val" / "good"
    for k, (lr, hr) in enumerate(calib):
        lr2 = hr.reshape(size // 2, 2, size // 2, 2, 1).astype(np.float32).mean((1, 3)).round().astype(np.uint8)
        for sub, img in (("HR", hr), ("LR_2", lr2), (f"LR_{scale}", lr)):     # DRN-L x4 reads the x2 level too
            (base / sub).mkdir(parents=True, exist_ok=True)
            Image.fromarray(img[:, :, 0]).save(base / sub / f"v{k:03d}.png")
    return calib


def test_cli_operating_point_and_saved_masks(tmp_path, capsys):
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    from srad_amd import options as Opt
    from srad_amd.model import Model
    size, scale = 64, 4
    root, out_dir = tmp_path / "data", tmp_path / "out"
    names = _write_prepared_tree(root, 3, 4, size, scale)
    cfg = S.DRNConfig.for_scale(scale, 1)
    sd = S.synth_state(S.drn_spec(cfg), seed=9, gain=0.4, cfg=cfg)
    ckpt = tmp_path / "model.pt"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, ckpt)
    common = ["--model-type", "drn-l", "--classe", "grid", "--scale", str(scale), "--resolution", str(size), "--data-root", str(root),
              "--checkpoint", str(ckpt), "--output-dir", str(out_dir), "--dtype", "fp32"]
    with pytest.raises(SystemExit) as e:                                    # no val/good yet: refused, with the path
        E.main(common + ["--threshold-fpr", "0.05"])
    assert str(root / "grid" / "val" / "good") in str(e.value)
    capsys.readouterr()
    _write_val_good(root, size, scale, 4)
    out = E.main(common + ["--threshold-fpr", "0.05", "--min-region-area", "2", "--save-masks"])
    text = capsys.readouterr().out
    line = [ln for ln in text.splitlines() if ln.startswith("Operating point - ")]
    assert len(line) == 1, text
    assert out["threshold_source"] == "fpr" and out["calib_images"] == 4 and out["min_region_area"] == 2
    assert PIXEL_KEYS <= set(out) and IMAGE_KEYS <= set(out)                # the GT masks of the tree were read
    # the returned dict matches the line
    assert float(re.search(r"threshold=(\S+) ", line[0]).group(1)) == float(f"{out['threshold']:.9g}")
    assert "min_area=2:" in line[0] and f"(ws={out['map_ws']})" in line[0]
    image, pixel = line[0].split(": image ")[1].split("; pixel ")
    for part, prefix in ((image, "image_"), (pixel, "pixel_")):
        for k in ("tp", "fp", "fn", "tn"):
            assert int(re.search(rf"\b{k}=(\d+)", part).group(1)) == out[prefix + k], (k, part)
    assert abs(float(re.search(r"tpr=(\S+)", image).group(1)) - out["image_tpr"]) <= 5e-5
    for k, name in (("precision", "precision"), ("recall", "recall"), ("f1", "f1"), ("iou", "iou"), ("pro", "pro_at_threshold")):
        assert abs(float(re.search(rf"\b{k}=(\S+)", pixel).group(1)) - out[name]) <= 5e-5, k
    # the saved masks are the prediction, 0 / 255: recomputed from the tree with numpy
    opt = Opt.build_opt("drn-l", "grid", size, scale, 1, "fp32", pre_train=str(ckpt), data_root=str(root))
    opt.test_only = True
    model = Model(opt, None, dual_model=True)
    model.eval()
    G = _generator()
    for split in ("good", "bad"):
        items = list(E.iter_split(str(root), "grid", split, opt.scale, opt.n_colors))
        sr, hr = E.super_resolve_u8(model, [lr for _, lr, _ in items], [h for _, _, h in items], float(opt.rgb_range))
        maps = M.anomaly_maps(sr, hr, out["map_ws"]).cpu().numpy()
        pred = maps.astype(np.float64) > out["threshold"]
        pred &= G.uf_sizes(pred)[0] >= 2
        for k, (name, _, _) in enumerate(items):
            a = np.array(Image.open(out_dir / "anomaly_masks" / split / f"{name}.png"))
            assert a.dtype == np.uint8 and np.array_equal(a, pred[k].astype(np.uint8) * 255), (split, name)
    assert sorted(p.name for p in (out_dir / "anomaly_masks").rglob("*.png")) == sorted(f"{n}.png" for _, n in names)
    # a given threshold needs no val/good; without --save-masks nothing more is written
    n_files = len(list(out_dir.rglob("*.png")))
    out2 = E.main(common + [f"--threshold={out['threshold']!r}"])
    text = capsys.readouterr().out
    assert len([ln for ln in text.splitlines() if ln.startswith("Operating point - ")]) == 1
    assert out2["threshold_source"] == "given" and out2["threshold"] == out["threshold"] and not FPR_KEYS & set(out2)
    assert out2["min_region_area"] == 1 and out2["pixel_tp"] + out2["pixel_fp"] >= out["pixel_tp"] + out["pixel_fp"]
    assert len(list(out_dir.rglob("*.png"))) == n_files
