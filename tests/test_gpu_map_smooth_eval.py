"""GPU: smoothed anomaly maps and the map-maximum image score in the evaluator (evaluate_on_test(map_sigma=..., map_image_score=...)
and the CLI's --map-sigma / --map-image-score), against the same numbers computed from the raw maps smoothed by the numpy
restatement of scipy's filter (tests/golden/make_map_smooth_golden.py) and uploaded."""
import importlib.util
import os

import numpy as np
import pytest
import torch
from PIL import Image

from srad_amd import spec as S
from tests.test_gpu_pixel_eval import _model, _pairs_and_masks, _write_prepared_tree

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_map_smooth_golden", os.path.join(GOLDEN_DIR, "make_map_smooth_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("model_type", ["drct", "drn-l"])
def test_smoothed_pixel_metrics_and_map_max_score(model_type):
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    scale, hr_size, sigma = 4, 64, 4.0
    opt, model, cfg, sd = _model(model_type, hr_size, scale)
    y, good, bad, masks = _pairs_and_masks(6, 8, hr_size, scale, 1)
    plain = E.evaluate_on_test(opt, model, good, bad)
    got = E.evaluate_on_test(opt, model, good, bad, masks=masks, pixel_metrics=True, aupro=True, map_sigma=sigma,
                             map_image_score=True)
    for k in plain:
        assert got[k] == plain[k], k
    assert set(got) - set(plain) == {"auc_pixel", "aupro", "pro_fpr_limit", "map_ws", "map_sigma", "auc_map_max"}
    assert got["map_sigma"] == sigma and got["map_ws"] == got["best_ws"]
    # the same numbers from the raw maps, smoothed on the host by the restatement of scipy's filter
    pairs = good + bad
    sr, hr = E.super_resolve_u8(model, [p[0] for p in pairs], [p[1] for p in pairs], float(opt.rgb_range))
    raw = M.anomaly_maps(sr, hr, got["map_ws"])
    smoothed = torch.from_numpy(_generator().smooth_ref(raw.cpu().numpy(), sigma)).cuda()
    labels = torch.from_numpy(np.stack(masks)).cuda()
    assert got["auc_pixel"] == M.pixel_roc_auc(smoothed, labels)
    assert abs(got["aupro"] - M.aupro(smoothed, labels)) <= 1e-12
    img_max = smoothed.amax((1, 2)).double().cpu().numpy()
    assert got["auc_map_max"] == M.roc_auc(y, img_max)
    # smoothing changes the pixel numbers (the raw ones are what the plain pixel run reports)
    raw_run = E.evaluate_on_test(opt, model, good, bad, masks=masks, pixel_metrics=True)
    assert raw_run["auc_pixel"] == M.pixel_roc_auc(raw, labels) and "map_sigma" not in raw_run
    assert raw_run["auc_pixel"] != got["auc_pixel"]
    # the image score alone, on the raw maps: no masks needed, two keys
    only = E.evaluate_on_test(opt, model, good, bad, map_image_score=True)
    assert set(only) - set(plain) == {"auc_map_max", "map_ws"}
    assert only["auc_map_max"] == M.roc_auc(y, raw.amax((1, 2)).double().cpu().numpy())


def test_cli_map_sigma_and_image_score(tmp_path, capsys):
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    size, scale, sigma = 64, 4, 4.0
    root, out = tmp_path / "data", tmp_path / "out"
    names = _write_prepared_tree(root, 3, 4, size, scale)
    cfg = S.DRNConfig.for_scale(scale, 1)
    sd = S.synth_state(S.drn_spec(cfg), seed=9, gain=0.4, cfg=cfg)
    ckpt = tmp_path / "model.pt"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, ckpt)
    res = E.main(["--model-type", "drn-l", "--classe", "grid", "--scale", str(scale), "--resolution", str(size), "--data-root",
                  str(root), "--checkpoint", str(ckpt), "--output-dir", str(out), "--dtype", "fp32", "--map-sigma", "4",
                  "--map-image-score", "--pixel-metrics", "--save-anomaly-maps"])
    text = capsys.readouterr().out
    ws = res["map_ws"]
    line = [ln for ln in text.splitlines() if ln.startswith("Image AUC - max of the SSIM map (")]
    assert line == [f"Image AUC - max of the SSIM map (ws={ws}, sigma=4): {res['auc_map_max']:.4f}"], text
    pix = [ln for ln in text.splitlines() if ln.startswith("Pixel AUC - SSIM map (ws=")]
    assert pix == [f"Pixel AUC - SSIM map (ws={ws}, sigma=4): {res['auc_pixel']:.4f}"], text
    assert res["map_sigma"] == sigma and 0.0 <= res["auc_map_max"] <= 1.0
    # the saved maps are the truncated u8 of the smoothed maps of the saved SR images
    sr, hr = [], []
    for split, name in names:
        sr.append(np.array(Image.open(out / split / f"x{scale}" / f"{name}.png")))
        hr.append(np.array(Image.open(root / "grid" / "test" / split / "HR" / f"{name}.png")))
    sr_t = torch.from_numpy(np.stack(sr)[..., None]).cuda()
    hr_t = torch.from_numpy(np.stack(hr)[..., None]).cuda()
    raw = M.anomaly_maps(sr_t, hr_t, ws).cpu().numpy()
    want = M.to_u8_hwc(torch.from_numpy(_generator().smooth_ref(raw, sigma))[:, None].cuda(), rgb_range=1.0).cpu().numpy()
    for k, (split, name) in enumerate(names):
        a = np.array(Image.open(out / "anomaly_maps" / split / f"{name}.png"))
        assert np.array_equal(a, want[k, :, :, 0]), (split, name)
