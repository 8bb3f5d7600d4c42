"""GPU: squared-error maps in the evaluator (evaluate_on_test(map_source='mse') and the CLI's --map-source): every pixel-level
number equals, exactly, the same ``metrics`` functions applied to ``error_maps`` / ``error_maps_multi`` (then ``smooth_maps``) of
the evaluator's own SR images - the calibration images of the threshold included - and nothing changes for the SSIM source."""
import numpy as np
import pytest
import torch

from srad_amd import spec as S
from tests.test_gpu_operating_point_eval import _write_val_good
from tests.test_gpu_pixel_eval import _model, _pairs_and_masks, _write_prepared_tree

pytestmark = pytest.mark.gpu

SIGMA, FPR = 2.0, 0.05


def _recompute(E, M, opt, model, good, bad, calib, masks, y, ws, scales, reduce="mean"):
    """The pixel-level keys of the result from the public metrics functions, on maps made here."""
    def raw_maps(pairs):
        sr, hr = E.super_resolve_u8(model, [p[0] for p in pairs], [p[1] for p in pairs], float(opt.rgb_range))
        return M.error_maps_multi(sr, hr, scales, reduce) if scales else M.error_maps(sr, hr, ws)
    maps, img_max = M.smooth_maps(raw_maps(good + bad), SIGMA, with_max=True)
    labels = torch.from_numpy(np.stack(masks)).cuda()
    want = dict(map_source="mse", map_sigma=SIGMA, auc_map_max=M.roc_auc(y, img_max.double().cpu().numpy()),
                auc_pixel=M.pixel_roc_auc(maps, labels), aupro=M.aupro(maps, labels, 0.3), pro_fpr_limit=0.3)
    want.update(dict(map_scales=scales, map_reduce=reduce) if scales else dict(map_ws=ws))
    cmaps = M.smooth_maps(raw_maps(calib), SIGMA)
    t, achieved = M.map_threshold(cmaps, FPR)
    want.update(threshold=t, threshold_source="fpr", threshold_fpr=FPR, threshold_level="pixel", calib_images=len(calib),
                calib_rate=achieved, min_region_area=1)
    _, img_pred, counts = M.operating_point(maps, t, labels, 1)
    want.update(M.operating_point_stats(counts, img_pred, y))
    return want


@pytest.mark.parametrize("scales", [None, [3, 11]])
def test_pixel_numbers_come_from_the_error_maps(scales, capsys):
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    scale, hr_size = 4, 64
    opt, model, cfg, sd = _model("drn-l", hr_size, scale)
    y, good, bad, masks = _pairs_and_masks(6, 8, hr_size, scale, 1)
    _, calib, _, _ = _pairs_and_masks(5, 1, hr_size, scale, 1, seed=21)
    plain = E.evaluate_on_test(opt, model, good, bad)
    capsys.readouterr()
    flags = dict(masks=masks, pixel_metrics=True, aupro=True, map_image_score=True, map_sigma=SIGMA,
                 operating_point=E.OperatingPoint(fpr=FPR, calib=calib))
    if scales:
        flags.update(map_scales=scales)
    got = E.evaluate_on_test(opt, model, good, bad, map_source="mse", **flags)
    lines = capsys.readouterr().out.splitlines()
    for k in plain:                                          # the image-level part is the SSIM sweep's, untouched
        assert got[k] == plain[k], k
    want = _recompute(E, M, opt, model, good, bad, calib, masks, y, 1, scales)
    new = {k: v for k, v in got.items() if k not in plain}
    assert new == want, {k: (new.get(k), want.get(k)) for k in set(new) | set(want) if new.get(k) != want.get(k)}
    assert got["map_source"] == "mse"
    if scales:
        assert got["map_scales"] == scales and got["map_reduce"] == "mean" and "map_ws" not in got
    else:
        assert got["map_ws"] == 1 and got["best_ws"] != 1 and "map_scales" not in got
    pixel_lines = [l for l in lines if " map (" in l]         # the four lines of the pixel stage
    assert len(pixel_lines) == 4 and all("MSE map" in l and "SSIM map" not in l for l in pixel_lines), pixel_lines
    what = "scales=[3, 11], mean" if scales else "ws=1"
    assert f"Pixel AUC - MSE map ({what}, sigma=2): {got['auc_pixel']:.4f}" in lines
    # the source decides the maps: the SSIM maps under the same flags give other numbers
    other = E.evaluate_on_test(opt, model, good, bad, **flags)
    assert "map_source" not in other and other["auc_pixel"] != got["auc_pixel"] and other["threshold"] != got["threshold"]


def test_map_ws_under_mse_and_refusals():
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    scale, hr_size = 4, 64
    opt, model, cfg, sd = _model("drct", hr_size, scale)
    y, good, bad, masks = _pairs_and_masks(6, 8, hr_size, scale, 1)
    got = E.evaluate_on_test(opt, model, good, bad, masks=masks, pixel_metrics=True, map_source="mse", map_ws=11)
    assert got["map_ws"] == 11 and got["map_source"] == "mse" and "map_sigma" not in got
    pairs = good + bad
    sr, hr = E.super_resolve_u8(model, [p[0] for p in pairs], [p[1] for p in pairs], float(opt.rgb_range))
    assert got["auc_pixel"] == M.pixel_roc_auc(M.error_maps(sr, hr, 11), torch.from_numpy(np.stack(masks)).cuda())
    with pytest.raises(ValueError, match="map_source"):
        E.evaluate_on_test(opt, None, good, bad, map_source="psnr", pixel_metrics=True, masks=masks)
    with pytest.raises(ValueError, match="window 129"):
        E.evaluate_on_test(opt, None, good, bad, map_source="mse", map_scales=[11, 129], pixel_metrics=True, masks=masks)
    with pytest.raises(ValueError, match="exclude"):
        E.evaluate_on_test(opt, None, good, bad, map_source="mse", map_scales=[11], map_ws=3, pixel_metrics=True, masks=masks)


def test_ssim_source_changes_nothing(capsys):
    from srad_amd import evaluate as E
    scale, hr_size = 4, 64
    opt, model, cfg, sd = _model("drn-l", hr_size, scale)
    y, good, bad, masks = _pairs_and_masks(6, 8, hr_size, scale, 1)
    _, calib, _, _ = _pairs_and_masks(5, 1, hr_size, scale, 1, seed=21)
    for extra in (dict(), dict(map_scales=[3, 11], map_reduce="max"), dict(map_ws=5)):
        flags = dict(masks=masks, pixel_metrics=True, aupro=True, map_image_score=True, map_sigma=SIGMA,
                     operating_point=E.OperatingPoint(fpr=FPR, calib=calib), **extra)
        capsys.readouterr()
        old = E.evaluate_on_test(opt, model, good, bad, **flags)
        old_text = capsys.readouterr().out
        new = E.evaluate_on_test(opt, model, good, bad, map_source="ssim", **flags)
        new_text = capsys.readouterr().out
        assert new == old and list(new) == list(old) and new_text == old_text and "map_source" not in new
        assert "SSIM map" in old_text and "MSE map" not in old_text


def test_cli_map_source(tmp_path, capsys):
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    size, scale = 64, 4
    root, out = tmp_path / "data", tmp_path / "out"
    _write_prepared_tree(root, 3, 4, size, scale)
    _write_val_good(root, size, scale, 4)
    cfg = S.DRNConfig.for_scale(scale, 1)
    sd = S.synth_state(S.drn_spec(cfg), seed=9, gain=0.4, cfg=cfg)
    ckpt = tmp_path / "model.pt"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, ckpt)
    res = E.main(["--model-type", "drn-l", "--classe", "grid", "--scale", str(scale), "--resolution", str(size), "--data-root",
                  str(root), "--checkpoint", str(ckpt), "--output-dir", str(out), "--dtype", "fp32", "--map-source", "mse",
                  "--map-image-score", "--pixel-metrics", "--aupro", "--threshold-fpr", "0.05", "--save-anomaly-maps"])
    text = capsys.readouterr().out.splitlines()
    assert res["map_source"] == "mse" and res["map_ws"] == 1 and res["calib_images"] == 4
    assert f"Image AUC - max of the MSE map (ws=1, sigma=0): {res['auc_map_max']:.4f}" in text
    assert f"Pixel AUC - MSE map (ws=1): {res['auc_pixel']:.4f}" in text
    assert f"AU-PRO - MSE map (ws=1, fpr <= 0.3): {res['aupro']:.4f}" in text
    assert any(l.startswith("Operating point - MSE map (ws=1), threshold=") for l in text)
    assert len(list((out / "anomaly_maps" / "bad").glob("*.png"))) == 4
    assert M.MAP_SOURCES == ("ssim", "mse")
