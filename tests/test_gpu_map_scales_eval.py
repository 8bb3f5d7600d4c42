"""GPU: multi-scale anomaly maps in the evaluator (evaluate_on_test(map_scales=..., map_reduce=...) and the CLI's --map-scales /
--map-reduce): the pixel-level numbers equal, exactly, the same ``metrics`` functions applied to ``anomaly_maps_multi`` (and
``smooth_maps``) of the evaluator's own SR images, and nothing changes when the scales are not given."""
import numpy as np
import pytest
import torch

from srad_amd import spec as S
from tests.test_gpu_pixel_eval import _model, _pairs_and_masks, _write_prepared_tree

pytestmark = pytest.mark.gpu

SCALES = [11, 21, 31]


@pytest.mark.parametrize("sigma", [0.0, 4.0])
@pytest.mark.parametrize("reduce", ["mean", "max"])
def test_pixel_numbers_come_from_the_multi_scale_maps(reduce, sigma):
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    scale, hr_size = 4, 64
    opt, model, cfg, sd = _model("drn-l", hr_size, scale)
    y, good, bad, masks = _pairs_and_masks(6, 8, hr_size, scale, 1)
    plain = E.evaluate_on_test(opt, model, good, bad)
    got = E.evaluate_on_test(opt, model, good, bad, masks=masks, pixel_metrics=True, aupro=True, map_image_score=True,
                             map_scales=SCALES, map_reduce=reduce, map_sigma=sigma)
    for k in plain:
        assert got[k] == plain[k], k
    extra = {"auc_pixel", "aupro", "pro_fpr_limit", "auc_map_max", "map_scales", "map_reduce"} | ({"map_sigma"} if sigma else set())
    assert set(got) - set(plain) == extra and "map_ws" not in got
    assert got["map_scales"] == SCALES and got["map_reduce"] == reduce
    pairs = good + bad
    sr, hr = E.super_resolve_u8(model, [p[0] for p in pairs], [p[1] for p in pairs], float(opt.rgb_range))
    maps = M.anomaly_maps_multi(sr, hr, SCALES, reduce)
    if sigma:
        maps = M.smooth_maps(maps, sigma)
    labels = torch.from_numpy(np.stack(masks)).cuda()
    assert got["auc_pixel"] == M.pixel_roc_auc(maps, labels)
    assert got["aupro"] == M.aupro(maps, labels)
    assert got["auc_map_max"] == M.roc_auc(y, maps.amax((1, 2)).double().cpu().numpy())
    # the scales decide the maps: another reduction or a single window gives other numbers
    single = E.evaluate_on_test(opt, model, good, bad, masks=masks, pixel_metrics=True, map_sigma=sigma)
    assert "map_ws" in single and "map_scales" not in single and single["auc_pixel"] != got["auc_pixel"]


def test_sweep_scales_and_unchanged_default():
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    scale, hr_size = 4, 64
    opt, model, cfg, sd = _model("drct", hr_size, scale)
    y, good, bad, masks = _pairs_and_masks(6, 8, hr_size, scale, 1)
    flags = dict(masks=masks, pixel_metrics=True, aupro=True, map_image_score=True, map_sigma=4.0)
    old = E.evaluate_on_test(opt, model, good, bad, **flags)
    assert E.evaluate_on_test(opt, model, good, bad, map_scales=(), map_reduce="max", **flags) == old
    assert E.evaluate_on_test(opt, model, good, bad, map_scales=[], **flags) == old
    assert "map_ws" in old and "map_scales" not in old and "map_reduce" not in old
    got = E.evaluate_on_test(opt, model, good, bad, map_scales="sweep", **flags)
    assert got["map_scales"] == M.sweep_window_sizes(hr_size) == got["window_sizes"] and got["map_reduce"] == "mean"
    pairs = good + bad
    sr, hr = E.super_resolve_u8(model, [p[0] for p in pairs], [p[1] for p in pairs], float(opt.rgb_range))
    maps = M.smooth_maps(M.anomaly_maps_multi(sr, hr, M.sweep_window_sizes(hr_size), "mean"), 4.0)
    assert got["auc_pixel"] == M.pixel_roc_auc(maps, torch.from_numpy(np.stack(masks)).cuda())
    with pytest.raises(ValueError, match="window 129"):
        E.evaluate_on_test(opt, model, good, bad, map_scales=[11, 129], **flags)
    with pytest.raises(ValueError, match="exclude"):
        E.evaluate_on_test(opt, model, good, bad, map_scales=[11], map_ws=3, **flags)
    with pytest.raises(ValueError, match="map_reduce"):
        E.evaluate_on_test(opt, model, good, bad, map_scales=[11], map_reduce="sum", **flags)


def test_cli_map_scales(tmp_path, capsys):
    from srad_amd import evaluate as E
    size, scale = 64, 4
    root, out = tmp_path / "data", tmp_path / "out"
    _write_prepared_tree(root, 3, 4, size, scale)
    cfg = S.DRNConfig.for_scale(scale, 1)
    sd = S.synth_state(S.drn_spec(cfg), seed=9, gain=0.4, cfg=cfg)
    ckpt = tmp_path / "model.pt"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, ckpt)
    res = E.main(["--model-type", "drn-l", "--classe", "grid", "--scale", str(scale), "--resolution", str(size), "--data-root",
                  str(root), "--checkpoint", str(ckpt), "--output-dir", str(out), "--dtype", "fp32", "--map-scales", "11,21,31",
                  "--map-reduce", "max", "--map-sigma", "4", "--map-image-score", "--pixel-metrics", "--aupro"])
    text = capsys.readouterr().out.splitlines()
    assert res["map_scales"] == SCALES and res["map_reduce"] == "max" and "map_ws" not in res
    assert f"Image AUC - max of the SSIM map (scales=[11, 21, 31], max, sigma=4): {res['auc_map_max']:.4f}" in text
    assert f"Pixel AUC - SSIM map (scales=[11, 21, 31], max, sigma=4): {res['auc_pixel']:.4f}" in text
    assert f"AU-PRO - SSIM map (scales=[11, 21, 31], max, fpr <= 0.3, sigma=4): {res['aupro']:.4f}" in text
