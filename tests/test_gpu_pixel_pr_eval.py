"""GPU: the precision-recall metrics in the evaluator (evaluate_on_test(pr_metrics=True) and the CLI's --pr-metrics) end to end:
the pixel-level numbers are ``metrics.pixel_pr`` of the maps the evaluator's own ``MapSpec`` makes, the image-level numbers are
``metrics.average_precision`` of the score columns, the reported threshold passed back as an operating point counts the best
point, and without the flag the result is what it was."""
import numpy as np
import pytest
import torch

from srad_amd import spec as S
from tests.test_gpu_pixel_eval import _model, _pairs_and_masks, _write_prepared_tree

pytestmark = pytest.mark.gpu

IMAGE_KEYS = ["ap_ssim", "ap_mse", "ap_psnr", "f1max_ssim", "f1max_mse", "f1max_psnr"]
PIXEL_KEYS = ["ap_pixel", "f1max_pixel", "f1max_pixel_threshold", "f1max_pixel_precision", "f1max_pixel_recall"]


def test_pr_metrics_equal_the_metrics_on_the_evaluators_maps(capsys):
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    scale, hr_size = 4, 64
    opt, model, cfg, sd = _model("drct", hr_size, scale)
    y, good, bad, masks = _pairs_and_masks(6, 8, hr_size, scale, 1)
    base = E.evaluate_on_test(opt, model, good, bad, masks=masks, pixel_metrics=True, map_image_score=True)
    capsys.readouterr()
    got = E.evaluate_on_test(opt, model, good, bad, masks=masks, pixel_metrics=True, map_image_score=True, pr_metrics=True)
    lines = capsys.readouterr().out.splitlines()
    assert [k for k in got if k not in base] == IMAGE_KEYS + ["ap_map_max", "f1max_map_max"] + PIXEL_KEYS
    assert all(got[k] == v for k, v in base.items())
    assert [ln.split(" - ")[0] for ln in lines] == ["Test AUCs", "Test APs", "Image AUC", "Image AP", "Pixel AUC", "Pixel AP"]
    # the same stacks, scores and maps, made the evaluator's way
    pairs = good + bad
    sr, hr = E.super_resolve_u8(model, [p[0] for p in pairs], [p[1] for p in pairs], float(opt.rgb_range))
    sizes = got["window_sizes"]
    ssim, mse, psnr = (t.cpu().numpy() for t in M.score_pairs(sr, hr, sizes))
    cols = dict(ssim=1.0 - ssim[:, sizes.index(got["best_ws"])], mse=mse, psnr=-psnr)
    for k, col in cols.items():
        assert (got[f"ap_{k}"], got[f"f1max_{k}"]) == M.average_precision(y, col), k
    spec = E.MapSpec(ws=got["map_ws"]).resolve(hr_size, hr_size)
    maps, img_max = spec.make(sr, hr, True)
    assert (got["ap_map_max"], got["f1max_map_max"]) == M.average_precision(y, img_max.double().cpu().numpy())
    labels = torch.from_numpy(np.stack(masks)).cuda()
    r = M.pixel_pr(maps, labels)
    assert [got[k] for k in PIXEL_KEYS] == [r[k] for k in ("ap", "f1max", "threshold", "precision", "recall")]
    assert 0.0 < r["ap"] <= 1.0 and 0 < r["tp"] and r["f1max"] == 2 * r["tp"] / (2 * r["tp"] + r["fp"] + r["fn"])
    # the threshold goes back in as --threshold does: the operating point counts the best point
    at = E.evaluate_on_test(opt, model, good, bad, masks=masks, operating_point=dict(threshold=got["f1max_pixel_threshold"]))
    assert (at["pixel_tp"], at["pixel_fp"], at["pixel_fn"]) == (r["tp"], r["fp"], r["fn"])
    assert at["f1"] == got["f1max_pixel"] and at["precision"] == got["f1max_pixel_precision"]
    # pr_metrics alone asks for the pixel level too (it is gated like the pixel AUC); a missing mask leaves the image level
    alone = E.evaluate_on_test(opt, model, good, bad, masks=masks, pr_metrics=True)
    assert [alone[k] for k in PIXEL_KEYS] == [got[k] for k in PIXEL_KEYS] and "auc_pixel" not in alone
    holey = list(masks)
    holey[-1] = None
    skipped = E.evaluate_on_test(opt, model, good, bad, masks=holey, pr_metrics=True)
    assert not set(PIXEL_KEYS) & set(skipped) and [skipped[k] for k in IMAGE_KEYS] == [got[k] for k in IMAGE_KEYS]


def test_cli_pr_metrics(tmp_path, capsys):
    from srad_amd import evaluate as E
    size, scale = 64, 4
    root = tmp_path / "data"
    _write_prepared_tree(root, 3, 4, size, scale)
    cfg = S.DRNConfig.for_scale(scale, 1)
    sd = S.synth_state(S.drn_spec(cfg), seed=9, gain=0.4, cfg=cfg)
    ckpt = tmp_path / "model.pt"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, ckpt)
    argv = ["--model-type", "drn-l", "--classe", "grid", "--scale", str(scale), "--resolution", str(size), "--data-root", str(root),
            "--checkpoint", str(ckpt), "--output-dir", str(tmp_path / "out"), "--dtype", "fp32", "--pixel-metrics"]
    plain = E.main(argv)
    plain_text = capsys.readouterr().out
    out = E.main(argv + ["--pr-metrics"])
    text = capsys.readouterr().out
    new = [ln for ln in text.splitlines() if ln not in plain_text.splitlines()]
    assert [ln.split(" - ")[0] for ln in new] == ["Test APs", "Pixel AP"], text
    assert [ln for ln in text.splitlines() if ln not in new] == plain_text.splitlines()     # the rest is byte for byte the same
    assert new[1].startswith(f"Pixel AP - SSIM map (ws={out['map_ws']}): {out['ap_pixel']:.4f}, F1-max: {out['f1max_pixel']:.4f} (")
    assert new[1].endswith(f"at threshold={out['f1max_pixel_threshold']:.9g})")
    assert {k: v for k, v in out.items() if k in plain} == plain and set(out) - set(plain) == set(IMAGE_KEYS + PIXEL_KEYS)
    # ... and the printed threshold, passed to --threshold, reproduces the best point
    at = E.main(argv[:-1] + ["--threshold", f"{out['f1max_pixel_threshold']:.9g}"])
    assert at["f1"] == out["f1max_pixel"] and at["recall"] == out["f1max_pixel_recall"]
