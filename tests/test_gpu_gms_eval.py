"""GPU: the gradient-magnitude similarity end to end - the evaluator under map_source='gms' / 'msgms' (every pixel-level number
equals, exactly, the public metrics functions applied to ``metrics.gms_maps`` of the evaluator's own SR images), predict's
calibrate / predict round trip of a GMS spec through operating_point.json, and two eager DRCT training steps under
--loss 0.8*L1+0.2*MSGMS next to the unchanged choice of the graphed step for 1*L1."""
import json
import os
import re

import numpy as np
import pytest
import torch

from srad_amd import spec as S
from tests.test_gpu_pixel_eval import _model, _pairs_and_masks
from tests.test_gpu_predict import HR, SCALE, _write_raw
from tests.test_gpu_train import _write_grid_class

pytestmark = pytest.mark.gpu

SIGMA, FPR = 2.0, 0.05


@pytest.mark.parametrize("model_type", ["drct", "drn-l"])
def test_pixel_numbers_come_from_the_gms_maps(model_type, capsys):
    """Every pixel-level number is the public metrics on ``gms_maps`` of the evaluator's own SR images, for both synthetic
    models of the eval tests.  The sanity check on the planted blobs of ``synth_pairs`` (pixel AUC above 0.5) is asserted
    with the DRCT model: 0.5260 (the same figure from the CPU oracle's forward and tests/gms_ref.py).  With the DRN-L model
    the figure is 0.3360, on the GPU and from the CPU oracle and restatement alike to every digit, so it is a fact about
    that pairing and not about the kernels: the blob is a constant brightness offset, which a gradient measure sees only at
    its rim, and DRN-L's random-weight SR (bicubic plus noise at x4) has lost the grid texture everywhere, so d is high over
    the whole image and LOWER at the rim, where SR gains an edge.  That case is printed, not asserted."""
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    scale, hr_size = 4, 64
    opt, model, cfg, sd = _model(model_type, hr_size, scale)
    y, good, bad, masks = _pairs_and_masks(6, 8, hr_size, scale, 1)
    _, calib, _, _ = _pairs_and_masks(5, 1, hr_size, scale, 1, seed=21)
    plain = E.evaluate_on_test(opt, model, good, bad)
    capsys.readouterr()
    flags = dict(masks=masks, pixel_metrics=True, aupro=True, map_image_score=True, map_sigma=SIGMA,
                 operating_point=E.OperatingPoint(fpr=FPR, calib=calib))
    got = E.evaluate_on_test(opt, model, good, bad, map_source="msgms", **flags)
    lines = capsys.readouterr().out.splitlines()
    for k in plain:                                          # the image-level part is the SSIM sweep's, untouched
        assert got[k] == plain[k], k

    def raw_maps(pairs):
        sr, hr = E.super_resolve_u8(model, [p[0] for p in pairs], [p[1] for p in pairs], float(opt.rgb_range))
        return M.gms_maps(sr, hr, 4)
    maps, img_max = M.smooth_maps(raw_maps(good + bad), SIGMA, with_max=True)
    labels = torch.from_numpy(np.stack(masks)).cuda()
    want = dict(map_source="msgms", map_levels=4, map_sigma=SIGMA, auc_map_max=M.roc_auc(y, img_max.double().cpu().numpy()),
                auc_pixel=M.pixel_roc_auc(maps, labels), aupro=M.aupro(maps, labels, 0.3), pro_fpr_limit=0.3)
    t, achieved = M.map_threshold(M.smooth_maps(raw_maps(calib), SIGMA), FPR)
    want.update(threshold=t, threshold_source="fpr", threshold_fpr=FPR, threshold_level="pixel", calib_images=len(calib),
                calib_rate=achieved, min_region_area=1)
    _, img_pred, counts = M.operating_point(maps, t, labels, 1)
    want.update(M.operating_point_stats(counts, img_pred, y))
    new = {k: v for k, v in got.items() if k not in plain}
    assert new == want, {k: (new.get(k), want.get(k)) for k in set(new) | set(want) if new.get(k) != want.get(k)}
    assert "map_ws" not in got and "map_scales" not in got
    with capsys.disabled():
        print(f"{model_type}: pixel AUC of the MSGMS maps (sigma 2) on the planted blobs {got['auc_pixel']:.4f}")
    if model_type == "drct":
        assert got["auc_pixel"] > 0.5                         # the planted blobs: a sanity check, not a calibration
    pixel_lines = [l for l in lines if " map (" in l]
    assert len(pixel_lines) == 4 and all("GMS map (levels=4" in l for l in pixel_lines), pixel_lines
    assert f"Pixel AUC - GMS map (levels=4, sigma=2): {got['auc_pixel']:.4f}" in lines
    # one level, no smoothing
    one = E.evaluate_on_test(opt, model, good, bad, map_source="gms", masks=masks, pixel_metrics=True)
    sr, hr = E.super_resolve_u8(model, [p[0] for p in good + bad], [p[1] for p in good + bad], float(opt.rgb_range))
    assert one["map_source"] == "gms" and one["map_levels"] == 1 and "map_sigma" not in one
    assert one["auc_pixel"] == M.pixel_roc_auc(M.gms_maps(sr, hr, 1), labels) and one["auc_pixel"] != got["auc_pixel"]
    # the SSIM source is the run without the argument
    capsys.readouterr()
    old = E.evaluate_on_test(opt, model, good, bad, **flags)
    old_text = capsys.readouterr().out
    same = E.evaluate_on_test(opt, model, good, bad, map_source="ssim", **flags)
    assert same == old and list(same) == list(old) and capsys.readouterr().out == old_text and "map_source" not in same
    # refusals before any work
    with pytest.raises(ValueError, match="no window"):
        E.evaluate_on_test(opt, None, good, bad, map_source="msgms", map_ws=11, pixel_metrics=True, masks=masks)


def test_cli_calibrate_then_predict_with_gms(tmp_path, capsys):
    from srad_amd import metrics as M
    from srad_amd import predict as P
    raw = tmp_path / "raw"
    _write_raw(raw, "grid", False)
    run = tmp_path / "drn-l" / f"mvtec_grid_{HR}_X{SCALE}"
    (run / "model").mkdir(parents=True)
    cfg = S.DRNConfig.for_scale(SCALE, 1)
    sd = S.synth_state(S.drn_spec(cfg), seed=9, gain=0.4, cfg=cfg)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, run / "model" / "model_best.pt")
    common = ["--run-dir", str(run), "--dtype", "fp32"]
    inputs = ["--input", str(raw / "grid" / "test" / "good"), str(raw / "grid" / "test" / "crack")]
    out = P.main(common + ["--calibrate", str(raw / "grid" / "train" / "good"), "--threshold-fpr", "0.05", "--map-source", "gms"])
    doc = json.loads((run / "operating_point.json").read_text())
    assert out["operating_point"] == doc and doc["calib_images"] == 5
    assert doc["map_spec"] == dict(source="gms", ws=0, scales=[], reduce="mean", sigma=0.0)
    assert "Calibrated - GMS map (levels=1)" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        P.main(common + inputs + ["--map-source", "msgms"])
    assert "--map-source msgms contradicts" in str(e.value)
    res = P.main(common + inputs + ["--map-source", "gms"])
    again = P.main(common + inputs)                            # the stored spec needs no flag
    assert res["threshold"] == doc["threshold"] and torch.equal(res["maps"], again["maps"])
    assert torch.equal(res["maps"], M.gms_maps(res["sr"], res["hr"], 1))
    pred, img_pred, _ = M.operating_point(res["maps"], doc["threshold"], None, 1)
    assert torch.equal(res["masks"], pred) and res["defect_pixels"] == img_pred.tolist()
    ssim, _, _ = M.score_pairs(res["sr"], res["hr"], [P.MAP_WS_DEFAULT])
    assert res["ssim"] == ssim[:, 0].tolist()


def _trainer(tmp_path, extra, tag):
    from srad_amd import main as Mn
    from srad_amd import options as Opt
    from srad_amd.checkpoint import Checkpoint
    from srad_amd.data import Data
    from srad_amd.loss import Loss
    from srad_amd.model import Model
    from srad_amd.trainer import Trainer
    args = Opt.parse_train_args(["--model-type", "drct", "--classe", "grid", "--resolution", "64", "--scale", "4", "--epochs", "1",
                                 "--batch-size", "2", "--no-augment", "--data-root", str(tmp_path / "data"),
                                 "--save-dir", str(tmp_path / f"exp{tag}")] + extra)
    opt = Mn.build_train_opt(args)
    opt.depths, opt.num_heads, opt.test_every, opt.print_every = (6,), (6,), 2, 1         # 1 RDG, 2 steps per epoch
    Mn.set_seed(opt.seed)
    ckp = Checkpoint(opt)
    loader = Data(opt, 0, 1)
    model = Model(opt, ckp)
    return opt, ckp, Trainer(opt, loader, model, Loss(opt, ckp), ckp)


def test_two_training_steps_with_an_msgms_term(tmp_path):
    from srad_amd.train import GraphedTrainStep
    _write_grid_class(tmp_path / "data", n_train=2, n_val=1, n_test=(1, 0), px=64)       # its defect patch wants 128 px: none
    # 1*L1, given or not: the graphed step, as before
    for tag, extra in enumerate(([], ["--loss", "1*L1"])):
        opt, ckp, t = _trainer(tmp_path, extra, tag)
        assert opt.loss == "1*L1" and isinstance(t.graph_step, GraphedTrainStep)
        ckp.done()
    opt, ckp, t = _trainer(tmp_path, ["--loss", "0.8*L1+0.2*MSGMS"], 2)
    assert opt.loss == "0.8*L1+0.2*MSGMS" and t.graph_step is None and t.drn_graph_step is None          # eager
    t.train()
    torch.cuda.synchronize()
    ckp.done()
    log = open(os.path.join(opt.save, "log.txt")).read()
    rows = re.findall(r"\[L1: ([0-9.]+)\]\[MSGMS: ([0-9.]+)\]\[Total: ([0-9.]+)\]", log)
    assert len(rows) == 2, log
    (l1a, ga, ta), (l1b, gb, tb) = [[float(v) for v in r] for r in rows]
    assert ga > 0 and abs(ta - (l1a + ga)) < 2e-4
    # both steps see the same two whole images (no augmentation, patch = image): the second row is the running mean of the
    # two steps, so it is below the first iff the second step's loss is
    assert tb < ta, rows
    assert torch.isfinite(t.net.flat_params).all()
