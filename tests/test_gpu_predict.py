"""GPU: srad_amd.predict end to end against the project's own evaluator.  Raw PNGs of two source sizes (96x80 and 64x64; gray
for grid, true colour for carpet, plus one image of the other kind in each) go through prepare_mvtec_data into a prepared tree
(hr 32, scale 4); then, with synthetic weights, Detector.prepare of the RAW files must equal iter_split of the PREPARED tree
(LR as float32 bits, HR bytes), predict's maps must equal the maps recomputed the evaluator's way and the ones
evaluate_on_test saves, defective must equal the operating point's image prediction, and calibrate on the raw train/good
images must equal --threshold-fpr on the prepared val/good tree holding the same images.  Then the CLI: calibrate, predict,
the CSV, the saved masks, the JSON honoured, a contradicting flag refused.  Everything is equality; there is no tolerance."""
import csv
import json

import numpy as np
import pytest
import torch
from PIL import Image

from srad_amd import spec as S

pytestmark = pytest.mark.gpu

HR, SCALE, WS = 32, 4, 7
SIZES = ((80, 96), (64, 64))                                   # (height, width) of the raw sources: 96x80 and 64x64


def _raw_image(rng, shape, colour, defect):
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    base = 120 + 60 * np.sin(xx / 3.1) * np.cos(yy / 4.3)
    chans = [base + rng.normal(0, 6, shape) + 25 * c for c in range(3 if colour else 1)]
    a = np.stack(chans, axis=2)
    if defect:
        cy, cx = rng.randint(h // 4, 3 * h // 4), rng.randint(w // 4, 3 * w // 4)
        a[cy - 6:cy + 6, cx - 6:cx + 6] = 250 - a[cy - 6:cy + 6, cx - 6:cx + 6]
    a = np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return a if colour else a[..., 0]


def _write_raw(root, cls, colour):
    """<root>/<cls>/train/good, test/good, test/crack: MVTec's own layout.  Image 1 of every folder is of the other kind."""
    rng = np.random.RandomState(3 if colour else 4)
    for folder, n, defect in (("train/good", 5, False), ("test/good", 3, False), ("test/crack", 4, True)):
        d = root / cls / folder
        d.mkdir(parents=True)
        for k in range(n):
            Image.fromarray(_raw_image(rng, SIZES[k % 2], colour != (k == 1), defect)).save(d / f"{k:03d}.png")


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    from srad_amd import prepare_mvtec_data as Prep
    raw, prepared = tmp_path_factory.mktemp("raw"), tmp_path_factory.mktemp("prepared")
    for cls, colour in (("grid", False), ("carpet", True)):
        _write_raw(raw, cls, colour)
        Prep.process_test_data(raw / cls / "test", prepared / cls / "test", (2, SCALE), target_hr=(HR, HR))
        Prep.process_training_data(raw / cls / "train" / "good", prepared / cls / "train", prepared / cls / "val", (2, SCALE),
                                   target_hr=(HR, HR), val_ratio=1.0)       # every train/good image lands in val/good
    return raw, prepared


def _model(model_type, cls):
    from srad_amd import options as Opt
    from srad_amd.model import Model
    opt = Opt.build_opt(model_type, cls, HR, SCALE)
    opt.use_graph = False
    if model_type == "drct":
        opt.depths, opt.num_heads = (6,), (6,)
        cfg = S.DRCTConfig(in_chans=opt.n_colors, img_size=HR // SCALE, window_size=2, upscale=SCALE, n_rdg=1)
        sd = S.synth_state(S.drct_spec(cfg), seed=9, gain=0.7, cfg=cfg)
    else:
        cfg = S.DRNConfig.for_scale(SCALE, opt.n_colors)
        sd = S.synth_state(S.drn_spec(cfg), seed=9, gain=0.4, cfg=cfg)
    model = Model(opt, None, dual_model=(model_type == "drn-l"))
    model.get_model().load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return opt, model, sd


def _split(prepared, raw, cls, opt, split, part="test"):
    """(items of iter_split, the raw file each of them was made from)."""
    from srad_amd import evaluate as E
    items = list(E.iter_split(str(prepared), cls, split, opt.scale, opt.n_colors, part=part))
    folder = raw / cls / ("train/good" if part == "val" else "test/good" if split == "good" else "test/crack")
    return items, [folder / f"{name.replace('crack_', '')}.png" for name, _, _ in items]


@pytest.mark.parametrize("cls", ["grid", "carpet"])
@pytest.mark.parametrize("model_type", ["drct", "drn-l"])
def test_detector_equals_the_evaluator_on_the_prepared_tree(trees, model_type, cls, tmp_path):
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    from srad_amd import predict as P
    raw, prepared = trees
    opt, model, _ = _model(model_type, cls)
    good, good_files = _split(prepared, raw, cls, opt, "good")
    bad, bad_files = _split(prepared, raw, cls, opt, "bad")
    val, val_files = _split(prepared, raw, cls, opt, "good", part="val")
    assert (len(good), len(bad), len(val)) == (3, 4, 5)
    items, files = good + bad, good_files + bad_files
    det = P.Detector(opt, model, E.MapSpec(ws=WS), min_area=2)
    # 1. the pair: float32 bits of the LR images, bytes of the HR images - from files and from arrays alike
    for sources in (files, [np.array(Image.open(f)) for f in files]):
        lr, hr = det.prepare(sources)
        assert lr.dtype == torch.float32 and tuple(lr.shape) == (7, opt.n_colors, HR // SCALE, HR // SCALE)
        assert hr.dtype == torch.uint8 and tuple(hr.shape) == (7, HR, HR, opt.n_colors)
        lr_h, hr_h = lr.permute(0, 2, 3, 1).cpu().numpy(), hr.cpu().numpy()
        for k, (name, lr_ref, hr_ref) in enumerate(items):
            assert np.array_equal(lr_h[k].view(np.uint32), np.asarray(lr_ref, dtype=np.float32).view(np.uint32)), (name, "LR")
            assert np.array_equal(hr_h[k], hr_ref), (name, "HR")
    if cls == "grid":
        assert items[0][1].dtype == np.float32                 # the luma of a prepared gray image is not integral: the table matters
    # 2. calibrate on the raw train/good images = --threshold-fpr on the prepared val/good tree
    pairs = lambda its: [(lr_, hr_) for _, lr_, hr_ in its]
    names = [n for n, _, _ in items]
    for level in ("pixel", "image"):
        t, achieved = det.calibrate(val_files, 0.05, level)
        ref = E.evaluate_on_test(opt, model, pairs(good), pairs(bad), map_ws=WS,
                                 operating_point=E.OperatingPoint(fpr=0.05, level=level, calib=pairs(val), min_area=2))
        assert ref["threshold"] == t and ref["calib_rate"] == achieved and ref["calib_images"] == 5 and det.threshold == t, level
    # 3. predict at that threshold: the maps are the evaluator's, recomputed and as it saves them; defective is its image prediction
    res = det.predict(files)
    sr, hr = E.super_resolve_u8(model, [p[0] for p in pairs(items)], [p[1] for p in pairs(items)], float(opt.rgb_range))
    maps = M.anomaly_maps(sr, hr, WS)
    assert torch.equal(res["sr"], sr) and torch.equal(res["hr"], hr)
    assert res["maps"].dtype == torch.float32 and torch.equal(res["maps"], maps)
    pred, img_pred, _ = M.operating_point(maps, t, None, 2)
    assert torch.equal(res["masks"], pred) and res["defect_pixels"] == img_pred.tolist()
    assert res["defective"] == [v > 0 for v in img_pred.tolist()] and res["map_max"] == maps.amax((1, 2)).tolist()
    ssim, mse, psnr = M.score_pairs(sr, hr, [WS])
    assert res["ssim"] == ssim[:, 0].tolist() and res["mse"] == mse.tolist() and res["psnr"] == psnr.tolist()
    out_dir = tmp_path / "eval"
    ref = E.evaluate_on_test(opt, model, pairs(good), pairs(bad), names=names, output_dir=str(out_dir), save_maps=True, map_ws=WS,
                             operating_point=dict(threshold=t, min_area=2, save_masks=True))
    assert ref["image_fp"] == sum(res["defective"][:3]) and ref["image_tp"] == sum(res["defective"][3:]) and ref["map_ws"] == WS
    maps_u8 = M.to_u8_hwc(res["maps"][:, None], rgb_range=1.0).cpu().numpy()[..., 0]
    for k, name in enumerate(names):
        split = "good" if k < 3 else "bad"
        assert np.array_equal(np.array(Image.open(out_dir / "anomaly_maps" / split / f"{name}.png")), maps_u8[k]), name
        assert np.array_equal(np.array(Image.open(out_dir / "anomaly_masks" / split / f"{name}.png")), res["masks"][k].cpu().numpy() * 255), name
    # mixed sizes in another order give the same rows
    order = [5, 0, 3, 6, 1]
    again = det.predict([files[i] for i in order])
    assert torch.equal(again["maps"], res["maps"][order]) and again["defect_pixels"] == [res["defect_pixels"][i] for i in order]
    # the self-ensemble goes the evaluator's way too
    det8 = P.Detector(opt, model, E.MapSpec(source="mse", ws=0, sigma=1.0), threshold=0.01, self_ensemble=True)
    sr8, _ = E.super_resolve_u8(model, [p[0] for p in pairs(items)], [p[1] for p in pairs(items)], float(opt.rgb_range), self_ensemble=True)
    res8 = det8.predict(files)
    assert torch.equal(res8["sr"], sr8) and torch.equal(res8["maps"], M.smooth_maps(M.error_maps(sr8, hr, 1), 1.0))
    with pytest.raises(ValueError, match="no threshold"):
        P.Detector(opt, model, E.MapSpec(ws=WS)).predict(files)


def test_cli_calibrate_then_predict(trees, tmp_path, capsys):
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    from srad_amd import predict as P
    raw, prepared = trees
    run = tmp_path / "drn-l" / f"mvtec_grid_{HR}_X{SCALE}"
    (run / "model").mkdir(parents=True)
    cfg = S.DRNConfig.for_scale(SCALE, 1)
    sd = S.synth_state(S.drn_spec(cfg), seed=9, gain=0.4, cfg=cfg)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, run / "model" / "model_best.pt")
    common = ["--run-dir", str(run), "--dtype", "fp32"]
    inputs = ["--input", str(raw / "grid" / "test" / "good"), str(raw / "grid" / "test" / "crack")]
    with pytest.raises(SystemExit) as e:                                    # nothing calibrated yet, no --threshold
        P.main(common + inputs)
    assert "operating_point.json" in str(e.value)
    out = P.main(common + ["--calibrate", str(raw / "grid" / "train" / "good"), "--threshold-fpr", "0.05", "--min-region-area", "2",
                           "--map-ws", str(WS)])
    doc = json.loads((run / "operating_point.json").read_text())
    assert out["operating_point"] == doc and doc["calib_images"] == 5 and doc["min_region_area"] == 2 and doc["checkpoint"] == "model_best.pt"
    assert doc["map_spec"] == dict(source="ssim", ws=WS, scales=[], reduce="mean", sigma=0.0) and doc["self_ensemble"] is False
    assert doc["calib_rate"] <= 0.05 and "Calibrated - SSIM map (ws=7)" in capsys.readouterr().out
    # the same threshold as the evaluator's own CLI calibrates on the prepared val/good tree
    ref = E.main(["--model-type", "drn-l", "--classe", "grid", "--scale", str(SCALE), "--resolution", str(HR), "--data-root", str(prepared),
                  "--checkpoint", str(run / "model" / "model_best.pt"), "--output-dir", str(tmp_path / "eval"), "--dtype", "fp32",
                  "--threshold-fpr", "0.05", "--min-region-area", "2", "--map-ws", str(WS)])
    assert ref["threshold"] == doc["threshold"] and ref["calib_rate"] == doc["calib_rate"]
    capsys.readouterr()
    # predict: the file is honoured (threshold, window, area filter), a contradicting flag is refused
    with pytest.raises(SystemExit) as e:
        P.main(common + inputs + ["--map-ws", "5"])
    assert "--map-ws 5 contradicts" in str(e.value)
    out_dir = tmp_path / "out"
    res = P.main(common + inputs + ["--save-masks", "--save-anomaly-maps", "--output-dir", str(out_dir), "--map-ws", str(WS)])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Predicted - ")]
    assert len(line) == 1 and f"{sum(res['defective'])} of 7 images defective" in line[0] and "min_area=2" in line[0]
    assert res["threshold"] == doc["threshold"] and res["names"] == ["000", "001", "002", "000_2", "001_2", "002_2", "003"]
    opt, model, _ = _model("drn-l", "grid")
    items = _split(prepared, raw, "grid", opt, "good")[0] + _split(prepared, raw, "grid", opt, "bad")[0]
    sr, hr = E.super_resolve_u8(model, [lr for _, lr, _ in items], [h for _, _, h in items], float(opt.rgb_range))
    maps = M.anomaly_maps(sr, hr, WS)
    pred, img_pred, _ = M.operating_point(maps, doc["threshold"], None, 2)
    assert torch.equal(res["maps"], maps) and torch.equal(res["masks"], pred)
    with open(out_dir / "predictions.csv", newline="") as fh:
        rows = list(csv.DictReader(fh))
    assert [r["name"] for r in rows] == res["names"] and len(rows) == 7
    for k, r in enumerate(rows):
        assert int(r["defective"]) == int(img_pred[k] > 0) and int(r["defect_pixels"]) == int(img_pred[k])
        assert float(r["map_max"]) == float(maps[k].max()) and float(r["threshold"]) == doc["threshold"]
        assert float(r["ssim"]) == res["ssim"][k] and float(r["mse"]) == res["mse"][k] and float(r["psnr"]) == res["psnr"][k]
        kind = "bad" if img_pred[k] > 0 else "good"
        a = np.array(Image.open(out_dir / "anomaly_masks" / kind / f"{r['name']}.png"))
        assert a.dtype == np.uint8 and np.array_equal(a, pred[k].cpu().numpy() * 255), r["name"]
        assert (out_dir / "anomaly_maps" / kind / f"{r['name']}.png").is_file()
    assert len(list((out_dir / "anomaly_masks").rglob("*.png"))) == 7
    # a given threshold needs no file; +inf flags nothing
    res = P.main(["--model-type", "drn-l", "--classe", "grid", "--resolution", str(HR), "--scale", str(SCALE), "--checkpoint",
                  str(run / "model" / "model_best.pt"), "--dtype", "fp32", "--threshold", "inf", "--output-dir", str(tmp_path / "out2")] + inputs)
    assert res["defective"] == [False] * 7 and res["defect_pixels"] == [0] * 7
