"""GPU: the per-pixel baseline in the evaluator (evaluate_on_test(map_baseline=...), --map-baseline) and in predict
(Detector.fit_baseline, --baseline), on SR images the tests make themselves.  Everything is equality: the evaluator's numbers
against the same metrics on MapBaseline applied to spec.make of the same stacks, the threshold against map_threshold of the
leave-one-out maps, the saved maps against z / 16, and a detector reloaded from its written files against the one in the
process."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

from srad_amd import spec as S
from tests.test_gpu_pixel_eval import _model, _pairs_and_masks, _write_prepared_tree

pytestmark = pytest.mark.gpu

SIZE, SCALE = 64, 4
OP_KEYS = {"threshold", "threshold_source", "threshold_fpr", "threshold_level", "calib_images", "calib_rate", "min_region_area"}


def _stacks(E, opt, model, pairs):
    return E.super_resolve_u8(model, [p[0] for p in pairs], [p[1] for p in pairs], float(opt.rgb_range))


@pytest.mark.parametrize("model_type,source,level", [("drct", "ssim", "pixel"), ("drn-l", "mse", "image")])
def test_evaluator_equals_map_baseline_on_the_same_stacks(model_type, source, level, tmp_path, capsys):
    from srad_amd import baseline as B
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    opt, model, _, _ = _model(model_type, SIZE, SCALE)
    y, good, bad, masks = _pairs_and_masks(6, 8, SIZE, SCALE, 1)
    _, calib, _, _ = _pairs_and_masks(5, 0, SIZE, SCALE, 1, seed=21)
    names = [f"im{k:02d}" for k in range(14)]
    asked = dict(masks=masks, pixel_metrics=True, aupro=True, map_image_score=True, map_source=source, map_sigma=1.0)
    op = dict(fpr=0.01, level=level, min_area=2)
    # off: the call without the keyword, the call with None, and the printed lines are one and the same
    capsys.readouterr()
    plain = E.evaluate_on_test(opt, model, good, bad, operating_point=dict(op, calib=calib), **asked)
    text_plain = capsys.readouterr().out
    assert E.evaluate_on_test(opt, model, good, bad, operating_point=dict(op, calib=calib), map_baseline=None, **asked) == plain
    assert capsys.readouterr().out == text_plain and "baseline" not in text_plain and "map_baseline" not in plain
    assert OP_KEYS | {"map_ws", "map_sigma", "auc_map_max", "auc_pixel", "aupro", "pro_fpr_limit"} <= set(plain)
    # on
    got = E.evaluate_on_test(opt, model, good, bad, operating_point=op, names=names, output_dir=str(tmp_path), save_maps=True,
                             map_baseline=dict(calib=calib, floor_rel=0.2), **asked)
    text = capsys.readouterr().out
    assert set(got) - set(plain) == {"map_baseline"} and set(plain) <= set(got)
    for k in ("best_ws", "auc_ssim", "auc_mse", "auc_psnr", "n_images", "window_sizes", "map_ws", "map_sigma"):
        assert got[k] == plain[k], k
    # the same numbers from MapBaseline on spec.make of the same stacks
    spec = E._with_window(E.MapSpec(source=source, sigma=1.0).resolve(SIZE, SIZE), got["best_ws"], 1)
    sr, hr = _stacks(E, opt, model, good + bad)
    csr, chr_ = _stacks(E, opt, model, calib)
    cmaps, _ = spec.make(csr, chr_, False)
    bl = B.MapBaseline.fit(cmaps, 0.2)
    z, zmax = bl.apply(spec.make(sr, hr, False)[0], with_max=True)
    labels = torch.from_numpy(np.stack(masks)).cuda()
    assert got["map_baseline"] == bl.entries()["map_baseline"] and got["map_baseline"]["n_images"] == 5
    assert got["auc_pixel"] == M.pixel_roc_auc(z, labels) and got["aupro"] == M.aupro(z, labels)
    assert got["auc_map_max"] == M.roc_auc(y, zmax.double().cpu().numpy())
    loo, lmax = bl.apply_loo(cmaps, with_max=True)
    t, rate = M.map_threshold(lmax if level == "image" else loo, 0.01)
    assert got["threshold"] == t and got["calib_rate"] == rate and got["calib_images"] == 5 and got["threshold_level"] == level
    t_raw, _ = M.map_threshold(bl.apply(cmaps, with_max=True)[1 if level == "image" else 0], 0.01)
    assert t > t_raw                                           # in-sample scores would have set a lower bar
    pred, img_pred, counts = M.operating_point(z, t, labels, 2)
    for k, v in M.operating_point_stats(counts, img_pred, y).items():
        assert got[k] == v, k
    assert got["auc_pixel"] != plain["auc_pixel"] and got["threshold"] != plain["threshold"]
    # every printed map line says so, and only those
    note = " [baseline: 5 good images, floor 0.2]"
    lines = [ln for ln in text.splitlines() if " map (" in ln]
    assert len(lines) == 4 and all(note in ln for ln in lines), text
    assert [ln.split(" map (")[0] for ln in lines] == [ln.split(" map (")[0] for ln in text_plain.splitlines() if " map (" in ln]
    assert all(ln.split(")", 1)[1].startswith(note) for ln in lines)
    assert sum(note in ln for ln in text.splitlines()) == 4
    # the saved maps: z / 16 through the evaluator's converter
    want = M.to_u8_hwc((z * (1.0 / B.SAVED_MAP_SIGMAS))[:, None], rgb_range=1.0).cpu().numpy()[..., 0]
    assert B.SAVED_MAP_SIGMAS == 16.0 and want.max() > 0
    for k, name in enumerate(names):
        a = np.array(Image.open(tmp_path / "anomaly_maps" / ("good" if k < 6 else "bad") / f"{name}.png"))
        assert np.array_equal(a, want[k]), name
    # fewer than three calibration images are refused before any work
    with pytest.raises(ValueError, match="at least 3"):
        E.evaluate_on_test(opt, None, good, bad, map_baseline=dict(calib=calib[:2]), **asked)


def test_cli_map_baseline(tmp_path, capsys):
    from srad_amd import evaluate as E
    root, out = tmp_path / "data", tmp_path / "out"
    _write_prepared_tree(root, 3, 4, SIZE, SCALE)
    _, calib, _, _ = _pairs_and_masks(4, 0, SIZE, SCALE, 1, seed=21)
    for k, (lr, hr) in enumerate(calib):                       # val/good, as prepare_mvtec_data writes it
        lr2 = hr.reshape(SIZE // 2, 2, SIZE // 2, 2, 1).astype(np.float32).mean((1, 3)).round().astype(np.uint8)
        for sub, img in (("HR", hr), ("LR_2", lr2), (f"LR_{SCALE}", lr)):
            d = root / "grid" / "val" / "good" / sub
            d.mkdir(parents=True, exist_ok=True)
            Image.fromarray(img[:, :, 0]).save(d / f"{k:03d}.png")
    cfg = S.DRNConfig.for_scale(SCALE, 1)
    sd = S.synth_state(S.drn_spec(cfg), seed=9, gain=0.4, cfg=cfg)
    ckpt = tmp_path / "model.pt"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, ckpt)
    common = ["--model-type", "drn-l", "--classe", "grid", "--scale", str(SCALE), "--resolution", str(SIZE), "--data-root", str(root),
              "--checkpoint", str(ckpt), "--output-dir", str(out), "--dtype", "fp32", "--map-ws", "7", "--pixel-metrics"]
    off = E.main(common + ["--threshold-fpr", "0.01"])
    capsys.readouterr()
    on = E.main(common + ["--threshold-fpr", "0.01", "--map-baseline", "--baseline-floor", "0.25"])
    text = capsys.readouterr().out
    assert set(on) - set(off) == {"map_baseline"} and on["map_baseline"]["n_images"] == 4 and on["map_baseline"]["floor_rel"] == 0.25
    assert on["calib_images"] == 4 and on["threshold"] != off["threshold"]
    assert f"Pixel AUC - SSIM map (ws=7) [baseline: 4 good images, floor 0.25]: {on['auc_pixel']:.4f}" in text.splitlines()
    # the same through the keyword, where one super-resolve pass of the calibration images serves both
    only = E.main(common + ["--map-baseline"])
    assert only["map_baseline"] == dict(on["map_baseline"], floor_rel=0.1, floor=only["map_baseline"]["floor"]) and "threshold" not in only
    for f in (root / "grid" / "val" / "good" / "HR").glob("00[23].png"):
        f.unlink()
    with pytest.raises(SystemExit) as e:
        E.main(common + ["--map-baseline"])
    assert "fewer than 3" in str(e.value)


def test_detector_round_trip_through_the_written_files(tmp_path, capsys):
    from srad_amd import baseline as B
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    from srad_amd import predict as P
    from tests.test_gpu_predict import HR, SCALE as PSCALE, WS, _model as _pmodel, _raw_image
    rng = np.random.RandomState(8)
    good_dir, test_dir = tmp_path / "raw" / "good", tmp_path / "raw" / "test"
    good_dir.mkdir(parents=True)
    test_dir.mkdir(parents=True)
    for k in range(5):
        Image.fromarray(_raw_image(rng, (64, 64) if k % 2 else (80, 96), False, False)).save(good_dir / f"{k:03d}.png")
    for k in range(3):
        Image.fromarray(_raw_image(rng, (64, 64), False, k > 0)).save(test_dir / f"{k:03d}.png")
    good_files, test_files = sorted(good_dir.iterdir()), sorted(test_dir.iterdir())
    # in the process
    opt, model, sd = _pmodel("drn-l", "grid")
    det = P.Detector(opt, model, E.MapSpec(ws=WS), min_area=2)
    with pytest.raises(ValueError, match="at least 3"):
        det.fit_baseline(good_files[:2])
    fitted = det.fit_baseline(good_files, 0.1)
    assert fitted is det.baseline and fitted.n == 5 and fitted.shape == (HR, HR)
    with pytest.raises(ValueError, match="fitted on"):
        det.calibrate(good_files[:4], 0.05)
    t, achieved = det.calibrate(good_files, 0.05)
    _, _, raw, _, _ = det._maps(good_files, False, raw=True)
    assert (t, achieved) == M.map_threshold(fitted.apply_loo(raw), 0.05)
    res = det.predict(test_files)
    _, _, raw_t, _, _ = det._maps(test_files, False, raw=True)
    z, zmax = fitted.apply(raw_t, with_max=True)
    assert torch.equal(res["maps"], z) and res["map_max"] == zmax.tolist() and (z < 0).any()
    assert torch.equal(res["masks"], M.operating_point(z, t, None, 2)[0])
    # through the files
    run = tmp_path / "drn-l" / f"mvtec_grid_{HR}_X{PSCALE}"
    (run / "model").mkdir(parents=True)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, run / "model" / "model_best.pt")
    common = ["--run-dir", str(run), "--dtype", "fp32"]
    out = P.main(common + ["--calibrate", str(good_dir), "--threshold-fpr", "0.05", "--min-region-area", "2", "--map-ws", str(WS), "--baseline"])
    doc = json.loads((run / "operating_point.json").read_text())
    npz = run / "map_baseline.npz"
    assert out["operating_point"] == doc and doc["threshold"] == t and doc["calib_rate"] == achieved
    assert doc["baseline"] == dict(file="map_baseline.npz", n_images=5, floor_rel=0.1, floor=fitted.floor, sha256=B.file_sha256(npz))
    assert doc["map_spec"] == dict(source="ssim", ws=WS, scales=[], reduce="mean", sigma=0.0) and list(doc)[-1] == "baseline"
    assert "Calibrated - SSIM map (ws=7) [baseline: 5 good images, floor 0.1], threshold=" in capsys.readouterr().out
    inputs = ["--input", str(test_dir)]
    again = P.main(common + inputs + ["--save-anomaly-maps", "--output-dir", str(tmp_path / "out")])
    assert again["threshold"] == t and torch.equal(again["maps"], res["maps"]) and torch.equal(again["masks"], res["masks"])
    assert again["map_max"] == res["map_max"] and again["defective"] == res["defective"]
    assert "Predicted - SSIM map (ws=7) [baseline: 5 good images, floor 0.1], threshold=" in capsys.readouterr().out
    want = M.to_u8_hwc((z * (1.0 / 16.0))[:, None], rgb_range=1.0).cpu().numpy()[..., 0]
    for k, name in enumerate(again["names"]):
        kind = "bad" if again["defective"][k] else "good"
        assert np.array_equal(np.array(Image.open(tmp_path / "out" / "anomaly_maps" / kind / f"{name}.png")), want[k])
    # a given threshold with --baseline reads the run's file; without it the maps are the raw ones
    given = P.main(common + inputs + ["--threshold", "4", "--baseline", "--map-ws", str(WS)])
    assert given["threshold"] == 4.0 and torch.equal(given["maps"], res["maps"])
    assert torch.equal(P.main(common + inputs + ["--threshold", "4", "--map-ws", str(WS)])["maps"], raw_t)
    # another frame, another spec, a corrupted file: refused
    with pytest.raises(SystemExit) as e:
        P.main(common + inputs + ["--threshold", "4", "--baseline", "--map-ws", "5"])
    assert "other maps" in str(e.value)
    data = bytearray(npz.read_bytes())
    data[len(data) // 2] ^= 0x01
    npz.write_bytes(bytes(data))
    with pytest.raises(SystemExit) as e:
        P.main(common + inputs)
    assert "sha256" in str(e.value)
