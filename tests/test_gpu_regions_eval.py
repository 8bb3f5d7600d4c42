"""GPU: the defect regions end to end - Detector.predict(regions=True), predict --save-regions, evaluate_on_test's region
metrics and evaluate --region-metrics - with a tiny random-weight model on synthetic images with planted defects.  Every table
is recomputed by tests/regions_ref.py from the masks and maps the run itself returned or saved; everything is equality."""
import csv

import numpy as np
import pytest
import torch
from PIL import Image

from srad_amd import spec as S
from tests import regions_ref as R
from tests.test_gpu_pixel_eval import _model as _eval_model, _pairs_and_masks, _write_prepared_tree
from tests.test_gpu_predict import HR, SCALE, SIZES, WS, _model as _predict_model, _raw_image

pytestmark = pytest.mark.gpu

REGION_KEYS = {"region_pred", "region_hit", "region_precision", "region_false_alarms", "false_alarms_per_image",
               "false_alarms_on_good", "region_gt", "region_found", "region_recall", "region_min_overlap"}


def _same_result(a, b):
    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), k
        elif isinstance(a[k], list) and a[k] and isinstance(a[k][0], torch.Tensor):
            assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), k
        else:
            assert a[k] == b[k], k


def test_detector_regions():
    from srad_amd import evaluate as E
    from srad_amd import predict as P
    opt, model, _ = _predict_model("drn-l", "grid")
    rng = np.random.RandomState(8)
    images = [_raw_image(rng, SIZES[k % 2], False, k >= 2) for k in range(5)]
    det = P.Detector(opt, model, E.MapSpec(ws=WS), threshold=float("inf"), min_area=2)
    det.threshold = float(torch.quantile(det.predict(images)["maps"].double().flatten(), 0.85))
    plain, again = det.predict(images), det.predict(images)
    _same_result(plain, again)                                      # the default path: the same keys and values, call after call
    got = det.predict(images, regions=True)
    assert list(got)[:len(plain)] == list(plain) and list(got)[len(plain):] == ["regions", "region_count"]
    _same_result({k: got[k] for k in plain}, plain)
    want = R.region_table_ref(got["masks"].cpu().numpy(), got["maps"].cpu().numpy(), None)
    assert want["n_regions"] > 1 and want["n_nan"] == 0
    R.assert_tables_equal(got["regions"], want, where="predict")
    assert got["region_count"] == np.bincount(want["image"], minlength=5).tolist() and sum(got["region_count"]) == want["n_regions"]
    assert int(got["regions"]["area"].min()) >= 2                   # the area filter came first
    per_image = np.bincount(want["image"], weights=want["area"], minlength=5).astype(np.int64).tolist()
    assert per_image == got["defect_pixels"]
    src = det.predict(images, source_frame=True, regions=True)
    assert set(src) - set(got) == {"maps_src", "masks_src", "src_box"}
    R.assert_tables_equal(src["regions"], want, where="predict, source frame")
    assert src["src_box"].shape == (want["n_regions"], 4)
    for k in range(want["n_regions"]):
        size = tuple(src["maps_src"][int(want["image"][k])].shape)
        box = P.source_box(want["box"][k].tolist(), (HR, HR), size)
        assert tuple(src["src_box"][k].tolist()) == box and box[0] <= box[2] < size[0] and box[1] <= box[3] < size[1]


def test_cli_save_regions(tmp_path, capsys):
    from srad_amd import predict as P
    rng = np.random.RandomState(9)
    raw = tmp_path / "raw"
    raw.mkdir()
    for k in range(4):
        Image.fromarray(_raw_image(rng, SIZES[k % 2], False, k >= 1)).save(raw / f"{k:03d}.png")
    cfg = S.DRNConfig.for_scale(SCALE, 1)
    sd = S.synth_state(S.drn_spec(cfg), seed=9, gain=0.4, cfg=cfg)
    ckpt = tmp_path / "model.pt"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, ckpt)
    common = ["--model-type", "drn-l", "--classe", "grid", "--resolution", str(HR), "--scale", str(SCALE), "--checkpoint", str(ckpt),
              "--dtype", "fp32", "--map-ws", str(WS), "--min-region-area", "2", "--input", str(raw)]
    probe = P.main(common + ["--threshold", "inf", "--output-dir", str(tmp_path / "probe")])
    t = float(torch.quantile(probe["maps"].double().flatten(), 0.85))
    a = P.main(common + [f"--threshold={t!r}", "--output-dir", str(tmp_path / "a")])
    b = P.main(common + [f"--threshold={t!r}", "--output-dir", str(tmp_path / "b"), "--save-regions", "--source-frame"])
    capsys.readouterr()
    assert "regions" not in a and not (tmp_path / "a" / "regions.csv").exists()
    assert (tmp_path / "a" / "predictions.csv").read_bytes() == (tmp_path / "b" / "predictions.csv").read_bytes()
    want = R.region_table_ref(b["masks"].cpu().numpy(), b["maps"].cpu().numpy(), None)
    assert want["n_regions"] > 1
    with open(tmp_path / "b" / "regions.csv", newline="") as fh:
        rows = list(csv.DictReader(fh))
    assert list(rows[0]) == ["name", "kind", "region", "area", "y0", "x0", "y1", "x1", "centroid_y", "centroid_x", "peak", "peak_y",
                             "peak_x", "src_y0", "src_x0", "src_y1", "src_x1"]
    assert len(rows) == want["n_regions"]
    seen = {}
    for k, r in enumerate(rows):
        i = int(want["image"][k])
        seen[i] = seen.get(i, -1) + 1
        assert r["name"] == b["names"][i] and r["kind"] == "bad" and int(r["region"]) == seen[i]
        assert [int(r[c]) for c in ("area", "y0", "x0", "y1", "x1")] == [int(want["area"][k])] + want["box"][k].tolist()
        assert float(r["centroid_y"]) == int(want["sum_y"][k]) / int(want["area"][k])
        assert float(r["centroid_x"]) == int(want["sum_x"][k]) / int(want["area"][k])
        assert float(r["peak"]) == float(want["peak"][k]) and [int(r["peak_y"]), int(r["peak_x"])] == [want["peak_y"][k], want["peak_x"][k]]
        assert [int(r[c]) for c in ("src_y0", "src_x0", "src_y1", "src_x1")] == b["src_box"][k].tolist()


def _reference_stats(M, pred, gt, y, min_overlap):
    ptab = R.region_table_ref(pred, None, gt)
    gtab = R.region_table_ref(gt, None, pred)
    return dict(M.region_stats(ptab, gtab, len(y), y, min_overlap), region_min_overlap=min_overlap), ptab


def test_evaluate_region_metrics(tmp_path, capsys):
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    scale, hr_size = 4, 64
    opt, model, _, _ = _eval_model("drn-l", hr_size, scale)
    y, good, bad, masks = _pairs_and_masks(3, 4, hr_size, scale, 1)
    names = [f"g{k}" for k in range(3)] + [f"b{k}" for k in range(4)]
    plain = E.evaluate_on_test(opt, model, good, bad)
    sr, hr = E.super_resolve_u8(model, [p[0] for p in good + bad], [p[1] for p in good + bad], float(opt.rgb_range))
    maps = M.anomaly_maps(sr, hr, plain["best_ws"])
    t = float(torch.quantile(maps.double().flatten(), 0.9))
    off = E.evaluate_on_test(opt, model, good, bad, masks=masks, operating_point=dict(threshold=t, min_area=2))
    capsys.readouterr()
    out_dir = tmp_path / "eval"
    spec = dict(threshold=t, min_area=2, save_masks=True, region_metrics=True, region_min_overlap=0.25, save_regions=True)
    got = E.evaluate_on_test(opt, model, good, bad, masks=masks, names=names, output_dir=str(out_dir), operating_point=spec)
    text = capsys.readouterr().out
    assert len([ln for ln in text.splitlines() if ln.startswith("Regions - ")]) == 1, text
    assert set(got) - set(off) == REGION_KEYS
    for k in off:
        assert got[k] == off[k], k
    pred = np.stack([np.array(Image.open(out_dir / "anomaly_masks" / ("good" if k < 3 else "bad") / f"{n}.png")) != 0
                     for k, n in enumerate(names)])
    gt = np.stack(masks) != 0
    want, ptab = _reference_stats(M, pred, gt, list(y), 0.25)
    assert want["region_pred"] > 0 and want["region_gt"] == 4
    assert {k: got[k] for k in REGION_KEYS} == want
    with open(out_dir / "regions.csv", newline="") as fh:
        rows = list(csv.DictReader(fh))
    assert len(rows) == ptab["n_regions"] and "gt_overlap" in rows[0] and "src_y0" not in rows[0]
    assert [int(r["gt_overlap"]) for r in rows] == ptab["overlap"].tolist()
    assert [r["name"] for r in rows] == [names[i] for i in ptab["image"]]
    assert [r["kind"] for r in rows] == ["good" if i < 3 else "bad" for i in ptab["image"]]
    assert [int(r["area"]) for r in rows] == ptab["area"].tolist()
    # an image without a mask: every image counts as all-ok, as for the pixel counts
    holey = list(masks)
    holey[-1] = None
    got = E.evaluate_on_test(opt, model, good, bad, masks=holey, operating_point=dict(spec, save_masks=False, save_regions=False))
    want, _ = _reference_stats(M, pred, np.zeros_like(gt), list(y), 0.25)
    assert {k: got[k] for k in REGION_KEYS} == want and want["region_gt"] == 0 and want["region_hit"] == 0
    with pytest.raises(ValueError, match="region_min_overlap"):
        E.evaluate_on_test(opt, model, good, bad, masks=masks, operating_point=dict(spec, region_min_overlap=2.0))


def test_cli_region_metrics(tmp_path, capsys):
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    size, scale = 64, 4
    root, out_dir = tmp_path / "data", tmp_path / "out"
    names = _write_prepared_tree(root, 3, 4, size, scale)
    cfg = S.DRNConfig.for_scale(scale, 1)
    sd = S.synth_state(S.drn_spec(cfg), seed=9, gain=0.4, cfg=cfg)
    ckpt = tmp_path / "model.pt"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, ckpt)
    common = ["--model-type", "drn-l", "--classe", "grid", "--scale", str(scale), "--resolution", str(size), "--data-root", str(root),
              "--checkpoint", str(ckpt), "--output-dir", str(out_dir), "--dtype", "fp32", "--map-ws", "7"]
    with pytest.raises(SystemExit):
        E.main(common + ["--region-metrics"])
    assert "--threshold" in capsys.readouterr().err
    t = repr(E.main(common + ["--pr-metrics"])["f1max_pixel_threshold"])      # a threshold at which something is predicted
    capsys.readouterr()
    out = E.main(common + [f"--threshold={t}", "--min-region-area", "2", "--save-masks", "--region-metrics",
                           "--region-min-overlap", "0.5", "--save-regions"])
    text = capsys.readouterr().out
    line = [ln for ln in text.splitlines() if ln.startswith("Regions - ")]
    assert len(line) == 1 and "min_overlap=0.5" in line[0], text
    pred = np.stack([np.array(Image.open(out_dir / "anomaly_masks" / split / f"{n}.png")) != 0 for split, n in names])
    gt = np.stack([np.array(Image.open(root / "grid" / "test" / "bad" / "GT" / f"{n}.png")) != 0 if split == "bad"
                   else np.zeros((size, size), bool) for split, n in names])
    want, ptab = _reference_stats(M, pred, gt, [int(split == "bad") for split, _ in names], 0.5)
    assert {k: out[k] for k in REGION_KEYS} == want and want["region_pred"] > 0 and want["region_gt"] == 4
    for k in ("region_pred", "region_hit", "region_false_alarms", "region_gt", "region_found"):
        word = dict(region_pred="predicted", region_hit="hit", region_false_alarms="false_alarms", region_gt="ground truth",
                    region_found="found")[k]
        assert f"{word}={out[k]}" in line[0], (k, line[0])
    with open(out_dir / "regions.csv", newline="") as fh:
        assert len(list(csv.DictReader(fh))) == ptab["n_regions"]
    E.main(common + [f"--threshold={t}"])                           # without the flag: no line, no keys
    assert "Regions - " not in capsys.readouterr().out
