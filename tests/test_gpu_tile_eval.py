"""GPU: tiled inference (DESIGN.md "Tiled inference") through the evaluator and predict.  The evaluator's numbers equal the
same metrics on SR images the test makes itself with the tiled ``Model``; a ``Detector`` with a rectangular frame works in that
frame from ``prepare`` to the source-frame renderings; the command line round-trips the ``tile`` and ``frame`` entries of
operating_point.json and refuses flags that contradict them.  Everything is equality."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

from srad_amd import spec as S
from tests.test_gpu_eval import _pairs
from tests.test_gpu_tile_model import _drct_model

pytestmark = pytest.mark.gpu


def test_evaluator_numbers_are_those_of_the_tiled_model(capsys):
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    m = _drct_model(8, 2, "feather")
    opt = m.opt
    y, good, bad = _pairs(6, 8, 64, 4, 1)
    pairs = good + bad
    got = E.evaluate_on_test(opt, m, good, bad)
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Test AUCs")][-1]
    assert line.endswith("(tiles 8/2 feather)") and got["tile"] == [8, 2, "feather"]
    with torch.no_grad():                                     # the SR images made here: the evaluator's batches through the tiled Model
        x = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda().permute(0, 3, 1, 2).float() * (float(opt.rgb_range) / 255.0)
        assert len(pairs) <= 64                               # one outer batch at 16 x 16 LR pixels
        sr = M.to_u8_hwc(m(x), float(opt.rgb_range))
        plain = M.to_u8_hwc(m.model(x), float(opt.rgb_range))
    hr = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    assert not torch.equal(sr, plain)                         # tiling changes the images, so the comparison below means something
    ref = M.evaluate_pairs(y, sr, hr)
    for k in ("best_ws", "window_sizes", "auc_ssim", "auc_mse", "auc_psnr"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    sr2, _ = E.super_resolve_u8(m, [p[0] for p in pairs], [p[1] for p in pairs], float(opt.rgb_range))
    assert torch.equal(sr2, sr)
    # off: no suffix, no key, and the result of the model without the setting
    off_model = _drct_model(0)
    off = E.evaluate_on_test(off_model.opt, off_model, good, bad)
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Test AUCs")][-1]
    assert "tiles" not in line and "tile" not in off
    assert {k: v for k, v in got.items() if k != "tile"}.keys() == off.keys()


def _source(rng, h, w, defect):
    yy, xx = np.mgrid[0:h, 0:w]
    a = 120 + 60 * np.sin(xx / 3.1) * np.cos(yy / 4.3) + rng.normal(0, 6, (h, w))
    if defect:
        a[h // 2 - 8:h // 2 + 8, w // 3 - 12:w // 3 + 12] = 250 - a[h // 2 - 8:h // 2 + 8, w // 3 - 12:w // 3 + 12]
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def test_detector_with_a_rectangular_frame():
    from srad_amd import evaluate as E
    from srad_amd import predict as P
    rng = np.random.RandomState(8)
    good = [_source(rng, 100, 300, False) for _ in range(3)]
    images = [_source(rng, 100, 300, True), _source(rng, 100, 300, False), _source(rng, 60, 90, True)]
    # without tiling the network's own refusal stands: LR 12 x 20 is a multiple of window 4, LR 13 x 20 is not
    plain = _drct_model(0)
    with pytest.raises(ValueError, match="multiple of the window"):
        P.Detector(plain.opt, plain, E.MapSpec(ws=7), hr_size=(52, 80), threshold=0.5).predict(images)
    m = _drct_model(8, 2, "mean")
    for frame in ((48, 80), (52, 81)):                        # LR 12 x 20, and 13 x 20: any frame with tiling
        det = P.Detector(m.opt, m, E.MapSpec(ws=7), hr_size=frame, min_area=2)
        H, W = frame[0] // 4 * 4, frame[1] // 4 * 4
        lr, hr = det.prepare(images)
        assert tuple(lr.shape) == (3, 1, H // 4, W // 4) and lr.dtype == torch.float32
        assert tuple(hr.shape) == (3, H, W, 1) and hr.dtype == torch.uint8
        table = P.luma_table()
        for i, a in enumerate(images):                        # Pillow's own resizes, then the loader's luma
            hr_pil = Image.fromarray(a).convert("RGB").resize((frame[1], frame[0]), Image.LANCZOS)
            lr_pil = hr_pil.resize((frame[1] // 4, frame[0] // 4), Image.LANCZOS)
            assert np.array_equal(hr[i, :, :, 0].cpu().numpy(), table.astype(np.uint8)[np.asarray(hr_pil)[:H, :W, 0]]), (frame, i)
            assert np.array_equal(lr[i, 0].cpu().numpy(), table[np.asarray(lr_pil)[..., 0]]), (frame, i)
        t, _ = det.calibrate(good, 0.2, "pixel")              # a loose threshold: there are regions to place in the sources
        res = det.predict(images, source_frame=True, regions=True)
        assert tuple(res["maps"].shape) == (3, H, W) == tuple(res["masks"].shape) and tuple(res["sr"].shape) == (3, H, W, 1)
        assert [tuple(v.shape) for v in res["maps_src"]] == [(100, 300), (100, 300), (60, 90)] == [tuple(v.shape) for v in res["masks_src"]]
        assert sum(res["region_count"]) >= 1
        table_r = res["regions"]
        sizes = [(100, 300), (100, 300), (60, 90)]
        want = [P.source_box(b, (H, W), sizes[i]) for i, b in zip(table_r["image"].tolist(), table_r["box"].tolist())]
        assert res["src_box"].tolist() == [list(b) for b in want] and len(want) == sum(res["region_count"])
        for (y0, x0, y1, x1), i in zip(want, table_r["image"].tolist()):
            assert 0 <= y0 <= y1 < sizes[i][0] and 0 <= x0 <= x1 < sizes[i][1]
        # the SR images are the tiled Model's
        with torch.no_grad():
            sr = E.super_resolve_dev(m, lr, (H, W), float(m.opt.rgb_range))
        assert torch.equal(res["sr"], sr)


def test_cli_round_trips_tile_and_frame(tmp_path, capsys):
    from srad_amd import predict as P
    rng = np.random.RandomState(9)
    for folder, n, defect in (("good", 4, False), ("new", 3, True)):
        (tmp_path / folder).mkdir()
        for k in range(n):
            Image.fromarray(_source(rng, 100, 300, defect and k != 1)).save(tmp_path / folder / f"{k:03d}.png")
    run = tmp_path / "drn-l" / "mvtec_grid_32_X4"
    (run / "model").mkdir(parents=True)
    cfg = S.DRNConfig.for_scale(4, 1)
    sd = S.synth_state(S.drn_spec(cfg), seed=9, gain=0.4, cfg=cfg)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, run / "model" / "model_best.pt")
    common = ["--run-dir", str(run), "--dtype", "fp32"]
    tiling = ["--tile", "8", "--tile-overlap", "3", "--tile-blend", "feather", "--frame", "48", "80"]
    out = P.main(common + tiling + ["--calibrate", str(tmp_path / "good"), "--threshold-fpr", "0.05", "--map-ws", "7"])
    doc = json.loads((run / "operating_point.json").read_text())
    assert out["operating_point"] == doc and doc["tile"] == [8, 3, "feather"] and doc["frame"] == [48, 80]
    capsys.readouterr()
    inputs = ["--input", str(tmp_path / "new"), "--output-dir", str(tmp_path / "out")]
    res = P.main(common + inputs)                             # the file's setting is taken
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Predicted - ")][-1]
    assert line.endswith("(tiles 8/3 feather)") and tuple(res["maps"].shape) == (3, 48, 80)
    same = P.main(common + inputs + tiling)                   # the same flags pass
    assert torch.equal(same["maps"], res["maps"]) and same["threshold"] == doc["threshold"]
    for flags, what in ((["--tile", "16"], "--tile 16"), (["--tile", "8", "--tile-overlap", "3"], "--tile 8"), (["--frame", "80", "48"], "--frame 80 48")):
        with pytest.raises(SystemExit) as e:
            P.main(common + inputs + flags)
        assert what in str(e.value) and "contradicts the calibrated operating point" in str(e.value)
    # with a given threshold the flags stand on their own: whole images in the square frame, no suffix
    whole = P.main(common + inputs + ["--threshold", "0.5"])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Predicted - ")][-1]
    assert "tiles" not in line and tuple(whole["maps"].shape) == (3, 32, 32)
