"""GPU: predict's source-frame outputs, on the raw trees and synthetic models of tests/test_gpu_predict.py (sources of 96 x 80
and 64 x 64, gray and true colour, HR 32).  ``predict(files)`` and ``predict(files, source_frame=True, overlays=True)`` agree on
every old key; every ``maps_src[i]`` has its source's shape and equals Pillow's bilinear mode-F resize of ``maps[i]`` on the
bits; every ``masks_src[i]`` equals that resize of the float mask at >= 0.5; every overlay equals the numpy index loop on the
raw source.  Then the CLI: the PNGs exist, have the source sizes and decode to those arrays, the overlay's options arrive, and
``predictions.csv`` and ``operating_point.json`` are byte for byte what a run without the new flags writes.  Everything is
equality; there is no tolerance."""
import numpy as np
import pytest
import torch
from PIL import Image

from srad_amd import spec as S
from tests.overlay_ref import overlay_ref
from tests.test_gpu_predict import HR, SCALE, SIZES, WS, _model, _split, trees  # noqa: F401  (trees: the module's fixture)
from tests.test_resample_f_host import bits, pil_resize_f

pytestmark = pytest.mark.gpu

WHITE = (255, 255, 255)


def _expected(P, source, map_, mask, lut, scale, radius):
    """(map, mask, overlay) at the size of ``source`` from the model-frame ``map_`` and ``mask`` (numpy), Pillow's and numpy's way."""
    H, W = source.shape[:2]
    m = pil_resize_f(map_, H, W, "bilinear")
    k = (pil_resize_f(mask.astype(np.float32), H, W, "bilinear") >= 0.5).astype(np.uint8)
    src = source[None, :, :, None] if source.ndim == 2 else source[None]
    return m, k, overlay_ref(src, m[None], k[None], lut, scale, radius, WHITE)[0]


@pytest.mark.parametrize("model_type,cls", [("drct", "grid"), ("drn-l", "carpet")])
def test_source_frame_outputs(trees, model_type, cls):
    from srad_amd import evaluate as E
    from srad_amd import predict as P
    raw, prepared = trees
    opt, model, _ = _model(model_type, cls)
    files = _split(prepared, raw, cls, opt, "good")[1] + _split(prepared, raw, cls, opt, "bad")[1]
    val_files = _split(prepared, raw, cls, opt, "good", part="val")[1]
    det = P.Detector(opt, model, E.MapSpec(ws=WS), min_area=2)
    t, _ = det.calibrate(val_files, 0.05, "pixel")
    old = det.predict(files)
    res = det.predict(files, source_frame=True, overlays=True)
    assert set(res) == set(old) | {"maps_src", "masks_src", "overlays"}
    for key, value in old.items():
        assert torch.equal(res[key], value) if torch.is_tensor(value) else res[key] == value, key
    only = det.predict(files, source_frame=True)
    assert set(only) == set(old) | {"maps_src", "masks_src"}
    assert sum(old["defect_pixels"]) > 0                       # there is something to outline
    sources = [P.as_source(f) for f in files]
    assert {s.shape[:2] for s in sources} == set(SIZES) and {s.ndim for s in sources} == {2, 3}       # both sizes, gray and colour
    maps, masks = old["maps"].cpu().numpy(), old["masks"].cpu().numpy()
    lut, scale = P.heat_lut(153), P.overlay_scale(t)
    outlined = 0
    for i, source in enumerate(sources):
        m, k, o = _expected(P, source, maps[i], masks[i], lut, scale, 1)
        for r in (res, only):
            assert r["maps_src"][i].dtype == torch.float32 and tuple(r["maps_src"][i].shape) == source.shape[:2], i
            assert np.array_equal(bits(r["maps_src"][i].cpu().numpy()), bits(m)), i
            assert r["masks_src"][i].dtype == torch.uint8 and np.array_equal(r["masks_src"][i].cpu().numpy(), k), i
        assert res["overlays"][i].dtype == torch.uint8 and tuple(res["overlays"][i].shape) == source.shape[:2] + (3,), i
        assert torch.equal(res["overlays"][i].cpu(), torch.from_numpy(o)), i
        if not masks[i].any():
            assert not k.any(), i                              # what the area filter removed does not come back
        assert m.min() >= maps[i].min() and m.max() <= maps[i].max(), i      # bilinear taps are >= 0 and sum to 1
        outlined += int(((o == WHITE).all(-1) & (k != 0)).sum())
    assert outlined > 0
    # a part of the images in another order gives the same renderings
    order = [5, 0, 3]
    again = det.predict([files[i] for i in order], overlays=True)
    for j, i in enumerate(order):
        assert torch.equal(again["maps_src"][j], res["maps_src"][i]) and torch.equal(again["overlays"][j], res["overlays"][i]), i


def test_cli_source_frame_round_trip(trees, tmp_path):
    from srad_amd import metrics as M
    from srad_amd import predict as P
    raw, _ = trees
    run = tmp_path / "drn-l" / f"mvtec_grid_{HR}_X{SCALE}"
    (run / "model").mkdir(parents=True)
    cfg = S.DRNConfig.for_scale(SCALE, 1)
    sd = S.synth_state(S.drn_spec(cfg), seed=9, gain=0.4, cfg=cfg)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, run / "model" / "model_best.pt")
    common = ["--run-dir", str(run), "--dtype", "fp32"]
    inputs = ["--input", str(raw / "grid" / "test" / "good"), str(raw / "grid" / "test" / "crack")]
    P.main(common + ["--calibrate", str(raw / "grid" / "train" / "good"), "--threshold-fpr", "0.05", "--min-region-area", "2", "--map-ws", str(WS)])
    op_bytes = (run / "operating_point.json").read_bytes()
    plain, full = tmp_path / "plain", tmp_path / "full"
    old = P.main(common + inputs + ["--output-dir", str(plain), "--save-masks"])
    res = P.main(common + inputs + ["--output-dir", str(full), "--save-masks", "--save-overlays", "--overlay-alpha", "0.4", "--overlay-contour", "2"])
    assert (plain / "predictions.csv").read_bytes() == (full / "predictions.csv").read_bytes()
    assert (run / "operating_point.json").read_bytes() == op_bytes
    assert sorted(p.name for p in plain.iterdir()) == ["anomaly_masks", "predictions.csv"]                   # no new flag, no new output
    assert sorted(p.name for p in full.iterdir()) == ["anomaly_masks", "overlays", "predictions.csv", "source_maps", "source_masks"]
    for k in range(7):
        kind = "bad" if res["defective"][k] else "good"
        a, b = (np.array(Image.open(d / "anomaly_masks" / kind / f"{res['names'][k]}.png")) for d in (plain, full))
        assert np.array_equal(a, b), k
    assert torch.equal(old["maps"], res["maps"]) and torch.equal(old["masks"], res["masks"]) and "maps_src" not in old
    lut, scale = P.heat_lut(102), P.overlay_scale(res["threshold"])                  # int(0.4 * 255 + 0.5)
    for k, (name, file) in enumerate(zip(res["names"], res["files"])):
        kind = "bad" if res["defective"][k] else "good"
        source = P.as_source(file)
        size = source.shape[:2]
        got = {folder: np.array(Image.open(full / folder / kind / f"{name}.png")) for folder in ("source_maps", "source_masks", "overlays")}
        assert got["source_maps"].shape == size and got["source_masks"].shape == size and got["overlays"].shape == size + (3,), name
        assert all(a.dtype == np.uint8 for a in got.values())
        assert np.array_equal(got["source_maps"], M.to_u8_hwc(res["maps_src"][k][None, None], rgb_range=1.0)[0, :, :, 0].cpu().numpy()), name
        assert np.array_equal(got["source_masks"], res["masks_src"][k].cpu().numpy() * 255), name
        assert np.array_equal(got["overlays"], res["overlays"][k].cpu().numpy()), name
        m, mask, o = _expected(P, source, res["maps"][k].cpu().numpy(), res["masks"][k].cpu().numpy(), lut, scale, 2)
        assert np.array_equal(bits(res["maps_src"][k].cpu().numpy()), bits(m)) and np.array_equal(got["source_masks"], mask * 255), name
        assert np.array_equal(got["source_maps"], np.clip(m * np.float32(255.0), 0, 255).astype(np.uint8)), name      # 255 * clip(map, 0, 1), truncated
        assert np.array_equal(got["overlays"], o), name
    for folder in ("source_maps", "source_masks", "overlays"):
        assert len(list((full / folder).rglob("*.png"))) == 7
    only = tmp_path / "only"
    P.main(common + inputs + ["--output-dir", str(only), "--source-frame"])
    assert sorted(p.name for p in only.iterdir()) == ["predictions.csv", "source_maps", "source_masks"]
    assert (only / "predictions.csv").read_bytes() == (plain / "predictions.csv").read_bytes()
