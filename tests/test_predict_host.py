"""CPU: the host side of srad_amd.predict - option parsing, the operating_point.json round trip, the refusal of a --map-* flag
that contradicts a calibrated file, the refusal of an SSIM spec without a window, how sources are read, and the float32 luma
table against data.rgb2y on gray images of several shapes."""
import json

import numpy as np
import pytest
from PIL import Image


def test_option_parsing():
    from srad_amd import predict as P
    a = P.parse_predict_args(["--run-dir", "r", "--input", "a.png", "dir"])
    assert a.input == ["a.png", "dir"] and a.calibrate == "" and a.threshold is None and a.dtype == "bf16x3"
    assert (a.map_source, a.map_ws, a.map_scales, a.map_reduce, a.map_sigma, a.min_region_area) == (None,) * 6
    assert P.spec_from_args(a) == P.MapSpec(source="ssim", ws=11)                 # --map-ws defaults to 11
    a = P.parse_predict_args(["--calibrate", "good", "--threshold-fpr", "0.01", "--threshold-level", "image", "--min-region-area", "3",
                              "--map-scales", "7,11", "--map-reduce", "max", "--map-sigma", "2", "--self-ensemble", "--ema"])
    assert a.threshold_fpr == 0.01 and a.threshold_level == "image" and a.min_region_area == 3 and a.self_ensemble and a.ema
    assert P.spec_from_args(a) == P.MapSpec(source="ssim", ws=0, scales=[7, 11], reduce="max", sigma=2.0)
    a = P.parse_predict_args(["--input", "x", "--threshold", "0.25", "--map-source", "mse", "--map-ws", "0"])
    assert P.check_spec(P.spec_from_args(a)) == P.MapSpec(source="mse", ws=0)     # mse names its window: 0 is the raw squared error
    for bad in ([], ["--calibrate", "d"], ["--input", "x", "--threshold-fpr", "0.1"], ["--calibrate", "d", "--threshold-fpr", "1.5"],
                ["--calibrate", "d", "--threshold-fpr", "0.1", "--threshold", "0.5"], ["--input", "x", "--threshold", "nan"],
                ["--input", "x", "--min-region-area", "0"], ["--input", "x", "--ema", "--checkpoint", "f.pt"],
                ["--input", "x", "--map-scales", "3,x"]):
        with pytest.raises(SystemExit):
            P.parse_predict_args(bad)
    with pytest.raises(ValueError, match="exclude each other"):
        P.spec_from_args(P.parse_predict_args(["--input", "x", "--map-scales", "7,11", "--map-ws", "5"]))


def test_ssim_spec_without_a_window_is_refused():
    from srad_amd import predict as P
    a = P.parse_predict_args(["--input", "x", "--map-ws", "0"])
    with pytest.raises(ValueError, match="--map-ws"):
        P.check_spec(P.spec_from_args(a))
    with pytest.raises(ValueError, match="--map-ws"):
        P.check_spec(P.MapSpec())
    assert P.check_spec(P.MapSpec(ws=1)).ws == 1 and P.check_spec(P.MapSpec(scales="sweep")).scales == "sweep"

    class Opt:
        patch_size, scale, n_colors, rgb_range = 32, [2, 4], 1, 255
    with pytest.raises(ValueError, match="--map-ws"):          # before the model is touched
        P.Detector(Opt(), None, P.MapSpec(source="ssim", ws=0))
    with pytest.raises(ValueError, match="map scales"):        # the spec is resolved against the HR size
        P.Detector(Opt(), None, P.MapSpec(scales=[7, 99]))


def test_operating_point_file_round_trip_and_contradictions(tmp_path):
    from srad_amd import predict as P
    t = float(np.float32(0.1234567))                           # a float32 map value, as calibration returns it
    spec = P.MapSpec(source="mse", ws=0, scales=[7, 11], reduce="max", sigma=1.5)
    f = tmp_path / "run" / P.OPERATING_POINT_FILE
    doc = P.write_operating_point(f, t, 0.01, "image", 0.0078125, 12, 3, spec, True, "/some/where/model_best.pt")
    raw = json.loads(f.read_text())
    assert raw == doc and raw["version"] == 1 and raw["checkpoint"] == "model_best.pt" and raw["threshold_source"] == "fpr"
    assert set(raw) == {"version", "threshold", "threshold_source", "threshold_fpr", "threshold_level", "calib_rate", "calib_images",
                        "min_region_area", "map_spec", "self_ensemble", "checkpoint"}
    assert raw["map_spec"] == dict(source="mse", ws=0, scales=[7, 11], reduce="max", sigma=1.5)
    back = P.read_operating_point(f)
    assert back["threshold"] == t and back["map_spec"] == spec and back["min_region_area"] == 3 and back["self_ensemble"] is True
    assert (back["threshold_fpr"], back["threshold_level"], back["calib_rate"], back["calib_images"]) == (0.01, "image", 0.0078125, 12)
    for value in (1e-300, 0.1 + 0.2, float("inf"), float(np.nextafter(np.float32(1), np.float32(2)))):     # round-trip exact
        P.write_operating_point(f, value, 0.5, "pixel", 0.0, 1, 1, P.MapSpec(ws=11), False, "m.pt")
        assert P.read_operating_point(f)["threshold"] == value
    # flags against the stored spec: the same values pass, any other is refused with the flag's name
    stored = P.MapSpec(source="ssim", ws=11, sigma=2.0)
    ok = P.parse_predict_args(["--input", "x", "--map-ws", "11", "--map-sigma", "2", "--map-source", "ssim"])
    assert P.spec_from_args(ok, stored) == stored and P.spec_from_args(P.parse_predict_args(["--input", "x"]), stored) == stored
    for flags, name in ((["--map-ws", "7"], "--map-ws"), (["--map-sigma", "0"], "--map-sigma"), (["--map-source", "mse"], "--map-source"),
                        (["--map-scales", "7,11"], "--map-scales"), (["--map-reduce", "max"], "--map-reduce")):
        with pytest.raises(ValueError, match=f"{name} .* contradicts the calibrated operating point"):
            P.spec_from_args(P.parse_predict_args(["--input", "x"] + flags), stored)
    multi = P.MapSpec(scales=[3, 13, 23], reduce="mean")
    sweep = P.parse_predict_args(["--input", "x", "--map-scales", "sweep"])
    assert P.spec_from_args(sweep, multi, side=32) == multi                       # sweep of a 32 px image is 3, 13, 23
    with pytest.raises(ValueError, match="--map-scales"):
        P.spec_from_args(sweep, multi, side=64)
    # another version, a missing entry
    raw["version"] = 2
    f.write_text(json.dumps(raw))
    with pytest.raises(ValueError, match="version 2"):
        P.read_operating_point(f)
    raw["version"] = 1
    del raw["map_spec"]["sigma"]
    f.write_text(json.dumps(raw))
    with pytest.raises(ValueError, match="sigma"):
        P.read_operating_point(f)


def test_sources_and_file_lists(tmp_path):
    from srad_amd import predict as P
    rng = np.random.RandomState(0)
    g = rng.randint(0, 256, (9, 7)).astype(np.uint8)
    c = rng.randint(0, 256, (9, 7, 3)).astype(np.uint8)
    assert np.array_equal(P.as_source(g), g) and np.array_equal(P.as_source(g[..., None]), g)
    assert np.array_equal(P.as_source(np.stack([g] * 3, axis=2)), g)               # r = g = b is gray
    assert P.as_source(c).shape == (9, 7, 3)
    for bad in (g.astype(np.float32), np.zeros((3, 3, 4), np.uint8), np.zeros((0, 3), np.uint8), np.zeros((2, 2, 2, 2), np.uint8)):
        with pytest.raises(ValueError, match="uint8 images"):
            P.as_source(bad)
    d = tmp_path / "imgs"
    d.mkdir()
    Image.fromarray(g).save(d / "b.png")
    Image.fromarray(c).save(d / "a.png")
    Image.fromarray(np.dstack([c, c[..., :1]])).save(d / "c.png")                  # RGBA goes through convert('RGB')
    (d / "notes.txt").write_text("x")
    files = P.list_images([str(d), str(d / "b.png")])
    assert [f.name for f in files] == ["a.png", "b.png", "c.png", "b.png"] and P.unique_names(files) == ["a", "b", "c", "b_2"]
    assert np.array_equal(P.as_source(files[1]), g) and np.array_equal(P.as_source(files[0]), c) and np.array_equal(P.as_source(files[2]), c)
    with pytest.raises(FileNotFoundError):
        P.list_images([str(d / "missing.png")])


def test_luma_table_is_rgb2y_in_float32_whatever_the_shape():
    from srad_amd import data as D
    from srad_amd import predict as P
    table = P.luma_table()
    assert table.dtype == np.float32 and table.shape == (256,) and table[0] == 16.0 and table[255] == np.float32(235.0)
    assert (np.diff(table) > 0).all()
    rng = np.random.RandomState(5)
    for shape in ((1, 1), (1, 256), (256, 1), (8, 8), (32, 32), (7, 53), (128, 128), (33, 100), (64, 3)):
        g = rng.randint(0, 256, shape).astype(np.uint8)
        g.flat[:min(g.size, 256)] = np.arange(min(g.size, 256))
        y = D.set_channel([np.stack([g] * 3, axis=2)], np.stack([g] * 3, axis=2), n_channels=1)[1]      # what the loader computes
        assert y.dtype == np.float64 and np.array_equal(y[..., 0].astype(np.float32), table[g]), shape
        hr = np.clip(y[..., 0].astype(np.float32), 0, 255).astype(np.uint8)                              # the evaluator's truncation
        assert np.array_equal(hr, table.astype(np.uint8)[g]), shape
