"""CPU: the per-pixel map baseline (DESIGN.md "Baseline") where it needs no GPU - the numpy restatement against a literal
per-pixel loop, the Samuelson bound that makes leave-one-out necessary, the refusals, the npz round trip, the operating-point
document, the contradictions, the parsers, and the synthetic band-and-blob case on the restatement."""
import json

import numpy as np
import pytest
import torch

from tests import baseline_ref as R


def _maps(n, H, W, seed=5):
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.02, 0.6, (H, W))
    return (base[None] * (1.0 + 0.3 * rng.uniform(-1, 1, (n, H, W)))).astype(np.float32)


def test_restatement_equals_the_literal_loop():
    maps = _maps(7, 5, 7)
    lit = R.literal(maps, 0.1)
    s1, s2 = R.sums_ref(maps)
    assert R.same_bits(s1, lit["s1"]) and R.same_bits(s2, lit["s2"])
    p = R.planes_ref(s1, s2, 7, 0.1)
    assert abs(p["pooled"] - lit["pooled_loop"]) <= 1e-15 * lit["pooled_loop"] * 35        # numpy's mean sums pairwise
    assert p["floor"] == lit["floor"] and R.same_bits(p["mu32"], lit["mu32"]) and R.same_bits(p["inv32"], lit["inv32"])
    assert R.same_bits(R.loo_ref(maps, s1, s2, 7, p["floor"]), lit["loo"])
    # chunks give the bits of one pass; a NaN pixel makes that pixel's sums NaN and no other's
    a1, a2 = R.sums_ref(maps[:3])
    assert all(R.same_bits(x, y) for x, y in zip(R.sums_ref(maps[3:], a1, a2), (s1, s2)))
    holed = maps.copy()
    holed[2, 1, 3] = np.nan
    h1, h2 = R.sums_ref(holed)
    assert np.isnan(h1[1, 3]) and np.isnan(h2[1, 3]) and np.isnan(h1).sum() == 1 and np.isnan(h2).sum() == 1
    # the planes of srad_amd.baseline are the restatement's
    from srad_amd import baseline as B
    got = B.host_planes(s1, s2, 7, 0.1)
    assert R.same_bits(got["mu32"], p["mu32"]) and R.same_bits(got["inv32"], p["inv32"])
    assert got["floor"] == p["floor"] and got["pooled"] == p["pooled"]


def test_samuelson_bound_in_sample_and_leave_one_out_beyond_it():
    n = 12
    maps = _maps(n, 6, 6, seed=2)
    maps[4, 2, 3] += np.float32(5.0)                           # an outlier among the calibration maps themselves
    s1, s2 = R.sums_ref(maps)
    p = R.planes_ref(s1, s2, n, 1e-6)
    z_in = R.apply_ref(maps, p["mu32"], p["inv32"])
    bound = (n - 1) / np.sqrt(n)                               # 3.18 sigmas for 12 images
    assert np.abs(z_in).max() <= bound * (1 + 1e-5) and z_in[4, 2, 3] > 0.99 * bound
    z_loo = R.loo_ref(maps, s1, s2, n, p["floor"])
    assert z_loo[4, 2, 3] > 10 * bound


def test_refusals_need_no_gpu(tmp_path):
    from srad_amd import baseline as B
    two = torch.zeros(2, 4, 4)
    with pytest.raises(ValueError, match="at least 3"):
        B.MapBaseline.fit(two)                                 # before any GPU work: these are CPU tensors
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="floor_rel"):
            B.MapBaseline.fit(torch.zeros(3, 4, 4), floor_rel=bad)
        with pytest.raises(ValueError, match="floor_rel"):
            B.host_planes(np.ones((2, 2)), np.ones((2, 2)), 3, bad)
    const = np.full((3, 4, 4), 0.25, np.float32)
    with pytest.raises(ValueError, match="do not vary"):
        B.host_planes(*R.sums_ref(const), 3, 0.1)
    holed = _maps(4, 4, 4)
    holed[1, 0, 0] = np.nan
    with pytest.raises(ValueError, match="do not vary"):
        B.host_planes(*R.sums_ref(holed), 4, 0.1)
    with pytest.raises(ValueError, match="at least 3"):
        B.host_planes(np.ones((2, 2)), np.ones((2, 2)), 2, 0.1)
    with pytest.raises(RuntimeError, match="GPU only"):
        B.MapBaseline.fit(torch.zeros(3, 4, 4))                # and no CPU fallback behind the checks


def _host_baseline(maps, floor_rel=0.1):
    """A MapBaseline whose sums were made on the host by the restatement (what load() makes too)."""
    from srad_amd import baseline as B
    b = B.MapBaseline(floor_rel)
    s1, s2 = R.sums_ref(maps)
    b.s1, b.s2, b.n = torch.from_numpy(s1), torch.from_numpy(s2), len(maps)
    return b


def test_npz_round_trip_and_load_refusals(tmp_path):
    from srad_amd import baseline as B
    from srad_amd.evaluate import MapSpec
    maps = _maps(5, 6, 10)
    b = _host_baseline(maps, 0.25)
    spec = MapSpec(source="mse", ws=3, sigma=1.5)
    f = tmp_path / "sub" / B.BASELINE_FILE
    digest = b.save(f, spec)
    assert digest == B.file_sha256(f) and len(digest) == 64
    with np.load(f) as z:
        assert sorted(z.files) == ["floor", "floor_rel", "map_spec", "n", "s1", "s2", "version"]
        assert int(z["version"]) == B.BASELINE_VERSION == 1 and int(z["n"]) == 5 and float(z["floor_rel"]) == 0.25
        assert json.loads(str(z["map_spec"])) == dict(source="mse", ws=3, scales=[], reduce="mean", sigma=1.5)
    back = B.load(f, shape=(6, 10), spec=spec)
    assert back.n == 5 and back.floor_rel == 0.25 and back.shape == (6, 10)
    for k in ("mu32", "inv32"):
        assert R.same_bits(back.planes()[k], b.planes()[k])
    assert back.planes()["floor"] == b.planes()["floor"] and back.entries() == b.entries()
    e = b.entries()["map_baseline"]
    assert list(e) == ["n_images", "floor_rel", "floor", "pooled_sd"] and e["n_images"] == 5 and e["floor"] == 0.25 * e["pooled_sd"]
    with pytest.raises(ValueError, match=r"\(6, 10\).*\(10, 6\)"):
        B.load(f, shape=(10, 6))
    with pytest.raises(ValueError, match="other maps"):
        B.load(f, spec=MapSpec(source="mse", ws=3))
    with np.load(f) as z:
        doc = {k: z[k] for k in z.files}
    other = tmp_path / "v2.npz"
    np.savez(other, **dict(doc, version=np.int64(2)))
    with pytest.raises(ValueError, match="version 2"):
        B.load(other)
    np.savez(other, **dict(doc, floor=np.float64(float(doc["floor"]) * 2)))
    with pytest.raises(ValueError, match="stored floor"):
        B.load(other)
    np.savez(other, **{k: v for k, v in doc.items() if k != "s2"})
    with pytest.raises(ValueError, match="missing"):
        B.load(other)
    other.write_bytes(b"not a zip file")
    with pytest.raises(ValueError, match="not a readable"):
        B.load(other)


def test_operating_point_document(tmp_path):
    from srad_amd import predict as P
    spec = P.MapSpec(source="ssim", ws=11, sigma=2.0)
    f = tmp_path / P.OPERATING_POINT_FILE
    doc = P.write_operating_point(f, 0.25, 0.01, "pixel", 0.0078125, 12, 3, spec, False, "model_best.pt")
    assert list(doc) == ["version", "threshold", "threshold_source", "threshold_fpr", "threshold_level", "calib_rate", "calib_images",
                         "min_region_area", "map_spec", "self_ensemble", "checkpoint"]            # without a baseline: today's keys
    assert doc["map_spec"] == dict(source="ssim", ws=11, scales=[], reduce="mean", sigma=2.0) and json.loads(f.read_text()) == doc
    assert P.read_operating_point(f)["baseline"] is None
    b = _host_baseline(_maps(4, 8, 8))
    digest = b.save(tmp_path / P.B.BASELINE_FILE, spec)
    entry = P.baseline_entry(b, tmp_path / P.B.BASELINE_FILE, digest)
    assert entry == dict(file="map_baseline.npz", n_images=4, floor_rel=0.1, floor=b.floor, sha256=digest)
    doc2 = P.write_operating_point(f, 4.5, 0.01, "pixel", 0.0078125, 4, 3, spec, False, "model_best.pt", baseline=entry)
    assert list(doc2) == list(doc) + ["baseline"] and doc2["map_spec"] == doc["map_spec"] and doc2["baseline"] == entry
    back = P.read_operating_point(f)
    assert back["baseline"] == entry and back["threshold"] == 4.5 and back["tile"] is None and back["frame"] is None
    broken = dict(doc2, baseline={k: v for k, v in entry.items() if k != "sha256"})
    f.write_text(json.dumps(broken))
    with pytest.raises(ValueError, match="sha256"):
        P.read_operating_point(f)


def test_contradictions(tmp_path):
    from srad_amd import predict as P
    plain, with_b = dict(baseline=None), dict(baseline=dict(file="map_baseline.npz", n_images=4, floor_rel=0.1, floor=0.01, sha256="00"))
    args = lambda extra: P.parse_predict_args(["--input", "x"] + extra)
    assert P.baseline_from_args(args([]), plain, tmp_path) is None
    with pytest.raises(ValueError, match=r"--baseline contradicts the calibrated operating point \(calibrated without a baseline\): "
                                         r"calibrate again with it, or give --threshold"):
        P.baseline_from_args(args(["--baseline"]), plain, tmp_path)
    for extra in ([], ["--baseline"], ["--baseline", "--baseline-floor", "0.1"]):     # kept, like the tile setting
        assert P.baseline_from_args(args(extra), with_b, tmp_path) == dict(path=tmp_path / "map_baseline.npz", sha256="00", floor_rel=None)
    with pytest.raises(ValueError, match=r"--baseline-floor 0.2 contradicts the calibrated operating point \(floor_rel = 0.1\)"):
        P.baseline_from_args(args(["--baseline", "--baseline-floor", "0.2"]), with_b, tmp_path)
    # a given threshold: the run's own file, which must be there
    given = args(["--threshold", "4", "--baseline"])
    with pytest.raises(ValueError, match="map_baseline.npz"):
        P.baseline_from_args(given, None, tmp_path)
    assert P.baseline_from_args(args(["--threshold", "4"]), None, tmp_path) is None
    b = _host_baseline(_maps(4, 8, 8))
    spec = P.MapSpec(ws=11)
    digest = b.save(tmp_path / "map_baseline.npz", spec)
    assert P.baseline_from_args(given, None, tmp_path) == dict(path=tmp_path / "map_baseline.npz", sha256=None, floor_rel=None)

    class Det:
        device, map_shape = None, (8, 8)
    Det.spec = spec
    which = dict(path=tmp_path / "map_baseline.npz", sha256=digest, floor_rel=None)
    assert P.load_baseline(which, Det).n == 4
    with pytest.raises(ValueError, match="sha256"):
        P.load_baseline(dict(which, sha256="0" * 64), Det)
    Det.map_shape = (8, 12)
    with pytest.raises(ValueError, match=r"\(8, 8\).*\(8, 12\)"):
        P.load_baseline(which, Det)
    Det.map_shape, Det.spec = (8, 8), P.MapSpec(ws=7)
    with pytest.raises(ValueError, match="other maps"):
        P.load_baseline(which, Det)
    with pytest.raises(ValueError, match="missing"):
        P.load_baseline(dict(which, path=tmp_path / "gone.npz"), Det)


def test_parsers_and_a_config_value(tmp_path):
    from srad_amd import options as O
    from srad_amd import predict as P
    off = O.parse_eval_args([])
    assert off.map_baseline is False and off.baseline_floor is None
    on = O.parse_eval_args(["--map-baseline", "--pixel-metrics"])
    assert on.map_baseline is True and on.baseline_floor is None
    assert O.parse_eval_args(["--map-baseline", "--baseline-floor", "0.25", "--threshold-fpr", "0.01"]).baseline_floor == 0.25
    p_off = P.parse_predict_args(["--input", "x"])
    assert p_off.baseline is False and p_off.baseline_floor is None
    p_on = P.parse_predict_args(["--calibrate", "d", "--threshold-fpr", "0.01", "--baseline", "--baseline-floor", "0.5"])
    assert p_on.baseline is True and p_on.baseline_floor == 0.5
    for bad in (["--baseline-floor", "0.2", "--pixel-metrics"],               # the floor belongs to the flag
                ["--map-baseline", "--pixel-metrics", "--baseline-floor", "0"], ["--map-baseline", "--pixel-metrics", "--baseline-floor", "-1"],
                ["--map-baseline", "--pixel-metrics", "--baseline-floor", "nan"], ["--map-baseline", "--pixel-metrics", "--baseline-floor", "inf"],
                ["--map-baseline"]):                                           # nothing that makes maps
        with pytest.raises(SystemExit):
            O.parse_eval_args(bad)
    for bad in (["--input", "x", "--baseline-floor", "0.2"], ["--input", "x", "--baseline", "--baseline-floor", "0"]):
        with pytest.raises(SystemExit):
            P.parse_predict_args(bad)
    for flag in ("--map-baseline", "--baseline"):                              # training has no map stage
        with pytest.raises(SystemExit):
            O.parse_train_args([flag])
    cfg = tmp_path / "eval.yaml"
    cfg.write_text("map-baseline: true\nbaseline-floor: 0.2\naupro: true\n")
    a = O.parse_eval_args(["--config", str(cfg)])
    assert a.map_baseline is True and a.baseline_floor == 0.2 and a.aupro is True
    cfg.write_text("map-baseline: true\nbaseline-floor: -3\naupro: true\n")
    with pytest.raises(SystemExit):
        O.parse_eval_args(["--config", str(cfg)])
    cfg.write_text("map-baseline: maybe\naupro: true\n")
    with pytest.raises(SystemExit):
        O.parse_eval_args(["--config", str(cfg)])


def test_more_than_one_rank_is_refused_before_any_work(capsys):
    from srad_amd import evaluate as E
    from srad_amd import options as O
    with pytest.raises(SystemExit):
        O.parse_eval_args(["--map-baseline", "--pixel-metrics", "--gpus", "2"])
    assert "--map-baseline needs --gpus 1" in capsys.readouterr().err
    pair = (np.zeros((16, 16, 1), np.uint8), np.zeros((64, 64, 1), np.uint8))
    calib = [pair] * 3
    # the model is None: every refusal comes before it is touched
    with pytest.raises(ValueError, match="one rank"):
        E.evaluate_on_test(None, None, [pair], [pair], rank=0, world=2, pixel_metrics=True, map_baseline=dict(calib=calib, floor_rel=0.1))
    with pytest.raises(ValueError, match="at least 3"):
        E.evaluate_on_test(None, None, [pair], [pair], pixel_metrics=True, map_baseline=dict(calib=calib[:2], floor_rel=0.1))
    with pytest.raises(ValueError, match="floor_rel"):
        E.evaluate_on_test(None, None, [pair], [pair], pixel_metrics=True, map_baseline=dict(calib=calib, floor_rel=0.0))
    with pytest.raises(ValueError, match="dict"):
        E.evaluate_on_test(None, None, [pair], [pair], pixel_metrics=True, map_baseline=calib)
    other = (np.ones((16, 16, 1), np.uint8), np.ones((64, 64, 1), np.uint8))
    with pytest.raises(ValueError, match="baseline's calibration pairs"):
        E.evaluate_on_test(None, None, [pair], [pair], map_baseline=dict(calib=calib, floor_rel=0.1),
                           operating_point=dict(fpr=0.01, calib=[other] * 3))


def test_band_and_blob_on_the_restatement():
    calib, good, bad, _ = R.band_and_blob(seed=0)
    raw = R.auc(R.max_ref(good), R.max_ref(bad))
    assert raw <= 0.6, raw                                     # the noisy band decides the raw map maximum
    s1, s2 = R.sums_ref(calib)
    p = R.planes_ref(s1, s2, len(calib), 0.1)
    zg, zb = R.max_ref(R.apply_ref(good, p["mu32"], p["inv32"])), R.max_ref(R.apply_ref(bad, p["mu32"], p["inv32"]))
    assert R.auc(zg, zb) == 1.0
    assert zg.max() < 8.0 and zb.min() > 15.0, (zg.max(), zb.min())           # a wide margin: 3.9 against 30 sigmas
    # a threshold calibrated in-sample sits under the Samuelson bound and fires on fresh good maps; leave-one-out does not
    n = len(calib)
    t_in = R.apply_ref(calib, p["mu32"], p["inv32"]).max()
    t_loo = R.loo_ref(calib, s1, s2, n, p["floor"]).max()
    assert t_in <= (n - 1) / np.sqrt(n) * (1 + 1e-5) < zg.max() and t_loo > t_in
