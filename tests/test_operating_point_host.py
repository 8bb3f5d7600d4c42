"""CPU: the host side of the operating point - the evaluator's new flags and their two SystemExit cases, the rank of a
false-positive rate, the ratios of a report from hand-made counts, the argument checks of srad_select_kth /
srad_operating_point and their workspace queries, and where the new keyword sits in the evaluator's signatures."""
import ctypes as C
import inspect
import math

import pytest


def test_flag_defaults_and_parsing():
    from srad_amd import options as Opt
    a = Opt.parse_eval_args([])
    assert a.threshold is None and a.threshold_fpr is None and a.threshold_level == "pixel"
    assert a.min_region_area == 1 and a.save_masks is False
    a = Opt.parse_eval_args(["--threshold", "0.25", "--min-region-area", "4", "--save-masks"])
    assert a.threshold == 0.25 and a.threshold_fpr is None and a.min_region_area == 4 and a.save_masks is True
    a = Opt.parse_eval_args(["--threshold-fpr", "0.01", "--threshold-level", "image"])
    assert a.threshold is None and a.threshold_fpr == 0.01 and a.threshold_level == "image"
    assert Opt.parse_eval_args(["--threshold=-inf"]).threshold == -math.inf
    for bad in (["--threshold-fpr", "0"], ["--threshold-fpr", "1"], ["--threshold-fpr", "nan"], ["--threshold", "nan"],
                ["--min-region-area", "0"], ["--threshold-level", "region"]):
        with pytest.raises(SystemExit):
            Opt.parse_eval_args(bad)


def test_threshold_and_threshold_fpr_exclude_each_other():
    from srad_amd import evaluate as E
    with pytest.raises(SystemExit):
        E.main(["--threshold", "0.5", "--threshold-fpr", "0.05", "--checkpoint", "/nonexistent/model.pt"])


def test_threshold_fpr_without_val_good_exits_before_the_model(tmp_path):
    from srad_amd import evaluate as E
    (tmp_path / "grid" / "test" / "good" / "HR").mkdir(parents=True)
    with pytest.raises(SystemExit) as e:                      # no checkpoint either: the calibration check comes first
        E.main(["--model-type", "drn-l", "--classe", "grid", "--data-root", str(tmp_path), "--threshold-fpr", "0.05"])
    assert str(tmp_path / "grid" / "val" / "good") in str(e.value)


@pytest.mark.parametrize("n", [1, 2, 26, 16384])
@pytest.mark.parametrize("f", [0.01, 0.5, 0.999])
def test_rank_for_rate(n, f):
    from srad_amd import metrics as M
    k = M.rank_for_rate(n, f)
    m = min(max(math.floor(f * n), 0), n - 1)
    assert k == n - 1 - m and 0 <= k < n
    assert n - 1 - k <= f * n                                 # at most floor(f n) values above rank k
    want = {(1, 0.01): 0, (1, 0.5): 0, (1, 0.999): 0, (2, 0.01): 1, (2, 0.5): 0, (2, 0.999): 0, (26, 0.01): 25, (26, 0.5): 12,
            (26, 0.999): 0, (16384, 0.01): 16220, (16384, 0.5): 8191, (16384, 0.999): 16}
    assert k == want[(n, f)]


def test_rank_for_rate_refuses():
    from srad_amd import metrics as M
    for n, f in ((0, 0.5), (-3, 0.5), (10, 0.0), (10, 1.0), (10, -0.1), (10, float("nan"))):
        with pytest.raises(ValueError):
            M.rank_for_rate(n, f)


def test_operating_point_stats_from_hand_made_counts():
    from srad_amd import metrics as M
    R = 3
    num = 2 * (1 << 64) // 3 + (1 << 64) // 4                 # some 128-bit numerator: pro = (2/3 + 1/4) / 3
    counts = dict(tp=30, fp=10, fn=20, tn=940, n_nan=0, n_regions=R, pro_hi=num >> 64, pro_lo=num & ((1 << 64) - 1))
    st = M.operating_point_stats(counts, [0, 5, 0, 1, 0, 7], [0, 0, 0, 1, 1, 1])
    assert (st["image_tp"], st["image_fp"], st["image_fn"], st["image_tn"]) == (2, 1, 1, 2)
    assert st["image_tpr"] == 2 / 3 and st["image_fpr"] == 1 / 3
    assert (st["pixel_tp"], st["pixel_fp"], st["pixel_fn"], st["pixel_tn"]) == (30, 10, 20, 940)
    assert st["precision"] == 30 / 40 and st["recall"] == 30 / 50 and st["f1"] == 60 / 90 and st["iou"] == 30 / 60
    assert st["fpr"] == 10 / 950
    assert abs(st["pro_at_threshold"] - (2 / 3 + 1 / 4) / 3) <= 1e-12
    # without counts: the image level only
    assert set(M.operating_point_stats(None, [1, 0], [1, 0])) == {"image_tp", "image_fp", "image_fn", "image_tn", "image_tpr",
                                                                   "image_fpr"}
    with pytest.raises(ValueError):
        M.operating_point_stats(None, [1, 0, 0], [1, 0])


def test_operating_point_stats_zero_denominators():
    from srad_amd import metrics as M
    zero = dict(tp=0, fp=0, fn=0, tn=0, n_nan=0, n_regions=0, pro_hi=0, pro_lo=0)
    st = M.operating_point_stats(zero, [], [])
    for k in ("image_tpr", "image_fpr", "precision", "recall", "f1", "iou", "fpr", "pro_at_threshold"):
        assert st[k] == 0.0 and isinstance(st[k], float), k
    # each denominator on its own: no prediction (precision), no defect (recall, pro), no ok pixel (fpr)
    st = M.operating_point_stats(dict(zero, fn=5, tn=7, n_regions=1), [0, 0], [1, 1])
    assert st["precision"] == 0.0 and st["recall"] == 0.0 and st["f1"] == 0.0 and st["iou"] == 0.0 and st["fpr"] == 0.0
    assert st["image_tpr"] == 0.0 and st["image_fpr"] == 0.0 and st["image_fn"] == 2
    st = M.operating_point_stats(dict(zero, fp=4, tn=6), [3, 0], [0, 0])
    assert st["recall"] == 0.0 and st["pro_at_threshold"] == 0.0 and st["precision"] == 0.0 and st["fpr"] == 0.4
    assert st["image_tpr"] == 0.0 and st["image_fpr"] == 0.5
    st = M.operating_point_stats(dict(zero, tp=9, n_regions=1, pro_hi=1), [9], [1])
    assert st["fpr"] == 0.0 and st["precision"] == 1.0 and st["recall"] == 1.0 and st["pro_at_threshold"] == 1.0
    assert st["image_tpr"] == 1.0 and st["image_fpr"] == 0.0


def test_argument_errors_of_select_kth_without_gpu():
    from srad_amd import _lib as L
    lib = L.lib()
    nb = C.c_size_t()
    q = lib.srad_select_kth_workspace_bytes
    assert q(C.c_int64(0), C.byref(nb)) != 0
    assert q(C.c_int64(1 << 31), C.byref(nb)) != 0 and b"2^31" in lib.srad_last_error()
    assert q(C.c_int64(100), None) != 0
    assert q(C.c_int64(1), C.byref(nb)) == 0 and nb.value > 0
    small_n = nb.value
    assert q(C.c_int64((1 << 31) - 1), C.byref(nb)) == 0 and nb.value == small_n     # no n-sized workspace
    assert nb.value < (1 << 16)
    fake, big, small = C.c_void_p(4096), C.c_size_t(1 << 40), C.c_size_t(16)
    f = lib.srad_select_kth
    n, k = C.c_int64(1000), C.c_int64(10)
    assert f(None, n, k, fake, fake, fake, big, None) != 0 and b"NULL" in lib.srad_last_error()
    assert f(fake, n, k, None, fake, fake, big, None) != 0
    assert f(fake, n, k, fake, None, fake, big, None) != 0
    assert f(fake, n, k, fake, fake, None, big, None) != 0
    assert f(fake, C.c_int64(0), C.c_int64(0), fake, fake, fake, big, None) != 0
    assert f(fake, C.c_int64(1 << 31), k, fake, fake, fake, big, None) != 0 and b"2^31" in lib.srad_last_error()
    assert f(fake, n, C.c_int64(1000), fake, fake, fake, big, None) != 0 and b"rank" in lib.srad_last_error()      # k >= n
    assert f(fake, n, C.c_int64(-1), fake, fake, fake, big, None) != 0
    assert f(fake, n, k, fake, fake, fake, small, None) != 0 and b"workspace" in lib.srad_last_error()


def test_argument_errors_of_operating_point_without_gpu():
    from srad_amd import _lib as L
    lib = L.lib()
    nb = C.c_size_t()
    q = lib.srad_operating_point_workspace_bytes
    assert q(0, 32, 32, C.byref(nb)) != 0
    assert q(2, 0, 32, C.byref(nb)) != 0
    assert q(2, 32768, 32768, C.byref(nb)) != 0 and b"2^31" in lib.srad_last_error()
    assert q(2, 32, 32, None) != 0
    assert q(3, 40, 50, C.byref(nb)) == 0 and nb.value >= 8 * 3 * 40 * 50
    fake, big, small = C.c_void_p(4096), C.c_size_t(1 << 40), C.c_size_t(16)
    f = lib.srad_operating_point
    t = C.c_float(0.5)
    assert f(None, fake, 2, 32, 32, t, 1, fake, fake, fake, fake, big, None) != 0 and b"NULL" in lib.srad_last_error()
    assert f(fake, fake, 2, 32, 32, t, 1, None, fake, fake, fake, big, None) != 0
    assert f(fake, fake, 2, 32, 32, t, 1, fake, None, fake, fake, big, None) != 0
    assert f(fake, fake, 2, 32, 32, t, 1, fake, fake, None, fake, big, None) != 0
    assert f(fake, fake, 2, 32, 32, t, 1, fake, fake, fake, None, big, None) != 0
    assert f(fake, None, 0, 32, 32, t, 1, fake, fake, fake, fake, big, None) != 0                  # n = 0 (NULL masks are valid)
    assert f(fake, None, 2, 32768, 32768, t, 1, fake, fake, fake, fake, big, None) != 0 and b"2^31" in lib.srad_last_error()
    assert f(fake, None, 2, 32, 32, C.c_float(float("nan")), 1, fake, fake, fake, fake, big, None) != 0
    assert b"NaN" in lib.srad_last_error()
    assert f(fake, None, 2, 32, 32, t, 0, fake, fake, fake, fake, big, None) != 0 and b"min_area" in lib.srad_last_error()
    assert f(fake, None, 2, 32, 32, t, -4, fake, fake, fake, fake, big, None) != 0
    assert f(fake, None, 2, 32, 32, t, 1, fake, fake, fake, fake, small, None) != 0 and b"workspace" in lib.srad_last_error()


def test_wrappers_refuse_bad_arguments_before_the_gpu():
    import torch
    from srad_amd import metrics as M
    cpu = torch.zeros(2, 4, 4)
    with pytest.raises(ValueError, match="NaN"):
        M.operating_point(cpu, float("nan"))
    with pytest.raises(ValueError, match="min_area"):
        M.operating_point(cpu, 0.5, min_area=0)
    with pytest.raises(RuntimeError, match="GPU only"):
        M.operating_point(cpu, 0.5)
    with pytest.raises(RuntimeError, match="GPU only"):
        M.select_kth(cpu, 0)
    with pytest.raises(RuntimeError, match="GPU only"):
        M.map_threshold(cpu, 0.1)


def test_signature_positions():
    from srad_amd import evaluate as E
    ev = list(inspect.signature(E.evaluate_on_test).parameters)
    assert ev[-4:] == ["map_sigma", "map_image_score", "aupro", "pro_fpr_limit"]
    assert "operating_point" in ev[:-4] and inspect.signature(E.evaluate_on_test).parameters["operating_point"].default is None
    maps = E.MapSpec()
    assert (maps.source, maps.scales, maps.reduce, maps.ws, maps.sigma) == ("ssim", (), "mean", 0, 0.0)
    split = inspect.signature(E.iter_split).parameters
    assert list(split)[:6] == ["data_root", "classe", "split", "scale", "n_colors", "rgb_range"] and split["part"].default == "test"
    spec = E.OperatingPoint()
    assert (spec.threshold, spec.fpr, spec.level, spec.min_area, spec.save_masks, len(spec.calib)) == (None, None, "pixel", 1, False, 0)
    for bad in (dict(), dict(threshold=0.5, fpr=0.1), dict(threshold=float("nan")), dict(fpr=1.0), dict(threshold=0.5, level="x"),
                dict(threshold=0.5, min_area=0)):
        with pytest.raises(ValueError):
            E.OperatingPoint(**bad).check()
