"""CPU: the host side of the defect regions (DESIGN.md "Defect regions") - the numpy restatement of the table
(tests/regions_ref.py) against the scipy tables of tests/golden/regions_golden.npz, ``metrics.region_stats`` on hand-built
tables, ``predict.source_box``, the ``regions.csv`` writer, the new flags' parser errors and the argument checks of
srad_region_table without a GPU."""
import csv
import ctypes as C
import os

import numpy as np
import pytest

from tests import regions_ref as R

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL = ["blobs", "corner", "borders", "wrap64", "spiral", "almost_full", "good_plus_one_bad", "zeros"]


@pytest.fixture(scope="module")
def goldens():
    return np.load(os.path.join(GOLDEN_DIR, "pro_golden.npz")), np.load(os.path.join(GOLDEN_DIR, "regions_golden.npz"))


def golden_table(reg, case, role):
    t = {k: reg[f"{case}/{role}/{k}"] for k in R.FIELDS + R.PEAK}
    t["n_regions"] = len(t["area"])
    return t


@pytest.mark.parametrize("case", SMALL)
def test_ref_equals_the_scipy_golden(goldens, case):
    """Record order, boxes, sums, overlaps and the peak with its tie-break, in both roles."""
    pro, reg = goldens
    s, m = pro[f"{case}/s"], pro[f"{case}/m"] != 0
    pred = s.astype(np.float64) > float(reg["threshold"])
    for role, (a, b) in (("gt", (m, pred)), ("pred", (pred, m))):
        want = golden_table(reg, case, role)
        got = R.region_table_ref(a, s, b)
        R.assert_tables_equal(got, want, where=(case, role))
        assert got["n_nan"] == 0
        if role == "gt":
            assert want["n_regions"] == int(pro[f"{case}/counts"][0])
            sizes = pro[f"{case}/sizes"]                           # every area is the stored size at the region's first pixel
            firsts = [(i,) + root for i in range(len(m)) for root in sorted(set(R.label_roots(m[i]).values()))]
            assert [int(sizes[f]) for f in firsts] == want["area"].tolist()
    # the goldens have ties at the peak: somewhere the first of equal maxima is not the last
    if case in ("blobs", "zeros", "almost_full"):
        t = golden_table(reg, case, "gt")
        tied = 0
        for k in range(t["n_regions"]):
            i, (y0, x0, y1, x1) = int(t["image"][k]), t["box"][k]
            tied += int((s[i, y0:y1 + 1, x0:x1 + 1] == t["peak"][k]).sum() > 1)
        assert tied > 0


def _table(image, area, overlap):
    return dict(image=np.array(image, np.int32), area=np.array(area, np.int32), overlap=np.array(overlap, np.int32))


def test_region_stats_on_hand_built_tables():
    from srad_amd import metrics as M
    # images 0, 1 good, 2, 3 bad.  Predicted: one speck on good image 1; on image 2 two regions that both touch one ground-truth
    # region and one that touches nothing; on image 3 one region that spans two ground-truth regions.
    pred = _table([1, 2, 2, 2, 3], [3, 10, 12, 4, 50], [0, 6, 2, 0, 30])
    gt = _table([2, 3, 3, 3], [16, 20, 10, 8], [8, 20, 10, 0])     # the last one is missed
    st = M.region_stats(pred, gt, 4, [0, 0, 1, 1])
    assert st == dict(region_pred=5, region_hit=3, region_precision=3 / 5, region_false_alarms=2, false_alarms_per_image=2 / 4,
                      false_alarms_on_good=1, region_gt=4, region_found=3, region_recall=3 / 4)
    assert list(st) == ["region_pred", "region_hit", "region_precision", "region_false_alarms", "false_alarms_per_image",
                        "false_alarms_on_good", "region_gt", "region_found", "region_recall"]
    # min_overlap: needs max(1, ceil(f * area)) pixels - 8 of 16 is exactly one half, 20 of 20 and 10 of 10 are all
    assert M.region_stats(pred, gt, 4, [0, 0, 1, 1], 0.5)["region_found"] == 3
    assert M.region_stats(pred, _table([2], [17], [8]), 4, [0, 0, 1, 1], 0.5)["region_found"] == 0      # ceil(8.5) = 9
    assert M.region_stats(pred, gt, 4, [0, 0, 1, 1], 1.0)["region_found"] == 2
    assert M.region_stats(pred, gt, 4, [0, 0, 1, 1], 0.0)["region_found"] == 3                          # never without a pixel
    assert M.region_stats(pred, gt, 4, [0, 0, 1, 1], 1.0)["region_hit"] == 3                            # the prediction side is not moved
    # zero regions on either side: ratios with a zero denominator are 0.0
    none = _table([], [], [])
    st = M.region_stats(none, gt, 4, [0, 0, 1, 1])
    assert (st["region_pred"], st["region_precision"], st["false_alarms_per_image"], st["false_alarms_on_good"]) == (0, 0.0, 0.0, 0)
    assert (st["region_gt"], st["region_found"]) == (4, 3)
    st = M.region_stats(pred, none, 4, [0, 0, 1, 1])
    assert (st["region_gt"], st["region_found"], st["region_recall"]) == (0, 0, 0.0) and st["region_pred"] == 5
    st = M.region_stats(none, none, 0, [])
    assert st["false_alarms_per_image"] == 0.0 and st["region_precision"] == 0.0 and st["region_recall"] == 0.0
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="min_overlap"):
            M.region_stats(pred, gt, 4, [0, 0, 1, 1], bad)
    with pytest.raises(ValueError, match="labels"):
        M.region_stats(pred, gt, 4, [0, 0, 1])


def test_source_box():
    from fractions import Fraction
    from math import ceil, floor
    from srad_amd.predict import source_box
    assert source_box((3, 5, 7, 9), (32, 48), (32, 48)) == (3, 5, 7, 9)                  # M == S: the identity
    assert source_box((0, 0, 31, 47), (32, 48), (32, 48)) == (0, 0, 31, 47)
    assert source_box((1, 2, 1, 2), (4, 4), (8, 12)) == (2, 6, 3, 8)                      # upscaling: a pixel becomes a block
    assert source_box((2, 3, 5, 6), (8, 8), (4, 2)) == (1, 0, 2, 1)                       # downscaling
    assert source_box((5, 5, 5, 5), (8, 8), (2, 2)) == (1, 1, 1, 1)                       # several model pixels in one source pixel
    assert source_box((0, 0, 7, 7), (8, 8), (3, 5)) == (0, 0, 2, 4)                       # the whole frame is the whole image
    for m in range(1, 13):
        for s in range(1, 13):
            for c0 in range(m):
                for c1 in range(c0, m):
                    y0, _, y1, _ = source_box((c0, 0, c1, 0), (m, 1), (s, 1))
                    assert 0 <= y0 <= y1 <= s - 1, (m, s, c0, c1)
                    assert y0 == floor(Fraction(c0 * s, m)) and y1 == min(s - 1, ceil(Fraction((c1 + 1) * s, m)) - 1)
                    if m == s:
                        assert (y0, y1) == (c0, c1)
    for bad in ((3, 0, 2, 0), (0, 0, 4, 0), (-1, 0, 2, 0)):
        with pytest.raises(ValueError):
            source_box(bad, (4, 4), (8, 8))


def test_regions_csv_columns(tmp_path):
    from srad_amd.predict import write_regions_csv
    table = dict(image=np.array([0, 2, 2], np.int32), area=np.array([4, 3, 1], np.int32),
                 box=np.array([[1, 2, 2, 3], [0, 0, 0, 2], [5, 5, 5, 5]], np.int32), sum_y=np.array([6, 0, 5], np.int64),
                 sum_x=np.array([10, 3, 5], np.int64), overlap=np.array([0, 2, 0], np.int32),
                 peak=np.array([0.1, 0.75, 1e-30], np.float32), peak_y=np.array([1, 0, 5], np.int32),
                 peak_x=np.array([3, 1, 5], np.int32), n_regions=3)
    names, kinds = ["a", "b", "c"], ["good", "good", "bad"]
    base = ["name", "kind", "region", "area", "y0", "x0", "y1", "x1", "centroid_y", "centroid_x", "peak", "peak_y", "peak_x"]
    path = tmp_path / "plain" / "regions.csv"
    assert write_regions_csv(path, table, names, kinds) == 3
    rows = list(csv.reader(open(path, newline="")))
    assert rows[0] == base
    assert rows[1] == ["a", "good", "0", "4", "1", "2", "2", "3", repr(6 / 4), repr(10 / 4), repr(float(np.float32(0.1))), "1", "3"]
    assert rows[2][:4] == ["c", "bad", "0", "3"] and rows[3][:4] == ["c", "bad", "1", "1"]           # the index restarts per image
    assert float(rows[3][10]) == float(np.float32(1e-30)) and rows[2][8:10] == [repr(0.0), repr(1.0)]
    src = np.array([[2, 4, 5, 7], [0, 0, 1, 5], [10, 10, 11, 11]])
    write_regions_csv(tmp_path / "both.csv", dict(table, gt_overlap=table["overlap"]), names, kinds, src)
    rows = list(csv.reader(open(tmp_path / "both.csv", newline="")))
    assert rows[0] == base + ["gt_overlap", "src_y0", "src_x0", "src_y1", "src_x1"]
    assert rows[2][13:] == ["2", "0", "0", "1", "5"]
    write_regions_csv(tmp_path / "masks.csv", dict(table, gt_overlap=table["overlap"]), names, kinds)
    assert list(csv.reader(open(tmp_path / "masks.csv", newline="")))[0] == base + ["gt_overlap"]
    write_regions_csv(tmp_path / "src.csv", table, names, kinds, src)
    assert list(csv.reader(open(tmp_path / "src.csv", newline="")))[0] == base + ["src_y0", "src_x0", "src_y1", "src_x1"]
    empty = {k: v[:0] for k, v in table.items() if k != "n_regions"}
    assert write_regions_csv(tmp_path / "empty.csv", empty, names, kinds) == 0
    assert list(csv.reader(open(tmp_path / "empty.csv", newline=""))) == [base]


def test_parser_errors(capsys):
    from srad_amd.options import parse_eval_args
    from srad_amd.predict import parse_predict_args
    with pytest.raises(SystemExit):
        parse_eval_args(["--region-metrics"])
    err = capsys.readouterr().err
    assert "--threshold" in err and "--threshold-fpr" in err and "masks" in err
    for argv in (["--threshold", "0.5", "--save-regions"], ["--threshold", "0.5", "--region-min-overlap", "0.5"]):
        with pytest.raises(SystemExit):
            parse_eval_args(argv)
        assert "--region-metrics" in capsys.readouterr().err
    for bad in ("-0.1", "1.5", "nan"):
        with pytest.raises(SystemExit):
            parse_eval_args(["--threshold", "0.5", "--region-metrics", "--region-min-overlap", bad])
        assert "[0, 1]" in capsys.readouterr().err
    a = parse_eval_args(["--threshold-fpr", "0.01", "--region-metrics", "--region-min-overlap", "0.25", "--save-regions"])
    assert (a.region_metrics, a.region_min_overlap, a.save_regions) == (True, 0.25, True)
    a = parse_eval_args(["--threshold", "0.5"])
    assert (a.region_metrics, a.region_min_overlap, a.save_regions) == (False, 0.0, False)
    with pytest.raises(SystemExit):
        parse_predict_args(["--calibrate", "d", "--threshold-fpr", "0.01", "--save-regions"])
    assert "--input" in capsys.readouterr().err
    assert parse_predict_args(["--input", "x.png", "--threshold", "0.5", "--save-regions"]).save_regions is True
    assert parse_predict_args(["--input", "x.png", "--threshold", "0.5"]).save_regions is False


def test_operating_point_spec_defaults_and_checks():
    from srad_amd import evaluate as E
    spec = E.OperatingPoint()
    assert (spec.region_metrics, spec.region_min_overlap, spec.save_regions) == (False, 0.0, False)
    assert E.OperatingPoint(threshold=0.5).check().region_metrics is False
    with pytest.raises(ValueError, match="region_min_overlap"):
        E.OperatingPoint(threshold=0.5, region_metrics=True, region_min_overlap=1.5).check()
    with pytest.raises(ValueError, match="save_regions"):
        E.OperatingPoint(threshold=0.5, save_regions=True).check()


def test_argument_errors_of_region_table_without_gpu():
    from srad_amd import _lib as L
    lib = L.lib()
    nb = C.c_size_t()
    q = lib.srad_region_table_workspace_bytes
    assert q(0, 32, 32, C.byref(nb)) != 0
    assert q(2, 0, 32, C.byref(nb)) != 0
    assert q(2, 32768, 32768, C.byref(nb)) != 0 and b"2^31" in lib.srad_last_error()
    assert q(2, 32, 32, None) != 0 and b"NULL" in lib.srad_last_error()
    assert q(3, 40, 50, C.byref(nb)) == 0 and 12 * 3 * 40 * 50 <= nb.value < 14 * 3 * 40 * 50 + 4096
    fake, big, small = C.c_void_p(4096), C.c_size_t(1 << 40), C.c_size_t(16)
    f = lib.srad_region_table
    cap = C.c_int64(8)
    assert f(None, fake, fake, 2, 32, 32, fake, cap, fake, fake, big, None) != 0 and b"NULL" in lib.srad_last_error()
    assert f(fake, fake, fake, 2, 32, 32, None, cap, fake, fake, big, None) != 0 and b"records_out" in lib.srad_last_error()
    assert f(fake, fake, fake, 2, 32, 32, fake, cap, None, fake, big, None) != 0 and b"NULL" in lib.srad_last_error()
    assert f(fake, fake, fake, 2, 32, 32, fake, cap, fake, None, big, None) != 0 and b"NULL" in lib.srad_last_error()
    assert f(fake, None, None, 2, 32, 32, fake, C.c_int64(-1), fake, fake, big, None) != 0 and b"cap" in lib.srad_last_error()
    assert f(fake, None, None, 0, 32, 32, fake, cap, fake, fake, big, None) != 0
    assert f(fake, None, None, 2, 32768, 32768, fake, cap, fake, fake, big, None) != 0 and b"2^31" in lib.srad_last_error()
    assert f(fake, None, None, 2, 32, 32, fake, cap, fake, fake, small, None) != 0 and b"workspace" in lib.srad_last_error()
    q(2, 32, 32, C.byref(nb))
    assert f(fake, None, None, 2, 32, 32, fake, cap, fake, fake, C.c_size_t(nb.value - 1), None) != 0
    assert b"workspace" in lib.srad_last_error()


def test_wrapper_refuses_bad_arguments_before_the_gpu():
    import torch
    from srad_amd import metrics as M
    with pytest.raises(RuntimeError, match="GPU only"):
        M.region_table(torch.zeros(2, 4, 4, dtype=torch.uint8))
