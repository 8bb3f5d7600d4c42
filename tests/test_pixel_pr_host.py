"""CPU: the host side of the precision-recall metrics - ``metrics.average_precision`` (srad_average_precision) against
scikit-learn's numbers (tests/golden/pixel_pr_golden.npz, written by tests/golden/make_pixel_pr_golden.py), its error cases,
the argument checks of srad_pixel_pr, the evaluator's ``--pr-metrics`` flag, and ``evaluate_on_test(pr_metrics=True)`` under the
CPU stand-ins of tests/golden/make_eval_stage_golden.py: the new keys, their order, the new lines, and when the pixel-level
kernel is reached.  Bars: AP within 1e-12 of sklearn (DESIGN.md "Precision-recall"), F1-max equal to the exact fraction."""
import contextlib
import ctypes as C
import importlib.util
import io
import json
import os
import types
from fractions import Fraction

import numpy as np
import pytest

from tests import helpers as T

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN_DIR, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_pixel_pr_golden")
CASES = G.AUC_CASES + G.OWN_CASES


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "pixel_pr_golden.npz"))


@pytest.fixture(scope="module")
def inputs():
    return G.all_cases()


@pytest.mark.parametrize("case", CASES)
def test_average_precision_matches_sklearn_golden(golden, inputs, case):
    from srad_amd import metrics as M
    s, y = inputs[case]
    ap, f1 = M.average_precision(y, s.astype(np.float64))
    assert abs(ap - float(golden[f"{case}/ap"])) <= 1e-12, (case, ap, float(golden[f"{case}/ap"]))
    tp, fp, _ = (int(v) for v in golden[f"{case}/best"])
    assert f1 == float(Fraction(2 * tp, tp + fp + int(np.count_nonzero(y)))), (case, f1, tp, fp)


def test_golden_holds_the_cases(golden):
    assert len(CASES) == 17
    for case in CASES:
        n_pts = int(golden[f"{case}/n_points"])
        assert (f"{case}/thresholds" in golden) == (n_pts <= G.CURVE_MAX), case
    assert [int(v) for v in golden["f1_tie/best"]] == [1, 0, 0x40400000]              # the higher of two thresholds with F1 2/3
    assert [int(v) for v in golden["f1_tie_far/best"]] == [100, 0, 0x41100000]
    assert abs(float(golden["all_pos/ap"]) - 1.0) <= 2e-16 and float(golden["n1/ap"]) == 1.0       # sklearn's sum is one ulp off
    t = golden["inf_zero/thresholds"]
    assert t[0] == np.inf and t[-1] == -np.inf and np.count_nonzero(t == 0) == 1 and not np.signbit(t[t == 0][0])


def test_average_precision_tie_goes_to_the_higher_threshold_and_ignores_order(inputs):
    from srad_amd import metrics as M
    s, y = inputs["f1_tie_far"]
    want = M.average_precision(y, s)
    assert want[1] == 0.4
    p = np.random.default_rng(2).permutation(len(s))
    assert M.average_precision(y[p], s[p]) == want
    assert M.average_precision([0, 1], [0.0, -0.0]) == (0.5, 2 / 3)                   # one tie group: -0.0 == +0.0
    assert M.average_precision([1, 0], [np.inf, -np.inf]) == (1.0, 1.0)


def test_average_precision_errors():
    from srad_amd import metrics as M
    with pytest.raises(ValueError, match="No positive class"):
        M.average_precision([0, 0, 0], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="NaN"):
        M.average_precision([0, 1, 0], [0.1, float("nan"), 0.3])
    with pytest.raises(ValueError, match="equal length"):
        M.average_precision([0, 1], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="1-D"):
        M.average_precision([[0, 1]], [[0.1, 0.2]])
    with pytest.raises(ValueError, match="bad argument"):
        M.average_precision([], [])
    assert M.average_precision([1, 1], [0.3, 0.1]) == (1.0, 1.0)                      # no negative label: defined


def test_argument_errors_of_the_entry_points_without_gpu():
    from srad_amd import _lib as L
    lib = L.lib()
    nb = C.c_size_t()
    assert lib.srad_pixel_pr_workspace_bytes(C.c_int64(0), C.byref(nb)) != 0
    assert lib.srad_pixel_pr_workspace_bytes(C.c_int64(1 << 31), C.byref(nb)) != 0
    assert lib.srad_pixel_pr_workspace_bytes(C.c_int64(1000), C.byref(nb)) == 0 and nb.value >= 16 * 1000
    fake, big = C.c_void_p(4096), C.c_size_t(1 << 40)                                 # never dereferenced: the checks come first
    assert lib.srad_pixel_pr(fake, fake, C.c_int64(0), fake, fake, None, None, None, C.c_int64(0), fake, big, None) != 0
    assert b"[1, 2^31)" in lib.srad_last_error()
    assert lib.srad_pixel_pr(fake, fake, C.c_int64(100), fake, fake, None, None, None, C.c_int64(0), fake, C.c_size_t(16), None) != 0
    assert b"workspace" in lib.srad_last_error()
    assert lib.srad_pixel_pr(None, fake, C.c_int64(100), fake, fake, None, None, None, C.c_int64(0), fake, big, None) != 0
    assert lib.srad_pixel_pr(fake, fake, C.c_int64(100), fake, fake, fake, None, fake, C.c_int64(100), fake, big, None) != 0
    assert b"all be given or all be NULL" in lib.srad_last_error()
    assert lib.srad_pixel_pr(fake, fake, C.c_int64(100), fake, fake, fake, fake, fake, C.c_int64(-1), fake, big, None) != 0
    ap, f1 = C.c_double(), C.c_double()
    assert lib.srad_average_precision(None, None, 3, C.byref(ap), C.byref(f1)) != 0


def test_pr_metrics_flag_default_off():
    from srad_amd import options as Opt
    assert Opt.parse_eval_args([]).pr_metrics is False
    a = Opt.parse_eval_args(["--pr-metrics", "--pixel-metrics"])
    assert a.pr_metrics is True and a.pixel_metrics is True and a.aupro is False and a.threshold is None


def test_no_cpu_fallback():
    import torch
    from srad_amd import metrics as M
    with pytest.raises(RuntimeError, match="GPU only"):
        M.pixel_pr(torch.zeros(4), torch.ones(4))
    with pytest.raises(RuntimeError, match="GPU only"):
        M.pr_curve(torch.zeros(4), torch.ones(4))


# ---------------------------------------------------------------- the evaluator under CPU stand-ins
S = _load("make_eval_stage_golden")
PR_KEYS = ["ap_pixel", "f1max_pixel", "f1max_pixel_threshold", "f1max_pixel_precision", "f1max_pixel_recall"]
IMAGE_KEYS = ["ap_ssim", "ap_mse", "ap_psnr", "f1max_ssim", "f1max_mse", "f1max_psnr"]


def _pixel_pr_stand_in(calls):
    def pixel_pr(scores, labels):
        calls.append((scores.clone(), labels.clone()))
        _, _, thr, tp, fp = G.pr_ref(scores.numpy(), labels.numpy())
        k = G.best_point(tp, fp)
        a, b, P = int(tp[k]), int(fp[k]), int(tp[-1])
        return dict(ap=G.ap_ref(tp, fp), f1max=2 * a / (a + b + P), precision=a / (a + b), recall=a / P, score=float(thr[k]),
                    threshold=float(np.nextafter(thr[k], np.float32(-np.inf))), tp=a, fp=b, fn=P - a, n_pos=P,
                    n_neg=int(scores.numel()) - P)
    return pixel_pr


def _evaluate(masks="all", **kw):
    """``evaluate_on_test`` on the images and under the stand-ins of the eval-stage recording: (result, printed lines, the
    (maps, labels) the pixel_pr stand-in was called with)."""
    from srad_amd import evaluate as E
    calls, saved = [], []
    extra = dict(score_pairs=S._score_pairs, pixel_roc_auc=S._pixel_roc_auc, aupro=S._aupro, map_threshold=S._map_threshold,
                 operating_point=S._operating_point, pixel_pr=_pixel_pr_stand_in(calls))
    m = None if masks is None else S.masks_all()
    if masks == "one_missing":
        m[4] = None
    keep = E.super_resolve_u8
    buf = io.StringIO()
    try:
        E.super_resolve_u8 = S._super_resolve_u8
        with T.stand_ins(E, saved, **extra), contextlib.redirect_stdout(buf):
            res = E.evaluate_on_test(types.SimpleNamespace(rgb_range=255.0, scale=[4]), types.SimpleNamespace(eval=lambda: None),
                                     S._pairs(range(3)), S._pairs(range(3, T.N_IMG)), names=S.NAMES, output_dir="out", masks=m, **kw)
    finally:
        E.super_resolve_u8 = keep
    return res, buf.getvalue().splitlines(), calls


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN_DIR, "eval_stage.json")) as f:
        return json.load(f)


def test_without_the_flag_nothing_changes(recorded):
    for name, kw in (("flags_0000", {}), ("flags_0111", dict(map_image_score=True, pixel_metrics=True, aupro=True))):
        for flag in ({}, dict(pr_metrics=False)):
            res, lines, calls = _evaluate(**kw, **flag)
            assert [[k, v] for k, v in res.items()] == recorded[name]["result"] and lines == recorded[name]["lines"], name
            assert not calls


def test_image_level_keys_lines_and_values(recorded):
    from srad_amd import metrics as M
    res, lines, calls = _evaluate(masks=None, pr_metrics=True)
    base = recorded["flags_0000"]
    assert list(res) == [k for k, _ in base["result"]] + IMAGE_KEYS                   # no masks: the image level only
    assert all(res[k] == v for k, v in base["result"])
    assert lines[0] == base["lines"][0] and lines[1].startswith(f"Test APs - SSIM(best ws={res['best_ws']}): ")
    assert lines[2:] == ["Pixel metrics skipped: 7 test image(s) have no ground-truth mask"] and not calls
    sr, hr = T.stage_images(range(T.N_IMG))
    ssim, mse, psnr = S._score_pairs(sr, hr, res["window_sizes"])
    j = res["window_sizes"].index(res["best_ws"])
    for key, col in (("ssim", 1.0 - ssim[:, j].numpy()), ("mse", mse.numpy()), ("psnr", -psnr.numpy())):
        assert (res[f"ap_{key}"], res[f"f1max_{key}"]) == M.average_precision(T.Y_TRUE, col), key
    assert lines[1] == (f"Test APs - SSIM(best ws={res['best_ws']}): {res['ap_ssim']:.4f}, MSE: {res['ap_mse']:.4f}, "
                        f"PSNR: {res['ap_psnr']:.4f}; F1-max - SSIM: {res['f1max_ssim']:.4f}, MSE: {res['f1max_mse']:.4f}, "
                        f"PSNR: {res['f1max_psnr']:.4f}")
    # the map maximum: two more keys after auc_map_max, one more line after its line
    res2, lines2, calls = _evaluate(masks=None, pr_metrics=True, map_image_score=True)
    rec = recorded["flags_0100"]
    keys = [k for k, _ in rec["result"]]
    at = keys.index("auc_map_max")
    assert list(res2) == keys[:6] + IMAGE_KEYS + keys[6:at + 1] + ["ap_map_max", "f1max_map_max"] + keys[at + 1:] and not calls
    assert all(res2[k] == v for k, v in rec["result"])
    maps = T.cpu_smooth_maps(T.cpu_anomaly_maps(sr, hr, res2["map_ws"]), 0.0, with_max=True)[1]
    assert (res2["ap_map_max"], res2["f1max_map_max"]) == M.average_precision(T.Y_TRUE, maps.double().numpy())
    assert lines2[:1] + lines2[2:3] == rec["lines"][:2]
    assert lines2[3] == f"Image AP - max of the SSIM map (ws={res2['map_ws']}, sigma=0): {res2['ap_map_max']:.4f}, " \
                        f"F1-max: {res2['f1max_map_max']:.4f}"


@pytest.mark.parametrize("others", [dict(), dict(pixel_metrics=True, aupro=True), dict(map_source="mse", map_scales=[3, 7])])
def test_pixel_level_runs_exactly_where_the_gate_lets_it(others):
    res, lines, calls = _evaluate(masks="all", pr_metrics=True, **others)
    assert len(calls) == 1 and list(res)[-len(PR_KEYS):] == PR_KEYS
    maps, labels = calls[0]
    assert tuple(maps.shape) == tuple(labels.shape) == (T.N_IMG, T.HW, T.HW)
    assert np.array_equal(labels.numpy(), np.stack(S.masks_all()))
    want = _pixel_pr_stand_in([])(maps, labels)
    assert [res[k] for k in PR_KEYS] == [want[k] for k in ("ap", "f1max", "threshold", "precision", "recall")]
    what = "MSE map (scales=[3, 7], mean)" if others.get("map_source") == "mse" else f"SSIM map (ws={res['best_ws']})"
    assert lines[-1] == (f"Pixel AP - {what}: {want['ap']:.4f}, F1-max: {want['f1max']:.4f} (precision={want['precision']:.4f} "
                         f"recall={want['recall']:.4f} at threshold={want['threshold']:.9g})")
    if others.get("pixel_metrics"):
        assert list(res)[-len(PR_KEYS) - 3:-len(PR_KEYS)] == ["auc_pixel", "aupro", "pro_fpr_limit"]
        assert [ln.split(" - ")[0] for ln in lines] == ["Test AUCs", "Test APs", "Pixel AUC", "AU-PRO", "Pixel AP"]
    # a missing mask: the gate's own line, no call, and the image level stays
    res, lines, calls = _evaluate(masks="one_missing", pr_metrics=True, **others)
    assert not calls and not set(PR_KEYS) & set(res) and set(IMAGE_KEYS) <= set(res)
    assert lines[-1] == "Pixel metrics skipped: 1 test image(s) have no ground-truth mask"
    # ... but an operating point still runs there, at the image level, and pr adds nothing to it
    res, lines, calls = _evaluate(masks="one_missing", pr_metrics=True, operating_point=dict(threshold=0.02), **others)
    assert not calls and not set(PR_KEYS) & set(res) and "image_tp" in res and "pixel_tp" not in res


def test_f1max_threshold_feeds_the_operating_point():
    """The reported threshold is in the operating point's ``map > threshold`` convention: under the stand-ins, thresholding the
    same maps at it gives the best point's counts."""
    res, _, calls = _evaluate(masks="all", pr_metrics=True)
    maps, labels = calls[0]
    want = _pixel_pr_stand_in([])(maps, labels)
    _, _, counts = S._operating_point(maps, res["f1max_pixel_threshold"], labels)
    assert (counts["tp"], counts["fp"], counts["fn"]) == (want["tp"], want["fp"], want["fn"])
