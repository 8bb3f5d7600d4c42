"""CPU: the host side of AU-PRO - the evaluator's new flags, the argument checks of srad_mask_regions / srad_pixel_pro, and the
numpy restatement of the metric (tests/golden/make_pro_golden.py) against its own stored golden, so the reference the GPU tests
use is itself pinned."""
import ctypes as C
import importlib.util
import inspect
import os

import numpy as np
import pytest

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL = ["blobs", "corner", "borders", "wrap64", "spiral", "almost_full", "good_plus_one_bad", "zeros"]


def _generator():
    spec = importlib.util.spec_from_file_location("make_pro_golden", os.path.join(GOLDEN_DIR, "make_pro_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_aupro_flags_default_off():
    from srad_amd import evaluate as E
    from srad_amd import options as Opt
    a = Opt.parse_eval_args([])
    assert a.aupro is False and a.pro_fpr_limit == 0.3 and a.pixel_metrics is False
    a = Opt.parse_eval_args(["--aupro", "--pro-fpr-limit", "0.05"])
    assert a.aupro is True and a.pro_fpr_limit == 0.05 and a.pixel_metrics is False
    params = list(inspect.signature(E.evaluate_on_test).parameters.values())
    assert [p.name for p in params[-2:]] == ["aupro", "pro_fpr_limit"]
    assert params[-2].default is False and params[-1].default == 0.3


def test_argument_errors_of_the_pro_entry_points_without_gpu():
    from srad_amd import _lib as L
    lib = L.lib()
    nb = C.c_size_t()
    for fn in (lib.srad_mask_regions_workspace_bytes, lib.srad_pixel_pro_workspace_bytes):
        assert fn(0, 32, 32, C.byref(nb)) != 0
        assert fn(2, 0, 32, C.byref(nb)) != 0
        assert fn(2, 32, -1, C.byref(nb)) != 0
        assert fn(2, 32768, 32768, C.byref(nb)) != 0                       # 2^31 pixels
        assert b"2^31" in lib.srad_last_error()
        assert fn(2, 32, 32, None) != 0
    assert lib.srad_mask_regions_workspace_bytes(3, 40, 50, C.byref(nb)) == 0 and nb.value >= 4 * 3 * 40 * 50
    assert lib.srad_pixel_pro_workspace_bytes(3, 40, 50, C.byref(nb)) == 0 and nb.value >= 16 * 3 * 40 * 50


@pytest.mark.parametrize("limit", [0.0, -0.1, 1.5, float("nan")])
def test_pixel_pro_rejects_a_bad_limit_without_gpu(limit):
    from srad_amd import _lib as L
    lib = L.lib()
    fake, big = C.c_void_p(4096), C.c_size_t(1 << 40)
    assert lib.srad_pixel_pro(fake, fake, 2, 32, 32, C.c_double(limit), fake, fake, None, None, C.c_int64(0), fake, big, None) != 0
    assert b"fpr_limit" in lib.srad_last_error()


def test_pixel_pro_and_mask_regions_argument_checks_without_gpu():
    from srad_amd import _lib as L
    lib = L.lib()
    fake, big, small = C.c_void_p(4096), C.c_size_t(1 << 40), C.c_size_t(16)
    # mask_regions: NULLs, shape, workspace
    assert lib.srad_mask_regions(None, 2, 32, 32, fake, fake, fake, big, None) != 0
    assert b"NULL" in lib.srad_last_error()
    assert lib.srad_mask_regions(fake, 2, 32, 32, None, fake, fake, big, None) != 0
    assert lib.srad_mask_regions(fake, 2, 32, 32, fake, None, fake, big, None) != 0
    assert lib.srad_mask_regions(fake, 0, 32, 32, fake, fake, fake, big, None) != 0
    assert lib.srad_mask_regions(fake, 2, 32, 32, fake, fake, fake, small, None) != 0
    assert b"workspace" in lib.srad_last_error()
    # pixel_pro: NULLs, the curve pair, shape, workspace
    one = C.c_double(0.3)
    assert lib.srad_pixel_pro(None, fake, 2, 32, 32, one, fake, fake, None, None, C.c_int64(0), fake, big, None) != 0
    assert b"NULL" in lib.srad_last_error()
    assert lib.srad_pixel_pro(fake, None, 2, 32, 32, one, fake, fake, None, None, C.c_int64(0), fake, big, None) != 0
    assert lib.srad_pixel_pro(fake, fake, 2, 32, 32, one, None, fake, None, None, C.c_int64(0), fake, big, None) != 0
    assert lib.srad_pixel_pro(fake, fake, 2, 32, 32, one, fake, None, None, None, C.c_int64(0), fake, big, None) != 0
    assert lib.srad_pixel_pro(fake, fake, 2, 32, 32, one, fake, fake, None, None, C.c_int64(0), None, big, None) != 0
    assert lib.srad_pixel_pro(fake, fake, 2, 32, 32, one, fake, fake, fake, None, C.c_int64(8), fake, big, None) != 0
    assert b"curve" in lib.srad_last_error()
    assert lib.srad_pixel_pro(fake, fake, 2, 32, 32, one, fake, fake, fake, fake, C.c_int64(-1), fake, big, None) != 0
    assert lib.srad_pixel_pro(fake, fake, 2, 32768, 32768, one, fake, fake, None, None, C.c_int64(0), fake, big, None) != 0
    assert b"2^31" in lib.srad_last_error()
    assert lib.srad_pixel_pro(fake, fake, 2, 32, 32, one, fake, fake, None, None, C.c_int64(0), fake, small, None) != 0
    assert b"workspace" in lib.srad_last_error()


@pytest.mark.parametrize("case", SMALL)
def test_numpy_restatement_reproduces_the_golden(case):
    G = _generator()
    g = np.load(os.path.join(GOLDEN_DIR, "pro_golden.npz"))
    s, m, sizes = g[f"{case}/s"], g[f"{case}/m"], g[f"{case}/sizes"]
    R, n_ok, n_def = [int(v) for v in g[f"{case}/counts"]]
    assert n_ok == int((m == 0).sum()) and n_def == int((m != 0).sum()) and n_ok + n_def == m.size
    z, r = G.uf_sizes(m)                                                  # the pure-Python labeller the GPU tests use
    assert r == R and np.array_equal(z, sizes.astype(np.int64))
    fpr, pro = G.pro_curve_ref(s, sizes, R)
    assert np.array_equal(fpr, g[f"{case}/fpr"]) and np.array_equal(pro, g[f"{case}/pro"])
    assert fpr[0] == pro[0] == 0.0 and fpr[-1] == pro[-1] == 1.0
    assert np.all(np.diff(fpr) >= 0) and np.all(np.diff(pro) >= 0)
    assert len(fpr) == len(np.unique(s.astype(np.float64))) + 2
    for L, want in zip(g[f"{case}/limits"], g[f"{case}/aupro"]):
        assert G.aupro_ref(fpr, pro, float(L)) == float(want)


def test_golden_pins_the_definition():
    """Hand-checkable facts of the stored cases: 8- vs 4-connectivity, no merge across a row or image end, one spiral."""
    g = np.load(os.path.join(GOLDEN_DIR, "pro_golden.npz"))
    corner = g["corner/sizes"][0]
    assert corner[3, 3] == corner[4, 4] == 2 and int(g["corner/counts"][0]) == 2
    b = g["borders/sizes"]
    assert b[1, 5, 44] == 1 and b[1, 6, 0] == 1                           # row end / next row start: two regions
    assert b[1, 36, 31] == 3 and b[2, 0, 31] == 3                         # image end / next image start: two regions
    assert b[2, 20, 44] == 1 and b[2, 21, 0] == 2
    w = g["wrap64/sizes"]
    assert w[0, 31, 63] == 1 and w[0, 32, 0] == 1 and w[1, 31, 32] == 2 and w[1, 40, 31] == 2
    assert int(g["spiral/counts"][0]) == 1 and g["spiral/sizes"].max() == int(g["spiral/m"].sum())
    assert int(g["almost_full/counts"][1]) == 1
    lim = g["blobs/limits"]
    assert float(lim[3]) in set(g["blobs/fpr"].tolist())                  # a limit that is a curve point's fpr
