"""CPU: the host side of map smoothing and the map-maximum image score - the argument checks of srad_smooth_maps, scipy's
Gaussian weights, the numpy restatement (tests/golden/make_map_smooth_golden.py) against its own stored golden, the new
evaluator flags, and a gloo world-2 run of the evaluator's post-sweep stage with CPU stand-ins for the two map kernels: rank 0
gets the world-1 ``auc_map_max`` and both ranks make the same collective calls for every combination of flags."""
import ctypes as C
import inspect
import itertools
import os

import numpy as np
import pytest

from tests.helpers import BEST_WS, assert_saved_maps_complete, run_world2, stage_sweep
from tests.helpers import map_smooth_generator as _generator

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_map_smoothing_flags_default_off():
    from srad_amd import evaluate as E
    from srad_amd import options as Opt
    a = Opt.parse_eval_args([])
    assert a.map_sigma == 0.0 and a.map_image_score is False
    a = Opt.parse_eval_args(["--map-sigma", "4", "--map-image-score"])
    assert a.map_sigma == 4.0 and a.map_image_score is True and a.pixel_metrics is False and a.aupro is False
    params = inspect.signature(E.evaluate_on_test).parameters
    names = list(params)
    assert names[-4:] == ["map_sigma", "map_image_score", "aupro", "pro_fpr_limit"]      # aupro's pair stays last
    assert params["map_sigma"].default == 0.0 and params["map_image_score"].default is False


def test_bad_map_sigma_is_refused_before_any_work():
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    from srad_amd import options as Opt
    for bad in ("-1", "-0.5", "nan"):
        with pytest.raises(SystemExit):
            Opt.parse_eval_args(["--map-sigma", bad])
    assert M.smooth_radius(0.0, 64, 64) == 0 and M.smooth_radius(4.0, 64, 64) == 16 and M.smooth_radius(16.0, 64, 64) == 64
    with pytest.raises(ValueError, match="radius 65"):
        M.smooth_radius(16.2, 64, 64)
    with pytest.raises(ValueError, match="radius 129"):
        M.smooth_radius(32.2, 1024, 1024)
    with pytest.raises(ValueError, match=">= 0"):
        M.smooth_radius(-1.0, 64, 64)
    # the evaluator checks before it touches the model (None here) or super-resolves anything
    pair = (np.zeros((16, 16, 1), np.uint8), np.zeros((64, 64, 1), np.uint8))
    for sigma, msg in ((-1.0, ">= 0"), (20.0, "radius 80.*64x64")):
        with pytest.raises(ValueError, match=msg):
            E.evaluate_on_test(None, None, [pair], [pair], map_sigma=sigma, map_image_score=True)
    with pytest.raises(SystemExit, match="--map-sigma 20"):
        E.main(["--resolution", "64", "--map-sigma", "20", "--checkpoint", "does_not_exist.pt"])


def test_smooth_maps_workspace_bytes_checks_without_gpu():
    from srad_amd import _lib as L
    lib = L.lib()
    nb = C.c_size_t()
    assert lib.srad_smooth_maps_workspace_bytes(3, 40, 50, 16, C.byref(nb)) == 0 and nb.value >= 4 * 3
    assert lib.srad_smooth_maps_workspace_bytes(3, 40, 50, 16, None) != 0
    assert lib.srad_smooth_maps_workspace_bytes(0, 40, 50, 16, C.byref(nb)) != 0
    assert lib.srad_smooth_maps_workspace_bytes(3, 0, 50, 16, C.byref(nb)) != 0
    assert lib.srad_smooth_maps_workspace_bytes(3, 40, -1, 16, C.byref(nb)) != 0
    assert lib.srad_smooth_maps_workspace_bytes(2, 32768, 32768, 16, C.byref(nb)) != 0
    assert b"2^31" in lib.srad_last_error()
    assert lib.srad_smooth_maps_workspace_bytes(3, 40, 50, 41, C.byref(nb)) != 0
    assert b"more than one reflection" in lib.srad_last_error()
    assert lib.srad_smooth_maps_workspace_bytes(3, 400, 500, 129, C.byref(nb)) != 0
    assert b"[0, 128]" in lib.srad_last_error()
    assert lib.srad_smooth_maps_workspace_bytes(3, 400, 500, -1, C.byref(nb)) != 0
    assert lib.srad_smooth_maps_workspace_bytes(3, 40, 50, 0, C.byref(nb)) == 0
    assert lib.srad_smooth_maps_workspace_bytes(1, 40, 50, 40, C.byref(nb)) == 0          # radius == min(H, W): one reflection


def test_smooth_maps_argument_checks_without_gpu():
    from srad_amd import _lib as L
    lib = L.lib()
    w = (C.c_double * 129)(*([0.1] * 129))
    maps, out, ws = C.c_void_p(1 << 20), C.c_void_p(1 << 30), C.c_void_p(1 << 40)
    big, small = C.c_size_t(1 << 20), C.c_size_t(4)

    def call(maps=maps, n=2, H=32, W=32, w=w, r=4, out=out, mx=None, ws=ws, wb=big):
        return lib.srad_smooth_maps(maps, n, H, W, w, r, out, mx, ws, wb, None)

    assert call(r=33) != 0 and b"more than one reflection" in lib.srad_last_error()
    assert call(H=500, W=500, r=129) != 0 and b"[0, 128]" in lib.srad_last_error()
    assert call(r=-1) != 0
    assert call(n=0) != 0 and call(H=0) != 0 and call(W=0) != 0
    assert call(maps=None) != 0 and b"NULL" in lib.srad_last_error()
    assert call(out=None) != 0 and b"NULL" in lib.srad_last_error()
    assert call(w=None) != 0 and b"NULL" in lib.srad_last_error()
    assert call(ws=None) != 0 and b"NULL" in lib.srad_last_error()
    nbytes = 2 * 32 * 32 * 4
    for o in (maps.value, maps.value + 4, maps.value + nbytes - 4, maps.value - nbytes + 4):
        assert call(out=C.c_void_p(o)) != 0 and b"overlaps" in lib.srad_last_error(), o
    assert call(wb=small) != 0 and b"workspace" in lib.srad_last_error()
    assert call(wb=C.c_size_t(0)) != 0 and b"workspace" in lib.srad_last_error()


@pytest.mark.parametrize("sigma", [0.3, 0.5, 1.0, 1.5, 2.0, 3.3, 4.0, 7.0, 8.0, 16.0, 31.9])
def test_gaussian_weights_are_scipys(sigma):
    from scipy.ndimage._filters import _gaussian_kernel1d
    from srad_amd import metrics as M
    r = int(4.0 * sigma + 0.5)
    want = _gaussian_kernel1d(sigma, 0, r)[r:]
    got = M.gaussian_weights(sigma)
    assert got.dtype == np.float64 and got.shape == (r + 1,)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(_generator().gaussian_weights_ref(sigma).view(np.uint64), want.view(np.uint64))
    r3 = int(3.0 * sigma + 0.5)
    assert np.array_equal(M.gaussian_weights(sigma, truncate=3.0), _gaussian_kernel1d(sigma, 0, r3)[r3:])


def test_numpy_restatement_reproduces_the_golden():
    G = _generator()
    g = np.load(os.path.join(GOLDEN_DIR, "map_smooth_golden.npz"))
    n_checked = 0
    for name, (n, H, W, salt, sigmas) in G.CASES.items():
        m = g[f"{name}/maps"]
        assert m.dtype == np.float32 and m.shape == (n, H, W)
        assert np.array_equal(G.case_maps(name), m, equal_nan=True)
        assert tuple(g[f"{name}/sigmas"]) == sigmas
        for s in sigmas:
            want = g[f"{name}/out_{s:g}"]
            assert np.array_equal(G.smooth_ref(m, s).view(np.uint32), want.view(np.uint32)), (name, s)
            n_checked += 1
    assert n_checked == 12
    assert int(np.isnan(g["odd_45x63/maps"]).sum()) == 1 and (g["odd_45x63/maps"] == 0).mean() > 0.1
    assert int(4.0 * 4.0 + 0.5) == 16 == min(g["radius_eq_h_16x40/maps"].shape[1:])
    assert int(4.0 * 6.0 + 0.5) == 24 == min(g["radius_eq_w_40x24/maps"].shape[1:])


def test_golden_tells_the_tap_order_apart():
    """scipy adds the taps from the farthest inward; on the signed cancelling cases the other order gives other fp32 values, so
    the golden (and the GPU test against it) pins the order, not only the set of taps."""
    G = _generator()
    g = np.load(os.path.join(GOLDEN_DIR, "map_smooth_golden.npz"))
    for name in G.SIGNED:
        s = G.CASES[name][4][0]
        m, want = g[f"{name}/maps"], g[f"{name}/out_{s:g}"]
        assert m.min() < -0.5 and m.max() > 0.5
        assert np.array_equal(G.smooth_ref(m, s).view(np.uint32), want.view(np.uint32))
        assert int((G.smooth_ref(m, s, inward=False).view(np.uint32) != want.view(np.uint32)).sum()) >= 20, name


def test_restatement_tap_order_is_scipys_in_fp64():
    """The fp64 sum itself, before any fp32 rounding: gaussian_filter1d(..., output=float64) equals the inward order on every
    output and the outward order on far fewer."""
    from scipy import ndimage
    G = _generator()
    x = (((np.arange(4001) * 2654435761) % 1000003) / 1000003.0 - 0.5).astype(np.float64)
    w = G.gaussian_weights_ref(4.0)
    r = len(w) - 1
    ref = ndimage.gaussian_filter1d(x, 4.0, output=np.float64, mode='reflect', truncate=4.0)
    idx = np.arange(-r, len(x) + r)
    e = x[np.where(idx < 0, -idx - 1, np.where(idx >= len(x), 2 * len(x) - 1 - idx, idx))]
    n = len(x)
    for order, want_all in ((range(r, 0, -1), True), (range(1, r + 1), False)):
        acc = e[r:r + n] * w[0]
        for j in order:
            acc = acc + (e[r - j:r - j + n] + e[r + j:r + j + n]) * w[j]
        assert np.array_equal(acc, ref) == want_all


def test_numpy_restatement_matches_scipy_on_a_large_map():
    from scipy import ndimage
    G = _generator()
    m = G.hashed_maps(2, 200, 300, 9)
    for s in (3.0, 16.0):
        want = ndimage.gaussian_filter(m, (0, s, s), mode='reflect', truncate=4.0)
        assert np.array_equal(G.smooth_ref(m, s).view(np.uint32), want.view(np.uint32)), s


# ----------------------------------------------------------------------------------- the post-sweep stage under world 2
FLAG_SETS = [dict(save_maps=a, map_image_score=b, pixel_metrics=c, aupro=p, map_sigma=d, map_ws=e)
             for a, b, c, p, d, e in itertools.product((False, True), (False, True), (False, True), (False, True), (0.0, 4.0),
                                                       (0, 3))]


def _stage_job(rank, world, calls):
    from srad_amd import evaluate as E
    return stage_sweep(E, rank, world, FLAG_SETS, calls)


def test_map_image_score_stage_gloo_world2():
    from srad_amd import evaluate as E
    one = stage_sweep(E, 0, 1, FLAG_SETS)                    # world 1 in this process: the answers rank 0 must reproduce
    res = run_world2(_stage_job)
    for k, flags in enumerate(FLAG_SETS):
        (o0, c0, f0), (o1, c1, f1) = res[0][k], res[1][k]
        w1, _, wf = one[k]
        assert c0 == c1, (flags, c0, c1)                                  # the same collective sequence on both ranks
        assert o1 == {}, flags
        ws = flags["map_ws"] or BEST_WS
        if flags["map_image_score"]:
            assert o0["auc_map_max"] == w1["auc_map_max"] and o0["map_ws"] == w1["map_ws"] == ws, flags
            assert c0.count("all_gather_object") == 1
            assert ("map_sigma" in o0) == (flags["map_sigma"] > 0) and ("map_sigma" in w1) == (flags["map_sigma"] > 0)
        else:
            assert "auc_map_max" not in o0 and "auc_map_max" not in w1
        assert "auc_pixel" not in o0 and "aupro" not in o0                 # pixel metrics stay --gpus 1 only
        assert_saved_maps_complete(flags, f0, f1, wf)                      # every rank wrote its own images' maps
        if not (flags["save_maps"] or flags["map_image_score"]):
            assert c0 == [] and o0 == {}
    base = [one[k][0] for k, f in enumerate(FLAG_SETS) if f["map_image_score"] and f["map_sigma"] == 0 and f["map_ws"] == 0]
    smooth = [one[k][0] for k, f in enumerate(FLAG_SETS) if f["map_image_score"] and f["map_sigma"] > 0 and f["map_ws"] == 0]
    assert len({b["auc_map_max"] for b in base}) == 1 and len({s["auc_map_max"] for s in smooth}) == 1
    assert 0.5 < base[0]["auc_map_max"] <= 1.0
