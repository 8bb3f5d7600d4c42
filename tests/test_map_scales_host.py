"""CPU: the host side of the multi-scale anomaly maps - the evaluator's --map-scales / --map-reduce flags and their refusals
(each before a model or an image is touched), the argument checks of srad_anomaly_maps_multi that come before any launch, and
a gloo world-2 run of the evaluator's post-sweep stage with CPU stand-ins for the map kernels: with the scales set both ranks
make the same collective calls for every combination of the other flags, and the sweep's best_ws is never broadcast."""
import ctypes as C
import inspect
import itertools

import numpy as np
import pytest
import torch

from tests.helpers import assert_saved_maps_complete, must_not_be_called, run_world2, stage_sweep

SCALES = [3, 5, 9]
FLAG_SETS = [dict(save_maps=a, map_image_score=b, pixel_metrics=c, aupro=p, map_sigma=d, map_reduce=r)
             for a, b, c, p, d, r in itertools.product((False, True), (False, True), (False, True), (False, True), (0.0, 4.0),
                                                       ("mean", "max"))]


def test_map_scales_flags_default_off():
    from srad_amd import evaluate as E
    from srad_amd import options as Opt
    a = Opt.parse_eval_args([])
    assert a.map_scales == [] and a.map_reduce == "mean" and a.map_ws == 0
    params = inspect.signature(E.evaluate_on_test).parameters
    assert params["map_scales"].default == () and params["map_reduce"].default == "mean"
    assert E.MapSpec().scales == () and E.MapSpec().reduce == "mean" and E.MapSpec().ws == 0


def test_map_scales_parsing():
    from srad_amd import options as Opt
    a = Opt.parse_eval_args(["--map-scales", "11,21,31"])
    assert a.map_scales == [11, 21, 31] and a.map_reduce == "mean"
    a = Opt.parse_eval_args(["--map-scales", " 21, 3 ,11", "--map-reduce", "max", "--pixel-metrics"])
    assert a.map_scales == [21, 3, 11] and a.map_reduce == "max" and a.pixel_metrics is True
    assert Opt.parse_eval_args(["--map-scales", "7"]).map_scales == [7]
    assert Opt.parse_eval_args(["--map-scales", "11,11"]).map_scales == [11, 11]          # a size twice counts twice
    assert Opt.parse_eval_args(["--map-scales", "sweep"]).map_scales == "sweep"
    assert Opt.parse_eval_args(["--map-scales", "", "--map-ws", "5"]).map_scales == []
    assert Opt.parse_eval_args(["--map-scales", "11", "--map-ws", "0"]).map_scales == [11]


@pytest.mark.parametrize("argv", [["--map-scales", "11,21", "--map-ws", "5"], ["--map-scales", "sweep", "--map-ws", "3"],
                                  ["--map-scales", "11,0"], ["--map-scales", "-3"], ["--map-scales", "11,,21"],
                                  ["--map-scales", "11,x"], ["--map-scales", "2.5"], ["--map-scales", "Sweep"],
                                  ["--map-scales", "11", "--map-reduce", "sum"]])
def test_bad_flags_are_refused_when_parsed(argv):
    from srad_amd import options as Opt
    with pytest.raises(SystemExit):
        Opt.parse_eval_args(argv)


def test_map_scales_from_a_config_file(tmp_path):
    from srad_amd import options as Opt
    cfg = tmp_path / "eval.yaml"
    cfg.write_text("map_scales: [11, 21]\nmap_reduce: max\n")
    a = Opt.parse_eval_args(["--config", str(cfg)])
    assert a.map_scales == [11, 21] and a.map_reduce == "max"
    cfg.write_text("map_scales: [11, 0]\n")
    with pytest.raises(SystemExit):
        Opt.parse_eval_args(["--config", str(cfg)])
    cfg.write_text("map_scales: sweep\nmap_ws: 5\n")
    with pytest.raises(SystemExit):
        Opt.parse_eval_args(["--config", str(cfg)])


def test_scales_the_images_are_too_small_for_are_refused_before_any_work():
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    assert M.check_map_scales([1, 3, 127], 64, 64) == [1, 3, 127] and M.check_map_scales((65,), 40, 33) == [65]
    for bad in ([128], [11, 129], [0], [67]):
        with pytest.raises(ValueError, match="more than one reflection"):
            M.check_map_scales(bad, 64 if bad != [67] else 33, 64 if bad != [67] else 40)
    assert E.resolve_map_scales("sweep", 64, 128) == M.sweep_window_sizes(64) == [3, 13, 23, 33, 43, 53]
    assert E.resolve_map_scales("sweep", 1024, 1024) == M.sweep_window_sizes(1024) and len(M.sweep_window_sizes(1024)) == 102
    assert E.resolve_map_scales([21, 3], 64, 64) == [21, 3]
    with pytest.raises(ValueError):
        E.resolve_map_scales("all", 64, 64)
    # the evaluator checks before it touches the model (None here) or super-resolves anything
    pair = (np.zeros((16, 16, 1), np.uint8), np.zeros((64, 64, 1), np.uint8))
    with pytest.raises(ValueError, match="window 129.*64x64"):
        E.evaluate_on_test(None, None, [pair], [pair], map_scales=[11, 129], map_image_score=True)
    with pytest.raises(ValueError, match="exclude"):
        E.evaluate_on_test(None, None, [pair], [pair], map_scales=[11], map_ws=3, map_image_score=True)
    with pytest.raises(ValueError, match="map_reduce"):
        E.evaluate_on_test(None, None, [pair], [pair], map_scales="sweep", map_reduce="median", map_image_score=True)
    # the CLI checks against --resolution before it looks for the checkpoint
    with pytest.raises(SystemExit, match="--map-scales: .*window 129"):
        E.main(["--resolution", "64", "--map-scales", "11,129", "--checkpoint", "does_not_exist.pt"])
    with pytest.raises(FileNotFoundError):                   # fitting scales: the run gets as far as the missing checkpoint
        E.main(["--resolution", "64", "--map-scales", "11,127", "--run-dir", "does_not_exist_dir"])


def test_anomaly_maps_multi_argument_checks_without_gpu():
    from srad_amd import _lib as L
    lib = L.lib()
    SRAD_ERR_ARG = 1
    sr, hr, out, wsp = C.c_void_p(1 << 20), C.c_void_p(1 << 21), C.c_void_p(1 << 30), C.c_void_p(1 << 40)
    three = (C.c_int32 * 3)(3, 11, 21)
    nb = C.c_size_t()
    assert lib.srad_anomaly_map_workspace_bytes(2, 33, 40, C.byref(nb)) == 0 and nb.value > 0

    def call(sr=sr, hr=hr, n=2, H=33, W=40, ch=1, ws=three, n_ws=3, reduce=0, out=out, wsp=wsp, wb=None):
        return lib.srad_anomaly_maps_multi(sr, hr, n, H, W, ch, ws, n_ws, reduce, out, wsp, nb if wb is None else wb, None)

    def refused(msg, **kw):
        assert call(**kw) == SRAD_ERR_ARG, kw
        err = lib.srad_last_error()
        assert err.startswith(b"anomaly_maps_multi:") and msg in err, (kw, err)

    refused(b"empty", n_ws=0)
    refused(b"empty", n_ws=-1)
    refused(b"empty", ws=None)
    refused(b"reduce", reduce=2)
    refused(b"reduce", reduce=-1)
    refused(b"bad argument", out=None)
    refused(b"bad argument", sr=None)
    refused(b"bad argument", hr=None)
    refused(b"bad argument", wsp=None)
    refused(b"bad argument", n=0)
    refused(b"bad argument", H=1)
    refused(b"channels", ch=2)
    refused(b"too large", H=65536, W=65536)
    refused(b"window 67 needs more than one reflection of a 33x40", ws=(C.c_int32 * 3)(3, 67, 11))
    refused(b"window 0 needs", ws=(C.c_int32 * 3)(3, 11, 0))
    refused(b"window 67 needs", ws=(C.c_int32 * 18)(*([3] * 17 + [67])), n_ws=18)       # in the second launch's part of the list
    refused(b"workspace", wb=C.c_size_t(nb.value - 1))
    refused(b"workspace", wb=C.c_size_t(0))


def test_python_argument_errors_come_before_the_library():
    from srad_amd import metrics as M
    x = torch.zeros(1, 8, 8, 1, dtype=torch.uint8)           # a CPU tensor: the GPU check would raise RuntimeError
    with pytest.raises(ValueError, match="empty"):
        M.anomaly_maps_multi(x, x, [])
    with pytest.raises(ValueError, match="reduce"):
        M.anomaly_maps_multi(x, x, [3], reduce="sum")
    with pytest.raises(RuntimeError, match="GPU only"):
        M.anomaly_maps_multi(x, x, [3])


# ----------------------------------------------------------------------------------- the post-sweep stage under world 2
def _stage_sweep(rank, world, calls=None):
    from srad_amd import evaluate as E
    return stage_sweep(E, rank, world, [dict(f, map_scales=SCALES) for f in FLAG_SETS], calls,
                       anomaly_maps=must_not_be_called("anomaly_maps", "although map_scales is set"))


def test_map_scales_stage_gloo_world2():
    assert len(FLAG_SETS) == 64
    one = _stage_sweep(0, 1)                                 # world 1 in this process: the answers rank 0 must reproduce
    res = run_world2(_stage_sweep)
    for k, flags in enumerate(FLAG_SETS):
        (o0, c0, f0), (o1, c1, f1) = res[0][k], res[1][k]
        w1, _, wf = one[k]
        assert c0 == c1, (flags, c0, c1)                                  # the same collective sequence on both ranks
        assert "broadcast_object_list" not in c0 and "broadcast" not in c0, (flags, c0)       # best_ws does not travel
        assert c0 == (["all_gather_object"] if flags["map_image_score"] else []), (flags, c0)
        assert o1 == {}, flags
        assert "map_ws" not in o0 and "map_ws" not in w1
        if flags["map_image_score"]:
            assert o0["auc_map_max"] == w1["auc_map_max"], flags
            for o in (o0, w1):
                assert o["map_scales"] == SCALES and o["map_reduce"] == flags["map_reduce"]
                assert ("map_sigma" in o) == (flags["map_sigma"] > 0)
        else:
            assert o0 == {} and "auc_map_max" not in w1
        assert "auc_pixel" not in o0 and "aupro" not in o0                 # pixel metrics stay --gpus 1 only
        assert_saved_maps_complete(flags, f0, f1, wf)                      # every rank wrote its own images' maps
    by_reduce = {r: {one[k][0]["auc_map_max"] for k, f in enumerate(FLAG_SETS)
                     if f["map_image_score"] and f["map_sigma"] == 0 and f["map_reduce"] == r} for r in ("mean", "max")}
    assert all(len(v) == 1 for v in by_reduce.values())
