"""CPU: the host side of the squared-error maps - the evaluator's --map-source flag and its refusals (each before a model or an
image is touched), the argument checks of srad_error_maps / srad_error_maps_multi that come before any launch, and a gloo
world-2 run of the evaluator's post-sweep stage with CPU stand-ins for the map kernels: under map_source='mse' both ranks make
the same collective calls for every combination of the other flags, with scales and with the default window size, and none of
them is a broadcast; under map_source='ssim' the calls are those of a run without the argument."""
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
# (map_source or None = the argument is not passed, scales, map_ws)
MODES = [("mse", SCALES, 0), ("mse", (), 0), ("ssim", (), 0), (None, (), 0)]


def test_map_source_defaults_off():
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    from srad_amd import options as Opt
    assert Opt.parse_eval_args([]).map_source == "ssim"
    assert inspect.signature(E.evaluate_on_test).parameters["map_source"].default == "ssim"
    assert E.MapSpec().source == "ssim"
    assert inspect.signature(M.error_maps).parameters["ws"].default == 1
    assert inspect.signature(M.error_maps_multi).parameters["reduce"].default == "mean"
    assert M.MAP_SOURCES == ("ssim", "mse")


def test_map_source_parsing(tmp_path):
    from srad_amd import options as Opt
    assert Opt.parse_eval_args(["--map-source", "mse"]).map_source == "mse"
    assert Opt.parse_eval_args(["--map-source", "ssim"]).map_source == "ssim"
    a = Opt.parse_eval_args(["--map-source", "mse", "--map-scales", "11,21", "--map-reduce", "max", "--map-sigma", "4"])
    assert (a.map_source, a.map_scales, a.map_reduce, a.map_sigma, a.map_ws) == ("mse", [11, 21], "max", 4.0, 0)
    assert Opt.parse_eval_args(["--map-source", "mse", "--map-ws", "7"]).map_ws == 7
    cfg = tmp_path / "eval.yaml"
    cfg.write_text("map_source: mse\nmap_ws: 5\n")
    a = Opt.parse_eval_args(["--config", str(cfg)])
    assert a.map_source == "mse" and a.map_ws == 5
    assert Opt.parse_eval_args(["--config", str(cfg), "--map-source", "ssim"]).map_source == "ssim"     # the command line wins
    cfg.write_text("map_source: psnr\n")
    with pytest.raises(SystemExit):
        Opt.parse_eval_args(["--config", str(cfg)])
    cfg.write_text("map_source: mse\nmap_scales: [11]\nmap_ws: 5\n")
    with pytest.raises(SystemExit):
        Opt.parse_eval_args(["--config", str(cfg)])


@pytest.mark.parametrize("argv", [["--map-source", "psnr"], ["--map-source", "MSE"], ["--map-source", ""], ["--map-source"],
                                  ["--map-source", "mse", "--map-scales", "11,21", "--map-ws", "5"],
                                  ["--map-source", "mse", "--map-scales", "sweep", "--map-ws", "3"],
                                  ["--map-source", "mse", "--map-scales", "11,0"]])
def test_bad_flags_are_refused_when_parsed(argv):
    from srad_amd import options as Opt
    with pytest.raises(SystemExit):
        Opt.parse_eval_args(argv)


def test_refusals_come_before_any_work():
    from srad_amd import evaluate as E
    pair = (np.zeros((16, 16, 1), np.uint8), np.zeros((64, 64, 1), np.uint8))
    # the evaluator checks before it touches the model (None here) or super-resolves anything
    with pytest.raises(ValueError, match="map_source = 'psnr'"):
        E.evaluate_on_test(None, None, [pair], [pair], map_source="psnr", map_image_score=True)
    with pytest.raises(ValueError, match="window 129.*64x64"):
        E.evaluate_on_test(None, None, [pair], [pair], map_source="mse", map_scales=[11, 129], map_image_score=True)
    with pytest.raises(ValueError, match="exclude"):
        E.evaluate_on_test(None, None, [pair], [pair], map_source="mse", map_scales=[11], map_ws=3, map_image_score=True)
    with pytest.raises(ValueError, match="map_reduce"):
        E.evaluate_on_test(None, None, [pair], [pair], map_source="mse", map_scales="sweep", map_reduce="median")
    # the CLI checks against --resolution before it looks for the checkpoint
    with pytest.raises(SystemExit, match="--map-scales: .*window 129"):
        E.main(["--resolution", "64", "--map-source", "mse", "--map-scales", "11,129", "--checkpoint", "does_not_exist.pt"])
    with pytest.raises(FileNotFoundError):                   # fitting scales: the run gets as far as the missing checkpoint
        E.main(["--resolution", "64", "--map-source", "mse", "--map-scales", "11,127", "--run-dir", "does_not_exist_dir"])


def test_python_argument_errors_come_before_the_library():
    from srad_amd import metrics as M
    x = torch.zeros(1, 8, 8, 1, dtype=torch.uint8)           # a CPU tensor: the GPU check would raise RuntimeError
    with pytest.raises(ValueError, match="empty"):
        M.error_maps_multi(x, x, [])
    with pytest.raises(ValueError, match="reduce"):
        M.error_maps_multi(x, x, [3], reduce="sum")
    with pytest.raises(RuntimeError, match="GPU only"):
        M.error_maps_multi(x, x, [3])
    with pytest.raises(RuntimeError, match="GPU only"):
        M.error_maps(x, x)


def test_error_maps_argument_checks_without_gpu():
    from srad_amd import _lib as L
    lib = L.lib()
    SRAD_ERR_ARG = 1
    sr, hr, out, wsp = C.c_void_p(1 << 20), C.c_void_p(1 << 21), C.c_void_p(1 << 30), C.c_void_p(1 << 40)
    three = (C.c_int32 * 3)(3, 11, 21)
    nb, nb_ssim = C.c_size_t(), C.c_size_t()
    assert lib.srad_error_map_workspace_bytes(2, 33, 40, C.byref(nb)) == 0 and nb.value > 0
    assert lib.srad_anomaly_map_workspace_bytes(2, 33, 40, C.byref(nb_ssim)) == 0
    assert 4 * nb.value < nb_ssim.value                      # one table per image, not five
    assert lib.srad_error_map_workspace_bytes(2, 33, 40, None) == SRAD_ERR_ARG
    assert lib.srad_error_map_workspace_bytes(0, 33, 40, C.byref(nb_ssim)) == SRAD_ERR_ARG

    def multi(sr=sr, hr=hr, n=2, H=33, W=40, ch=1, ws=three, n_ws=3, reduce=0, out=out, wsp=wsp, wb=None):
        return lib.srad_error_maps_multi(sr, hr, n, H, W, ch, ws, n_ws, reduce, out, wsp, nb if wb is None else wb, None)

    def single(sr=sr, hr=hr, n=2, H=33, W=40, ch=1, ws=3, out=out, wsp=wsp, wb=None):
        return lib.srad_error_maps(sr, hr, n, H, W, ch, ws, out, wsp, nb if wb is None else wb, None)

    def refused(fn, name, msg, **kw):
        assert fn(**kw) == SRAD_ERR_ARG, kw
        err = lib.srad_last_error()
        assert err.startswith(name + b":") and msg in err, (kw, err)

    refused(multi, b"error_maps_multi", b"empty", n_ws=0)
    refused(multi, b"error_maps_multi", b"empty", n_ws=-1)
    refused(multi, b"error_maps_multi", b"empty", ws=None)
    refused(multi, b"error_maps_multi", b"reduce", reduce=2)
    refused(multi, b"error_maps_multi", b"reduce", reduce=-1)
    refused(multi, b"error_maps_multi", b"window 67 needs more than one reflection of a 33x40", ws=(C.c_int32 * 3)(3, 67, 11))
    refused(multi, b"error_maps_multi", b"window 0 needs", ws=(C.c_int32 * 3)(3, 11, 0))
    refused(multi, b"error_maps_multi", b"window 67 needs", ws=(C.c_int32 * 18)(*([3] * 17 + [67])), n_ws=18)
    refused(multi, b"error_maps_multi", b"window 67 needs", ws=(C.c_int32 * 1)(67), n_ws=1)
    refused(single, b"error_maps", b"window 67 needs more than one reflection of a 33x40", ws=67)
    refused(single, b"error_maps", b"window 0 needs", ws=0)
    for fn, name in ((multi, b"error_maps_multi"), (single, b"error_maps")):
        refused(fn, name, b"bad argument", out=None)
        refused(fn, name, b"bad argument", sr=None)
        refused(fn, name, b"bad argument", hr=None)
        refused(fn, name, b"bad argument", wsp=None)
        refused(fn, name, b"bad argument", n=0)
        refused(fn, name, b"bad argument", H=1)
        refused(fn, name, b"channels", ch=2)
        refused(fn, name, b"too large", H=65536, W=65536)
        refused(fn, name, b"workspace", wb=C.c_size_t(nb.value - 1))
        refused(fn, name, b"workspace", wb=C.c_size_t(0))
    refused(single, b"error_maps", b"workspace", ws=1, wb=C.c_size_t(0))      # ws 1 uses none of it, the contract is one


# ----------------------------------------------------------------------------------- the post-sweep stage under world 2
def _stage_sweeps(rank, world, calls=None):
    """{(mode, flag set): (result, collective calls, saved maps)}; under 'mse' the SSIM map functions must not be called at all."""
    from srad_amd import evaluate as E
    res = {}
    for m, (source, scales, map_ws) in enumerate(MODES):
        cases = [dict(f, map_scales=scales, map_ws=map_ws, map_source=source) for f in FLAG_SETS]
        refuse = {fn: must_not_be_called(fn, "under map_source='mse'") for fn in ("anomaly_maps", "anomaly_maps_multi")}
        for k, r in enumerate(stage_sweep(E, rank, world, cases, calls, **(refuse if source == "mse" else {}))):
            res[m, k] = r
    return res


def test_map_source_stage_gloo_world2():
    assert len(FLAG_SETS) == 64
    one = _stage_sweeps(0, 1)                                # world 1 in this process: the answers rank 0 must reproduce
    res = run_world2(_stage_sweeps)
    for m, (source, scales, map_ws) in enumerate(MODES):
        for k, flags in enumerate(FLAG_SETS):
            (o0, c0, f0), (o1, c1, f1) = res[0][m, k], res[1][m, k]
            w1, _, wf = one[m, k]
            tag = (source, scales, flags)
            assert c0 == c1, (tag, c0, c1)                                # the same collective sequence on both ranks
            assert o1 == {}, tag
            gathers = ["all_gather_object"] if flags["map_image_score"] else []
            if source == "mse":
                assert "broadcast_object_list" not in c0 and "broadcast" not in c0, (tag, c0)     # no best_ws travels
                assert c0 == gathers, (tag, c0)
                if flags["map_image_score"]:
                    assert o0["auc_map_max"] == w1["auc_map_max"], tag
                    for o in (o0, w1):
                        assert o["map_source"] == "mse" and ("map_sigma" in o) == (flags["map_sigma"] > 0)
                        if scales:
                            assert o["map_scales"] == SCALES and o["map_reduce"] == flags["map_reduce"] and "map_ws" not in o
                        else:
                            assert o["map_ws"] == 1 and "map_scales" not in o          # not the sweep's best_ws (5 here)
                else:
                    assert o0 == {} and "auc_map_max" not in w1
                assert "auc_pixel" not in o0 and "aupro" not in o0         # pixel metrics stay --gpus 1 only
            assert_saved_maps_complete(tag[2], f0, f1, wf)                 # every rank wrote its own images' maps
    # map_source='ssim' is the run without the argument: the same calls, results and saved maps, on both ranks and on one
    for with_arg, without in ((2, 3),):
        assert MODES[with_arg][0] == "ssim" and MODES[without][0] is None and MODES[with_arg][1:] == MODES[without][1:]
        for k, flags in enumerate(FLAG_SETS):
            for r in (0, 1):
                (oa, ca, fa), (ob, cb, fb) = res[r][with_arg, k], res[r][without, k]
                assert ca == cb and oa == ob and list(oa) == list(ob) and "map_source" not in oa, (flags, r)
                assert len(fa) == len(fb) and all(na == nb and np.array_equal(ma, mb) for (na, ma), (nb, mb) in zip(fa, fb))
            assert one[with_arg, k][0] == one[without, k][0]
            if not MODES[without][1] and (flags["save_maps"] or flags["map_image_score"]):
                assert "broadcast_object_list" in res[0][without, k][1]    # the default window size still travels for SSIM
