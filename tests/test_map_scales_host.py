"""CPU: the host side of the multi-scale anomaly maps - the evaluator's --map-scales / --map-reduce flags and their refusals
(each before a model or an image is touched), the argument checks of srad_anomaly_maps_multi that come before any launch, and
a gloo world-2 run of the evaluator's post-sweep stage with CPU stand-ins for the map kernels: with the scales set both ranks
make the same collective calls for every combination of the other flags, and the sweep's best_ws is never broadcast."""
import ctypes as C
import inspect
import itertools
import os
import socket

import numpy as np
import pytest
import torch

from tests.test_map_smooth_host import N_IMG, _cpu_anomaly_maps, _cpu_smooth_maps, _images

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
    stage = inspect.signature(E._pixel_stage).parameters
    assert list(stage)[-2:] == ["map_scales", "map_reduce"] and stage["map_scales"].default == ()


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
def _cpu_anomaly_maps_multi(sr, hr, sizes, reduce="mean"):
    acc = _cpu_anomaly_maps(sr, hr, sizes[0])
    for ws in sizes[1:]:
        m = _cpu_anomaly_maps(sr, hr, ws)
        acc = torch.maximum(acc, m) if reduce == "max" else acc + m
    return acc * float(np.float32(1.0 / len(sizes))) if reduce == "mean" else acc


def _refuse_single_map(*a, **k):
    raise AssertionError("anomaly_maps called although map_scales is set")


def _stage(E, rank, world, flags, saved):
    mine = E.shard_indices(N_IMG, rank, world)
    sr, hr = _images(mine)
    y_true = [0, 0, 0] + [1] * (N_IMG - 3)
    names = [f"im{i}" for i in range(N_IMG)]
    del saved[:]
    out = E._pixel_stage(sr, hr, mine, y_true, names, "unused_dir", None, flags["pixel_metrics"], flags["save_maps"], 0,
                         5 if rank == 0 else None, world, flags["aupro"], 0.3, flags["map_sigma"], flags["map_image_score"], rank,
                         map_scales=SCALES, map_reduce=flags["map_reduce"])
    return out, list(saved)


def _install_stand_ins(E, calls, saved):
    import torch.distributed as dist
    E.M.anomaly_maps = _refuse_single_map
    E.M.anomaly_maps_multi = _cpu_anomaly_maps_multi
    E.M.smooth_maps = _cpu_smooth_maps
    E.save_anomaly_maps = lambda maps, names, splits, d: saved.append((list(names), maps.clone()))
    for fn in ("all_gather_object", "broadcast_object_list", "all_reduce", "barrier", "gather_object", "broadcast", "all_gather"):
        real = getattr(dist, fn)

        def counted(*a, _real=real, _fn=fn, **k):
            calls.append(_fn)
            return _real(*a, **k)
        setattr(dist, fn, counted)


def _stage_worker(rank, world, port, q):
    import torch.distributed as dist
    from srad_amd import evaluate as E
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls, saved = [], []
    _install_stand_ins(E, calls, saved)
    res = []
    for flags in FLAG_SETS:
        del calls[:]
        out, files = _stage(E, rank, world, flags, saved)
        res.append((out, list(calls), [(names, m.numpy()) for names, m in files]))
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def test_map_scales_stage_gloo_world2():
    import torch.multiprocessing as mp
    from srad_amd import evaluate as E
    assert len(FLAG_SETS) == 64
    saved = []
    saved_fns = (E.M.anomaly_maps, E.M.anomaly_maps_multi, E.M.smooth_maps, E.save_anomaly_maps)
    try:                                                     # world 1 in this process: the answers rank 0 must reproduce
        E.M.anomaly_maps, E.M.anomaly_maps_multi, E.M.smooth_maps = _refuse_single_map, _cpu_anomaly_maps_multi, _cpu_smooth_maps
        E.save_anomaly_maps = lambda maps, names, splits, d: saved.append((list(names), maps.clone()))
        one = [_stage(E, 0, 1, f, saved) for f in FLAG_SETS]
    finally:
        E.M.anomaly_maps, E.M.anomaly_maps_multi, E.M.smooth_maps, E.save_anomaly_maps = saved_fns
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_stage_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in procs:
            r, out = q.get(timeout=240)
            res[r] = out
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert [p.exitcode for p in procs] == [0, 0]
    for k, flags in enumerate(FLAG_SETS):
        (o0, c0, f0), (o1, c1, f1) = res[0][k], res[1][k]
        w1, wf = one[k]
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
        if flags["save_maps"]:                                             # every rank wrote its own images' maps
            got = {n: m[j] for names, m in f0 + f1 for j, n in enumerate(names)}
            want = {n: m[j].numpy() for names, m in wf for j, n in enumerate(names)}
            assert sorted(got) == sorted(want) == [f"im{i}" for i in range(N_IMG)]
            for n in want:
                assert np.array_equal(got[n], want[n]), (flags, n)
        else:
            assert not f0 and not f1 and not wf
    by_reduce = {r: {one[k][0]["auc_map_max"] for k, f in enumerate(FLAG_SETS)
                     if f["map_image_score"] and f["map_sigma"] == 0 and f["map_reduce"] == r} for r in ("mean", "max")}
    assert all(len(v) == 1 for v in by_reduce.values())
