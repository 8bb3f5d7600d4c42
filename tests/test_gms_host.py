"""CPU: the host side of the gradient-magnitude similarity maps and loss - the restatement of tests/gms_ref.py against a
literal loop, torch's bilinear interpolation and its own invariants; the loss restatement against the maps; the parsers, the
map spec and the loss factory; a gloo world-2 run of the evaluator's post-sweep stage under both GMS sources; and the
argument checks of srad_gms_maps and the GMS loss kinds that come before any launch."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import gms_ref as R
from tests.helpers import assert_saved_maps_complete, must_not_be_called, run_world2, stage_sweep


def _pair(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_ref_matches_the_literal_loop(levels):
    sr, hr = _pair((2, 8, 12, 1), 10 + levels)
    assert np.array_equal(R.gms_maps(sr, hr, levels).view(np.uint32), R.literal(sr, hr, levels).view(np.uint32))


def test_ref_matches_the_literal_loop_rgb():
    sr, hr = _pair((1, 4, 6, 3), 5)
    assert np.array_equal(R.gms_maps(sr, hr, 2).view(np.uint32), R.literal(sr, hr, 2).view(np.uint32))


@pytest.mark.parametrize("f", [2, 4, 8])
def test_ref_upsampling_is_torch_bilinear(f):
    d = np.random.default_rng(f).random((2, 5, 7))
    want = torch.nn.functional.interpolate(torch.from_numpy(d)[:, None], scale_factor=f, mode="bilinear", align_corners=False)[:, 0].numpy()
    got = R.upsample(d, f)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("shape,levels", [((2, 16, 24, 1), 1), ((2, 16, 24, 1), 4), ((1, 24, 40, 3), 3)])
def test_ref_invariants(shape, levels):
    sr, hr = _pair(shape, 3)
    same = R.gms_maps(sr, sr, levels)
    assert same.dtype == np.float32 and not same.any() and not np.signbit(same).any()          # exactly +0.0 everywhere
    a, b = R.gms_maps(sr, hr, levels), R.gms_maps(hr, sr, levels)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))                                # bit-symmetric
    assert (a >= 0).all() and (a < 1).all() and a.max() > 0
    # the extremes: the largest channel sums against black have no edge, so they are exactly 0; a full step is below 1
    white = np.full(shape, 255, np.uint8)
    assert not R.gms_maps(white, np.zeros_like(white), levels).any()
    step = np.zeros(shape, np.uint8)
    step[:, :, shape[2] // 2:] = 255
    m = R.gms_maps(step, np.zeros_like(step), levels)
    assert 0 < m.max() < 1


# --------------------------------------------------------------------------------------------------- the loss restated
@pytest.mark.parametrize("levels", [1, 4])
def test_loss_ref_is_the_mean_of_the_maps(levels):
    sr, hr = _pair((2, 16, 24, 3), 7)
    maps = R.gms_maps(sr, hr, levels).astype(np.float64)      # float32 maps: compare the float64 planes' mean instead
    planes = R.level_planes(sr, hr, levels)
    mean = sum(p.mean() for p in planes) / levels
    t = lambda a: torch.from_numpy(a.astype(np.float64)).permute(0, 3, 1, 2)
    loss = float(R.gms_loss(t(sr), t(hr), levels))
    assert abs(loss - mean) <= 1e-12
    assert abs(maps.mean() - mean) <= 1e-7                     # bilinear upsampling by an integer factor keeps the mean


@pytest.mark.parametrize("levels", [1, 4])
def test_loss_ref_gradient_is_finite_on_a_constant_image(levels):
    sr = torch.full((1, 3, 16, 16), 97.0, dtype=torch.float64, requires_grad=True)
    hr = torch.from_numpy(_pair((1, 3, 16, 16), 1)[0].astype(np.float64))
    R.gms_loss(sr, hr, levels).backward()
    assert torch.isfinite(sr.grad).all() and not sr.grad.any()


def test_loss_inputs_are_well_conditioned():
    for shape, seed in itertools.product(R.LOSS_SHAPES, (1, 2, 3)):
        sr, _ = R.loss_inputs(shape, seed)
        for levels in (1, 4):
            ok, smallest = R.well_conditioned(sr, levels)
            assert ok, (shape, seed, levels, smallest)


# ------------------------------------------------------------------------------------------------------ parsers, specs
def test_map_source_parsing(tmp_path):
    from srad_amd import metrics as M
    from srad_amd import options as Opt
    for src in ("gms", "msgms"):
        a = Opt.parse_eval_args(["--map-source", src, "--map-sigma", "4"])
        assert (a.map_source, a.map_ws, a.map_scales, a.map_sigma) == (src, 0, [], 4.0)
        cfg = tmp_path / f"{src}.yaml"
        cfg.write_text(f"map_source: {src}\n")
        assert Opt.parse_eval_args(["--config", str(cfg)]).map_source == src
        cfg.write_text(f"map_source: {src}\nmap_ws: 5\n")
        with pytest.raises(SystemExit):
            Opt.parse_eval_args(["--config", str(cfg)])
    assert Opt.parse_eval_args([]).map_source == "ssim"
    assert M.MAP_SOURCES == ("ssim", "mse") and M.GMS_MAP_SOURCES == {"gms": 1, "msgms": 4}
    assert Opt.GMS_MAP_SOURCES == tuple(M.GMS_MAP_SOURCES) and Opt.ALL_MAP_SOURCES == M.MAP_SOURCES + tuple(M.GMS_MAP_SOURCES)


@pytest.mark.parametrize("argv", [["--map-source", "gms", "--map-ws", "5"], ["--map-source", "msgms", "--map-scales", "11"],
                                  ["--map-source", "GMS"], ["--map-source", "msgms", "--map-scales", "sweep"]])
def test_bad_map_flags_are_refused_when_parsed(argv):
    from srad_amd import options as Opt
    with pytest.raises(SystemExit):
        Opt.parse_eval_args(argv)


def test_predict_parser_and_spec():
    from srad_amd import predict as P
    base = ["--run-dir", "r", "--input", "x.png"]
    a = P.parse_predict_args(base + ["--map-source", "gms"])
    spec = P.spec_from_args(a)
    assert (spec.source, spec.ws, tuple(spec.scales), spec.levels) == ("gms", 0, (), 1)
    assert P.check_spec(spec) is spec
    assert P.spec_from_args(P.parse_predict_args(base)).ws == P.MAP_WS_DEFAULT                       # the default is as it was
    with pytest.raises(SystemExit):
        P.parse_predict_args(base + ["--map-source", "msgms", "--map-ws", "11"])
    with pytest.raises(SystemExit):
        P.parse_predict_args(base + ["--map-source", "gms", "--map-scales", "11,21"])
    # a stored spec: the same source passes, the other one contradicts it
    assert P.spec_from_args(P.parse_predict_args(base + ["--map-source", "gms"]), stored=spec) is spec
    assert P.spec_from_args(P.parse_predict_args(base), stored=spec) is spec
    with pytest.raises(ValueError, match="--map-source msgms contradicts"):
        P.spec_from_args(P.parse_predict_args(base + ["--map-source", "msgms"]), stored=spec)


def test_map_spec():
    from srad_amd import evaluate as E
    with pytest.raises(ValueError, match=r"^map_source = 'psnr'.*'ssim'.*'mse'.*'gms'.*'msgms'"):
        E.MapSpec("psnr")
    for kw in (dict(ws=5), dict(scales=[11]), dict(scales="sweep")):
        with pytest.raises(ValueError, match="the GMS maps have no window; smooth with map_sigma"):
            E.MapSpec("gms", **kw)
    with pytest.raises(ValueError, match="multiples of 8"):
        E.MapSpec("msgms").resolve(36, 64)
    with pytest.raises(ValueError, match="at least 16"):
        E.MapSpec("msgms").resolve(8, 64)
    assert E.MapSpec("gms").resolve(36, 63).levels == 1
    spec = E.MapSpec("msgms", sigma=4).resolve(64, 64)
    assert (spec.levels, spec.needs_best_ws, spec.ws, list(spec.scales)) == (4, False, 0, [])
    assert spec.text() == "GMS map (levels=4, sigma=4)"
    assert E.MapSpec("gms").text() == "GMS map (levels=1)" and E.MapSpec("gms").text(", fpr <= 0.3") == "GMS map (levels=1, fpr <= 0.3)"
    assert spec.entries(dict(a=1)) == dict(map_source="msgms", map_levels=4, a=1, map_sigma=4.0)
    assert list(E.MapSpec("gms").entries({})) == ["map_source", "map_levels"]
    assert E._with_window(spec, 5, 1) is spec
    # the windowed sources say what they said
    assert E.MapSpec(ws=11).text() == "SSIM map (ws=11)" and E.MapSpec("mse", ws=3).entries({}) == dict(map_source="mse", map_ws=3)
    assert E.MapSpec().levels == 0 and E.MapSpec().needs_best_ws
    # make calls metrics.gms_maps with the level count
    seen = []
    old = E.M.gms_maps
    E.M.gms_maps = lambda sr, hr, levels: seen.append(levels) or torch.zeros(1, 4, 4)
    try:
        maps, mx = E.MapSpec("msgms").make(None, None, False)
    finally:
        E.M.gms_maps = old
    assert seen == [4] and mx is None and maps.shape == (1, 4, 4)


def test_refusals_come_before_any_work():
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    pair = (np.zeros((9, 16, 1), np.uint8), np.zeros((36, 64, 1), np.uint8))
    with pytest.raises(ValueError, match="multiples of 8"):
        E.evaluate_on_test(None, None, [pair], [pair], map_source="msgms", map_image_score=True)
    with pytest.raises(ValueError, match="no window"):
        E.evaluate_on_test(None, None, [pair], [pair], map_source="gms", map_ws=3)
    x = torch.zeros(1, 16, 16, 1, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU only"):
        M.gms_maps(x, x, 4)


def test_loss_flag(tmp_path):
    from srad_amd import options as Opt
    assert Opt.parse_train_args([]).loss == "1*L1"
    assert Opt.parse_train_args(["--loss", "0.8*L1+0.2*MSGMS"]).loss == "0.8*L1+0.2*MSGMS"
    assert Opt.parse_train_args(["--loss", "1e-1*GMS+2*SSIM+1*PSNR+.5*MSE"]).loss == "1e-1*GMS+2*SSIM+1*PSNR+.5*MSE"
    for bad in ("L1", "x*L1", "1*VGG", "1*L1+", "inf*L1", "nan*L1", "1*L1*2", ""):
        with pytest.raises(SystemExit):
            Opt.parse_train_args(["--loss", bad])
    cfg = tmp_path / "train.yaml"
    cfg.write_text("loss: 0.5*L1+0.5*GMS\n")
    assert Opt.parse_train_args(["--config", str(cfg)]).loss == "0.5*L1+0.5*GMS"
    cfg.write_text("loss: 1*VGG\n")
    with pytest.raises(SystemExit):
        Opt.parse_train_args(["--config", str(cfg)])
    assert Opt.build_opt("drct", "grid", 64, 4).loss == "1*L1"
    assert Opt.build_opt("drct", "grid", 64, 4, loss="1*GMS").loss == "1*GMS"
    assert Opt.build_opt("drn-l", "grid", 64, 4, loss="1*GMS").loss == "1*GMS"


def test_train_opt_carries_the_loss_and_checks_its_geometry():
    from srad_amd import main as Mn
    from srad_amd import options as Opt
    assert Mn.build_train_opt(Opt.parse_train_args([])).loss == "1*L1"
    assert Mn.build_train_opt(Opt.parse_train_args(["--loss", "0.8*L1+0.2*MSGMS", "--resolution", "64"])).loss == "0.8*L1+0.2*MSGMS"
    # DRN evaluates the loss on its LR-side outputs too: 64 / 4 = 16 px serves MSGMS, 32 / 4 = 8 px does not
    assert Mn.build_train_opt(Opt.parse_train_args(["--model-type", "drn-l", "--loss", "1*MSGMS", "--resolution", "64"])).loss == "1*MSGMS"
    with pytest.raises(ValueError, match="MSGMS.*at 8 px"):
        Mn.build_train_opt(Opt.parse_train_args(["--model-type", "drn-l", "--loss", "1*MSGMS", "--resolution", "32"]))
    assert Mn.build_train_opt(Opt.parse_train_args(["--model-type", "drn-l", "--loss", "1*GMS", "--resolution", "32"])).loss == "1*GMS"


def test_loss_factory_without_a_gpu():
    from srad_amd import loss as Lo
    from srad_amd import options as Opt
    assert Lo.KINDS["GMS"] == 4 and Lo.KINDS["MSGMS"] == 5 and set(Opt.LOSS_TYPES) == set(Lo.KINDS)

    class Args:
        loss, rgb_range, batch_size = "0.8*L1+0.2*MSGMS", 255, 4
    lf = Lo.Loss(Args())
    assert [(l["type"], l["weight"]) for l in lf.loss] == [("L1", 0.8), ("MSGMS", 0.2), ("Total", 0)]
    assert isinstance(lf.loss[1]["function"], Lo.MSGMSLoss) and lf.loss[1]["function"].kind == 5
    Args.loss = "1*GMS"
    assert isinstance(Lo.Loss(Args()).loss[0]["function"], Lo.GMSLoss)
    Args.loss = "1*VGG"
    with pytest.raises(AssertionError, match="Unsupported loss type"):
        Lo.Loss(Args())
    with pytest.raises(RuntimeError, match="GPU only"):
        Lo.MSGMSLoss(Args())(torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 16, 16))
    from srad_amd.trainer import _plain_l1
    Args.loss = "1*L1"
    assert _plain_l1(Lo.Loss(Args())) and _plain_l1(None)
    Args.loss = "0.8*L1+0.2*MSGMS"
    assert not _plain_l1(Lo.Loss(Args()))


# ------------------------------------------------------------------------------------------ C ABI checks, no device
def test_gms_maps_argument_checks_without_gpu():
    from srad_amd import _lib as L
    lib = L.lib()
    SRAD_ERR_ARG = 1
    sr, hr, out, wsp = C.c_void_p(1 << 20), C.c_void_p(1 << 21), C.c_void_p(1 << 30), C.c_void_p(1 << 40)
    nb, nb1, nb2 = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.srad_gms_map_workspace_bytes(2, 64, 80, 4, C.byref(nb)) == 0
    assert lib.srad_gms_map_workspace_bytes(4, 64, 80, 4, C.byref(nb2)) == 0
    assert lib.srad_gms_map_workspace_bytes(2, 64, 80, 1, C.byref(nb1)) == 0
    cells = sum(2 * (64 >> l) * (80 >> l) for l in (1, 2, 3))
    assert 16 * cells <= nb.value <= 16 * cells + 9 * 256 and nb2.value <= 2 * nb.value and nb1.value <= 256      # linear in n
    assert lib.srad_gms_map_workspace_bytes(2, 64, 80, 4, None) == SRAD_ERR_ARG and b"null" in lib.srad_last_error()

    def maps(sr=sr, hr=hr, n=2, H=64, W=80, ch=1, levels=4, out=out, wsp=wsp, wb=None):
        return lib.srad_gms_maps(sr, hr, n, H, W, ch, levels, out, wsp, nb if wb is None else wb, None)

    def refused(msg, **kw):
        assert maps(**kw) == SRAD_ERR_ARG, kw
        err = lib.srad_last_error()
        assert err.startswith(b"gms_maps:") and msg in err, (kw, err)

    refused(b"levels must be 1..4 (got 0)", levels=0)
    refused(b"levels must be 1..4 (got 5)", levels=5)
    refused(b"channels must be 1 or 3 (got 2)", ch=2)
    refused(b"4 levels need H and W to be multiples of 8 and at least 16 (got 36x64)", H=36, W=64)
    refused(b"at least 16 (got 8x64)", H=8, W=64)
    refused(b"2 levels need H and W to be multiples of 2 and at least 4 (got 64x2)", W=2, levels=2)
    refused(b"at least 2 (got 1x8)", H=1, W=8, levels=1)
    refused(b"bad argument", n=0)
    for name in ("sr", "hr", "out", "wsp"):
        refused(b"null argument", **{name: None})
    refused(b"workspace", wb=C.c_size_t(nb.value - 1))
    refused(b"workspace", wb=C.c_size_t(0))
    for bad in (dict(levels=0), dict(levels=5), dict(H=36), dict(n=0)):
        kw = dict(dict(n=2, H=64, W=80, levels=4), **bad)
        assert lib.srad_gms_map_workspace_bytes(kw["n"], kw["H"], kw["W"], kw["levels"], C.byref(nb1)) == SRAD_ERR_ARG
        assert lib.srad_last_error().startswith(b"gms_map_workspace_bytes:")


def test_gms_loss_argument_checks_without_gpu():
    from srad_amd import _lib as L
    lib = L.lib()
    SRAD_ERR_ARG = 1
    GMS, MSGMS = 4, 5
    sr, hr, out2, wsp, dsr = (C.c_void_p(1 << k) for k in (20, 21, 22, 40, 23))
    nb, nb1 = C.c_size_t(), C.c_size_t()
    assert lib.srad_loss_workspace_bytes(MSGMS, 2, 3, 32, 48, C.byref(nb)) == 0
    assert lib.srad_loss_workspace_bytes(GMS, 2, 3, 32, 48, C.byref(nb1)) == 0 and 0 < nb1.value < nb.value
    for H, W in ((20, 20), (8, 32), (32, 36)):
        assert lib.srad_loss_workspace_bytes(MSGMS, 2, 1, H, W, C.byref(nb1)) == SRAD_ERR_ARG
        err = lib.srad_last_error()
        assert b"multiples of 8 and at least 16" in err and f"{H}x{W}".encode() in err, err
    assert lib.srad_loss_workspace_bytes(GMS, 2, 1, 20, 20, C.byref(nb1)) == 0
    assert lib.srad_loss_workspace_bytes(GMS, 2, 1, 1, 20, C.byref(nb1)) == SRAD_ERR_ARG and b"at least 2" in lib.srad_last_error()
    assert lib.srad_loss_workspace_bytes(GMS, 2, 2, 20, 20, C.byref(nb1)) == SRAD_ERR_ARG and b"1 or 3 channels" in lib.srad_last_error()

    def fwd(kind=MSGMS, sr=sr, hr=hr, C_=3, sH=32, sW=48, H=32, W=48, wb=None):
        return lib.srad_loss_forward(kind, sr, hr, 2, C_, sH, sW, H, W, 255.0, 1, out2, wsp, nb if wb is None else wb, None)

    def bwd(kind=MSGMS, sH=32, sW=48, H=32, W=48, wb=None, dsr=dsr):
        return lib.srad_loss_backward(kind, sr, hr, 2, 3, sH, sW, H, W, 255.0, 1, out2, None, 1.0, dsr, 0, wsp, nb if wb is None else wb, None)

    assert fwd(kind=6) == SRAD_ERR_ARG and b"unknown loss kind 6" in lib.srad_last_error()
    assert bwd(kind=6) == SRAD_ERR_ARG and b"unknown loss kind 6" in lib.srad_last_error()
    assert fwd(sr=None) == SRAD_ERR_ARG and b"null" in lib.srad_last_error()
    assert bwd(dsr=None) == SRAD_ERR_ARG and b"null" in lib.srad_last_error()
    assert fwd(sH=40) == SRAD_ERR_ARG and b"same size" in lib.srad_last_error()
    assert bwd(sW=56) == SRAD_ERR_ARG and b"same size" in lib.srad_last_error()
    assert fwd(sH=20, sW=20, H=20, W=20) == SRAD_ERR_ARG and b"multiples of 8" in lib.srad_last_error()
    assert bwd(sH=20, sW=20, H=20, W=20) == SRAD_ERR_ARG and b"multiples of 8" in lib.srad_last_error()
    assert fwd(C_=2) == SRAD_ERR_ARG and b"1 or 3 channels" in lib.srad_last_error()
    assert fwd(wb=C.c_size_t(nb.value - 1)) == SRAD_ERR_ARG and b"workspace" in lib.srad_last_error()
    assert bwd(wb=C.c_size_t(nb.value - 1)) == SRAD_ERR_ARG and b"workspace" in lib.srad_last_error()
    assert fwd(kind=GMS, wb=C.c_size_t(0)) == SRAD_ERR_ARG and b"workspace" in lib.srad_last_error()


# --------------------------------------------------------------------------- the post-sweep stage under world 2 (gloo)
FLAG_SETS = [dict(save_maps=a, map_image_score=b, pixel_metrics=c, aupro=p, map_sigma=d)
             for a, b, c, p, d in itertools.product((False, True), (False, True), (False, True), (False, True), (0.0, 4.0))]
SOURCES = ("gms", "msgms")


def cpu_gms_maps(sr, hr, levels=1):
    return torch.from_numpy(R.gms_maps(sr.numpy(), hr.numpy(), levels))


def _stage_sweeps(rank, world, calls=None):
    from srad_amd import evaluate as E
    refuse = {fn: must_not_be_called(fn, "under a GMS map source")
              for fn in ("anomaly_maps", "anomaly_maps_multi", "error_maps", "error_maps_multi")}
    res = {}
    for source in SOURCES:
        cases = [dict(f, map_source=source) for f in FLAG_SETS]
        for k, r in enumerate(stage_sweep(E, rank, world, cases, calls, gms_maps=cpu_gms_maps, **refuse)):
            res[source, k] = r
    return res


def test_gms_stage_gloo_world2():
    one = _stage_sweeps(0, 1)
    res = run_world2(_stage_sweeps)
    for source in SOURCES:
        for k, flags in enumerate(FLAG_SETS):
            (o0, c0, f0), (o1, c1, f1) = res[0][source, k], res[1][source, k]
            w1, _, wf = one[source, k]
            tag = (source, flags)
            assert c0 == c1, (tag, c0, c1)
            assert o1 == {}, tag
            assert "broadcast_object_list" not in c0 and "broadcast" not in c0, (tag, c0)      # no window travels
            assert c0 == (["all_gather_object"] if flags["map_image_score"] else []), (tag, c0)
            if flags["map_image_score"]:
                assert o0["auc_map_max"] == w1["auc_map_max"], tag
                for o in (o0, w1):
                    assert o["map_source"] == source and o["map_levels"] == {"gms": 1, "msgms": 4}[source]
                    assert "map_ws" not in o and "map_scales" not in o and ("map_sigma" in o) == (flags["map_sigma"] > 0)
            else:
                assert o0 == {} and "auc_map_max" not in w1
            assert "auc_pixel" not in o0 and "aupro" not in o0
            assert_saved_maps_complete(flags, f0, f1, wf)
