"""GPU: the weight EMA kept by the fused Adam step (DESIGN.md "Weight EMA"), from the kernel up to the command line.
Every comparison is ``torch.equal``: the average is DEFINED as ``fl(fl(d * ema) + fl((1 - d) * p'))`` of its previous value
and the parameter just stored, which numpy float32 evaluates with the same three roundings; and the parameters and Adam
moments must carry the bits of the plain step, which a twin running the plain step provides."""
import math
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_train import _write_grid_class, build_train

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
FULL_PASS = 4096 * 256                                       # the grid-stride loop's stride: at most 4096 workgroups of 256
SIZES = [1, 255, 257, FULL_PASS + 257]                        # the last: one element past a full pass, and a ragged tail


def _f32(v):
    return float(np.float32(v))


def ema_reference(ema: np.ndarray, params: np.ndarray, decay: float) -> np.ndarray:
    """The definition in numpy float32: two products and one sum, each rounded on its own."""
    d = np.float32(decay)
    omd = np.float32(1.0 - float(d))
    assert ema.dtype == params.dtype == np.float32
    return d * ema + omd * params


def _inputs(n, seed, pad=0):
    """p, m (either sign), v >= 0, ema and three gradients; ``pad`` floats of slack in front so that [pad:] is off the
    allocation's alignment."""
    g = torch.Generator().manual_seed(seed)
    p, m, ema = (torch.randn(n, generator=g) for _ in range(3))
    v = torch.rand(n, generator=g) * 1e-2
    grads = [torch.randn(n, generator=g) * 0.1 for _ in range(3)]

    def dev(t):
        buf = torch.empty(n + pad, device="cuda")
        buf[pad:].copy_(t)
        return buf[pad:]
    return [dev(t) for t in (p, m, v, ema)], [dev(t) for t in grads]


def _step(variant, ema_on, bufs, grad, step, wd, gs, decay):
    from srad_amd import _lib as L
    lib = L.lib()
    p, m, v, ema = bufs
    n, s = p.numel(), L.current_stream_ptr()
    assert grad.data_ptr() % 16 == p.data_ptr() % 16
    if variant == "host":
        if ema_on:
            rc = lib.srad_adam_ema_step(L.dptr(p), L.dptr(grad), L.dptr(m), L.dptr(v), L.dptr(ema), n, LR, B1, B2, EPS, wd, step, gs, decay, s)
        else:
            rc = lib.srad_adam_step(L.dptr(p), L.dptr(grad), L.dptr(m), L.dptr(v), n, LR, B1, B2, EPS, wd, step, gs, s)
    else:
        hyper = torch.tensor([LR, 1.0 - _f32(B1) ** step, math.sqrt(1.0 - _f32(B2) ** step), gs], dtype=torch.float32).cuda()
        if ema_on:
            rc = lib.srad_adam_ema_step_dev(L.dptr(p), L.dptr(grad), L.dptr(m), L.dptr(v), L.dptr(ema), n, B1, B2, EPS, wd, decay, L.dptr(hyper), s)
        else:
            rc = lib.srad_adam_step_dev(L.dptr(p), L.dptr(grad), L.dptr(m), L.dptr(v), n, B1, B2, EPS, wd, L.dptr(hyper), s)
        torch.cuda.synchronize()                              # hyper stays alive until the kernel has read it
    L.check(rc, f"adam {variant} ema={ema_on}")


SETTINGS = [(wd, gs, decay) for wd in (0.0, 1e-4) for gs in (1.0, 0.5) for decay in (0.999, 0.5, 0.0)]


# ---------------------------------------------------------------- 1: the kernel against the definition
@pytest.mark.parametrize("variant", ["host", "dev"])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_the_definition(n, variant):
    for k, (wd, gs, decay) in enumerate(SETTINGS):
        mine, grads = _inputs(n, seed=100 + k)
        twin = [t.clone() for t in mine[:3]] + [None]
        e = mine[3].cpu().numpy()
        for step in (1, 2, 3):
            _step(variant, True, mine, grads[step - 1], step, wd, gs, decay)
            _step(variant, False, twin, grads[step - 1], step, wd, gs, decay)
            for name, a, b in zip(("params", "exp_avg", "exp_avg_sq"), mine, twin):
                assert torch.equal(a, b), (name, n, variant, wd, gs, decay, step)
            e = ema_reference(e, mine[0].cpu().numpy(), decay)
            assert torch.equal(mine[3].cpu(), torch.from_numpy(e)), (n, variant, wd, gs, decay, step)
            if decay == 0.0:
                assert torch.equal(mine[3], mine[0])
        assert not torch.equal(mine[0], _inputs(n, seed=100 + k)[0][0])          # the steps moved the parameters


@pytest.mark.parametrize("variant", ["host", "dev"])
@pytest.mark.parametrize("n", [1, 257, FULL_PASS + 257])
def test_buffers_one_float_off_a_16_byte_boundary_give_the_same_bits(n, variant):
    wd, gs, decay = 1e-4, 0.5, 0.999
    aligned, g0 = _inputs(n, seed=7)
    shifted, g1 = _inputs(n, seed=7, pad=1)
    assert aligned[0].data_ptr() % 16 == 0 and all(t.data_ptr() % 16 == 4 for t in shifted + g1)
    for step in (1, 2, 3):
        _step(variant, True, aligned, g0[step - 1], step, wd, gs, decay)
        _step(variant, True, shifted, g1[step - 1], step, wd, gs, decay)
    for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "ema"), aligned, shifted):
        assert torch.equal(a, b), (name, n, variant)


def test_refusals_on_device_buffers_leave_them_untouched():
    """The argument errors of tests/test_ema_host.py once more with real buffers: a refused call launches nothing."""
    from srad_amd import _lib as L
    (p, m, v, ema), (g, _, _) = _inputs(300, seed=3)
    before = [t.clone() for t in (p, m, v, ema)]
    lib, s = L.lib(), L.current_stream_ptr()
    for bad_ema, decay in ((None, 0.9), (ema, 1.0), (ema, float("nan")), (p[100:], 0.9), (v, 0.9)):
        assert lib.srad_adam_ema_step(L.dptr(p), L.dptr(g), L.dptr(m), L.dptr(v), L.dptr(bad_ema), 200, LR, B1, B2, EPS, 0.0, 1, 1.0,
                                      decay, s) == 1
    torch.cuda.synchronize()
    for a, b in zip(before, (p, m, v, ema)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- 2: the optimizer through all three step paths
def _tiny_drct(use_graph=False):
    """The smallest DRCT tests/test_gpu_train.py builds: 2 RDGs of 8 x 8 windows, 16 x 16 input, DropPath off."""
    from srad_amd import spec as S
    from srad_amd.nets import DRCT
    from tests.test_gpu_drct import Opt
    cfg = S.DRCTConfig(in_chans=1, img_size=16, window_size=8, upscale=2, n_rdg=2)
    sd = S.synth_state(S.drct_spec(cfg), seed=9, gain=1.0, cfg=cfg)
    x = torch.from_numpy(S.synth_image("ema", (2, 1, 16, 16), seed=5)).cuda()
    hr = torch.from_numpy(S.synth_image("ema/hr", (2, 1, 32, 32), seed=6)).cuda()

    def make(state=sd, train=True):
        o = Opt(cfg, "fp32", use_graph=use_graph)
        o.drop_path_rate = 0.0
        m = DRCT(o).cuda()
        m.load_state_dict({k: torch.as_tensor(np.asarray(v.cpu() if torch.is_tensor(v) else v)) for k, v in state.items()}, strict=True)
        if train:
            m.train()
            m.enable_training()
        else:
            m.eval()
        return m
    return make, x, hr


def _check_trajectory(run_step, m, twin_step, twin, decay, steps=5):
    """``run_step(i)`` / ``twin_step(i)`` advance the EMA model and its plain twin by one step: the parameters stay equal, the
    average follows the numpy recurrence over the parameter snapshots, starting from the initial weights."""
    e = m.flat_params.cpu().numpy().copy()
    assert torch.equal(m.flat_ema, m.flat_params) and m.flat_ema.data_ptr() != m.flat_params.data_ptr()
    for i in range(steps):
        run_step(i)
        twin_step(i)
        assert torch.equal(m.flat_params, twin.flat_params), i
        e = ema_reference(e, m.flat_params.cpu().numpy(), decay)
        assert torch.equal(m.flat_ema.cpu(), torch.from_numpy(e)), i
    assert not torch.equal(m.flat_ema, m.flat_params)


def test_optimizer_eager_train_step():
    from srad_amd.train import FusedAdam, train_step
    make, x, hr = _tiny_drct()
    m, twin = make(), make()
    opt, topt = FusedAdam(m, lr=LR, ema_decay=0.999), FusedAdam(twin, lr=LR)
    assert list(topt.state_dict()) == ["step", "exp_avg", "exp_avg_sq", "lr"] and not hasattr(twin, "flat_ema")
    assert m.enable_ema() is m and opt.hyper() == topt.hyper()
    _check_trajectory(lambda i: train_step(m, x + i, hr, opt), m, lambda i: train_step(twin, x + i, hr, topt), twin, 0.999)
    assert torch.equal(opt.exp_avg, topt.exp_avg) and torch.equal(opt.exp_avg_sq, topt.exp_avg_sq)
    # the optimizer's state carries the average in this mode, and only in this mode
    sd = opt.state_dict()
    assert list(sd) == ["step", "exp_avg", "exp_avg_sq", "lr", "ema", "ema_decay"] and sd["ema"] is m.flat_ema and sd["ema_decay"] == 0.999
    saved = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
    m.flat_ema.zero_()
    opt.load_state_dict({k: v for k, v in saved.items() if k not in ("ema", "ema_decay")})      # no key: the average is left alone
    assert float(m.flat_ema.abs().max()) == 0.0
    opt.load_state_dict(saved)
    assert torch.equal(m.flat_ema, saved["ema"])
    with pytest.raises(ValueError):
        FusedAdam(twin, ema_decay=1.0)
    with pytest.raises(ValueError):
        FusedAdam(twin, ema_decay=float("nan"))
    assert not hasattr(twin, "flat_ema")


def test_optimizer_graphed_train_step():
    from srad_amd.train import FusedAdam, GraphedTrainStep
    make, x, hr = _tiny_drct()
    m, twin = make(), make()
    opt, topt = FusedAdam(m, lr=LR, ema_decay=0.999), FusedAdam(twin, lr=LR)
    step, tstep = GraphedTrainStep(m, opt, warmup=2), GraphedTrainStep(twin, topt, warmup=2)
    _check_trajectory(lambda i: step(x + i, hr), m, lambda i: tstep(x + i, hr), twin, 0.999)      # steps 3 to 5 are replays
    assert len(step._graphs) == 1 and len(tstep._graphs) == 1 and opt.step_count == 5


def test_optimizer_graphed_drn_step():
    """A 2-block DRN-L x4 on one 4 x 4 image: every MeanShift gradient is then the sum of one workgroup per launch, so two
    runs of the plain step agree bit for bit and the twin is a reference."""
    from srad_amd.train import FusedAdam, GraphedDrnTrainStep, TensorAdam
    from tests.test_gpu_drn_train import _setup
    sides = []
    for ema in (0.999, None):
        cfg, sd, duals, lrs, hr, m, dms = _setup(4, 1, 2, 20, 1, 4, 4)
        opt = FusedAdam(m, lr=LR, weight_decay=1e-8, **({} if ema is None else dict(ema_decay=ema)))
        dopts = [TensorAdam(dm.parameters(), lr=LR, weight_decay=1e-8) for dm in dms]
        lr_t, hr_t = [torch.from_numpy(a).cuda() for a in lrs], torch.from_numpy(hr).cuda()
        step = GraphedDrnTrainStep(m, dms, opt, dopts, warmup=2)
        sides.append((m, step, lambda i, step=step, lr_t=lr_t, hr_t=hr_t: step([t + 0.5 * i for t in lr_t], hr_t)))
    (m, step, run), (twin, tstep, trun) = sides
    _check_trajectory(run, m, trun, twin, 0.999)
    assert len(step._graphs) == 1 and len(tstep._graphs) == 1 and not hasattr(twin, "flat_ema")


# ---------------------------------------------------------------- 3: ema_weights()
@pytest.mark.parametrize("use_graph", [False, True])
def test_ema_weights_context(use_graph):
    from srad_amd.train import FusedAdam, train_step
    make, x, hr = _tiny_drct(use_graph)
    m, twin = make(), make()
    opt, topt = FusedAdam(m, lr=LR, ema_decay=0.5), FusedAdam(twin, lr=LR)
    for i in range(3):
        train_step(m, x + i, hr, opt)
        train_step(twin, x + i, hr, topt)
    params, ema = m.flat_params.clone(), m.flat_ema.clone()
    fresh = make(m.ema_state_dict(), train=False)
    m.eval()
    with torch.no_grad():
        before = m(x)
        want = fresh(x)
        with m.ema_weights():
            inside = m(x)
            inside_again = m(x)
            m.train()
            with pytest.raises(RuntimeError, match="ema_weights"), torch.enable_grad():
                m(x)
            with pytest.raises(RuntimeError, match="ema_weights"):
                m._backward(torch.zeros_like(hr), need_dx=False)
            with pytest.raises(RuntimeError, match="ema_weights"):
                opt.step()
            with pytest.raises(RuntimeError, match="ema_weights"):
                opt.step_dev(torch.zeros(4, device="cuda"))
            with pytest.raises(RuntimeError, match="ema_weights"):
                with m.ema_weights():
                    pass
            m.eval()
        after = m(x)
    assert torch.equal(inside, want) and torch.equal(inside_again, want)
    assert torch.equal(after, before)
    assert not torch.equal(inside, before)                    # a context that does nothing would pass the two lines above
    assert torch.equal(m.flat_params, params) and torch.equal(m.flat_ema, ema) and opt.step_count == 3
    m.train()
    train_step(m, x + 3, hr, opt)
    train_step(twin, x + 3, hr, topt)
    assert torch.equal(m.flat_params, twin.flat_params)
    with pytest.raises(RuntimeError, match="no weight average"):
        with twin.ema_weights():
            pass
    from srad_amd.nets import DRCT
    from tests.test_gpu_drct import Opt
    with pytest.raises(RuntimeError, match="enable_training"):
        DRCT(Opt(m.cfg, "fp32")).cuda().enable_ema()


# ---------------------------------------------------------------- 4: the files
def test_model_save_writes_the_averaged_network(tmp_path):
    from srad_amd.train import FusedAdam, train_step
    from tests.test_gpu_self_ensemble import _drct_model, _lr
    _, plain, _, _ = _drct_model(False, self_ensemble=False)
    plain.save(str(tmp_path / "plain"), is_best=True)
    assert sorted(os.listdir(tmp_path / "plain" / "model")) == ["model_best.pt", "model_latest.pt"]

    _, wrapper, _, _ = _drct_model(False, self_ensemble=False)
    net = wrapper.get_model().train()
    opt = FusedAdam(net, lr=LR, ema_decay=0.9)
    x, hr = _lr((2, 1, 16, 16)), _lr((2, 1, 64, 64), seed=5)
    for i in range(2):
        train_step(net, x, hr, opt)
    run = tmp_path / "run"
    wrapper.save(str(run), is_best=False)
    assert sorted(os.listdir(run / "model")) == ["model_ema_latest.pt", "model_latest.pt"]
    wrapper.save(str(run), is_best=True)
    assert sorted(os.listdir(run / "model")) == ["model_best.pt", "model_ema_best.pt", "model_ema_latest.pt", "model_latest.pt"]
    live = net.state_dict()
    params = dict(net.named_parameters())
    engine = {name for name, _ in net._engine_params}
    assert engine and engine <= set(params)
    for fname in ("model_ema_latest.pt", "model_ema_best.pt"):
        sd = torch.load(run / "model" / fname, weights_only=True, map_location="cuda")
        assert list(sd) == list(live)
        for k, t in sd.items():
            if k in engine:                                   # its slice of the average, found from where the parameter lives
                off = (params[k].data_ptr() - net.flat_params.data_ptr()) // 4
                assert torch.equal(t, net.flat_ema[off:off + t.numel()].view(t.shape)), k
            else:
                assert torch.equal(t, live[k]), k
    raw = torch.load(run / "model" / "model_latest.pt", weights_only=True, map_location="cuda")
    assert list(raw) == list(live) and all(torch.equal(raw[k], live[k]) for k in raw)
    assert any(not torch.equal(raw[k], sd[k]) for k in engine)
    # loadable by Model.load like any checkpoint
    _, other, _, _ = _drct_model(False, self_ensemble=False)
    other.load(str(run / "model" / "model_ema_best.pt"))
    other.eval(), wrapper.eval()
    with torch.no_grad(), net.ema_weights():
        assert torch.equal(other(x), wrapper(x))


# ---------------------------------------------------------------- 5: end to end
def test_cli_train_and_evaluate_with_ema(tmp_path, capsys):
    from srad_amd import evaluate as E
    from srad_amd import main as Mn
    from srad_amd import options as Opt
    from srad_amd.model import Model
    data = str(tmp_path / "data")
    _write_grid_class(tmp_path / "data", n_test=(2, 2))
    args = Opt.parse_train_args(["--model-type", "drct", "--classe", "grid", "--resolution", "128", "--scale", "4", "--epochs", "1",
                                 "--batch-size", "4", "--data-root", data, "--save-dir", str(tmp_path / "exp"),
                                 "--ema", "--ema-decay", "0.9"])
    opt = Mn.build_train_opt(args)
    assert opt.ema is True and opt.ema_decay == 0.9
    opt.depths, opt.num_heads, opt.test_every, opt.print_every = (6, 6), (6, 6), 3, 1       # 2 RDG, 3 steps per epoch
    Mn.train_drct(opt)
    run = opt.save
    assert sorted(os.listdir(os.path.join(run, "model"))) == ["model_best.pt", "model_ema_best.pt", "model_ema_latest.pt", "model_latest.pt"]
    log = open(os.path.join(run, "log.txt")).read()
    line = [l for l in log.splitlines() if "\tPSNR:" in l]
    assert len(line) == 1 and line[0].endswith(" [EMA]"), line
    osd = torch.load(os.path.join(run, "optimizer.pt"))
    assert osd["step"] == 3 and osd["ema_decay"] == 0.9 and osd["ema"].numel() == osd["exp_avg"].numel()
    cfg = open(os.path.join(run, "config.txt")).read()
    assert "ema: True" in cfg and "ema_decay: 0.9" in cfg

    # the evaluator rebuilds the full-depth model and loads the 2-RDG weights with strict=False: the same seed gives the same rest
    capsys.readouterr()
    torch.manual_seed(11)
    got = E.main(["--run-dir", run, "--data-root", data, "--ema"])
    out = capsys.readouterr().out
    assert got["ema"] is True and "model_ema_best.pt" in out
    ckpt = os.path.join(run, "model", "model_ema_best.pt")
    eopt = Opt.build_opt("drct", "grid", 128, 4, 1, "bf16x3", pre_train=ckpt, data_root=data)
    eopt.test_only = True
    torch.manual_seed(11)
    model = Model(eopt, None)
    good = [(lr, hr) for _, lr, hr in E.iter_split(data, "grid", "good", eopt.scale, eopt.n_colors)]
    bad = [(lr, hr) for _, lr, hr in E.iter_split(data, "grid", "bad", eopt.scale, eopt.n_colors)]
    want = E.evaluate_on_test(eopt, model, good, bad)
    for k in ("best_ws", "auc_ssim", "auc_mse", "auc_psnr"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert {k: v for k, v in got.items() if k != "ema"}.keys() == want.keys()
    # without the flag: the raw weights, and no key
    capsys.readouterr()
    raw = E.main(["--run-dir", run, "--data-root", data])
    out = capsys.readouterr().out
    assert "ema" not in raw and "model_best.pt" in out and "model_ema" not in out
