"""GPU: DRCT training at the 512 and 1024 px presets (window_size = img_size // 4 = 32 and 64): the unfused launches with the
tiled attention backward.
 * training forward + backward with explicit DropPath factors against autograd of the oracle, bars as
   tests/test_gpu_train.py::test_training_other_window_sizes_matches_oracle_autograd;
 * FusedAdam steps lower the loss, GraphedTrainStep walks the eager trajectory, the Trainer accepts both presets;
 * every other window size above 16 is still refused."""
import types

import pytest
import torch
import torch.nn.functional as F

from tests.grad_ref import leaf_state
from tests.helpers import rel_err
from tests.test_gpu_drct import Opt
from tests.test_gpu_train import build_train

pytestmark = pytest.mark.gpu


def _small(ws):
    """One RDG, grey, x4, one 64 x 64 input: 2 x 2 windows of 32 (DRCT-L width: head dims 30 .. 122, one to four 32-column
    chunks), or one shifted window of 64 at a reduced width (60 / 2 heads: head dims 30 .. 94) that keeps the CPU autograd of
    five 4096 x 4096 attention maps small."""
    from srad_amd import spec as S
    if ws == 32:
        return S.DRCTConfig(in_chans=1, img_size=128, window_size=32, upscale=4, n_rdg=1)
    return S.DRCTConfig(in_chans=1, img_size=256, window_size=64, upscale=4, n_rdg=1, embed_dim=60, num_heads=2)


_ORACLE = {}


def _case(ws):
    """(cfg, state, x, hr, keep, oracle output, oracle dx, oracle parameter gradients) - the CPU autograd runs once per window size."""
    if ws not in _ORACLE:
        from oracle import sr_ref as R
        from srad_amd import spec as S
        cfg = _small(ws)
        sd = S.synth_state(S.drct_spec(cfg), seed=70 + ws, gain=1.0, cfg=cfg)
        B, H, W, up = 1, 64, 64, cfg.upscale
        x = S.synth_image("trbig", (B, 1, H, W), seed=5)
        hr = S.synth_image("trbig/hr", (B, 1, H * up, W * up), seed=6)
        gen = torch.Generator().manual_seed(2)
        keep = torch.floor(0.8 + torch.rand(2 * cfg.n_rdg * 5, B, generator=gen)) / 0.8
        if float(keep.min()) > 0:
            keep[3, 0] = 0.0                                     # B = 1: make sure one branch IS dropped
        sdt = leaf_state(sd)
        keeps = [[(keep[2 * (i * 5 + k)], keep[2 * (i * 5 + k) + 1]) for k in range(5)] for i in range(cfg.n_rdg)]
        xr = torch.from_numpy(x).requires_grad_(True)
        ref = R.drct_forward(sdt, xr, cfg, keeps=keeps)
        F.l1_loss(ref, torch.from_numpy(hr)).backward()
        _ORACLE[ws] = (cfg, sd, x, hr, keep, ref.detach().numpy(), xr.grad.numpy(), {k: v.grad for k, v in sdt.items() if v.grad is not None})
    return _ORACLE[ws]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("ws", [32, 64])
def test_training_big_windows_matches_oracle_autograd(ws, prec):
    cfg, sd, x, hr, keep, ref, ref_dx, ref_grads = _case(ws)
    m = build_train(cfg, sd, prec, drop_path_rate=0.1)
    assert m._can_train()
    m.keep_scale_override = keep.cuda()
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    out = m(xt)
    F.l1_loss(out, torch.from_numpy(hr).cuda()).backward()
    if prec == "fp32":
        e_out, e_dx = rel_err(out.detach().cpu().numpy(), ref), rel_err(xt.grad.cpu().numpy(), ref_dx)
        worst = ("", 0.0)
        for n, p in m.named_parameters():
            worst = max(worst, (n, rel_err(p.grad.cpu().numpy(), ref_grads[n].numpy())), key=lambda t: t[1])
        print(f"window {ws}: output {e_out:.2e}, dx {e_dx:.2e}, worst parameter-gradient error {worst}")
        assert e_out < 2e-4
        assert e_dx < 1e-3
        assert worst[1] < 1e-3, worst
    else:
        a = torch.cat([ref_grads[n].reshape(-1) for n, _ in m.named_parameters()]).double()
        b = torch.cat([p.grad.reshape(-1).cpu() for _, p in m.named_parameters()]).double()
        cos = float((a * b).sum() / (a.norm() * b.norm()))
        print(f"window {ws} bf16: cosine(oracle fp32 grad, engine bf16 grad) = {cos}, norm ratio {float(b.norm() / a.norm())}")
        assert cos > 0.99 and 0.9 < float(b.norm() / a.norm()) < 1.1


def test_fused_adam_lowers_the_loss_at_window_32():
    from srad_amd.train import FusedAdam, train_step
    cfg, sd, x, hr = _case(32)[:4]
    m = build_train(cfg, sd, "fp32")
    opt = FusedAdam(m, lr=1e-4)
    xt, hrt = torch.from_numpy(x).cuda(), torch.from_numpy(hr).cuda()
    losses = [float(train_step(m, xt, hrt, opt)) for _ in range(3)]
    print("losses", losses)
    assert losses[-1] < losses[0]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_graphed_train_step_matches_eager_at_window_32(prec):
    """As tests/test_gpu_train.py::test_graphed_train_step_matches_eager: same kernels, same fixed-order reductions -> same bits."""
    from srad_amd.train import FusedAdam, GraphedTrainStep, train_step
    cfg, sd, x, hr = _case(32)[:4]
    xt, hrt = torch.from_numpy(x).cuda(), torch.from_numpy(hr).cuda()
    runs = {}
    for mode in ("eager", "graph"):
        m = build_train(cfg, sd, prec)
        opt = FusedAdam(m, lr=1e-3)
        step = GraphedTrainStep(m, opt, warmup=2) if mode == "graph" else (lambda a, b: train_step(m, a, b, opt))
        losses = []
        for i in range(5):
            if i == 4:
                opt.param_groups[0]["lr"] = 5e-4
            losses.append(step(xt + i, hrt))
        torch.cuda.synchronize()
        runs[mode] = (torch.stack([l.double() for l in losses]).cpu(), m.flat_params.clone(), opt.step_count)
        if mode == "graph":
            assert len(step._graphs) == 1
    assert runs["graph"][2] == runs["eager"][2] == 5
    assert torch.equal(runs["graph"][0], runs["eager"][0]), (runs["graph"][0], runs["eager"][0])
    assert torch.equal(runs["graph"][1], runs["eager"][1])


@pytest.mark.parametrize("resolution,ws", [(512, 32), (1024, 64)])
def test_trainer_accepts_the_512_and_1024_px_presets(resolution, ws):
    """The option set the CLI builds for --resolution 512 / 1024 at x4 (one RDG instead of twelve: construction only)."""
    from srad_amd.main import build_train_opt
    from srad_amd.model import Model
    from srad_amd.options import parse_train_args
    from srad_amd.trainer import Trainer
    opt = build_train_opt(parse_train_args(["--resolution", str(resolution), "--scale", "4"]))
    assert opt.window_size == ws
    opt.depths, opt.num_heads = (6,), (6,)
    t = Trainer(opt, types.SimpleNamespace(loader_train=None, loader_test=None), Model(opt), None, None)
    assert t.net._can_train() and t.optimizer is not None


@pytest.mark.parametrize("ws", [20, 33, 63])
def test_other_big_windows_are_still_refused(ws):
    from srad_amd import spec as S
    from srad_amd.nets import DRCT
    cfg = S.DRCTConfig(in_chans=1, img_size=4 * ws, window_size=ws, upscale=2, n_rdg=1)
    m = DRCT(Opt(cfg, "fp32")).cuda().train()
    assert not m._can_train()
    with pytest.raises(NotImplementedError, match="window sizes up to 16"):
        m(torch.zeros(1, 1, ws, ws, device="cuda"))
