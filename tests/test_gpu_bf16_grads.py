"""GPU: every gradient tensor of the bf16 training step, one by one, against autograd of the oracle.

The bar of a tensor is 4 x the error a bf16-operand restatement of the oracle (tests/grad_ref.py: ``bf16_matmuls``) makes on
that tensor, measured in the test on three image seeds, capped at 0.5 relative L2 ("bf16 gradients, tensor by
tensor").  The flat cosine the other bf16 engine tests assert does not see a missing bias gradient, a table gradient in the wrong
block or a DropPath factor on the wrong branch (tests/test_grad_ref_host.py shows it); this does.  Each case is the smallest shape
that still takes the plan named in its id."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import grad_ref as G
from tests.helpers import drct_case

pytestmark = pytest.mark.gpu

KEEP_P = 0.7
EMU_SEEDS = (0, 1000, 2000)       # added to the case's image seeds; the first is the case itself


def _keep(cfg, B, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.floor(KEEP_P + torch.rand(2 * cfg.n_rdg * 5, B, generator=gen)) / KEEP_P


def _oracle_pairs(run):
    """``run(seed offset, emulate) -> tensors``: the exact run of the case and [(emulated, exact)] per seed."""
    exact = run(EMU_SEEDS[0], False)
    return exact, [(run(s, True), exact if s == EMU_SEEDS[0] else run(s, False)) for s in EMU_SEEDS]


def _drct_engine(cfg, sd, x, hr, keep, unfused=False, probe_plan=False):
    """One training forward + backward of the bf16 engine under L1 -> tensors as ``G.as_tensors``."""
    from srad_amd import ops
    from tests.test_gpu_train import build_train
    with ops.path_override(unfused_blocks=unfused):
        m = build_train(cfg, sd, "bf16", drop_path_rate=0.1)
        assert m._can_train()
        m.keep_scale_override = keep.cuda()
        xt = torch.from_numpy(x).cuda().requires_grad_(True)
        hrt = torch.from_numpy(hr).cuda()
        out = m(xt)
        F.l1_loss(out, hrt).backward()
        torch.cuda.synchronize()
    got = G.as_tensors(out.detach().cpu(), xt.grad.cpu(), {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()})
    if probe_plan:
        # What the forward saved for the backward says which plan it chose, and the backward refuses (before it touches a block)
        # a call that would take other kernels than the saves were made for.  Under the unfused_blocks override the backward
        # takes fp32 saves: it goes through after a forward below 8192 tokens, and must refuse after one that chose the all-bf16
        # plan (q | k | v and the fc1 pre-activation saved as bf16).
        out = m(xt)
        with ops.path_override(unfused_blocks=True):
            with pytest.raises(RuntimeError, match=r"q\|k\|v bf16, fc1 pre-activation bf16"):
                F.l1_loss(out, hrt).backward()
        torch.cuda.synchronize()
    return got


_ORACLE = {}       # label -> (exact, pairs): the reference of a case is computed once and shared by the tests that take it


def _check_drct(label, cfg, sd, shapes, seeds, keep, x=None, hr=None, **engine):
    (xs, hs), (sx, sh) = shapes, seeds
    from srad_amd import spec as S

    def images(off):
        if off == EMU_SEEDS[0] and x is not None:
            return x, hr
        return S.synth_image(label, xs, seed=sx + off), S.synth_image(label + "/hr", hs, seed=sh + off)

    def run(off, emulate):
        xi, hi = images(off)
        out, loss, dx, grads = G.oracle_grads(G.drct_l1(cfg, hi, G.keeps_of(keep, cfg.n_rdg)), sd, xi, emulate)
        return G.as_tensors(out, dx, grads)

    if label not in _ORACLE:
        _ORACLE[label] = _oracle_pairs(run)
    exact, pairs = _ORACLE[label]
    got = _drct_engine(cfg, sd, *images(EMU_SEEDS[0]), keep, **engine)
    assert sorted(got) == sorted(exact)                    # every named parameter, the output and dx
    path = "".join(f" [{k}]" for k, v in engine.items() if v)
    G.assert_report(G.per_tensor_report(got, exact, pairs), 0.0, label + path)        # DRCT: no tensor may be left out of the bar


def _ws8_gray(B, H):
    from srad_amd import spec as S
    cfg = S.DRCTConfig(in_chans=1, img_size=16, window_size=8, upscale=2, n_rdg=1)
    sd = S.synth_state(S.drct_spec(cfg), seed=77, gain=1.0, cfg=cfg)
    return cfg, sd, ((B, 1, H, H), (B, 1, 2 * H, 2 * H)), (5, 6), _keep(cfg, B, 1)


@pytest.mark.parametrize("unfused", [False, True], ids=["fused", "unfused_blocks"])
def test_drct_ws8_512_tokens(unfused):
    """One RDG, gray x2, B = 2 at 16 x 16.  fused: the forward saves of the fused block kernels, mlp_bwd / lin_ln_bwd on 16-row
    tiles, fp32 hand-offs, all five block widths (d = 180 .. 308).  unfused_blocks: the eight-launch path that
    test_bf16_training_fused_forward_matches_unfused and test_bf16_fused_mlp_backward_matches_unfused take as their reference,
    on the same weights, images and masks (one oracle reference for both)."""
    _check_drct("ws8/512", *_ws8_gray(2, 16), unfused=unfused)


def test_drct_ws8_8192_tokens_all_bf16_plan():
    """B = 8 at 32 x 32: the plan that only exists from 8192 tokens - q | k | v, dO per head, dqkv, dh and the fc1 pre-activation as
    bf16, 32-row mlp_bwd instances, the all-bf16 attention backward.  The engine is asked which plan it took (see _drct_engine):
    the case fails if the threshold moves off this shape."""
    _check_drct("ws8/8192", *_ws8_gray(8, 32), probe_plan=True)


def test_drct_rgb_x4_two_rdgs(sr_golden):
    """The drct_r2_rgb_x4 golden configuration on its own x and hr: three-channel stem and mean, two upsample stages, gradients
    across an RDG boundary."""
    name = "drct_r2_rgb_x4"
    cfg, sd, x, _ = drct_case(sr_golden, name)
    hr = np.asarray(sr_golden[name + "/hr"])
    _check_drct("rgb_x4/r2", cfg, sd, (x.shape, hr.shape), (5, 6), _keep(cfg, x.shape[0], 3), x=np.asarray(x), hr=hr)


@pytest.mark.parametrize("ws,img,up,B,H,W", [(4, 16, 4, 2, 16, 8), (16, 64, 4, 1, 32, 32)])
def test_drct_other_window_sizes(ws, img, up, B, H, W):
    """The window-4 and window-16 bf16 rows of test_training_other_window_sizes_matches_oracle_autograd (its configurations,
    weights and images): unfused launches and the general attention backward in bf16 mode."""
    from srad_amd import spec as S
    cfg = S.DRCTConfig(in_chans=1, img_size=img, window_size=ws, upscale=up, n_rdg=2)
    sd = S.synth_state(S.drct_spec(cfg), seed=70 + ws, gain=1.0, cfg=cfg)
    _check_drct(f"ws{ws}", cfg, sd, ((B, 1, H, W), (B, 1, H * up, W * up)), (5, 6), _keep(cfg, B, 2))


@pytest.mark.parametrize("lr_px", [16, 64])
def test_drn_x4_rgb(lr_px):
    """DRN x4, RGB, 20 feats, 2 blocks, B = 2, with the dual models' parameters, under the composite loss.  16 px: tiled GEMM
    convolutions, thin head / tail kernels, channel-attention backward.  64 px: the weight-resident 80-channel kernel forward and
    for the data gradients (ReLU' and skip epilogues), the nine-tap weight gradient, the four-launch upsampler.  The engine hands
    no gradient to the LR input (the reference never asks for one), so there is no dx here; the three outputs are tensors."""
    from srad_amd import spec as S
    from srad_amd.train import drn_loss
    from tests.test_gpu_drn_train import _setup
    B = 2
    cfg, sd, duals, lrs, hr, m, dms = _setup(4, 3, 2, 20, B, lr_px, lr_px, prec="bf16")
    sds = {"": sd, **{f"dual{i}.": d for i, d in enumerate(duals)}}

    def run(off, emulate):
        if off == EMU_SEEDS[0]:
            li, hi = lrs, hr
        else:       # _setup's images, other seeds
            li = [S.synth_image("drn_tr", lrs[0].shape, seed=5 + off)] + \
                 [S.synth_image(f"drn_tr/lr{i}", lrs[i].shape, seed=6 + i + off) for i in range(1, cfg.phase)]
            hi = S.synth_image("drn_tr/hr", hr.shape, seed=9 + off)
        out, loss, dx, grads = G.oracle_grads(G.drn_composite(cfg, li, hi), sds, li[0], emulate)
        return G.as_tensors(out, None, grads)

    exact, pairs = _oracle_pairs(run)
    lr_t = [torch.from_numpy(a).cuda() for a in lrs]
    sr = m(lr_t[0])
    sr2lr = [dms[i](sr[i - len(dms)]) for i in range(len(dms))]
    drn_loss(sr, lr_t, torch.from_numpy(hr).cuda(), sr2lr).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}
    for i, dm in enumerate(dms):
        grads.update({f"dual{i}.{n}": p.grad.detach().cpu().clone() for n, p in dm.named_parameters()})
    got = G.as_tensors([o.detach().cpu() for o in sr], None, grads)
    assert sorted(got) == sorted(exact)
    G.assert_report(G.per_tensor_report(got, exact, pairs), 0.05, f"drn/{lr_px}px")
