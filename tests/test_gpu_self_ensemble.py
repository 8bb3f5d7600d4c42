"""GPU: the x8 self-ensemble (DESIGN.md "Self-ensemble") from the two kernels up to ``evaluate_on_test``.  Every comparison
but the last is ``torch.equal``: the oracle is torch's own flip / transpose and an explicit loop of seven ``+`` and one
``* 0.125`` (``members`` / ``back_mean`` of tests/test_self_ensemble_host.py, checked there against an index loop), applied
around the PLAIN network with the forwards grouped as the definition groups them."""
import numpy as np
import pytest
import torch

from tests.helpers import rel_err
from tests.test_gpu_eval import _pairs
from tests.test_self_ensemble_host import back_mean, members

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 5, 7), (1, 3, 8, 8), (2, 3, 33, 70), (1, 1, 64, 65)]


def composed(net, x):
    """The definition around ``net``: square input is ONE forward of the stacked [8B,...] batch, other input two forwards of
    [4B,...]; a list of outputs is ensembled output by output."""
    B, _, H, W = x.shape
    ms = members(x)
    ys = [net(torch.cat(ms))] if H == W else [net(torch.cat(ms[:4])), net(torch.cat(ms[4:]))]
    many = isinstance(ys[0], (list, tuple))
    outs = []
    for j in range(len(ys[0]) if many else 1):
        halves = [y[j] if many else y for y in ys]
        per_member = [h[k * B:(k + 1) * B] for h in halves for k in range(h.shape[0] // B)]
        assert len(per_member) == 8
        outs.append(back_mean(per_member))
    return outs if many else outs[0]


# ---------------------------------------------------------------- 1, 2: the kernels
@pytest.mark.parametrize("shape", SHAPES)
def test_ensemble_inputs_match_the_definition(shape):
    from srad_amd import ops
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda()
    a, b = ops.ensemble_inputs(x)
    ms = members(x)
    B, Cc, H, W = shape
    assert tuple(a.shape) == (4 * B, Cc, H, W) and tuple(b.shape) == (4 * B, Cc, W, H)
    assert torch.equal(a, torch.cat(ms[:4])) and torch.equal(b, torch.cat(ms[4:]))
    if H == W:                                                # views of one [8B,...] allocation, b right behind a
        assert a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
        assert b.data_ptr() == a.data_ptr() + 4 * a.numel()
        (stack,) = ops.ensemble_batches(x)
        assert torch.equal(stack, torch.cat(ms))
    else:
        assert len(ops.ensemble_batches(x)) == 2


@pytest.mark.parametrize("shape", SHAPES)
def test_ensemble_mean_matches_the_definition(shape):
    """Eight INDEPENDENT random members: a wrong member order or back-transform cannot cancel."""
    from srad_amd import ops
    B, Cc, H, W = shape
    g = torch.Generator().manual_seed(2)
    ys = [torch.randn((B, Cc, W, H) if t & 4 else shape, generator=g).cuda() for t in range(8)]
    ref = back_mean(ys)
    assert torch.equal(ops.ensemble_mean(torch.cat(ys[:4]), torch.cat(ys[4:])), ref)
    if H == W:                                                # the two halves as views of one stacked output
        stack = torch.cat(ys)
        assert torch.equal(ops.ensemble_mean(stack[:4 * B], stack[4 * B:]), ref)


@pytest.mark.parametrize("shape", SHAPES)
def test_ensemble_mean_member_order(shape):
    """Member t is the constant 2^t with one marked pixel: every sum is a small integer, so the result is exact whatever the
    order of the additions, and a member read with another member's back-transform moves its mark."""
    from srad_amd import ops
    B, Cc, H, W = shape
    ys = []
    for t in range(8):
        y = torch.full((B, Cc, W, H) if t & 4 else shape, float(2 ** t))
        hh, ww = y.shape[2:]
        y[t % B, t % Cc, (3 * t + 1) % hh, (5 * t + 2) % ww] += 256.0 * (t + 1)
        ys.append(y.cuda())
    out = ops.ensemble_mean(torch.cat(ys[:4]), torch.cat(ys[4:]))
    assert torch.equal(out, back_mean(ys))
    assert float(out.min()) == 255.0 * 0.125 and 1 <= int((out != 255.0 * 0.125).sum()) <= 8


@pytest.mark.parametrize("shape", SHAPES)
def test_round_trip_is_exact(shape):
    from srad_amd import ops
    x = torch.randint(-64, 65, shape, generator=torch.Generator().manual_seed(3)).float().cuda()
    assert torch.equal(ops.ensemble_mean(*ops.ensemble_inputs(x)), x)          # eight equal small integers sum exactly


def test_argument_errors_on_tensors():
    from srad_amd import ops
    x = torch.zeros(1, 1, 4, 6, device='cuda')
    with pytest.raises(ValueError, match="4-d fp32"):
        ops.ensemble_inputs(x[0])
    with pytest.raises(ValueError, match="4-d fp32"):
        ops.ensemble_inputs(x.double())
    with pytest.raises(ValueError, match="two halves"):
        ops.ensemble_mean(torch.zeros(4, 1, 4, 6, device='cuda'), torch.zeros(4, 1, 4, 6, device='cuda'))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ensemble_inputs(x.cpu())


# ---------------------------------------------------------------- 3, 6: Model, DRCT
def _drct_model(use_graph, self_ensemble=True):
    from srad_amd import options as Opt
    from srad_amd import spec as S
    from srad_amd.model import Model
    opt = Opt.build_opt('drct', 'grid', 64, 4)                # the tiny config of tests/test_gpu_eval.py: window 4, one RDG
    opt.use_graph, opt.depths, opt.num_heads = use_graph, (6,), (6,)
    opt.self_ensemble, opt.drop_path_rate = self_ensemble, 0.0
    cfg = S.DRCTConfig(in_chans=1, img_size=16, window_size=4, upscale=4, n_rdg=1)
    sd = S.synth_state(S.drct_spec(cfg), seed=9, gain=0.7, cfg=cfg)
    m = Model(opt, None)
    m.get_model().load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return opt, m, cfg, sd


def _lr(shape, seed=4):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 255).cuda()


@pytest.mark.parametrize("use_graph", [False, True])
def test_model_drct_applies_the_definition(use_graph):
    _, m, _, _ = _drct_model(use_graph)
    m.eval()
    for shape in ((2, 1, 16, 16), (2, 1, 16, 24)):
        x = _lr(shape)
        with torch.no_grad():
            got, plain, want = m(x), m.model(x), composed(m.model, x)
            direct = m.forward_x8(x)
        assert tuple(got.shape) == (2, 1, 4 * shape[2], 4 * shape[3]) and not got.requires_grad
        assert torch.equal(got, want), float((got - want).abs().max())
        assert torch.equal(direct, want)
        assert not torch.equal(got, plain)                    # the flag is no longer ignored
    # training mode ignores the flag, as upstream: the plain output, with a graph
    m.train()
    x = _lr((2, 1, 16, 16))
    y = m(x)
    assert y.requires_grad and tuple(y.shape) == (2, 1, 64, 64)
    m.eval()
    with torch.no_grad():
        # DropPath is off here; the training and the inference forward are two fp32 implementations of one function, each
        # within the 1e-3 bar of tests/test_gpu_drct.py of the oracle
        assert rel_err(y.detach().cpu().numpy(), m.model(x).cpu().numpy()) < 2e-3


def test_model_flag_off_is_the_plain_forward():
    _, m, _, _ = _drct_model(False, self_ensemble=False)
    m.eval()
    x = _lr((2, 1, 16, 16))
    with torch.no_grad():
        assert torch.equal(m(x), m.model(x))


def test_drct_ensemble_against_the_cpu_oracle():
    """fp32 mode against the same composition run through the CPU oracle, at the bar of a single fp32 forward
    (tests/test_gpu_drct.py: 1e-3 relative): the mean of eight outputs that each meet a bar meets it."""
    from oracle import sr_ref as R
    _, m, cfg, sd = _drct_model(False)
    m.eval()
    x = _lr((1, 1, 16, 16))
    with torch.no_grad():
        got = m(x).cpu()
        ref = composed(lambda t: R.drct_forward(sd, t, cfg), x.cpu())
    assert rel_err(got.numpy(), ref.numpy()) < 1e-3, rel_err(got.numpy(), ref.numpy())


# ---------------------------------------------------------------- 4: Model, DRN-L x4 (a list of three outputs)
def test_model_drn_ensembles_every_output():
    from srad_amd import options as Opt
    from srad_amd.model import Model
    opt = Opt.build_opt('drn-l', 'grid', 64, 4)
    opt.n_blocks, opt.use_graph, opt.self_ensemble = 2, False, True
    m = Model(opt, None).eval()
    for shape in ((1, 1, 16, 16), (1, 1, 16, 24)):
        x = _lr(shape)
        with torch.no_grad():
            got, plain, want = m(x), m.model(x), composed(m.model, x)
        assert isinstance(got, list) and len(got) == 3 == len(want)
        for j in range(3):
            assert tuple(got[j].shape) == (1, 1, shape[2] * 2 ** j, shape[3] * 2 ** j)
            assert torch.equal(got[j], want[j]), (j, float((got[j] - want[j]).abs().max()))
        assert not torch.equal(got[-1], plain[-1])


# ---------------------------------------------------------------- 5: the evaluator
PARENT_KEYWORDS = dict(rank=0, world=1, names=(), output_dir='', save_images=False, masks=None, pixel_metrics=False, save_maps=False,
                       map_ws=0, map_scales=(), map_reduce='mean', map_source='ssim', operating_point=None, pr_metrics=False,
                       map_sigma=0.0, map_image_score=False, aupro=False, pro_fpr_limit=0.3)


def test_evaluator_self_ensemble():
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    opt, m, _, _ = _drct_model(False, self_ensemble=False)    # the evaluator's switch is its own argument
    y, good, bad = _pairs(6, 8, 64, 4, 1)
    pairs = good + bad
    lrs, hrs = [p[0] for p in pairs], [p[1] for p in pairs]
    m.eval()
    sr, hr = E.super_resolve_u8(m, lrs, hrs, float(opt.rgb_range), self_ensemble=True)
    batch = max(1, min(64, 65536 // (16 * 16)) // 8)          # what the function chooses: an eighth of the automatic batch
    assert batch == 8
    want = []
    with torch.no_grad():
        for i in range(0, len(lrs), batch):
            x = torch.from_numpy(np.stack(lrs[i:i + batch])).cuda().permute(0, 3, 1, 2).float() * (float(opt.rgb_range) / 255.0)
            want.append(M.to_u8_hwc(composed(m.model, x), float(opt.rgb_range)))
    assert torch.equal(sr, torch.cat(want))
    assert torch.equal(hr.cpu(), torch.from_numpy(np.stack(hrs)))
    plain_sr, _ = E.super_resolve_u8(m, lrs, hrs, float(opt.rgb_range))
    assert not torch.equal(plain_sr, sr)
    # an explicit batch is taken as given
    sr3, _ = E.super_resolve_u8(m, lrs[:3], hrs[:3], float(opt.rgb_range), batch=3, self_ensemble=True)
    with torch.no_grad():
        x = torch.from_numpy(np.stack(lrs[:3])).cuda().permute(0, 3, 1, 2).float() * (float(opt.rgb_range) / 255.0)
        assert torch.equal(sr3, M.to_u8_hwc(composed(m.model, x), float(opt.rgb_range)))

    got = E.evaluate_on_test(opt, m, good, bad, self_ensemble=True)
    ref = M.evaluate_pairs(y, sr, hr)
    assert got["self_ensemble"] is True
    for k in ("best_ws", "window_sizes", "auc_ssim", "auc_mse", "auc_psnr"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    off = E.evaluate_on_test(opt, m, good, bad)
    assert "self_ensemble" not in off
    assert off == E.evaluate_on_test(opt, m, good, bad, **PARENT_KEYWORDS)     # every parameter the function had before, and no other
    assert {k: v for k, v in got.items() if k != "self_ensemble"}.keys() == off.keys()


def test_evaluator_prints_the_suffix_only_when_on(capsys):
    from srad_amd import evaluate as E
    opt, m, _, _ = _drct_model(False, self_ensemble=False)
    _, good, bad = _pairs(2, 2, 64, 4, 1)
    E.evaluate_on_test(opt, m, good, bad)
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Test AUCs")][-1]
    assert "self-ensemble" not in line
    E.evaluate_on_test(opt, m, good, bad, self_ensemble=True)
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Test AUCs")][-1]
    assert line.endswith("(self-ensemble x8)")
