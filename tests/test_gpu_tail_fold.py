"""GPU: DRCT's folded output end (csrc/tail_fold.h, kernels_tail_fold.hip) - the device builder against an fp64
fold taken from impulse responses of torch.nn.functional on the CPU, the kernel (ops.tail_fold) against the fp64 chain and held
to the error of the bf16 chain of launches it replaces, and the engine: fold against chain on the reference goldens, weight
updates under graph replay, the modes that keep the chain, and the launch counts."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import drct_case
from tests.test_gpu_drct import build

pytestmark = pytest.mark.gpu

FEAT = 64
RGB_MEAN = (0.4488, 0.4371, 0.4040)
CONFIGS = [(2, 1), (2, 3), (4, 1), (4, 3)]                      # (scale, in_chans)
SHAPES = [(2, 8, 8), (1, 8, 24), (1, 16, 40), (1, 24, 16)]      # (B, H, W): one and several tiles per row, widths that are no multiple of 16


def _uniform(seed, *shape):
    """Default conv init: uniform in +-1/sqrt(fan_in) with fan_in = 64 * 9, fp32 values."""
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) / np.sqrt(FEAT * 9)).float()


@functools.lru_cache(maxsize=None)
def up_stages(scale):
    return [(_uniform(10 * scale + j, 4 * FEAT, FEAT, 3, 3), _uniform(10 * scale + j + 5, 4 * FEAT)) for j in range(1 if scale == 2 else 2)]


@functools.lru_cache(maxsize=None)
def weights(scale, C):
    """The Upsample stages (shared by the gray and the RGB case of a scale) and conv_last."""
    return up_stages(scale), _uniform(100 * scale + C, C, FEAT, 3, 3), _uniform(100 * scale + C + 50, C)


def upsampled64(x, ups, bias=True):
    t = x.double()
    for w, b in ups:
        t = F.pixel_shuffle(F.conv2d(t, w.double(), b.double() if bias else None, padding=1), 2)
    return t


@functools.lru_cache(maxsize=None)
def impulse_features(scale):
    """Upsample's response, without biases and in fp64, to an impulse in every feature at every pixel of a 5 x 5 map:
    [25 pixels * 64 features][64][5 s][5 s].  An impulse in feature f passes the first stage as that stage's weight slice."""
    S = 5
    ups = up_stages(scale)
    eye = torch.eye(S * S, dtype=torch.float64).reshape(S * S, 1, S, S)
    w0 = ups[0][0].double()
    first = torch.stack([F.pixel_shuffle(F.conv2d(eye, w0[:, f:f + 1], padding=1), 2) for f in range(FEAT)], 1)   # [25][64 f][64][2S][2S]
    first = first.reshape(S * S * FEAT, FEAT, 2 * S, 2 * S)
    return upsampled64(first, ups[1:], bias=False)


def chain64(x, ups, last_w, last_b):
    """conv_last(PixelShuffle(up(...))) in fp64 on the CPU, x [B, F, H, W]."""
    return F.conv2d(upsampled64(x, ups), last_w.double(), last_b.double(), padding=1)


@functools.lru_cache(maxsize=None)
def reference_fold(scale, C):
    """The fold in fp64 from impulse responses on a 5 x 5 map, whose pixels 0, 2 and 4 stand for the first, interior and last class
    of an axis (the interior one sees its whole 5 x 5 window and no border): wf [9, N, 25, F] and bias [9, N]."""
    ups, last_w, last_b = weights(scale, C)
    S, N = 5, scale * scale * C
    # [impulse pixel p = (p // S, p % S)][feature] -> output map
    resp = F.conv2d(impulse_features(scale), last_w.double(), padding=1).reshape(S * S, FEAT, C, scale * S, scale * S)
    const = chain64(torch.zeros(1, FEAT, S, S, dtype=torch.float64), ups, last_w, last_b)[0]
    wf = torch.zeros(9, N, 25, FEAT, dtype=torch.float64)
    bias = torch.zeros(9, N, dtype=torch.float64)
    rep = (0, 2, 4)
    for cls in range(9):
        yr, xr = rep[cls // 3], rep[cls % 3]
        for oc in range(N):
            c, py, px = oc // (scale * scale), oc // scale % scale, oc % scale
            bias[cls, oc] = const[c, scale * yr + py, scale * xr + px]
            for tap in range(25):
                yy, xx = yr + tap // 5 - 2, xr + tap % 5 - 2
                if 0 <= yy < S and 0 <= xx < S:
                    wf[cls, oc, tap] = resp[yy * S + xx, :, c, scale * yr + py, scale * xr + px]
    return wf, bias


@pytest.mark.parametrize("scale,C", CONFIGS)
def test_builder_against_fp64_impulse_responses(scale, C):
    """fp32 accumulation of at most 9 * 64 * 9 * 64 = 36 864 products per folded weight predicts about 1e-6 of the largest one;
    the bar is 1e-5.  The bf16 pack is the correctly rounded device fold in the kernel's fragment order, bit for bit."""
    from srad_amd import ops
    ups, last_w, last_b = weights(scale, C)
    fold = ops.tail_fold_build([w.cuda() for w, _ in ups], [b.cuda() for _, b in ups], last_w.cuda(), last_b.cuda())
    wf_ref, bias_ref = reference_fold(scale, C)
    N, NT = scale * scale * C, (scale * scale * C + 15) // 16
    wf = fold["wf"].cpu()
    ew = float((wf.double() - wf_ref).abs().max() / wf_ref.abs().max())
    bias = fold["bias"].cpu()
    eb = float((bias[:, :N].double() - bias_ref).abs().max() / bias_ref.abs().max())
    print(f"x{scale} C={C}: device fold against fp64, relative to the largest entry: weights {ew:.3e}, bias {eb:.3e}")
    assert ew < 1e-5 and eb < 1e-5
    assert float(bias[:, N:].abs().max()) == 0.0 if NT * 16 > N else True
    padded = torch.zeros(9, NT * 16, 25, FEAT)
    padded[:, :N] = wf
    # [cls][nt][fr][tap][j][fq][e] -> [cls][nt][tap][j][fq][fr][e], lane = 16 fq + fr
    want = padded.reshape(9, NT, 16, 25, FEAT // 32, 4, 8).permute(0, 1, 3, 4, 5, 2, 6).reshape(9, NT, 25, FEAT // 32, 64, 8)
    assert torch.equal(fold["pack"].cpu().view(torch.int16), want.to(torch.bfloat16).view(torch.int16))


def errors(out, ref):
    d = (out.double() - ref).abs()
    edge = torch.cat([d[..., :2, :].flatten(), d[..., -2:, :].flatten(), d[..., :, :2].flatten(), d[..., :, -2:].flatten()])
    return float(d.max()), float(d.pow(2).mean().sqrt()), float(edge.max())


@pytest.mark.parametrize("scale,C", CONFIGS)
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_kernel_against_fp64_and_the_chain_it_replaces(scale, C, B, H, W):
    """The bar is the code the fold replaces: on the same input the folded launch's max and RMS error against the fp64 chain
    must not exceed those of the bf16 chain of launches (every conv rounding its input and weights to bf16; the fold rounds the
    input once and the folded weights once - a CPU emulation of the rounding points gave about half the error).  The first and
    last two HR rows and columns, where a wrong position class would show, are held to the chain's max error on their own."""
    from srad_amd import ops
    ups, last_w, last_b = weights(scale, C)
    img_range, mean = (255.0, RGB_MEAN) if C == 3 else (1.0, (0.25,))
    g = torch.Generator().manual_seed(B * 10000 + H * 100 + W)
    x = F.leaky_relu(torch.randn(B, FEAT, H, W, generator=g), 0.01)                 # what conv_before_upsample hands on
    mean_t = torch.tensor(mean, dtype=torch.float64).view(1, C, 1, 1)
    ref = chain64(x, ups, last_w, last_b) / img_range + mean_t
    c2 = x.permute(0, 2, 3, 1).reshape(B * H * W, FEAT).contiguous().cuda()
    upw, upb = [w.cuda() for w, _ in ups], [b.cuda() for _, b in ups]
    y = ops.tail_fold(c2, upw, upb, last_w.cuda(), last_b.cuda(), B, H, W, img_range, mean)
    t, h, w = c2, H, W
    for uw, ub in zip(upw, upb):
        t = ops.gemm(t, uw, ub, B=B, H=h, W=w, pixel_shuffle=True, precision="bf16")
        h, w = 2 * h, 2 * w
    t = ops.gemm(t, last_w.cuda(), last_b.cuda(), B=B, H=h, W=w, precision="bf16")
    chain = t.reshape(B, h, w, C).permute(0, 3, 1, 2) / img_range + mean_t.float().cuda()
    assert y.shape == ref.shape == chain.shape
    fmax, frms, fedge = errors(y.cpu(), ref)
    cmax, crms, cedge = errors(chain.cpu(), ref)
    rng = float(ref.max() - ref.min())
    print(f"x{scale} C={C} {B}x{H}x{W}: fold max {fmax / rng:.3e} rms {frms / rng:.3e} edge {fedge / rng:.3e} | "
          f"chain max {cmax / rng:.3e} rms {crms / rng:.3e} edge {cedge / rng:.3e} (of the output range)")
    assert fmax <= cmax and frms <= crms
    assert fedge <= cmax


# ------------------------------------------------------------------------------------------------ engine
FOLD_GOLDENS = ["drct_full_gray_x4", "drct_r2_rgb_x4", "drct_r2_gray_x4_dyn64"]     # the goldens the bf16 bars are set on


def golden_errors(out, y):
    rng = float(y.max() - y.min())
    err = np.abs(out.astype(np.float64) - y)
    return err.max() / rng, np.sqrt(np.mean(err ** 2)) / rng, 10 * np.log10(rng ** 2 / np.mean(err ** 2))


@pytest.mark.parametrize("name", FOLD_GOLDENS)
def test_engine_fold_against_chain_on_goldens(sr_golden, name):
    """Both ends meet the bf16 bars against the reference's output (max error / range < 1e-2, PSNR > 50 dB); the fold's max and
    RMS error are at most 1.25 x the chain's - the body's bf16 error dominates both, so they can come out level."""
    from srad_amd import ops
    cfg, sd, x, y = drct_case(sr_golden, name)
    xt = torch.from_numpy(x).cuda()
    with torch.no_grad():
        fold = build(cfg, sd, "bf16")(xt).cpu().numpy()
        with ops.path_override(tail_chain=True):
            chain = build(cfg, sd, "bf16")(xt).cpu().numpy()
    fmax, frms, fpsnr = golden_errors(fold, y)
    cmax, crms, cpsnr = golden_errors(chain, y)
    print(f"{name}: fold max/range {fmax:.3e} rms/range {frms:.3e} psnr {fpsnr:.2f} | chain {cmax:.3e} {crms:.3e} {cpsnr:.2f} | "
          f"ratio max {fmax / cmax:.3f} rms {frms / crms:.3f}")
    assert not np.array_equal(fold, chain)                     # two different ends did run
    assert fmax < 1e-2 and fpsnr > 50.0 and cmax < 1e-2 and cpsnr > 50.0
    assert fmax <= 1.25 * cmax and frms <= 1.25 * crms


def test_engine_weight_update_under_graph_replay(sr_golden):
    """conv_last.weight and upsample.0.bias change in place between replays: the next forward equals a fresh model with the
    changed weights bit for bit (the fold was rebuilt ahead of the replayed graph), and differs from the forward before."""
    cfg, sd, x, y = drct_case(sr_golden, "drct_r2_rgb_x4")
    m = build(cfg, sd, "bf16", use_graph=True)
    xt = torch.from_numpy(x).cuda()
    with torch.no_grad():
        outs = [m(xt).cpu().numpy() for _ in range(3)]          # eager, capture, replay
        assert all(np.array_equal(outs[0], o) for o in outs[1:])
        m.get_parameter("conv_last.weight").mul_(1.5)
        m.get_parameter("upsample.0.bias").add_(0.05)
        after = [m(xt).cpu().numpy() for _ in range(2)]
        fresh = build(cfg, {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, "bf16")(xt).cpu().numpy()
    assert np.array_equal(after[0], fresh) and np.array_equal(after[1], fresh)
    assert not np.array_equal(after[0], outs[0])


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16-training"])
def test_modes_that_do_not_fold(sr_golden, mode):
    """fp32, split-bf16 and a bf16 model bound for training run the launches they always ran: the tail_chain override changes
    nothing, bit for bit."""
    from srad_amd import ops
    cfg, sd, x, y = drct_case(sr_golden, "drct_r2_rgb_x4")
    xt = torch.from_numpy(x).cuda()

    def run():
        m = build(cfg, sd, "bf16" if mode == "bf16-training" else mode)
        if mode == "bf16-training":
            m.enable_training()
            m.eval()
        with torch.no_grad():
            return m(xt).cpu().numpy()
    plain = run()
    with ops.path_override(tail_chain=True):
        forced = run()
    assert np.array_equal(plain, forced)


def test_launch_counts():
    """A 1-RDG bf16 model at B = 1, 8 x 8: with the fold one tail_fold launch, no nhwc_to_nchw (one layout launch, the input's,
    instead of two) and three GEMM launches fewer than with the chain (two Upsample stages and conv_last)."""
    from srad_amd import _lib as L, ops, spec as S
    cfg = S.DRCTConfig(n_rdg=1)
    sd = S.synth_state(S.drct_spec(cfg), seed=5, cfg=cfg)
    x = torch.from_numpy(S.synth_image("fold/launches", (1, 1, 8, 8), seed=2, rgb_range=1.0)).cuda()

    def profile(**override):
        with ops.path_override(**override), torch.no_grad():
            m = build(cfg, sd, "bf16")
            m(x)                                               # weights packed, fold built
            torch.cuda.synchronize()
            L.prof_enable(True)
            L.prof_collect()
            try:
                m(x)
                torch.cuda.synchronize()
                return L.prof_collect()
            finally:
                L.prof_enable(False)

    def count(prof, *classes):
        return sum(prof[c]["launches"] for c in classes if c in prof)
    fold, chain = profile(), profile(tail_chain=True)
    gemm = ("gemm_bn64", "gemm_bn32", "gemm_bn16")
    print("fold", {k: v["launches"] for k, v in fold.items()}, "chain", {k: v["launches"] for k, v in chain.items()})
    assert count(fold, "tail_fold") == 1 and count(chain, "tail_fold") == 0
    assert count(fold, "layout") == 1 and count(chain, "layout") == 2
    assert count(chain, *gemm) - count(fold, *gemm) == 3
    assert count(fold, "pack_weight") == 0                     # the fold is not rebuilt by a forward that changed nothing
