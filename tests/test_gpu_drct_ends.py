"""GPU: the end of the DRCT bf16 inference forward's body as one launch (csrc/kernels_drct_ends.hip) - the op
(ops.drct_body_end) against fp64 and held to the error of the chain of launches it replaces, its borders on impulses, and the
engine: default path against the ends_chain override, graph replay, the launch counts and the rule that keeps the chain."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_drct import build

pytestmark = pytest.mark.gpu

E, FEAT, D = 180, 64, 308
RGB_MEAN = (0.4488, 0.4371, 0.4040)
BODY_SHAPES = [(1, 8, 8), (2, 16, 24), (1, 3, 33), (1, 1, 16), (4, 32, 32)]     # (B, H, W)


def _conv_init(seed, n, cin):
    """Default conv init: weight and bias uniform in +-1/sqrt(fan_in), fan_in = cin * 9, fp32 values."""
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / np.sqrt(cin * 9)
    return ((torch.rand(n, cin, 3, 3, generator=g, dtype=torch.float64) * 2 - 1) * k).float(), \
           ((torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1) * k).float()


@functools.lru_cache(maxsize=None)
def body_weights():
    g = torch.Generator().manual_seed(7)
    ln_g = (1.0 + 0.1 * torch.randn(E, generator=g)).float()
    ln_b = (0.1 * torch.randn(E, generator=g)).float()
    return (ln_g, ln_b) + _conv_init(11, E, E) + _conv_init(12, FEAT, E)


def body_ref64(x, feat0, w, B, H, W):
    """LN -> conv + feat0 -> conv -> LeakyReLU(0.01) in fp64 on the CPU; x [T, >= E], feat0 [T, E] -> [T, FEAT]."""
    ln_g, ln_b, w1, b1, w2, b2 = [t.double() for t in w]
    t = F.layer_norm(x[:, :E].double(), (E,), ln_g, ln_b, 1e-5).reshape(B, H, W, E).permute(0, 3, 1, 2)
    c1 = F.conv2d(t, w1, b1, padding=1) + feat0.double().reshape(B, H, W, E).permute(0, 3, 1, 2)
    c2 = F.leaky_relu(F.conv2d(c1, w2, b2, padding=1), 0.01)
    return c2.permute(0, 2, 3, 1).reshape(B * H * W, FEAT)


def body_chain(x, feat0, w, B, H, W):
    """The launches the body end replaces: ops.layernorm and two ops.gemm convolutions in bf16 mode."""
    from srad_amd import _lib as L, ops
    ln_g, ln_b, w1, b1, w2, b2 = w
    body = ops.layernorm(x[:, :E].contiguous(), ln_g, ln_b)
    c1 = ops.gemm(body, w1, b1, B=B, H=H, W=W, residual=feat0, precision="bf16")
    return ops.gemm(c1, w2, b2, B=B, H=H, W=W, act=L.ACT_LRELU, slope=0.01, precision="bf16")


def body_new(x, feat0, w, B, H, W):
    from srad_amd import ops
    ln_g, ln_b, w1, b1, w2, b2 = w
    return ops.drct_body_end(x, ln_g, ln_b, w1, b1, feat0, w2, b2, B, H, W)


@pytest.mark.parametrize("B,H,W", BODY_SHAPES)
def test_body_end_against_fp64_and_the_chain_it_replaces(B, H, W):
    """Both forms round the LayerNorm output and c1 to bf16 and accumulate in fp32, so their errors against fp64 should be
    level; the bar is DESIGN.md 5h's ratio form: max and RMS error at most 1.25 x the chain's own on the same input."""
    g = torch.Generator().manual_seed(B * 10000 + H * 100 + W)
    x = torch.randn(B * H * W, D, generator=g)                   # the dense buffer: only the first E columns are read
    feat0 = torch.randn(B * H * W, E, generator=g)
    w = body_weights()
    ref = body_ref64(x, feat0, w, B, H, W)
    wc = [t.cuda() for t in w]
    new = body_new(x.cuda(), feat0.cuda(), wc, B, H, W).cpu()
    chain = body_chain(x.cuda(), feat0.cuda(), wc, B, H, W).cpu()
    assert new.shape == chain.shape == ref.shape
    emax, erms = float((new - ref).abs().max()), float((new - ref).pow(2).mean().sqrt())
    cmax, crms = float((chain - ref).abs().max()), float((chain - ref).pow(2).mean().sqrt())
    print(f"{B}x{H}x{W}: body end max {emax:.3e} rms {erms:.3e} | chain max {cmax:.3e} rms {crms:.3e} | ratio {emax / cmax:.3f} {erms / crms:.3f}")
    assert emax <= 1.25 * cmax and erms <= 1.25 * crms


@pytest.mark.parametrize("H,W", [(8, 8), (16, 32)])
def test_body_end_borders_on_impulses(H, W):
    """An input that is zero except one pixel, at the four corners, an edge midpoint and an interior pixel: the new launch and
    the chain agree to 1e-3 of the response's max everywhere, and beyond two pixels from the impulse the response is exactly
    zero.  Biases and feat0 are zero and LayerNorm's weight and bias are 1 and 0, so that a zero pixel stays zero through
    LayerNorm and only the impulse (a pixel whose channels differ) spreads."""
    w = [t.cuda() for t in body_weights()]
    w[0], w[1], w[3], w[5] = torch.ones_like(w[0]), torch.zeros_like(w[1]), torch.zeros_like(w[3]), torch.zeros_like(w[5])
    feat0 = torch.zeros(H * W, E, device="cuda")
    g = torch.Generator().manual_seed(H * 100 + W)
    pulse = torch.randn(E, generator=g).cuda()
    for (py, px) in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, W // 2 - 1)]:
        x = torch.zeros(H * W, D, device="cuda")
        x[py * W + px, :E] = pulse
        new = body_new(x, feat0, w, 1, H, W).reshape(H, W, FEAT)
        chain = body_chain(x, feat0, w, 1, H, W).reshape(H, W, FEAT)
        peak = float(chain.abs().max())
        assert peak > 0 and float((new - chain).abs().max()) <= 1e-3 * peak, (py, px)
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        far = ((yy - py).abs() > 2) | ((xx - px).abs() > 2)
        assert float(new[far.cuda()].abs().max()) == 0.0 if bool(far.any()) else True, (py, px)
        assert float(new[py, px].abs().max()) > 0


@pytest.mark.parametrize("H,W", [(8, 8), (3, 33)])
def test_body_end_is_zero_on_a_constant_pixel_input(H, W):
    """feat0 = 0, all biases = 0 and an input that is constant over the channels of every pixel: LayerNorm gives exactly 0 (its
    bias is 0), so every output is exactly 0.  A c1 halo that was not zeroed outside the image, or a wrong LayerNorm, shows.
    The pixels' constants are multiples of 1/8 in [-2, 2]: the fp32 sum of 180 equal values and its division by 180 are then
    exact in any order, so x - mean is exactly 0 (with arbitrary floats the rounded mean leaves ~1e-7 x, times rstd ~ 316)."""
    w = [t.cuda() for t in body_weights()]
    w[1], w[3], w[5] = torch.zeros_like(w[1]), torch.zeros_like(w[3]), torch.zeros_like(w[5])
    g = torch.Generator().manual_seed(3)
    x = (torch.randint(-16, 17, (H * W, 1), generator=g).float() / 8).expand(H * W, D).contiguous().cuda()
    out = body_new(x, torch.zeros(H * W, E, device="cuda"), w, 1, H, W)
    assert float(out.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ engine
def _model_case(B, H, W, C=1):
    from srad_amd import spec as S
    cfg = S.DRCTConfig(n_rdg=1, in_chans=C)
    sd = S.synth_state(S.drct_spec(cfg), seed=5, cfg=cfg)
    x = torch.from_numpy(S.synth_image(f"ends/{B}x{H}x{W}", (B, C, H, W), seed=2, rgb_range=1.0)).cuda()
    return cfg, sd, x


@pytest.mark.parametrize("B,H,W", [(1, 8, 8), (2, 16, 16)])
def test_model_default_against_ends_chain(B, H, W):
    """No bf16 rounding point moved: the default path and the ends_chain override differ by at most 1e-3 of the output range;
    graph replay is bit-equal to eager; toggling the override between forwards of one model gives each path's own output again."""
    from srad_amd import ops
    cfg, sd, x = _model_case(B, H, W)
    with torch.no_grad():
        new = build(cfg, sd, "bf16")(x).cpu().numpy()
        with ops.path_override(ends_chain=True):
            chain = build(cfg, sd, "bf16")(x).cpu().numpy()
        rng = float(chain.max() - chain.min())
        diff = float(np.abs(new - chain).max()) / rng
        print(f"{B}x{H}x{W}: default against ends_chain, max difference / range {diff:.3e}")
        assert not np.array_equal(new, chain) and diff <= 1e-3
        m = build(cfg, sd, "bf16", use_graph=True)
        outs = [m(x).cpu().numpy() for _ in range(3)]           # eager, capture, replay
        assert all(np.array_equal(new, o) for o in outs)
        with ops.path_override(ends_chain=True):
            forced = [m(x).cpu().numpy() for _ in range(3)]      # the recorded graph was dropped
        assert all(np.array_equal(chain, o) for o in forced)
        assert np.array_equal(m(x).cpu().numpy(), new)


def _profile(m, x):
    from srad_amd import _lib as L
    with torch.no_grad():
        m(x)                                                     # weights packed, fold built
        torch.cuda.synchronize()
        L.prof_enable(True)
        L.prof_collect()
        try:
            m(x)
            torch.cuda.synchronize()
            return L.prof_collect()
        finally:
            L.prof_enable(False)


def _count(prof, *classes):
    return sum(prof[c]["launches"] for c in classes if c in prof)


GEMM = ("gemm_bn64", "gemm_bn32", "gemm_bn16")


def test_launch_counts():
    """A 1-RDG bf16 model at B = 1, 8 x 8: one body_end launch, one layernorm launch (patch_embed.norm; the final norm is in the
    body end) and two GEMM launches fewer than with ends_chain (conv_after_body, conv_before_upsample), one layout launch either
    way; with tail_chain as well the output end's layout launch comes back."""
    from srad_amd import ops
    cfg, sd, x = _model_case(1, 8, 8)

    def run(**override):
        with ops.path_override(**override):
            return _profile(build(cfg, sd, "bf16"), x)
    new, chain, both = run(), run(ends_chain=True), run(tail_chain=True)
    print("new", {k: v["launches"] for k, v in new.items()}, "chain", {k: v["launches"] for k, v in chain.items()})
    assert _count(new, "body_end") == 1 and _count(chain, "body_end") == 0
    assert _count(new, "layout") == 1 and _count(chain, "layout") == 1
    assert _count(new, "layernorm") == 1 and _count(chain, "layernorm") == 2      # patch_embed.norm and norm; the blocks fuse theirs
    assert _count(chain, *GEMM) - _count(new, *GEMM) == 2
    assert _count(both, "layout") == 2 and _count(both, "body_end") == 1
    assert _count(new, "pack_weight") == 0                       # no pack is rebuilt by a forward that changed nothing


def test_rule_keeps_the_chain_beyond_one_round_of_tiles():
    """A batch whose 16-pixel tiles exceed the CU count runs today's launches: bit-equal to ends_chain, no body_end launch."""
    from srad_amd import ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = cus // 64 + 1                                            # 32 x 32: 64 tiles per image
    assert not ops.drct_ends_supported("bf16", E, FEAT, 1, B, 32, 32) and ops.drct_ends_supported("bf16", E, FEAT, 1, B - 1, 32, 32)
    cfg, sd, x = _model_case(B, 32, 32)
    m = build(cfg, sd, "bf16")
    prof = _profile(m, x)
    assert _count(prof, "body_end") == 0 and _count(prof, "layernorm") == 2 and _count(prof, "layout") == 1
    with torch.no_grad():
        plain = m(x).cpu().numpy()
        with ops.path_override(ends_chain=True):
            forced = build(cfg, sd, "bf16")(x).cpu().numpy()
    assert np.array_equal(plain, forced)


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16-training"])
def test_modes_that_keep_the_chain(mode):
    """fp32, split-bf16 and a bf16 model bound for training never take the new launches: the override changes nothing."""
    from srad_amd import ops
    cfg, sd, x = _model_case(1, 8, 8)

    def run():
        m = build(cfg, sd, "bf16" if mode == "bf16-training" else mode)
        if mode == "bf16-training":
            m.enable_training()
            m.eval()
        prof = _profile(m, x)
        with torch.no_grad():
            return m(x).cpu().numpy(), prof
    plain, prof = run()
    with ops.path_override(ends_chain=True):
        forced, _ = run()
    assert np.array_equal(plain, forced)
    assert _count(prof, "body_end") == 0
