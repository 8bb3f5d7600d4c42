"""GPU: fc2 folded into the RDG's adjust conv in the one-launch Swin block (csrc/mlp_fold.h,
kernels_mlp_fold.hip, swin_block_kernel's FOLD form): the composed weight against float64, the folded op against the unfolded
one with float64 of the unfolded math as the referee, the x1 | h seam, the epilogue forms, and the engine's rule, freshness and
graph behaviour.

Bars (set by the change's issue from a CPU emulation of the bf16 rounding points, not from this code's results): the folded op's
RMS error against float64 at most 1.05 x the unfolded op's on the same inputs, its max error at most 1.5 x, the two outputs
within 1e-2 of the output's max of each other.

Measured on MI355X over the 14 op cases below: RMS ratio 0.913 - 0.964, max ratio 0.757 - 1.043, folded against unfolded
5.3e-4 - 2.9e-3 of the output's max; composition 0.00 ulp; the 1-RDG model 2.2e-3 - 2.3e-3 of the range from its chain and
63.3 - 63.4 dB against the oracle.  The tests print each figure.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sr_ref as R
from srad_amd import _lib as L
from srad_amd import ops
from tests import mlp_fold_ref as MR
from tests.test_gpu_fused_ops import make_block

pytestmark = pytest.mark.gpu

D = 308                                                      # columns of the RDG's dense buffer
# DRCT-L's five block shapes, then the same-key off-table shape (d = 168: k padding inside the x1 part, next to the seam) and a
# part-filled column tile (28 adjust outputs)
SHAPES = [(180, 6, 360, 32), (212, 4, 424, 32), (244, 2, 488, 32), (276, 6, 276, 32), (308, 4, 308, 180), (168, 6, 360, 32), (180, 6, 360, 28)]
GEOM = {0: (1, 8, 8), 4: (1, 16, 16)}                        # one window (four workgroups); four windows with the shift's masks live
KEYS = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.relative_position_bias_table", "attn.proj.weight",
        "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "adjust.weight",
        "adjust.bias")


def ref64(sd, dense, B, H, W, d, heads, shift, no, last):
    """The unfolded math of the whole block + adjust in float64 (oracle.sr_ref.swin_block on double tensors, no rounding)."""
    sd64 = {k: v.double() for k, v in sd.items()}
    x = dense[:, :d].double().reshape(B, H * W, d).contiguous()
    x2 = R.swin_block(sd64, "", x, H, W, 8, heads, shift).reshape(B * H * W, d)
    assert x2.dtype == torch.float64
    a = F.linear(x2, sd64["adjust.weight"], sd64["adjust.bias"])
    return (a * 0.2 + dense[:, :no].double()) if last else F.leaky_relu(a, 0.2)


def run(fn, sd, dense, B, H, W, shift, heads, last, alpha=0.2):
    """The op as the engine calls it: adjust_k in place behind the block's columns (yoff = d), adjust5 (residual from one buffer,
    output into another, NaN-filled).  Returns the adjust output's columns."""
    d, no = sd["norm1.weight"].numel(), sd["adjust.bias"].numel()
    w = [sd[k].cuda() for k in KEYS]
    dg = dense.cuda()
    before = dg.clone()
    if last:
        out = torch.full_like(dg, float("nan"))
        fn(dg, *w, B, H, W, shift, heads, act=L.ACT_NONE, slope=0.0, alpha=alpha, residual=dg, out=out, out_offset=0)
        assert torch.isnan(out[:, no:]).all() and torch.equal(dg, before)
        return out[:, :no].cpu()
    fn(dg, *w, B, H, W, shift, heads, act=L.ACT_LRELU, slope=0.2, alpha=1.0, out=dg, out_offset=d)
    assert torch.equal(dg[:, :d], before[:, :d]) and torch.equal(dg[:, d + no:], before[:, d + no:])
    return dg[:, d:d + no].cpu()


@functools.lru_cache(maxsize=None)
def case(d, heads, hidden, no, shift):
    B, H, W = GEOM[shift]
    sd = make_block(d, heads, hidden, no, seed=d + shift, round_weights=False)      # fp32 weights: what the fold is composed from
    dense = (torch.randn(B, H * W, D, generator=torch.Generator().manual_seed(7)) * 1.5 + 0.3).reshape(B * H * W, D)
    last = no == 180
    return sd, dense, ref64(sd, dense, B, H, W, d, heads, shift, no, last), last


# ------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize("d,heads,hidden,no", SHAPES)
def test_composition_against_float64(d, heads, hidden, no):
    """Every element of [A | A W2] and of A b2 + b_a within 1 fp32 ulp of the float64 result rounded once; the A part exact; the
    padding columns of both parts exactly zero."""
    sd = make_block(d, heads, hidden, no, seed=d, round_weights=False)
    got = ops.mlp_fold_compose(sd["mlp.fc2.weight"].cuda(), sd["mlp.fc2.bias"].cuda(), sd["adjust.weight"].cuda(), sd["adjust.bias"].cuda())
    wf, bf = got["wf"].cpu().numpy(), got["bias"].cpu().numpy()
    a64, w64 = sd["adjust.weight"].double().numpy(), sd["mlp.fc2.weight"].double().numpy()
    ref_w = np.float32(a64 @ w64)
    ref_b = np.float32(a64 @ sd["mlp.fc2.bias"].double().numpy() + sd["adjust.bias"].double().numpy())
    kc32 = got["kc32"]
    assert kc32 == MR.layout(d, hidden, no)["kc32"] and wf.shape == (no, MR.layout(d, hidden, no)["kf"])
    part = wf[:, kc32:kc32 + hidden]
    ulps = np.abs(part.astype(np.float64) - ref_w) / np.spacing(np.abs(ref_w))
    ulps_b = np.abs(bf.astype(np.float64) - ref_b) / np.spacing(np.abs(ref_b))
    print(f"compose d={d} m={hidden} no={no}: max ulp weight {ulps.max():.2f} bias {ulps_b.max():.2f}")
    assert ulps.max() <= 1.0 and ulps_b.max() <= 1.0
    assert np.array_equal(wf[:, :d], sd["adjust.weight"].numpy())
    assert not wf[MR.padding_mask(d, hidden, no)].any()
    # the pack is the rounded matrix in 16 x 32 fragment tiles, rows padded to 128 with zeros
    pack = got["pack"].view(torch.bfloat16).float().cpu().numpy().reshape(-1, wf.shape[1] // 32, 16, 32)
    rows = pack.transpose(0, 2, 1, 3).reshape(-1, wf.shape[1])
    assert np.array_equal(rows[:no], torch.from_numpy(wf).bfloat16().float().numpy()) and not rows[no:].any()


# ------------------------------------------------------------------------------------------------ ops against float64
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("d,heads,hidden,no", SHAPES)
def test_folded_block_is_as_accurate_as_the_chain(d, heads, hidden, no, shift):
    B, H, W = GEOM[shift]
    sd, dense, ref, last = case(d, heads, hidden, no, shift)
    assert ops.swin_block_fold_supported(B, H, W, d, heads, hidden, no)
    chain = run(ops.swin_block, sd, dense, B, H, W, shift, heads, last).double()
    fold = run(ops.swin_block_folded, sd, dense, B, H, W, shift, heads, last).double()
    assert not torch.isnan(fold).any()
    ef, ec = fold - ref, chain - ref
    rms = float(ef.pow(2).mean().sqrt() / ec.pow(2).mean().sqrt())
    mx = float(ef.abs().max() / ec.abs().max())
    apart = float((fold - chain).abs().max() / ref.abs().max())
    print(f"fold/chain d={d} m={hidden} no={no} shift={shift} {B}x{H}x{W}: rms ratio {rms:.3f} max ratio {mx:.3f} apart/max {apart:.2e} "
          f"(chain rms err / max {float(ec.pow(2).mean().sqrt() / ref.abs().max()):.2e})")
    assert rms <= 1.05, rms
    assert mx <= 1.5, mx
    assert apart <= 1e-2, apart


# ------------------------------------------------------------------------------------------------ the x1 | h seam
@pytest.mark.parametrize("d,heads,hidden,no", [(180, 6, 360, 32), (168, 6, 360, 32), (308, 4, 308, 180)])
def test_seam_and_padding_indexing(d, heads, hidden, no):
    """W2 is zero but for ONE entry (i, j) at the ends of both k ranges, A's rows are one-hot with power-of-two values: an output
    reads single columns of x1 and, through (i, j), one column of h.  An indexing error at the seam or in the padding is O(1)."""
    B, H, W = GEOM[0]
    last = no == 180
    for i, j in [(0, 0), (d - 1, hidden - 1), (0, hidden - 1), (d - 1, 0)]:
        sd = dict(make_block(d, heads, hidden, no, seed=3, round_weights=False))
        w2 = torch.zeros(d, hidden)
        w2[i, j] = 1.5
        a = torch.zeros(no, d)
        cols = [0, d - 1, i] + [(37 * r + 5) % d for r in range(3, no)]
        for r in range(no):
            a[r, cols[r]] = 2.0 ** (r % 4 - 1)
        sd["mlp.fc2.weight"], sd["adjust.weight"] = w2, a
        dense = (torch.randn(B * H * W, D, generator=torch.Generator().manual_seed(11)) * 1.5 + 0.3)
        ref = ref64(sd, dense, B, H, W, d, heads, 0, no, last)
        fold = run(ops.swin_block_folded, sd, dense, B, H, W, 0, heads, last).double()
        e = float((fold - ref).abs().max() / ref.abs().max())
        print(f"seam d={d} m={hidden} no={no} (i, j)=({i}, {j}): err/max {e:.2e}")
        assert e <= 1e-2, (i, j, e)


# ------------------------------------------------------------------------------------------------ epilogue
@pytest.mark.parametrize("d,heads,hidden,no", [(180, 6, 360, 32), (308, 4, 308, 180)])
def test_zero_adjust_weight_leaves_the_epilogue_alone(d, heads, hidden, no):
    """A = 0: the output is exactly act(b_a) * alpha + R.  (adjust5's alpha is 0.25 here: with a power of two the product is
    exact, so a fused and an unfused multiply-add give the same float.)"""
    B, H, W = GEOM[0]
    last = no == 180
    sd = dict(make_block(d, heads, hidden, no, seed=5, round_weights=False))
    sd["adjust.weight"] = torch.zeros(no, d)
    dense = (torch.randn(B * H * W, D, generator=torch.Generator().manual_seed(13)) * 1.5 + 0.3)
    got = run(ops.swin_block_folded, sd, dense, B, H, W, 0, heads, last, alpha=0.25)
    ba = sd["adjust.bias"]
    want = (ba * 0.25 + dense[:, :no]) if last else F.leaky_relu(ba, 0.2).expand(B * H * W, no)
    assert torch.equal(got, want)


def test_folded_op_refuses_what_it_does_not_do():
    assert not ops.swin_block_fold_supported(1, 8, 8, 180, 6, 360, 64)             # one column group, more than two column tiles
    assert not ops.swin_block_fold_supported(1, 8, 8, 180, 6, 360, 32, precision="fp32")
    sd = make_block(180, 6, 360, 64, seed=1)
    x = torch.zeros(64, D, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.swin_block_folded(x, *[sd[k].cuda() for k in KEYS], 1, 8, 8, 0, 6, out=x, out_offset=180)
    assert torch.count_nonzero(x) == 0


# ------------------------------------------------------------------------------------------------ engine
def _cfg_sd(seed=5):
    from srad_amd import spec as S
    cfg = S.DRCTConfig(n_rdg=1)
    return cfg, S.synth_state(S.drct_spec(cfg), seed=seed, cfg=cfg)


def _x(shape, seed=2):
    from srad_amd import spec as S
    return torch.from_numpy(S.synth_image("mlp_fold/model", shape, seed=seed, rgb_range=1.0)).cuda()


def _build(cfg, sd, precision="bf16", use_graph=False):
    from tests.test_gpu_drct import build
    return build(cfg, sd, precision, use_graph)


@pytest.mark.parametrize("shape", [(1, 1, 8, 8), (2, 1, 16, 16)])
def test_model_fold_against_chain_and_oracle(shape):
    cfg, sd = _cfg_sd()
    x = _x(shape)
    with torch.no_grad():
        ref = R.drct_forward(sd, x.cpu(), cfg).numpy()
        fold = _build(cfg, sd)(x).cpu().numpy()
        with ops.path_override(fc2_chain=True):
            chain = _build(cfg, sd)(x).cpu().numpy()
    rng = float(ref.max() - ref.min())
    assert not np.array_equal(fold, chain)                     # two different second halves did run
    print(f"model {shape}: fold vs chain / range {np.abs(fold - chain).max() / rng:.2e}")
    assert np.abs(fold - chain).max() / rng < 1e-2
    for name, out in (("fold", fold), ("chain", chain)):
        err = np.abs(out.astype(np.float64) - ref)
        psnr = 10 * np.log10(rng ** 2 / np.mean(err ** 2))
        print(f"  {name}: max err / range {err.max() / rng:.2e} psnr {psnr:.1f}")
        assert err.max() / rng < 1e-2 and psnr > 50.0


def test_model_graph_replay_and_toggle():
    cfg, sd = _cfg_sd()
    x = _x((1, 1, 16, 16))
    m = _build(cfg, sd, use_graph=True)
    with torch.no_grad():
        outs = [m(x).cpu().numpy() for _ in range(4)]           # eager, capture, replay, replay
        assert all(np.array_equal(outs[0], o) for o in outs[1:])
        with ops.path_override(fc2_chain=True):
            chain = [m(x).cpu().numpy() for _ in range(3)]
            fresh_chain = _build(cfg, sd)(x).cpu().numpy()
        again = [m(x).cpu().numpy() for _ in range(3)]
    assert all(np.array_equal(chain[0], o) for o in chain[1:]) and np.array_equal(chain[0], fresh_chain)
    assert not np.array_equal(chain[0], outs[0])
    assert all(np.array_equal(outs[0], o) for o in again)


def test_model_freshness_and_no_rebuild():
    """After load_state_dict of other weights the folded model equals a freshly built one bit for bit; a forward that changed
    nothing launches no pack_weight; one changed source is rebuilt ahead of the replayed graph."""
    cfg, sd = _cfg_sd(seed=5)
    _, sd2 = _cfg_sd(seed=6)
    x = _x((1, 1, 8, 8))
    m = _build(cfg, sd, use_graph=True)
    with torch.no_grad():
        first = [m(x).cpu().numpy() for _ in range(3)]
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd2.items()}, strict=True)
        after = [m(x).cpu().numpy() for _ in range(3)]
        fresh = _build(cfg, sd2)(x).cpu().numpy()
        assert all(np.array_equal(fresh, o) for o in after) and not np.array_equal(fresh, first[0])
        L.prof_enable(True)
        L.prof_collect()
        try:
            m(x)
            torch.cuda.synchronize()
            prof = L.prof_collect()
        finally:
            L.prof_enable(False)
        assert prof.get("pack_weight", {"launches": 0})["launches"] == 0
        m.get_parameter("layers.0.swin2.mlp.fc2.weight").mul_(1.25)
        m.get_parameter("layers.0.adjust5.bias").add_(0.05)
        changed = [m(x).cpu().numpy() for _ in range(2)]
        fresh2 = _build(cfg, {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()})(x).cpu().numpy()
    assert np.array_equal(changed[0], fresh2) and np.array_equal(changed[1], fresh2) and not np.array_equal(changed[0], fresh)


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16-training", "bf16-32-row-tiles"])
def test_what_does_not_fold_is_bit_equal_under_the_override(mode):
    """fp32, split-bf16, a handle bound for training and a batch whose mlp_block takes 32-row tiles (8192 tokens: too many
    windows for the one-launch block, enough rows for the wider tile) run the launches they always ran."""
    cfg, sd = _cfg_sd()
    x = _x((2, 1, 64, 64) if mode == "bf16-32-row-tiles" else (1, 1, 8, 8))

    def go():
        m = _build(cfg, sd, mode if mode in ("fp32", "bf16x3") else "bf16")
        if mode == "bf16-training":
            m.enable_training()
            m.eval()
        with torch.no_grad():
            return m(x).cpu().numpy()
    plain = go()
    with ops.path_override(fc2_chain=True):
        forced = go()
    assert np.array_equal(plain, forced)
