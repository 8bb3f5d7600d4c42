"""GPU: fc2 folded into the RDG's adjust conv in the two-launch form of a Swin block (mlp_block_kernel's FOLD
form): the folded op against the unfolded one with float64 of the unfolded math as the referee at every tile height with a
folded instance, both adjust epilogues, and the engine's rule, graph and freshness behaviour with the pair forced.

Bars are tests/test_gpu_mlp_fold.py's (set by that change's issue from a CPU emulation of the bf16 rounding points): the folded
op's RMS error against float64 at most 1.05 x the unfolded op's on the same inputs, its max error at most 1.5 x, the two
outputs within 1e-2 of the output's max of each other; a bf16 model within 1e-2 of the range and above 50 dB against the
oracle, fold and chain within 1e-2 of the range of each other.  The tests print each figure.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sr_ref as R
from srad_amd import _lib as L
from srad_amd import ops
from tests.test_gpu_fused_ops import make_block
from tests.test_gpu_mlp_fold import SHAPES

pytestmark = pytest.mark.gpu

D = 308                                                      # columns of the RDG's dense buffer
KEYS = ("attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias",
        "adjust.weight", "adjust.bias")
# (rows, rows per workgroup; 0 = the launcher's choice): four 16-row tiles, sixteen, five (no multiple of 32 or 64), and two
# tiles of each wider height
TILES = [(64, 0), (256, 0), (80, 0), (64, 32), (128, 64)]


def has_instance(d, hidden, fm):
    """64-row tiles at d = 244 have no folded instance (the tile does not fit the LDS): that launch keeps the chain."""
    return not (fm == 64 and (d, hidden) == (244, 488))


@functools.lru_cache(maxsize=None)
def case(d, heads, hidden, no, M):
    """Weights in fp32 (what the fold is composed from), the attention output as the bf16 values both kernels take, and the
    unfolded math in float64."""
    sd = make_block(d, heads, hidden, no, seed=d + M, round_weights=False)
    g = torch.Generator().manual_seed(7 + M)
    dense = torch.randn(M, D, generator=g) * 1.5 + 0.3
    attn = (torch.randn(M, d, generator=g) * 0.8).bfloat16()
    last = no == 180
    s = {k: v.double() for k, v in sd.items()}
    x1 = dense[:, :d].double() + F.linear(attn.double(), s["attn.proj.weight"], s["attn.proj.bias"])
    h = F.gelu(F.linear(F.layer_norm(x1, (d,), s["norm2.weight"], s["norm2.bias"], 1e-5), s["mlp.fc1.weight"], s["mlp.fc1.bias"]))
    a = F.linear(x1 + F.linear(h, s["mlp.fc2.weight"], s["mlp.fc2.bias"]), s["adjust.weight"], s["adjust.bias"])
    ref = (a * 0.2 + dense[:, :no].double()) if last else F.leaky_relu(a, 0.2)
    assert ref.dtype == torch.float64
    return sd, dense, attn, ref, last


def run(fn, sd, dense, attn, last, fm, alpha=0.2):
    """The op as the engine calls it: adjust_k in place behind the block's columns (yoff = d), adjust5 with the residual from
    one buffer and the output into another, NaN-filled.  Returns the adjust output's columns."""
    d, no = sd["norm2.weight"].numel(), sd["adjust.bias"].numel()
    w = [sd[k].cuda() for k in KEYS]
    dg = dense.cuda()
    before = dg.clone()
    if last:
        out = torch.full_like(dg, float("nan"))
        fn(attn.cuda(), dg, *w, act=L.ACT_NONE, slope=0.0, alpha=alpha, residual=dg, out=out, out_offset=0, fm=fm)
        assert torch.isnan(out[:, no:]).all() and torch.equal(dg, before)
        return out[:, :no].cpu()
    fn(attn.cuda(), dg, *w, act=L.ACT_LRELU, slope=0.2, alpha=1.0, out=dg, out_offset=d, fm=fm)
    assert torch.equal(dg[:, :d], before[:, :d]) and torch.equal(dg[:, d + no:], before[:, d + no:])     # columns [0, d) untouched
    return dg[:, d:d + no].cpu()


# ------------------------------------------------------------------------------------------------ ops against float64
@pytest.mark.parametrize("M,fm", TILES)
@pytest.mark.parametrize("d,heads,hidden,no", SHAPES)
def test_folded_mlp_block_is_as_accurate_as_the_chain(d, heads, hidden, no, M, fm):
    if not has_instance(d, hidden, fm):
        sd, dense, attn, ref, last = case(d, heads, hidden, no, M)
        x = torch.zeros(M, D, device="cuda")
        with pytest.raises(RuntimeError, match="unsupported"):
            ops.mlp_block_folded(attn.cuda(), x, *[sd[k].cuda() for k in KEYS], out=x, out_offset=d, fm=fm)
        assert torch.count_nonzero(x) == 0
        return
    sd, dense, attn, ref, last = case(d, heads, hidden, no, M)
    chain = run(ops.mlp_block, sd, dense, attn, last, fm).double()
    fold = run(ops.mlp_block_folded, sd, dense, attn, last, fm).double()
    assert not torch.isnan(fold).any()
    ef, ec = fold - ref, chain - ref
    rms = float(ef.pow(2).mean().sqrt() / ec.pow(2).mean().sqrt())
    mx = float(ef.abs().max() / ec.abs().max())
    apart = float((fold - chain).abs().max() / ref.abs().max())
    print(f"mlp_block fold/chain d={d} m={hidden} no={no} M={M} fm={fm}: rms ratio {rms:.3f} max ratio {mx:.3f} apart/max {apart:.2e} "
          f"(chain rms err / max {float(ec.pow(2).mean().sqrt() / ref.abs().max()):.2e})")
    assert rms <= 1.05, rms
    assert mx <= 1.5, mx
    assert apart <= 1e-2, apart


@pytest.mark.parametrize("fm", [16, 32, 64])
@pytest.mark.parametrize("d,heads,hidden,no", [(180, 6, 360, 32), (168, 6, 360, 32), (308, 4, 308, 180)])
def test_seam_and_padding_indexing(d, heads, hidden, no, fm):
    """W2 is zero but for ONE entry (i, j) at the ends of both k ranges, A's rows are one-hot with power-of-two values: an output
    reads single columns of x1 and, through (i, j), one column of h.  An indexing error at the seam, in the padding or in the
    row tiles of a wider workgroup is O(1)."""
    M = 2 * fm
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
        g = torch.Generator().manual_seed(11)
        dense = torch.randn(M, D, generator=g) * 1.5 + 0.3
        attn = (torch.randn(M, d, generator=g) * 0.8).bfloat16()
        s = {k: v.double() for k, v in sd.items()}
        x1 = dense[:, :d].double() + F.linear(attn.double(), s["attn.proj.weight"], s["attn.proj.bias"])
        h = F.gelu(F.linear(F.layer_norm(x1, (d,), s["norm2.weight"], s["norm2.bias"], 1e-5), s["mlp.fc1.weight"], s["mlp.fc1.bias"]))
        av = F.linear(x1 + F.linear(h, s["mlp.fc2.weight"], s["mlp.fc2.bias"]), s["adjust.weight"], s["adjust.bias"])
        ref = (av * 0.2 + dense[:, :no].double()) if last else F.leaky_relu(av, 0.2)
        fold = run(ops.mlp_block_folded, sd, dense, attn, last, fm).double()
        e = float((fold - ref).abs().max() / ref.abs().max())
        print(f"seam d={d} m={hidden} no={no} fm={fm} (i, j)=({i}, {j}): err/max {e:.2e}")
        assert e <= 1e-2, (i, j, e)


@pytest.mark.parametrize("fm", [16, 64])
@pytest.mark.parametrize("d,heads,hidden,no", [(180, 6, 360, 32), (308, 4, 308, 180)])
def test_zero_adjust_weight_leaves_the_epilogue_alone(d, heads, hidden, no, fm):
    """A = 0: the output is exactly act(b_a) * alpha + R.  (adjust5's alpha is 0.25 here: with a power of two the product is
    exact, so a fused and an unfused multiply-add give the same float.)"""
    M = 2 * fm
    last = no == 180
    sd = dict(make_block(d, heads, hidden, no, seed=5, round_weights=False))
    sd["adjust.weight"] = torch.zeros(no, d)
    g = torch.Generator().manual_seed(13)
    dense = torch.randn(M, D, generator=g) * 1.5 + 0.3
    attn = (torch.randn(M, d, generator=g) * 0.8).bfloat16()
    got = run(ops.mlp_block_folded, sd, dense, attn, last, fm, alpha=0.25)
    ba = sd["adjust.bias"]
    want = (ba * 0.25 + dense[:, :no]) if last else F.leaky_relu(ba, 0.2).expand(M, no)
    assert torch.equal(got, want)


def test_folded_op_refuses_what_it_does_not_do():
    assert not ops.mlp_block_fold_supported(64, 180, 360, 64)                     # one column group, more than two column tiles
    assert not ops.mlp_block_fold_supported(64, 180, 360, 32, precision="fp32")
    assert not ops.mlp_block_fold_supported(65536, 244, 488, 32) and ops.mlp_block_fold_supported(8192, 244, 488, 32)
    sd = make_block(180, 6, 360, 64, seed=1)
    x = torch.zeros(64, D, device="cuda")
    attn = torch.zeros(64, 180, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.mlp_block_folded(attn, x, *[sd[k].cuda() for k in KEYS], out=x, out_offset=180)
    sd = make_block(180, 6, 360, 32, seed=1)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.mlp_block_folded(attn, x, *[sd[k].cuda() for k in KEYS], out=x, out_offset=180, precision="bf16x3")
    assert torch.count_nonzero(x) == 0


# ------------------------------------------------------------------------------------------------ engine, the pair forced
def _cfg_sd(n_rdg=1, seed=5, **kw):
    from srad_amd import spec as S
    cfg = S.DRCTConfig(n_rdg=n_rdg, **kw)
    return cfg, S.synth_state(S.drct_spec(cfg), seed=seed, cfg=cfg)


def _x(shape, seed=2):
    from srad_amd import spec as S
    return torch.from_numpy(S.synth_image("mlp_block_fold/model", shape, seed=seed, rgb_range=1.0)).cuda()


def _build(cfg, sd, precision="bf16", use_graph=False):
    from tests.test_gpu_drct import build
    return build(cfg, sd, precision, use_graph)


def _check_fold_chain_oracle(cfg, sd, x, label):
    with torch.no_grad():
        ref = R.drct_forward(sd, x.cpu(), cfg).numpy()
        fold = _build(cfg, sd)(x).cpu().numpy()
        with ops.path_override(fc2_chain=True):
            chain = _build(cfg, sd)(x).cpu().numpy()
    rng = float(ref.max() - ref.min())
    assert not np.array_equal(fold, chain)                     # two different second halves did run
    print(f"model {label}: fold vs chain / range {np.abs(fold - chain).max() / rng:.2e}")
    assert np.abs(fold - chain).max() / rng < 1e-2
    for name, out in (("fold", fold), ("chain", chain)):
        err = np.abs(out.astype(np.float64) - ref)
        psnr = 10 * np.log10(rng ** 2 / np.mean(err ** 2))
        print(f"  {name}: max err / range {err.max() / rng:.2e} psnr {psnr:.1f}")
        assert err.max() / rng < 1e-2 and psnr > 50.0
    return fold


@pytest.mark.parametrize("n_rdg", [1, 2])
@pytest.mark.parametrize("shape", [(1, 1, 8, 8), (2, 1, 16, 16)])
def test_model_pair_fold_against_chain_and_oracle(shape, n_rdg):
    """All five blocks of an RDG as qkv_attn + the folded mlp_block (that the pair runs under the override is
    test_model_pair_second_forward_builds_nothing's launch count)."""
    cfg, sd = _cfg_sd(n_rdg)
    with ops.path_override(block_two_launches=True):
        _check_fold_chain_oracle(cfg, sd, _x(shape), f"{shape} {n_rdg} RDG, pair")


def test_model_window16_takes_the_fold():
    """Window 16 (window attention + mlp_block: no one-launch block there) at the smallest size whose shifted blocks still
    shift: 2 x 2 windows."""
    cfg, sd = _cfg_sd(1, in_chans=1, img_size=32, window_size=16, upscale=4)
    _check_fold_chain_oracle(cfg, sd, _x((1, 1, 32, 32)), "window 16")


def test_model_pair_graph_replay_and_toggle():
    cfg, sd = _cfg_sd()
    x = _x((1, 1, 16, 16))
    with ops.path_override(block_two_launches=True), torch.no_grad():
        eager = _build(cfg, sd)(x).cpu().numpy()
        m = _build(cfg, sd, use_graph=True)
        outs = [m(x).cpu().numpy() for _ in range(4)]           # eager, capture, replay, replay
        assert all(np.array_equal(eager, o) for o in outs)
        with ops.path_override(fc2_chain=True):
            chain = [m(x).cpu().numpy() for _ in range(3)]
            fresh_chain = _build(cfg, sd)(x).cpu().numpy()
        again = [m(x).cpu().numpy() for _ in range(3)]
    assert all(np.array_equal(chain[0], o) for o in chain[1:]) and np.array_equal(chain[0], fresh_chain)
    assert not np.array_equal(chain[0], outs[0])
    assert all(np.array_equal(outs[0], o) for o in again)


def test_model_pair_second_forward_builds_nothing():
    cfg, sd = _cfg_sd()
    x = _x((1, 1, 8, 8))
    with ops.path_override(block_two_launches=True), torch.no_grad():
        m = _build(cfg, sd)
        m(x)
        L.prof_enable(True)
        L.prof_collect()
        try:
            m(x)
            torch.cuda.synchronize()
            prof = L.prof_collect()
        finally:
            L.prof_enable(False)
    assert prof.get("pack_weight", {"launches": 0})["launches"] == 0
    assert prof.get("mlp_block", {"launches": 0})["launches"] == 5 and prof.get("swin_block", {"launches": 0})["launches"] == 0
