"""GPU: the two launch geometries of qkv_attn_kernel (kernels_fused_attn.hip).

The engines pick the grid from the shape: (windows, heads), or - when that leaves CUs idle - the query split (windows,
2 heads): two workgroups per (window, head), each with the softmax and P.V of 32 of the window's 64 queries.  For each of
DRCT-L's five block shapes at the C2 / C4 geometries (B = 4 and 8, 32 x 32 tokens) this runs the launch the engine picks
against the oracle (as tests/test_gpu_fused_ops.py does, same bar) and checks the grid it reports.  The query split runs the
same MFMAs on the same 16-row tiles in the same order as the plain grid, so its output and every training save (LN1(x),
q | k | v in fp32 and as the bf16 operands) must equal the plain launch's bit for bit; that is checked wherever the split is
chosen, and at small geometries where every block shape takes it."""
import pytest
import torch

from oracle import sr_ref as R
from srad_amd import ops

from tests.test_gpu_fused_ops import BLOCKS, bf16r, make_block, rel

pytestmark = pytest.mark.gpu
# the bar of tests/test_gpu_fused_ops.py is for its 64 - 768-token geometries; over the 4096 / 8192 tokens here the largest
# error of the max-normalised output is larger (d = 212, heads 4, B = 4: 2.1e-3, the same at the parent commit's kernel)
BAR_C2 = 3e-3


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _args(sd):
    return [sd[k].cuda() for k in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.relative_position_bias_table")]


def _expected_grid(B, H, W, heads):
    n = B * (H // 8) * (W // 8)
    return (n, 2 * heads) if n * heads < _cus() else (n, heads)


def _check_split_matches_plain(x, sd, B, H, W, shift, d, heads):
    hd = d // heads
    hdp, hp_h = (hd + 3) // 4 * 4, (hd + 7) // 8 * 8
    assert ops.qkv_attn_grid(B, H, W, d, heads) == (B * (H // 8) * (W // 8), 2 * heads)
    assert ops.qkv_attn_grid(B, H, W, d, heads, no_qsplit=True) == (B * (H // 8) * (W // 8), heads)
    split = ops.qkv_attn_train(x, *_args(sd), B, H, W, shift, heads, hdp, hp_h, fill=7.0)
    plain = ops.qkv_attn_train(x, *_args(sd), B, H, W, shift, heads, hdp, hp_h, no_qsplit=True, fill=7.0)
    for k in plain:
        assert torch.equal(split[k], plain[k]), f"query split differs from the plain grid in {k}"
    # every save was written (the fill survives only in the head padding of the q | k | v slots)
    assert not (plain["xn"] == 7.0).any() and not (plain["out_h"] == 7.0).any()
    assert not (plain["qkv"][..., :hd] == 7.0).any() and not (plain["qkv_h"][..., :hd] == 7.0).any()
    return split


@pytest.mark.parametrize("d,heads,hidden", BLOCKS)
@pytest.mark.parametrize("B", [4, 8])
def test_engine_launch_matches_oracle(d, heads, hidden, B):
    H = W = 32
    shift = 4 if B == 4 else 0
    grid = ops.qkv_attn_grid(B, H, W, d, heads)
    assert grid == _expected_grid(B, H, W, heads)
    sd = make_block(d, heads, hidden, 32, seed=d + B)
    g = torch.Generator().manual_seed(11)
    D = 308
    x = torch.randn(B, H * W, D, generator=g) * 1.5 + 0.3
    taps = {}
    R.swin_block(dict(sd), "", x[..., :d].contiguous(), H, W, 8, heads, shift, rnd=bf16r, taps=taps)
    ref = taps["attn"].reshape(B * H * W, d)
    xg = x.reshape(B * H * W, D).cuda()
    out = ops.qkv_attn(xg, *_args(sd), B, H, W, shift, heads)
    e = rel(out.cpu(), ref)
    print(f"qkv_attn d={d} heads={heads} B={B} grid={grid}: rel err {e:.2e}")
    assert e < BAR_C2, e
    if grid[1] == 2 * heads:
        split = _check_split_matches_plain(xg, sd, B, H, W, shift, d, heads)
        assert torch.equal(split["out_h"], out.to(torch.bfloat16))


@pytest.mark.parametrize("d,heads,hidden", BLOCKS)
@pytest.mark.parametrize("B,H,W,shift", [(1, 8, 8, 0), (2, 16, 24, 4)])
def test_query_split_saves_match_plain_grid(d, heads, hidden, B, H, W, shift):
    sd = make_block(d, heads, hidden, 32, seed=d + 3)
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(B * H * W, 320, generator=g) * 1.5 + 0.3).cuda()
    _check_split_matches_plain(x, sd, B, H, W, shift, d, heads)


def test_split_bf16_keeps_the_plain_grid():
    assert ops.qkv_attn_grid(1, 8, 8, 244, 2, precision="bf16x3") == (1, 2)
