"""GPU: a whole Swin block + the adjust conv as ONE launch (swin_block_kernel, kernels_fused_block.hip) through the C ABI
(srad_op_swin_block): against the oracle, against the two launches it replaces, inside the DRCT engine, and its refusals.

Reference: oracle.sr_ref.swin_block in fp32 on bf16-ROUNDED weights with the ``rnd`` hook rounding what the kernel rounds when
it stages MFMA operands, followed by the RDG's adjust step computed as in test_gpu_fused_ops.test_mlp_block_kernel_matches_oracle.
Bar: that file's 2e-3 of the output's max (BAR).  Against the pair (qkv_attn with the bf16 hand-off, then mlp_block on
16-row tiles) the products and the rounding points are the same, so only the order of a sum or a fused multiply-add may differ:
PAIR_BAR, four times the largest difference measured."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sr_ref as R
from srad_amd import _lib as L
from srad_amd import ops
from tests.test_gpu_fused_ops import BAR, BLOCKS, bf16r, make_block, rel

pytestmark = pytest.mark.gpu

D = 308                                                      # columns of the RDG's dense buffer
# one window (the four quarters and the wrap of the shift meet inside it); non-square, several windows, two images; shift on 2 x 2 windows
CASES = [(1, 8, 8, 0), (1, 8, 8, 4), (2, 16, 24, 0), (2, 16, 24, 4), (1, 16, 16, 4)]
# measured on MI355X: 18 of the 20 cases bit-equal, the largest difference 9.8e-5 (one token row, one bf16 rounding apart); x 4
PAIR_BAR = 4e-4
assert PAIR_BAR <= BAR


def oracle_out(sd, dense, B, H, W, d, heads, shift, last):
    """swin_block + adjust_k (32 outputs, LeakyReLU 0.2) or, for the RDG's fifth block, adjust5 (180 outputs, * 0.2 + x)."""
    x2 = R.swin_block(dict(sd), "", dense[:, :d].reshape(B, H * W, d).contiguous(), H, W, 8, heads, shift, rnd=bf16r).reshape(B * H * W, d)
    a = F.linear(bf16r(x2), sd["adjust.weight"], sd["adjust.bias"])
    return (a * 0.2 + dense[:, :180]) if last else F.leaky_relu(a, 0.2)


@functools.lru_cache(maxsize=None)
def case(d, heads, hidden, B, H, W, shift):
    """Weights, the dense buffer and the oracle's output of one case: computed once, shared by the tests, never written."""
    last = d == 308
    no = 180 if last else 32
    # the weights and rows of test_gpu_fused_ops.test_qkv_attn_kernel_matches_oracle: the two files check the same data
    sd = make_block(d, heads, hidden, no, seed=d + shift)
    dense = (torch.randn(B, H * W, D, generator=torch.Generator().manual_seed(7)) * 1.5 + 0.3).reshape(B * H * W, D)
    return sd, dense, oracle_out(sd, dense, B, H, W, d, heads, shift, last), last, no


def run_block(sd, dense, B, H, W, shift, heads, last):
    """ops.swin_block as the engine calls it: adjust_k in place behind the block's columns, adjust5 into a NaN-filled second
    buffer.  Returns (the buffer that was written, the dense buffer as it was before)."""
    c = lambda k: sd[k].cuda()
    w = (c("norm1.weight"), c("norm1.bias"), c("attn.qkv.weight"), c("attn.qkv.bias"), c("attn.relative_position_bias_table"),
         c("attn.proj.weight"), c("attn.proj.bias"), c("norm2.weight"), c("norm2.bias"), c("mlp.fc1.weight"), c("mlp.fc1.bias"),
         c("mlp.fc2.weight"), c("mlp.fc2.bias"), c("adjust.weight"), c("adjust.bias"))
    dg = dense.cuda()
    before = dg.clone()
    if last:
        out = torch.full_like(dg, float("nan"))
        ops.swin_block(dg, *w, B, H, W, shift, heads, act=L.ACT_NONE, slope=0.0, alpha=0.2, residual=dg, out=out, out_offset=0)
        return out, before, dg
    ops.swin_block(dg, *w, B, H, W, shift, heads, act=L.ACT_LRELU, slope=0.2, alpha=1.0, out=dg, out_offset=sd["norm1.weight"].numel())
    return dg, before, dg


def run_pair(sd, dense, B, H, W, shift, heads, last):
    c = lambda k: sd[k].cuda()
    d = sd["norm1.weight"].numel()
    dg = dense.cuda()
    attn = ops.qkv_attn(dg, c("norm1.weight"), c("norm1.bias"), c("attn.qkv.weight"), c("attn.qkv.bias"), c("attn.relative_position_bias_table"),
                        B, H, W, shift, heads, out_bf16=True)
    w = (c("attn.proj.weight"), c("attn.proj.bias"), c("norm2.weight"), c("norm2.bias"), c("mlp.fc1.weight"), c("mlp.fc1.bias"),
         c("mlp.fc2.weight"), c("mlp.fc2.bias"), c("adjust.weight"), c("adjust.bias"))
    if last:
        out = torch.full_like(dg, float("nan"))
        ops.mlp_block(attn, dg, *w, act=L.ACT_NONE, slope=0.0, alpha=0.2, residual=dg, out=out, out_offset=0, fm=16)
        return out[:, :180]
    ops.mlp_block(attn, dg, *w, act=L.ACT_LRELU, slope=0.2, alpha=1.0, out=dg, out_offset=d, fm=16)
    return dg[:, d:d + 32]


@pytest.mark.parametrize("d,heads,hidden", BLOCKS)
@pytest.mark.parametrize("B,H,W,shift", CASES)
def test_swin_block_matches_oracle(d, heads, hidden, B, H, W, shift):
    sd, dense, ref, last, no = case(d, heads, hidden, B, H, W, shift)
    out, before, dg = run_block(sd, dense, B, H, W, shift, heads, last)
    if last:
        got = out[:, :180]
        assert torch.isnan(out[:, 180:]).all()               # nothing written outside the adjust output's columns
        assert torch.equal(dg, before)                       # ... and the input buffer is only read
    else:
        got = out[:, d:d + 32]
        assert torch.equal(out[:, :d], before[:, :d]) and torch.equal(out[:, d + 32:], before[:, d + 32:])
    e = rel(got.cpu(), ref)
    print(f"swin_block d={d} heads={heads} m={hidden} no={no} shift={shift} {B}x{H}x{W}: rel err {e:.2e}")
    assert not torch.isnan(got).any()
    assert e < BAR, e


@pytest.mark.parametrize("d,heads,hidden", BLOCKS)
@pytest.mark.parametrize("B,H,W,shift", [(1, 8, 8, 4), (2, 16, 24, 0), (2, 16, 24, 4), (1, 16, 16, 4)])
def test_swin_block_matches_the_two_launches(d, heads, hidden, B, H, W, shift):
    sd, dense, ref, last, no = case(d, heads, hidden, B, H, W, shift)
    out, _, _ = run_block(sd, dense, B, H, W, shift, heads, last)
    got = out[:, :180] if last else out[:, d:d + 32]
    pair = run_pair(sd, dense, B, H, W, shift, heads, last)
    diff = float((got - pair).abs().max() / pair.abs().max())
    print(f"swin_block vs qkv_attn + mlp_block d={d} shift={shift} {B}x{H}x{W}: rel diff {diff:.2e}")
    assert diff < PAIR_BAR, diff


def test_swin_block_check_is_sensitive_to_bias_and_mask():
    """The data of test_gpu_fused_ops.test_qkv_attn_check_is_sensitive_to_bias_and_mask (unit-variance rows, in the first d
    columns of the dense buffer), the comparison carried through the rest of the block."""
    d, heads, hidden, B, H, W, shift = 212, 4, 424, 1, 16, 16, 4
    sd = make_block(d, heads, hidden, 32, seed=1)
    dense = torch.zeros(B * H * W, D)
    dense[:, :d] = torch.randn(B, H * W, d, generator=torch.Generator().manual_seed(3)).reshape(-1, d)
    ref = oracle_out(sd, dense, B, H, W, d, heads, shift, False)
    got = lambda s, sh: run_block(s, dense, B, H, W, sh, heads, False)[0][:, d:d + 32].cpu()
    assert rel(got(sd, shift), ref) < BAR
    bad = dict(sd)
    bad["attn.relative_position_bias_table"] = sd["attn.relative_position_bias_table"].clone()
    bad["attn.relative_position_bias_table"][37, 2] += 0.5                       # ONE entry of one head
    e_bias, e_shift = rel(got(bad, shift), ref), rel(got(sd, 0), ref)
    print(f"one bias entry off by 0.5: {e_bias:.2e} (> {5 * BAR:.0e}); shift dropped: {e_shift:.2e} (> {20 * BAR:.0e})")
    assert e_bias > 5 * BAR
    assert e_shift > 20 * BAR                                                    # shift / mask ignored


def test_swin_block_refuses_what_it_does_not_do():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert ops.swin_block_supported(1, 8, 8, 180, 6, 360, 32)
    assert not ops.swin_block_supported(1, 8, 8, 180, 6, 360, 32, precision="bf16x3")
    assert not ops.swin_block_supported(1, 8, 8, 180, 6, 360, 32, precision="fp32")
    assert not ops.swin_block_supported(1, 64, 64, 180, 6, 360, 32, ws=64)
    side = 8
    while (side // 8) ** 2 * 4 <= cus:
        side += 8
    assert not ops.swin_block_supported(1, side, side, 180, 6, 360, 32)           # windows x 4 > CUs
    sd = make_block(180, 6, 360, 32, seed=1)
    c = lambda k: sd[k].cuda()
    w = (c("norm1.weight"), c("norm1.bias"), c("attn.qkv.weight"), c("attn.qkv.bias"), c("attn.relative_position_bias_table"),
         c("attn.proj.weight"), c("attn.proj.bias"), c("norm2.weight"), c("norm2.bias"), c("mlp.fc1.weight"), c("mlp.fc1.bias"),
         c("mlp.fc2.weight"), c("mlp.fc2.bias"), c("adjust.weight"), c("adjust.bias"))
    x = torch.zeros(64, D, device="cuda")
    for prec in ("bf16x3", "fp32"):
        with pytest.raises(RuntimeError, match="unsupported"):
            ops.swin_block(x, *w, 1, 8, 8, 0, 6, out=x, out_offset=180, precision=prec)
    big = torch.zeros(side * side, D, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.swin_block(big, *w, 1, side, side, 0, 6, out=big, out_offset=180)
    with pytest.raises(RuntimeError, match="in-place output"):
        ops.swin_block(x, *w, 1, 8, 8, 0, 6, out=x, out_offset=0)                # would overwrite columns other workgroups read
    assert torch.count_nonzero(x) == 0 and torch.count_nonzero(big) == 0          # errors, not launches


def _model(cfg, sd, use_graph=False):
    from srad_amd.nets import DRCT
    from tests.test_gpu_drct import Opt
    m = DRCT(Opt(cfg, "bf16", use_graph)).cuda().eval()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m


def test_engine_takes_the_single_launch_and_the_override_restores_the_pair(sr_golden):
    """DRCT forward (bf16) on a reference fixture: the path the engine picks against the same engine forced back to the
    qkv_attn + mlp_block pair.  Block shapes that are in the engine's table of measured wins run as one launch (the profiler
    classes show which kernels ran); under the override none does."""
    from tests.helpers import drct_case
    cfg, sd, x, y = drct_case(sr_golden, "drct_r2_rgb_x4")
    xt = torch.from_numpy(x).cuda()
    assert xt.shape[0] * (xt.shape[2] // 8) * (xt.shape[3] // 8) * 4 <= torch.cuda.get_device_properties(0).multi_processor_count
    rng = float(y.max() - y.min())

    def profiled(m):
        L.prof_enable(True)
        L.prof_collect()
        with torch.no_grad():
            out = m(xt).cpu().numpy()
        torch.cuda.synchronize()
        prof = L.prof_collect()
        L.prof_enable(False)
        return out, {k: v["launches"] for k, v in prof.items()}

    new, ran = profiled(_model(cfg, sd))
    with ops.path_override(block_two_launches=True):
        two, ran2 = profiled(_model(cfg, sd))
    print("one launch per block: classes", ran, "| override:", ran2)
    nblk = 5 * cfg.n_rdg
    assert ran2.get("swin_block", 0) == 0 and ran2["qkv_attn"] == nblk and ran2["mlp_block"] == nblk
    assert ran.get("swin_block", 0) > 0, "no block shape of this model is in the engine's table"
    assert ran.get("swin_block", 0) + ran.get("qkv_attn", 0) == nblk and ran.get("qkv_attn", 0) == ran.get("mlp_block", 0)
    err = np.abs(new - y)
    print("new vs pair max/range", np.abs(new - two).max() / rng, "new vs ref", err.max() / rng)
    assert np.abs(new - two).max() / rng < 1e-2
    assert err.max() / rng < 1e-2                                                  # test_drct_bf16_close_to_reference's bars
    assert 10 * np.log10(rng ** 2 / np.mean(err.astype(np.float64) ** 2)) > 50.0
    g = _model(cfg, sd, use_graph=True)
    with torch.no_grad():
        outs = [g(xt).cpu().numpy() for _ in range(4)]                             # eager, capture, replay, replay
    assert np.array_equal(outs[2], outs[3]) and np.array_equal(outs[0], outs[2]) and np.array_equal(outs[0], new)
