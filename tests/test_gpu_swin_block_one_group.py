"""GPU: the d = 276 / 308 instances of swin_block_kernel with compact head rows and all heads in one group.
Their values are checked by test_gpu_swin_block.py (oracle and the two launches, all five shapes); this file
adds what that one cannot see:

- repeatability: with one head group the probability tiles and the attention tile are laid over the normalised window tile.
  A wave that still read the window while another wrote probabilities would give outputs that depend on timing, so five calls
  on the same buffers must be bit-equal (12 windows = 48 workgroups, and one window);
- the engine path on a 1-RDG model of DRCT-L's widths, where all five block shapes occur once;
- the refusals, for these two shapes."""
import numpy as np
import pytest
import torch

from srad_amd import _lib as L
from srad_amd import ops
from tests.test_gpu_fused_ops import make_block
from tests.test_gpu_swin_block import D, case

pytestmark = pytest.mark.gpu

WIDE = [(276, 6, 276, 32), (308, 4, 308, 180)]               # (d, heads, hidden, adjust outputs) of swin4 and swin5


def _weights(sd):
    c = lambda k: sd[k].cuda()
    return (c("norm1.weight"), c("norm1.bias"), c("attn.qkv.weight"), c("attn.qkv.bias"), c("attn.relative_position_bias_table"),
            c("attn.proj.weight"), c("attn.proj.bias"), c("norm2.weight"), c("norm2.bias"), c("mlp.fc1.weight"), c("mlp.fc1.bias"),
            c("mlp.fc2.weight"), c("mlp.fc2.bias"), c("adjust.weight"), c("adjust.bias"))


@pytest.mark.parametrize("d,heads,hidden,no", WIDE)
@pytest.mark.parametrize("B,H,W", [(2, 16, 24), (1, 8, 8)])
def test_five_calls_on_the_same_buffers_are_bit_equal(d, heads, hidden, no, B, H, W):
    shift = 4
    sd, dense, ref, last, _ = case(d, heads, hidden, B, H, W, shift)
    w = _weights(sd)
    dg = dense.cuda()
    out = torch.full_like(dg, float("nan")) if last else dg    # adjust5 writes a second buffer, adjust_k behind the block's columns
    got = []
    for _ in range(5):
        if last:
            ops.swin_block(dg, *w, B, H, W, shift, heads, act=L.ACT_NONE, slope=0.0, alpha=0.2, residual=dg, out=out, out_offset=0)
            got.append(out[:, :no].clone())
        else:
            ops.swin_block(dg, *w, B, H, W, shift, heads, act=L.ACT_LRELU, slope=0.2, alpha=1.0, out=dg, out_offset=d)
            got.append(out[:, d:d + no].clone())
    assert not torch.isnan(got[0]).any()
    assert float((got[0].cpu() - ref).abs().max() / ref.abs().max()) < 2e-3    # the runs repeat the RIGHT values (test_gpu_swin_block's BAR)
    for i in range(1, 5):
        assert torch.equal(got[0], got[i]), f"call {i} differs from call 0 in {int((got[0] != got[i]).sum())} values"


def test_engine_runs_every_block_shape_of_a_one_rdg_model():
    """DRCT-L's widths (embed 180, growth 32: d = 180 .. 308), one RDG, synthetic weights, B = 1, 16 x 16 LR, bf16: the path the
    engine picks against the same engine forced back to the pair, and against the oracle."""
    from oracle import sr_ref as R
    from srad_amd import spec as S
    from srad_amd.nets import DRCT
    from tests.test_gpu_drct import Opt
    cfg = S.DRCTConfig(n_rdg=1, img_size=16)
    assert [b[0] for b in cfg.block_table()] == [180, 212, 244, 276, 308]
    sd = S.synth_state(S.drct_spec(cfg), seed=11, cfg=cfg)
    x = S.synth_image("one_group", (1, 1, 16, 16), seed=5)
    with torch.no_grad():
        y = R.drct_forward(sd, torch.from_numpy(x), cfg).numpy()
    rng = float(y.max() - y.min())
    xt = torch.from_numpy(x).cuda()

    def model(use_graph=False):
        m = DRCT(Opt(cfg, "bf16", use_graph)).cuda().eval()
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        return m

    def profiled(m):
        L.prof_enable(True)
        L.prof_collect()
        with torch.no_grad():
            out = m(xt).cpu().numpy()
        torch.cuda.synchronize()
        prof = L.prof_collect()
        L.prof_enable(False)
        return out, {k: v["launches"] for k, v in prof.items()}

    new, ran = profiled(model())
    with ops.path_override(block_two_launches=True):
        two, ran2 = profiled(model())
    print("classes", ran, "| override:", ran2)
    assert ran2.get("swin_block", 0) == 0 and ran2["qkv_attn"] == 5 and ran2["mlp_block"] == 5
    assert ran.get("swin_block", 0) >= 3                       # d = 180 / 212 / 244 stay on one launch
    assert ran.get("swin_block", 0) + ran.get("qkv_attn", 0) == 5
    err = np.abs(new - y)
    psnr = 10 * np.log10(rng ** 2 / np.mean(err.astype(np.float64) ** 2))
    print("new vs pair max/range", np.abs(new - two).max() / rng, "new vs oracle", err.max() / rng, "psnr", psnr)
    assert np.abs(new - two).max() / rng < 1e-2
    assert err.max() / rng < 1e-2 and psnr > 50.0              # test_drct_bf16_close_to_reference's bars
    g = model(use_graph=True)
    with torch.no_grad():
        outs = [g(xt).cpu().numpy() for _ in range(4)]         # eager, capture, replay, replay
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]) and np.array_equal(outs[0], outs[3])
    assert np.array_equal(outs[0], new)


@pytest.mark.parametrize("d,heads,hidden,no", WIDE)
def test_wide_blocks_refuse_what_they_do_not_do(d, heads, hidden, no):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert ops.swin_block_supported(1, 8, 8, d, heads, hidden, no)
    assert not ops.swin_block_supported(1, 8, 8, d, heads, hidden, no, precision="bf16x3")
    assert not ops.swin_block_supported(1, 8, 8, d, heads, hidden, no, precision="fp32")
    side = 8
    while (side // 8) ** 2 * 4 <= cus:
        side += 8
    assert not ops.swin_block_supported(1, side, side, d, heads, hidden, no)      # windows x 4 > CUs
    w = _weights(make_block(d, heads, hidden, no, seed=1))
    x, y = torch.zeros(64, D + 32, device="cuda"), torch.zeros(64, D, device="cuda")
    for prec in ("bf16x3", "fp32"):
        with pytest.raises(RuntimeError, match="unsupported"):
            ops.swin_block(x, *w, 1, 8, 8, 0, heads, out=y, out_offset=0, precision=prec)
    big, ybig = torch.zeros(side * side, D + 32, device="cuda"), torch.zeros(side * side, D, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.swin_block(big, *w, 1, side, side, 0, heads, out=ybig, out_offset=0)
    assert torch.count_nonzero(y) == 0 and torch.count_nonzero(ybig) == 0         # errors, not launches
