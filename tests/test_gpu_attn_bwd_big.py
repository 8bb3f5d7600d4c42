"""GPU: the tiled window-attention backward (window_attn_bwd_tiled_kernel: 32 x 32 and 64 x 64 windows, 1024 / 4096 tokens per
window, the 512 / 1024 px presets) through the op entry point.
 * dq | dk | dv and the bias-table gradient against autograd of the oracle's attention, built as tests/test_gpu_bwd_ops.py builds
   it for the general kernel, at that test's bar (2e-4 of each tensor's largest value);
 * two calls on the same inputs give the same bits;
 * keys the shift mask hides from a query do not reach its dq row;
 * window sizes nobody built a kernel for come back as an error status, not a launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _inputs(ws, shift, B, H, W, d, heads):
    g = torch.Generator().manual_seed(ws * 1000 + d + shift)
    T = B * H * W
    qkv = torch.randn(T, 3 * d, generator=g) * 0.7
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g) * 0.5
    dout = torch.randn(T, d, generator=g)
    return qkv, table, dout


def _oracle(qkv, table, dout, ws, shift, B, H, W, d, heads):
    from oracle import sr_ref as R
    T, N, hd = B * H * W, ws * ws, d // heads
    qkv = qkv.clone().requires_grad_(True)
    table = table.clone().requires_grad_(True)
    x = qkv.view(B, H, W, 3 * d)
    if shift:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    xw = R.window_partition(x, ws).view(-1, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    mask = R.calculate_mask(H, W, ws, shift) if shift else None
    o = R.attention_from_qkv(xw[0] * hd ** -0.5, xw[1], xw[2], table, ws, mask)             # src/drct.py:282-299
    o = R.window_reverse(o.transpose(1, 2).reshape(-1, ws, ws, d), ws, H, W)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    o.reshape(T, d).backward(dout)
    return qkv.grad, table.grad


def _engine(dev, qkv, table, dout, ws, shift, B, H, W, heads, prec="fp32"):
    from srad_amd import ops
    return ops.window_attention_bwd(qkv.to(dev), dout.to(dev), table.to(dev), B, H, W, ws, shift, heads, precision=prec)


# ws 32: 2 x 2 windows, head dim 30 (no multiple of the MFMA K, one 32-column chunk), shift 0 and 16; two images of two windows at
# head dim 128 (four chunks).  ws 64: two windows side by side at shift 0 and 32, and ONE shifted window (four mask regions).
CASES = [(32, 0, 1, 64, 64, 180, 6), (32, 16, 1, 64, 64, 180, 6), (32, 16, 2, 32, 64, 256, 2),
         (64, 0, 1, 64, 128, 60, 2), (64, 32, 1, 64, 128, 60, 2), (64, 32, 1, 64, 64, 60, 2)]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("ws,shift,B,H,W,d,heads", CASES)
def test_tiled_attention_backward_matches_oracle_autograd(dev, prec, ws, shift, B, H, W, d, heads):
    """fp32 MFMAs in both precision modes, so both are held to the general kernel's 2e-4."""
    qkv, table, dout = _inputs(ws, shift, B, H, W, d, heads)
    if prec == "fp32":
        ref = _oracle(qkv, table, dout, ws, shift, B, H, W, d, heads)
        _REF[(ws, shift, B, H, W, d, heads)] = ref
    else:
        ref = _REF.get((ws, shift, B, H, W, d, heads)) or _oracle(qkv, table, dout, ws, shift, B, H, W, d, heads)
    dqkv, dtable = _engine(dev, qkv, table, dout, ws, shift, B, H, W, heads, prec)
    e1, e2 = _rel(dqkv, ref[0]), _rel(dtable, ref[1])
    print(f"tiled attention backward ws={ws} shift={shift} B={B} {H}x{W} d={d} heads={heads} {prec}: dqkv {e1:.2e} dtable {e2:.2e}")
    assert e1 < 2e-4 and e2 < 2e-4


_REF = {}     # the oracle's gradients of a case, computed once (the fp32 run) and shared with the bf16 run


@pytest.mark.parametrize("ws", [32, 64])
def test_table_gradient_is_the_sum_of_the_per_window_rows(dev, ws):
    """Shift 0: each window of the image is an image of its own, so the table gradient of the two-window image must be the
    sum of the two single-window gradients (each of them one partial row).  Two fp32 terms per entry in both: 1e-6."""
    B, H, W, d, heads = 1, ws, 2 * ws, 60, 2
    qkv, table, dout = _inputs(ws, 0, B, H, W, d, heads)
    _, full = _engine(dev, qkv, table, dout, ws, 0, B, H, W, heads)
    parts = []
    for wx in range(2):
        crop = lambda t: t.view(H, W, -1)[:, wx * ws:(wx + 1) * ws].reshape(ws * ws, -1).contiguous()
        parts.append(_engine(dev, crop(qkv), table, crop(dout), ws, 0, 1, ws, ws, heads)[1])
    assert float(parts[0].abs().max()) > 0 and float(parts[1].abs().max()) > 0
    e = _rel(full, parts[0] + parts[1])
    print(f"ws={ws}: table gradient vs sum of per-window rows {e:.2e}")
    assert e < 1e-6


@pytest.mark.parametrize("ws,shift,B,H,W,d,heads", [(32, 16, 1, 64, 64, 180, 6), (64, 32, 1, 64, 128, 60, 2)])
def test_tiled_attention_backward_is_deterministic(dev, ws, shift, B, H, W, d, heads):
    qkv, table, dout = _inputs(ws, shift, B, H, W, d, heads)
    a = _engine(dev, qkv, table, dout, ws, shift, B, H, W, heads)
    b = _engine(dev, qkv, table, dout, ws, shift, B, H, W, heads)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("ws", [32, 64])
def test_masked_keys_do_not_reach_a_query(dev, ws):
    """Shifted image, last window (four mask regions).  The k / v rows of two tokens that lie in other mask regions than the
    chosen query are swapped: that query's dq row must not move.  The kernel keeps the exp(-100) terms the existing kernels keep
    (a masked score is the real one minus 100, its probability about 4e-44 of the row's largest), so the bar is 1e-30 absolute,
    not equality."""
    shift, H, W, d, heads = ws // 2, 2 * ws, 2 * ws, 60, 2
    qkv, table, dout = _inputs(ws, shift, 1, H, W, d, heads)

    def token(r, c):     # (row, column) of the SHIFTED image -> token of the unshifted one
        return ((r + shift) % H) * W + (c + shift) % W
    # last window: rows / columns ws .. 2 ws - 1; the mask cuts it at 2 ws - shift
    q = token(ws + 1, ws + 1)                            # region (1, 1)
    m1, m2 = token(2 * ws - 3, 2 * ws - 2), token(2 * ws - 5, ws + 2)      # regions (2, 2) and (2, 1)
    a, _ = _engine(dev, qkv, table, dout, ws, shift, 1, H, W, heads)
    swapped = qkv.clone()
    swapped[m1, d:], swapped[m2, d:] = qkv[m2, d:], qkv[m1, d:]
    b, _ = _engine(dev, swapped, table, dout, ws, shift, 1, H, W, heads)
    diff = float((a[q, :d] - b[q, :d]).abs().max())
    moved = float((a[m1, d:] - b[m1, d:]).abs().max())
    print(f"ws={ws}: dq row of the query moved by {diff:.3e}; dk | dv rows of a swapped token by {moved:.3e}")
    assert float(a[q, :d].abs().max()) > 0 and moved > 0       # the swap did change something
    assert diff <= 1e-30


@pytest.mark.parametrize("ws", [20, 33, 63])
def test_other_window_sizes_are_an_error_status(dev, ws):
    from srad_amd import ops
    d, heads = 60, 2
    qkv, table, dout = _inputs(ws, 0, 1, ws, ws, d, heads)
    with pytest.raises(RuntimeError, match="window sizes 1 .. 16, 32 and 64"):
        ops.window_attention_bwd(qkv.to(dev), dout.to(dev), table.to(dev), 1, ws, ws, ws, 0, heads)
