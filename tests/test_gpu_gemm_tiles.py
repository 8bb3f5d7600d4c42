"""GPU: the tiled GEMM (csrc/kernels_gemm.hip) at every tile shape, K-stage depth and template variant its launcher can
pick, against the fp64 reference of tests/gemm_ref.py with a derived bound for every single output element.

Every case first asks ops.gemm_plan which kernel the call takes and asserts the family, tile, CPS and variant the case was
built for: a retune of the selection thresholds then fails here instead of quietly turning these into 32x32 tests.  The
output buffer is wider and longer than the result and pre-filled with NaN, the padding columns of x and of the residual hold
NaN as well: the checker wants every defined element finite and inside its bound and every other element untouched.

The largest |err| / bound seen per precision is printed when the module finishes (pytest -s)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu

_WORST = {}
_DEVICE_ERROR = []


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield torch.device("cuda:0")
    if _WORST:
        print("\nlargest |err| / bound per precision: " + ", ".join(f"{k} {v[0]:.3f} ({v[1]})" for k, v in sorted(_WORST.items())))


def _kwargs(c, t, dev):
    kw = dict(precision=c.prec, act=c.act, slope=c.slope, alpha=c.alpha, out_offset=c.out_offset, pixel_shuffle=c.ps)
    if c.ntaps == 9:
        kw.update(B=c.B, H=c.H, W=c.W, stride=c.stride)
    if c.ln:
        kw["ln"] = (t["g"].to(dev), t["b"].to(dev))
    if c.residual:
        kw["residual"] = t["r"].to(dev)
    return kw


def _launch(c, t, dev, out=None, check_plan=True):
    """Plan assertion, then the launch into a NaN-filled buffer.  A device error ends the module: nothing more is launched on
    a card that may have faulted."""
    from srad_amd import ops
    if _DEVICE_ERROR:
        pytest.exit(f"stopped after a device error in {_DEVICE_ERROR[0]}", returncode=3)
    Ho, Wo, xrows, ldx, ldr, ldy, orows = G.geometry(c)
    x = t["x"].to(dev)[:, :c.Cin]
    w, bias = t["w"].to(dev), t["bias"].to(dev)
    kw = _kwargs(c, t, dev)
    if out is None:
        out = torch.full((orows, ldy), float("nan"), device=dev)
    if check_plan:
        p = ops.gemm_plan(x, w, bias, out=out, **kw)
        assert p.family == "tiled" and G.Plan(*p[1:7]) == c.plan, f"{c.name}: built for {c.plan}, the launcher plans {p}"
        bm, bn = c.plan.BM, c.plan.BN
        assert p.grid == ((c.N + bn - 1) // bn, (c.M + bm - 1) // bm) and p.launches == 1
    try:
        ops.gemm(x, w, bias, out=out, **kw)
        torch.cuda.synchronize()
    except RuntimeError:
        _DEVICE_ERROR.append(c.name)
        raise
    return out


def _run(c, dev):
    t = G.make_inputs(c)
    out = _launch(c, t, dev)
    ratio = G.check(c, out, G.reference(c, t, device=dev))
    print(f"{c.name}: |err| / bound {ratio:.4f}")
    if ratio > _WORST.get(c.prec, (0.0, ""))[0]:
        _WORST[c.prec] = (ratio, c.name)


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("c", G.linear_cases(), ids=_ids(G.linear_cases()))
def test_linear_tiles(dev, c):
    """Every tile x precision x Cin in {36, 180} (Cp 64 / 192: zero-filled K padding, a partial last K stage under CPS 4 and 8)
    x epilogue (plain, GELU, LeakyReLU * alpha + residual with ldr != N, offset store), and 17 K chunks at 64x64."""
    _run(c, dev)


@pytest.mark.parametrize("c", G.ln_cases(), ids=_ids(G.ln_cases()))
def test_layernorm_prologue(dev, c):
    """The fused LayerNorm at every tile it can take, Cin 180 and 320 (the whole resident K)."""
    _run(c, dev)


@pytest.mark.parametrize("c", G.conv_cases(), ids=_ids(G.conv_cases()))
def test_conv3x3_tiles(dev, c):
    """The 3x3 gather at every tile, at image sizes with no friendly factor; the 80-channel conv kernel's real fall-back (width
    no multiple of 32 -> 128x80, CPS 4); stride 2 with odd input sizes; PixelShuffle(2) at 64x64 and at a 128-row tile."""
    _run(c, dev)


@pytest.mark.parametrize("prec", G.PRECS)
def test_layernorm_dispatch_edges(dev, prec):
    """N <= 32 at a row count that would give a 128-row tile stays on 32x32 with the LayerNorm prologue; 324 channels are
    refused with an error status, before anything is launched."""
    from srad_amd import ops
    M, N = G.M128, 20
    x = torch.zeros(M, 192, device=dev)[:, :180]
    w, b = torch.zeros(N, 180, device=dev), torch.zeros(N, device=dev)
    ln = (torch.ones(180, device=dev), torch.zeros(180, device=dev))
    assert ops.gemm_plan(x, w, b, precision=prec)[:3] == ("tiled", 128, 32)
    p = ops.gemm_plan(x, w, b, ln=ln, precision=prec)
    assert (p.family, p.BM, p.BN, p.LN) == ("tiled", 32, 32, True), p
    x = torch.zeros(77, 336, device=dev)[:, :324]
    w = torch.zeros(N, 324, device=dev)
    ln = (torch.ones(324, device=dev), torch.zeros(324, device=dev))
    out = torch.full((77, N), float("nan"), device=dev)
    with pytest.raises(RuntimeError, match="up to 320 channels"):
        ops.gemm_plan(x, w, b, ln=ln, precision=prec)
    with pytest.raises(RuntimeError, match="up to 320 channels"):
        ops.gemm(x, w, b, ln=ln, out=out, precision=prec)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize("c", G.determinism_cases(), ids=_ids(G.determinism_cases()))
def test_two_launches_are_bit_equal(dev, c):
    t = G.make_inputs(c)
    a = _launch(c, t, dev)
    b = _launch(c, t, dev, check_plan=False)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert G.check(c, a, G.reference(c, t, device=dev)) <= 1.0
