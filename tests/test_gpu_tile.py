"""GPU: the two kernels of tiled inference (DESIGN.md "Tiled inference") against the numpy restatements of
tests/test_tile_host.py (checked there against a literal per-pixel loop).  Every comparison is bit for bit: gather is a copy,
and the blend's sums, products and division are defined operation by operation."""
import numpy as np
import pytest
import torch

from tests.test_tile_host import axis_rule, blend_ref, gather_ref

pytestmark = pytest.mark.gpu

# (B, C, h, w, T, O, g): odd sizes with padding; one tile, no pad; image smaller than the tile; the pad longer than the image
# (periodic reflection); stride 1 with up to 64 tiles per pixel
CASES = [(2, 1, 37, 50, 16, 4, 8), (1, 3, 16, 16, 16, 0, 8), (1, 3, 5, 7, 8, 3, 4), (1, 1, 2, 3, 8, 2, 8), (2, 3, 40, 24, 8, 7, 1)]
SCALES = (1, 2, 4)
MODES = ("mean", "feather")

_cache = {}


def _image(case):
    if ("x", case) not in _cache:
        _cache[("x", case)] = np.random.RandomState(11).randn(*case[:4]).astype(np.float32)
    return _cache[("x", case)]


def _tile_data(case, s):
    """Random tile outputs, independent of any network, and their blends by the restatement (computed once per case)."""
    key = ("y", case, s)
    if key not in _cache:
        B, C, h, w, T, O, g = case
        _, ty, _, oy = axis_rule(h, T, O, g)
        _, tx, _, ox = axis_rule(w, T, O, g)
        y = np.random.RandomState(12 + s).randn(B * len(oy) * len(ox), C, ty * s, tx * s).astype(np.float32)
        _cache[key] = (y, {m: blend_ref(y, B, h, w, T, O, g, s, m) for m in MODES})
    return _cache[key]


def _bits(a, b):
    """torch.equal on the bit patterns (so -0.0 and NaN payloads count)."""
    return torch.equal(a.cpu().view(torch.int32), torch.from_numpy(np.ascontiguousarray(b)).view(torch.int32))


def _off_boundary(t, floats=1):
    """The same values in a tensor whose storage starts `floats` floats off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device="cuda")
    off = (-(buf.data_ptr() // 4)) % 4 + floats
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * floats and v.is_contiguous()
    return v


@pytest.mark.parametrize("case", CASES)
def test_gather_is_the_restatement(case):
    from srad_amd import ops
    B, C, h, w, T, O, g = case
    x = _image(case)
    want = gather_ref(x, T, O, g)
    got = ops.tile_gather(torch.from_numpy(x).cuda(), T, O, g)
    assert tuple(got.shape) == want.shape
    assert _bits(got, want)
    assert _bits(ops.tile_gather(_off_boundary(torch.from_numpy(x).cuda()), T, O, g), want)


def test_gather_vector_path_and_its_edges():
    """Shapes that take the float4 instance (w, tile extent, stride and last origin multiples of 4), with a reflected quad at
    the right edge, and the neighbouring shapes that fall to the scalar one."""
    from srad_amd import ops
    for (B, C, h, w, T, O, g) in ((2, 2, 21, 36, 16, 4, 8), (1, 1, 8, 44, 16, 8, 16), (1, 1, 9, 38, 16, 4, 8), (1, 2, 12, 40, 16, 3, 8)):
        x = np.random.RandomState(h + w).randn(B, C, h, w).astype(np.float32)
        assert _bits(ops.tile_gather(torch.from_numpy(x).cuda(), T, O, g), gather_ref(x, T, O, g)), (h, w, T, O, g)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("case", CASES)
def test_blend_is_the_restatement(case, s, mode):
    from srad_amd import ops
    B, C, h, w, T, O, g = case
    y, want = _tile_data(case, s)
    got = ops.tile_blend(torch.from_numpy(y).cuda(), h, w, T, O, g, s, mode)
    assert tuple(got.shape) == (B, C, h * s, w * s)
    assert _bits(got, want[mode]), float(np.abs(got.cpu().numpy() - want[mode]).max())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [CASES[0], CASES[4]])
def test_blend_off_a_16_byte_boundary(case, mode):
    from srad_amd import ops
    B, C, h, w, T, O, g = case
    y, want = _tile_data(case, 4)                             # scale 4: the float4 instance wherever the pointers allow it
    yd = torch.from_numpy(y).cuda()
    assert _bits(ops.tile_blend(_off_boundary(yd), h, w, T, O, g, 4, mode), want[mode])
    out = _off_boundary(torch.empty(B, C, h * 4, w * 4, device="cuda"), 3)
    assert ops.tile_blend(yd, h, w, T, O, g, 4, mode, out=out) is out
    assert _bits(out, want[mode])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_blend_of_gather_returns_the_input(case, mode):
    """All covering values of a pixel are equal, and small integers keep every sum exact (weights up to 8^2, up to 64 tiles,
    |x| <= 64: below 2^24), so both modes return the value."""
    from srad_amd import ops
    B, C, h, w, T, O, g = case
    x = torch.randint(-64, 65, case[:4], generator=torch.Generator().manual_seed(13)).float().cuda()
    assert torch.equal(ops.tile_blend(ops.tile_gather(x, T, O, g), h, w, T, O, g, 1, mode), x)
    if h % T == 0 and w % T == 0:                             # overlap 0 and no tile snapped: a copy of any values
        xr = torch.from_numpy(_image(case)).cuda()
        assert torch.equal(ops.tile_blend(ops.tile_gather(xr, T, 0, g), h, w, T, 0, g, 1, mode), xr)


def test_single_cover_and_zero_overlap_are_copies():
    from srad_amd import ops
    y = torch.randn(6, 2, 16, 16, generator=torch.Generator().manual_seed(14)).cuda()       # 2 x 3 tiles of 8 at scale 2, no overlap, no snap
    want = y.view(1, 2, 3, 2, 16, 16).permute(0, 3, 1, 4, 2, 5).reshape(1, 2, 32, 48)
    for mode in MODES:
        assert torch.equal(ops.tile_blend(y, 16, 24, 8, 0, 1, 2, mode), want)
    # overlap 3: the pixels that one tile covers are that tile's values in both modes
    y = torch.randn(2, 1, 8, 8, generator=torch.Generator().manual_seed(15)).cuda()         # 1 x 2 tiles of 8, origins 0 and 5
    for mode in MODES:
        out = ops.tile_blend(y, 8, 13, 8, 3, 1, 1, mode)
        assert torch.equal(out[0, 0, :, :5], y[0, 0, :, :5]) and torch.equal(out[0, 0, :, 8:], y[1, 0, :, 3:])
        assert not torch.equal(out[0, 0, :, 5:8], y[0, 0, :, 5:])


def test_argument_errors():
    from srad_amd import _lib as L
    from srad_amd import ops
    x = torch.zeros(1, 1, 8, 8, device="cuda")
    with pytest.raises(ValueError, match="4-d fp32"):
        ops.tile_gather(x[0], 8)
    with pytest.raises(ValueError, match="4-d fp32"):
        ops.tile_gather(x.double(), 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.tile_gather(x.cpu(), 8)
    with pytest.raises(ValueError, match="granule"):
        ops.tile_gather(x, 6, 0, 4)
    with pytest.raises(ValueError, match="overlap"):
        ops.tile_gather(x, 8, 8)
    with pytest.raises(ValueError, match="not a batch of"):
        ops.tile_blend(torch.zeros(3, 1, 8, 8, device="cuda"), 8, 12, 8, 2, 1, 1)          # 2 tiles per image
    with pytest.raises(ValueError, match="not a batch of"):
        ops.tile_blend(torch.zeros(2, 1, 8, 9, device="cuda"), 8, 12, 8, 2, 1, 1)
    with pytest.raises(ValueError, match="4094"):
        ops.tile_blend(torch.zeros(1, 1, 8, 8, device="cuda"), 2, 2, 4096, 2048, 1, 2)
    with pytest.raises(ValueError, match="out must be"):
        ops.tile_blend(x, 8, 8, 8, 0, 1, 1, out=torch.zeros(1, 1, 8, 9, device="cuda"))
    # the library's own checks: its error code and srad_last_error
    lib, s = L.lib(), L.current_stream_ptr()
    y = torch.zeros(2, 1, 8, 8, device="cuda")
    assert lib.srad_tile_blend(L.dptr(y), 1, 1, 8, 12, 8, 2, 1, 1, 2, L.dptr(x), s) == 1 and b"unknown mode" in lib.srad_last_error()
    assert lib.srad_tile_blend(None, 1, 1, 8, 12, 8, 2, 1, 1, 0, L.dptr(x), s) == 1 and b"null" in lib.srad_last_error()
    assert lib.srad_tile_blend(L.dptr(y), 0, 1, 8, 12, 8, 2, 1, 1, 0, L.dptr(x), s) == 1 and b"positive" in lib.srad_last_error()
    assert lib.srad_tile_blend(L.dptr(y), 1, 1, 8, 12, 8, 2, 1, 1, 0, L.dptr(y[1:]), s) == 1 and b"overlaps" in lib.srad_last_error()
    assert lib.srad_tile_gather(L.dptr(x), 1, 1, 8, 8, 8, 0, 1, L.dptr(x), s) == 1 and b"overlaps" in lib.srad_last_error()
    assert lib.srad_tile_gather(L.dptr(x), 1, 1, 8, 8, 0, 0, 1, L.dptr(y), s) == 1 and b"tile must be" in lib.srad_last_error()
    torch.cuda.synchronize()
