"""GPU: ops.resize_f32 (srad_resize_f32, csrc/kernels_resize.hip) against Pillow's mode-F ``Image.resize``, compared as uint32
views - every bit equal, no tolerance.  Three maps per call, with negative values and values of magnitude 1e-6: bilinear at an
up-scale, a down-scale, the horizontal pass alone, the copy, and an up-scale of more than one workgroup per pass with odd sizes;
bicubic and lanczos at one up-scale and one down-scale each.  Then given ``out`` / ``tmp`` buffers, a constant map, and the
refusals that need real tensors."""
import numpy as np
import pytest
import torch

from tests.test_resample_f_host import SHAPES, bits, maps_f, pil_resize_f

pytestmark = pytest.mark.gpu

N = 3


@pytest.fixture(scope="module")
def stacks():
    """{(H, W): float32 [N,H,W]}: the inputs of every test here, made once and never changed."""
    return {src: np.stack([maps_f(src, seed=11 * k + src[1]) for k in range(N)]) for src, _ in SHAPES}


def _reference(x, size, name):
    return np.stack([pil_resize_f(a, size[0], size[1], name) for a in x])


def _check(x, size, name, **kw):
    from srad_amd import ops
    got = ops.resize_f32(torch.from_numpy(x).cuda(), size, name, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (x.shape[0],) + tuple(size) and got.is_contiguous()
    got, ref = got.cpu().numpy(), _reference(x, size, name)
    diff = bits(got) != bits(ref)
    print(f"{name} {x.shape[1:]} -> {size}: {int(diff.sum())} of {diff.size} values differ from Pillow")
    assert np.array_equal(bits(got), bits(ref)), (name, x.shape, size, int(diff.sum()))
    return got


@pytest.mark.parametrize("src,size", SHAPES)
def test_bilinear_equals_pil(stacks, src, size):
    _check(stacks[src], size, "bilinear")


@pytest.mark.parametrize("name", ["bicubic", "lanczos"])
@pytest.mark.parametrize("src,size", [SHAPES[0], SHAPES[1]])            # one up-scale, one down-scale
def test_bicubic_and_lanczos_equal_pil(stacks, name, src, size):
    _check(stacks[src], size, name)


def test_given_buffers(stacks):
    from srad_amd import ops
    (H, W), (h, w) = SHAPES[0]
    x = torch.from_numpy(stacks[(H, W)]).cuda()
    ref = _reference(stacks[(H, W)], (h, w), "bilinear")
    out = torch.full((N, h, w), 9.0, dtype=torch.float32, device="cuda")
    tmp = torch.full((N, H, w), 9.0, dtype=torch.float32, device="cuda")
    assert ops.resize_f32(x, (h, w), out=out, tmp=tmp) is out               # bilinear is the default
    assert np.array_equal(bits(out.cpu().numpy()), bits(ref))
    tmp_ref = _reference(stacks[(H, W)], (H, w), "bilinear")                 # the horizontal pass alone, rounded to float32
    assert np.array_equal(bits(tmp.cpu().numpy()), bits(tmp_ref))
    again = ops.resize_f32(x, (h, w), "bilinear", out=out)
    assert again is out and np.array_equal(bits(out.cpu().numpy()), bits(ref))
    assert ops.resample_table_f(W, w, "bilinear", x.device)[0] is ops.resample_table_f(W, w, "bilinear", x.device)[0]      # cached
    for bad, what in ((torch.zeros(N, h, w + 1, device="cuda"), "out"), (torch.zeros(N, h, w, dtype=torch.float64, device="cuda"), "out"),
                      (torch.zeros(N, h, w), "out"), (torch.zeros(N, w, h, device="cuda").transpose(1, 2), "out")):
        with pytest.raises(ValueError, match=f"{what} must be"):
            ops.resize_f32(x, (h, w), out=bad)
    with pytest.raises(ValueError, match="tmp must be"):
        ops.resize_f32(x, (h, w), tmp=torch.zeros(N, h, w, device="cuda"))


def test_constant_map_stays_constant():
    from srad_amd import ops
    for value in (0.3, 1.0, -2.5e-6):
        x = torch.full((N, 16, 24), value, dtype=torch.float32, device="cuda")
        for size in ((40, 57), (5, 7), (16, 57), (33, 24)):
            got = ops.resize_f32(x, size, "bilinear")
            assert torch.equal(got, torch.full_like(got, value)), (value, size)


def test_refusals(stacks):
    from srad_amd import ops
    x = torch.from_numpy(stacks[(16, 24)]).cuda()
    with pytest.raises(ValueError, match="not contiguous"):
        ops.resize_f32(x.transpose(1, 2), (5, 7))
    with pytest.raises(ValueError, match="not contiguous"):
        ops.resize_f32(x[:, :, ::2], (5, 7))
    for wrong in (x.double(), x.half(), (x * 100).to(torch.uint8)):
        with pytest.raises(ValueError, match="float32"):
            ops.resize_f32(wrong, (5, 7))
    with pytest.raises(ValueError, match="float32"):
        ops.resize_f32(x[0], (5, 7))                                        # [H,W]: not a stack
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.resize_f32(x.cpu(), (5, 7))
    with pytest.raises(ValueError, match="resample filter"):
        ops.resize_f32(x, (5, 7), "nearest")
    with pytest.raises(ValueError, match="every size must be >= 1"):
        ops.resize_f32(x, (0, 7))
    flat = torch.zeros(4096, dtype=torch.float32, device="cuda")
    src = flat[:N * 16 * 24].view(N, 16, 24)
    with pytest.raises(RuntimeError, match="dst overlaps src"):
        ops.resize_f32(src, (5, 7), out=flat[1000:1000 + N * 5 * 7].view(N, 5, 7))
    with pytest.raises(RuntimeError, match="tmp overlaps src or dst"):
        ops.resize_f32(src, (5, 7), tmp=flat[1100:1100 + N * 16 * 7].view(N, 16, 7))
