"""GPU: ops.resize_u8 (srad_resize_u8, csrc/kernels_resize.hip) against PIL.Image.resize, every byte equal, for both filters on
random and 0/255 images: both passes, one pass skipped, the copy, upscaling, 49 taps, one to four channels, a source that does
not start on a 16-byte boundary (the staging loop's bytewise head), more rows than one workgroup takes with a remainder, and a
row too long for the LDS staging (the other instance of the horizontal kernel).  Then the refusals that need real tensors."""
import numpy as np
import pytest
import torch

from tests.test_resample_host import images, pil_resize

pytestmark = pytest.mark.gpu

SHAPES = [((3, 37, 53, 1), (12, 17)), ((2, 100, 75, 3), (33, 20)), ((1, 64, 64, 3), (8, 8)), ((1, 40, 40, 3), (57, 57)),
          ((2, 64, 48, 1), (16, 48)), ((1, 32, 32, 1), (32, 32)), ((1, 5, 5, 4), (1, 1)),
          ((1, 64, 48, 2), (64, 19)),                        # the vertical pass skipped
          ((1, 3, 4200, 4), (2, 33))]                        # rows of 16800 bytes: read from global memory, not staged


def _reference(x, size, name):
    return np.stack([pil_resize(img, size[0], size[1], name).reshape(size[0], size[1], x.shape[3]) for img in x])


@pytest.mark.parametrize("name", ["lanczos", "bicubic"])
@pytest.mark.parametrize("kind", ["random", "binary"])
def test_resize_equals_pil(name, kind):
    from srad_amd import ops
    for shape, size in SHAPES:
        x = np.stack([images(kind, shape[1:], seed=7 * k + shape[2]) for k in range(shape[0])])
        got = ops.resize_u8(torch.from_numpy(x).cuda(), size, name)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (shape[0],) + size + (shape[3],)
        ref = _reference(x, size, name)
        assert np.array_equal(got.cpu().numpy(), ref), (shape, size, int(np.abs(got.cpu().numpy().astype(int) - ref).max()))


def test_unaligned_source_and_given_buffers():
    from srad_amd import ops
    shape, size = (2, 37, 53, 3), (12, 17)
    x = np.stack([images("random", shape[1:], seed=k) for k in range(shape[0])])
    ref = _reference(x, size, "lanczos")
    flat = torch.zeros(x.size + 64, dtype=torch.uint8, device="cuda")
    for off in (1, 7, 16, 21):                               # the first row's address modulo 16
        flat[off:off + x.size] = torch.from_numpy(x).cuda().reshape(-1)
        view = flat[off:off + x.size].view(shape)
        assert view.data_ptr() % 16 == off % 16
        out = torch.full((shape[0],) + size + (3,), 9, dtype=torch.uint8, device="cuda")
        tmp = torch.empty(shape[0], shape[1], size[1], 3, dtype=torch.uint8, device="cuda")
        assert ops.resize_u8(view, size, "lanczos", out=out, tmp=tmp) is out
        assert np.array_equal(out.cpu().numpy(), ref), off


def test_refusals():
    from srad_amd import _lib as L, ops
    x = torch.zeros(2, 16, 12, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="uint8"):
        ops.resize_u8(x.float(), (4, 6))
    with pytest.raises(ValueError, match="resample filter"):
        ops.resize_u8(x, (4, 6), "nearest")
    with pytest.raises(ValueError, match="out must be"):
        ops.resize_u8(x, (4, 6), out=torch.zeros(2, 4, 6, 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.resize_u8(x.cpu(), (4, 6))
    with pytest.raises(RuntimeError, match="channels"):
        ops.resize_u8(torch.zeros(1, 8, 8, 5, dtype=torch.uint8, device="cuda"), (4, 4))
    # overlap: dst inside src, tmp inside src, tmp on dst
    flat = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    src = flat[:2 * 16 * 12 * 3].view(2, 16, 12, 3)
    with pytest.raises(RuntimeError, match="dst overlaps src"):
        ops.resize_u8(src, (4, 6), out=flat[1000:1000 + 2 * 4 * 6 * 3].view(2, 4, 6, 3))
    with pytest.raises(RuntimeError, match="tmp overlaps src or dst"):
        ops.resize_u8(src, (4, 6), tmp=flat[1100:1100 + 2 * 16 * 6 * 3].view(2, 16, 6, 3))
    both = torch.zeros(2048, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="tmp overlaps src or dst"):
        ops.resize_u8(src, (4, 6), out=both[:144].view(2, 4, 6, 3), tmp=both[143:143 + 576].view(2, 16, 6, 3))
    # bounds: a table whose host bounds leave the source is refused before anything is launched
    table, keep = ops.resample_table(12, 6, "lanczos", x.device)
    bad = keep[0].copy()
    bad[5, 1] += 1
    forged = L.ResampleTable(12, 6, table.ksize, bad.ctypes.data, table.dev_bounds, table.dev_coeffs)
    ytable = ops.resample_table(16, 4, "lanczos", x.device)[0]
    out = torch.full((2, 4, 6, 3), 9, dtype=torch.uint8, device="cuda")
    tmp = torch.empty(2, 16, 6, 3, dtype=torch.uint8, device="cuda")
    rc = L.lib().srad_resize_u8(L.dptr(x), 2, 16, 12, 3, L.dptr(out), 4, 6, forged, ytable, L.dptr(tmp), L.current_stream_ptr())
    assert rc == 1 and b"the x table's bounds leave the source" in L.lib().srad_last_error()
    torch.cuda.synchronize()
    assert int(out.min()) == 9 and int(out.max()) == 9        # nothing was written
    # the cache hands the same table out again
    assert ops.resample_table(12, 6, "lanczos", x.device)[0] is table
