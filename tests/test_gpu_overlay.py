"""GPU: ops.overlay_rgb (srad_overlay_rgb, csrc/kernels_overlay.hip) against the numpy index loop of tests/overlay_ref.py with
torch.equal: gray and colour sources, a random table, contour radius 0, 1 and 2, masks that touch every border, a one-pixel
mask, a NaN pixel, values at and above the 255 level, negative values, more than one workgroup with a width that is no
multiple of anything.  Then a given ``out`` buffer and the refusals."""
import numpy as np
import pytest
import torch

from tests.overlay_ref import overlay_ref

pytestmark = pytest.mark.gpu

CASES = [((2, 5, 7), 1), ((1, 33, 70), 3), ((1, 64, 65), 1)]            # (n, H, W), source channels
SCALE = np.float32(255.0 / 0.9)                                         # map values above 0.9 reach the 255 level
COLOUR = (250, 3, 77)


def _inputs(shape, Cs, seed):
    n, H, W = shape
    rng = np.random.RandomState(seed)
    src = rng.randint(0, 256, (n, H, W, Cs)).astype(np.uint8)
    maps = rng.uniform(-0.1, 1.0, shape).astype(np.float32)
    maps[0, 1, 2] = np.nan
    maps[0, 2, 3] = np.float32(255.0) / SCALE                           # at the 255 level, within a rounding
    maps[0, 3, 1] = 0.9000001
    maps[0, 0, 4] = 7.5                                                 # far above
    maps[0, 4, 5] = np.inf
    maps[0, 4, 0] = 0.0
    masks = np.zeros(shape, dtype=np.uint8)
    masks[0, :3, :4] = 1                                                # touches the top and the left border
    masks[0, 2, 5] = 1                                                  # one pixel
    if H > 20:
        masks[0, 8:20, 10:30] = 1                                       # a block with an interior at radius 1 and 2 ...
        masks[0, 12, 15] = 0                                            # ... and a one-pixel hole in it
        masks[0, 25:, :] = rng.randint(0, 2, (H - 25, W))               # noise down to the bottom border
    masks[0, H - 1:, W - 2:] = 255                                      # the bottom and the right border; any nonzero value is set
    if n > 1:
        masks[1] = 1                                                    # a whole image set: only its border is contour
    lut = rng.randint(0, 256, (256, 4)).astype(np.uint8)
    lut[0, 3], lut[255, 3] = 0, 255                                     # both ends of the alpha range are met
    return src, maps, masks, lut


@pytest.fixture(scope="module")
def cases():
    return [_inputs(shape, Cs, seed=5 + k) for k, (shape, Cs) in enumerate(CASES)]


@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("k", range(len(CASES)))
def test_overlay_equals_the_index_loop(cases, k, radius):
    from srad_amd import ops
    src, maps, masks, lut = cases[k]
    ref = overlay_ref(src, maps, masks, lut, SCALE, radius, COLOUR)
    got = ops.overlay_rgb(*(torch.from_numpy(a).cuda() for a in (src, maps, masks, lut)), SCALE, radius, COLOUR)
    assert got.dtype == torch.uint8 and tuple(got.shape) == maps.shape + (3,)
    differ = int((got.cpu() != torch.from_numpy(ref)).any(-1).sum())
    print(f"{CASES[k]} radius {radius}: {differ} of {maps.size} pixels differ from the index loop")
    assert torch.equal(got.cpu(), torch.from_numpy(ref))
    contour = (ref == COLOUR).all(-1) & (masks != 0)
    assert (contour.sum() > 0) == (radius > 0) and not (contour & (masks == 0)).any()
    if radius:
        assert contour[0, 2, 5] and contour[0, 0, 0] and contour[0, -1, -1]      # the one-pixel mask and two corners


def test_given_out_buffer_and_defaults(cases):
    from srad_amd import ops
    src, maps, masks, lut = cases[0]
    dev = [torch.from_numpy(a).cuda() for a in (src, maps, masks, lut)]
    out = torch.full(maps.shape + (3,), 9, dtype=torch.uint8, device="cuda")
    assert ops.overlay_rgb(*dev, SCALE, out=out) is out                    # radius 1, white
    assert torch.equal(out.cpu(), torch.from_numpy(overlay_ref(src, maps, masks, lut, SCALE, 1, (255, 255, 255))))


def test_refusals(cases):
    from srad_amd import ops
    src, maps, masks, lut = (torch.from_numpy(a).cuda() for a in cases[0])
    with pytest.raises(ValueError, match="source"):
        ops.overlay_rgb(src.float(), maps, masks, lut, 1.0)
    with pytest.raises(ValueError, match="source"):
        ops.overlay_rgb(src.expand(-1, -1, -1, 2), maps, masks, lut, 1.0)
    with pytest.raises(ValueError, match="maps must be"):
        ops.overlay_rgb(src, maps.double(), masks, lut, 1.0)
    with pytest.raises(ValueError, match="masks must be"):
        ops.overlay_rgb(src, maps, masks[:, :, :-1], lut, 1.0)
    with pytest.raises(ValueError, match="lut must be"):
        ops.overlay_rgb(src, maps, masks, lut[:, :3], 1.0)
    with pytest.raises(ValueError, match="out must be"):
        ops.overlay_rgb(src, maps, masks, lut, 1.0, out=torch.zeros(2, 5, 7, 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.overlay_rgb(src, maps.cpu(), masks, lut, 1.0)
    with pytest.raises(RuntimeError, match="contour radius"):
        ops.overlay_rgb(src, maps, masks, lut, 1.0, 5)
    with pytest.raises(RuntimeError, match="contour colour"):
        ops.overlay_rgb(src, maps, masks, lut, 1.0, 1, (0, 300, 0))
    with pytest.raises(ValueError, match="contour"):
        ops.overlay_rgb(src, maps, masks, lut, 1.0, 1.5)
