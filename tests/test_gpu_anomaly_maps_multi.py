"""GPU: multi-scale anomaly maps (srad_anomaly_maps_multi: the maps 1 - SSIM map of a list of window sizes reduced per pixel by
one kernel, mean or max).  Bit for bit against the composition it replaces (``anomaly_maps`` per size, torch fp32 ops in the
defined order), against the per-pixel map oracle accumulated in numpy float32 (bars below), against the reference fixtures by
linearity of the mean, and through properties that need no reference."""
import numpy as np
import pytest
import torch

from oracle import scorer_ref as O
from tests.test_gpu_anomaly_maps import blob_masks, map_oracle

pytestmark = pytest.mark.gpu

SHAPES = [(128, 1), (64, 3), (33, 1)]
TWENTY = list(range(3, 42, 2))                               # 20 sizes: two launches (16 + 4)
SEVENTEEN = [3] * 16 + [11]                                  # a second launch of exactly one size, continued from the stored accumulator


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _compose(sr, hr, sizes, reduce):
    """The path the fused kernel replaces: one ``anomaly_maps`` per size, accumulated by torch in fp32 in list order."""
    from srad_amd import metrics as M
    acc = M.anomaly_maps(sr, hr, sizes[0])
    for ws in sizes[1:]:
        m = M.anomaly_maps(sr, hr, ws)
        acc = torch.maximum(acc, m) if reduce == "max" else acc + m
    if reduce == "mean":
        acc = acc * torch.tensor(np.float32(1.0 / len(sizes)), device=acc.device)
    return acc


def _lists(size):
    from srad_amd import metrics as M
    return [[11], [3, 11, 21], [21, 3, 11], M.sweep_window_sizes(size), TWENTY, SEVENTEEN]


@pytest.mark.parametrize("reduce", ["mean", "max"])
@pytest.mark.parametrize("size,ch", SHAPES)
def test_bit_identical_to_the_composition(size, ch, reduce):
    from srad_amd import metrics as M
    assert len(TWENTY) == 20 and TWENTY[-1] == 41
    _, sr, hr = O.synth_pairs(2, 3, size, ch, seed=4)
    sr, hr = _dev(np.stack(sr)), _dev(np.stack(hr))
    got = {}
    for sizes in _lists(size):
        multi = M.anomaly_maps_multi(sr, hr, sizes, reduce)
        assert multi.dtype == torch.float32 and tuple(multi.shape) == (5, size, size)
        assert torch.equal(multi, _compose(sr, hr, sizes, reduce)), (size, ch, reduce, sizes)
        got[tuple(sizes)] = multi
    assert torch.equal(got[(11,)], M.anomaly_maps(sr, hr, 11))
    if reduce == "max":                                      # order-independent; the mean may differ in the last bit
        assert torch.equal(got[(3, 11, 21)], got[(21, 3, 11)])
    else:                                                    # each order: (K - 1) 2^-23 from its additions, 2^-24 from the multiply
        assert float((got[(3, 11, 21)] - got[(21, 3, 11)]).abs().max()) <= 5 * 2.0 ** -23
    # a size listed twice counts twice
    twice = M.anomaly_maps_multi(sr, hr, [11, 11, 3], reduce)
    assert torch.equal(twice, _compose(sr, hr, [11, 11, 3], reduce))


@pytest.mark.parametrize("H,W,C", [(33, 45, 1), (64, 64, 3)])
def test_a_list_of_one_size_is_the_single_map(H, W, C):
    """The smallest windows and the largest that fits, per-lane instance (33 x 45) and scalar-row instance (64 x 64)."""
    from srad_amd import metrics as M
    from tests.test_gpu_error_maps import random_pairs
    sr, hr = (_dev(a) for a in random_pairs(2, H, W, C, seed=21))
    for ws in (1, 2, 2 * min(H, W) - 1):
        single = M.anomaly_maps(sr, hr, ws)
        for reduce in ("mean", "max"):
            assert torch.equal(M.anomaly_maps_multi(sr, hr, [ws], reduce), single), (H, W, C, ws, reduce)


@pytest.mark.parametrize("reduce", ["mean", "max"])
def test_bit_identical_to_the_composition_1024px(reduce):
    from srad_amd import metrics as M
    g = torch.Generator().manual_seed(8)
    hr = (torch.rand(1, 1024, 1024, 1, generator=g) * 255).to(torch.uint8)
    sr = (hr.int() + torch.randint(-9, 10, hr.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    sr, hr = sr.cuda(), hr.cuda()
    assert torch.equal(M.anomaly_maps_multi(sr, hr, [11, 21, 31], reduce), _compose(sr, hr, [11, 21, 31], reduce))


@pytest.mark.parametrize("reduce", ["mean", "max"])
@pytest.mark.parametrize("size,ch", SHAPES)
def test_parity_with_the_map_oracle(size, ch, reduce):
    """Each scale is within the single map's bars (mean |d| <= 1e-6, max |d| <= 1e-4), and so is a mean or a max of them; the
    two sides may round their K - 1 fp32 additions differently: partial sums are below 2 K, so half an ulp is at most K 2^-23,
    scaled by 1 / K.  Hence mean |d| <= 1e-6 + (K - 1) 2^-23 and max |d| <= 1e-4 + (K - 1) 2^-23."""
    from srad_amd import metrics as M
    _, sr, hr = O.synth_pairs(2, 3, size, ch, seed=4)
    sr, hr = np.stack(sr), np.stack(hr)
    for sizes in ([3, 11, 21], M.sweep_window_sizes(size)):
        K = len(sizes)
        got = M.anomaly_maps_multi(_dev(sr), _dev(hr), sizes, reduce).cpu().numpy()
        want = None
        for ws in sizes:
            m = np.stack([map_oracle(s, h, ws) for s, h in zip(sr, hr)]).astype(np.float32)
            want = m if want is None else (np.maximum(want, m) if reduce == "max" else (want + m).astype(np.float32))
        if reduce == "mean":
            want = (want * np.float32(1.0 / K)).astype(np.float32)
        assert want.dtype == np.float32
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        print(f"map_multi oracle parity {size}px C={ch} {reduce} K={K}: mean |d| {d.mean():.3e}  max |d| {d.max():.3e}")
        slack = (K - 1) * 2.0 ** -23
        assert d.mean() <= 1e-6 + slack and d.max() <= 1e-4 + slack, (size, ch, reduce, sizes, d.mean(), d.max())


@pytest.mark.parametrize("tag", ["gray", "rgb"])
def test_mean_map_means_match_reference_golden(scorer_golden, tag):
    """By linearity the spatial mean of the mean-reduced map over all of the fixture's window sizes is 1 - the mean of the
    reference's image-level SSIMs over those sizes; bar 2e-6, the single map's."""
    from srad_amd import metrics as M
    g = scorer_golden
    sr, hr, wss = g[f"{tag}/sr"], g[f"{tag}/hr"], [int(w) for w in g[f"{tag}/ws"]]
    multi = M.anomaly_maps_multi(_dev(sr), _dev(hr), wss, "mean")
    got = multi.double().mean(dim=(1, 2)).cpu().numpy()
    want = 1.0 - g[f"{tag}/ssim"].astype(np.float64).mean(axis=1)
    assert np.abs(got - want).max() < 2e-6, (tag, np.abs(got - want).max())


@pytest.mark.parametrize("reduce", ["mean", "max"])
def test_arg_max_lies_in_the_planted_blob(reduce):
    """Each bad pair of synth_pairs data: the maximum of the 11 / 21 / 31 map is inside the blob planted in its SR image."""
    from srad_amd import metrics as M
    n_good, n_bad, size = 2, 6, 128
    _, sr, hr = O.synth_pairs(n_good, n_bad, size, 1, seed=6)
    masks = blob_masks(n_good, n_bad, size, 1, seed=6)
    assert not any(m.any() for m in masks[:n_good]) and all(m.any() for m in masks[n_good:])
    maps = M.anomaly_maps_multi(_dev(np.stack(sr)), _dev(np.stack(hr)), [11, 21, 31], reduce).cpu().numpy()
    for k in range(n_good, n_good + n_bad):
        iy, ix = np.unravel_index(np.argmax(maps[k]), maps[k].shape)
        assert masks[k][iy, ix], (reduce, k, iy, ix)


def test_map_is_batch_invariant_across_table_chunks():
    """4096 px pairs: one summed-area table chunk per image, so a batch of two runs as two chunks; the second pair's map is the
    same bits whether it is scored alone or in the batch."""
    from srad_amd import metrics as M
    g = torch.Generator().manual_seed(5)
    hr = (torch.rand(2, 4096, 4096, 1, generator=g) * 255).to(torch.uint8).cuda()
    sr = (hr.int() + torch.randint(-5, 6, hr.shape, generator=g).cuda()).clamp(0, 255).to(torch.uint8)
    for reduce in ("mean", "max"):
        both = M.anomaly_maps_multi(sr, hr, [11, 21], reduce)
        one = M.anomaly_maps_multi(sr[1:].contiguous(), hr[1:].contiguous(), [11, 21], reduce)
        assert torch.equal(both[1], one[0])
        assert not torch.equal(both[0], both[1])


def test_identical_images_give_zero_maps():
    from srad_amd import metrics as M
    _, _, hr = O.synth_pairs(1, 1, 64, 3, seed=2)
    hr = _dev(np.stack(hr))
    for reduce in ("mean", "max"):
        assert float(M.anomaly_maps_multi(hr, hr, [3, 21, 67], reduce).abs().max()) <= 1e-6
        assert float(M.anomaly_maps_multi(hr, hr, TWENTY, reduce).abs().max()) <= 1e-6


def test_invalid_arguments_raise():
    from srad_amd import metrics as M
    x = torch.zeros(1, 33, 40, 1, dtype=torch.uint8, device="cuda")
    for sizes in ([0], [11, 67], [2 * 33, 3], [3] * 17 + [67]):
        with pytest.raises(RuntimeError, match="anomaly_maps_multi"):
            M.anomaly_maps_multi(x, x, sizes)
    with pytest.raises(ValueError, match="empty"):
        M.anomaly_maps_multi(x, x, [])
    for reduce in ("sum", "", None, "MEAN"):
        with pytest.raises(ValueError, match="reduce"):
            M.anomaly_maps_multi(x, x, [3], reduce)
    assert tuple(M.anomaly_maps_multi(x, x, [3, 65]).shape) == (1, 33, 40)       # 65 / 2 = 32 < 33: one reflection
