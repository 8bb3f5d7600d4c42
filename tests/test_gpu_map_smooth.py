"""GPU: Gaussian smoothing of anomaly maps (srad_smooth_maps via metrics.smooth_maps) against tests/golden/map_smooth_golden.npz
(scipy.ndimage.gaussian_filter outputs, written by tests/golden/make_map_smooth_golden.py) and against the generator's numpy
restatement on 1024 x 1024 maps, all bit for bit; batch invariance; the fused per-image maximum.  No scipy here."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_map_smooth_golden", os.path.join(GOLDEN_DIR, "make_map_smooth_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "map_smooth_golden.npz"))


def _bits_equal(got, want):
    """NaN at the same positions, the same bits everywhere else (a NaN's payload is not compared)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def _cases():
    G = _generator()
    return [(name, s) for name, (_, _, _, _, sigmas) in G.CASES.items() for s in sigmas]


@pytest.mark.parametrize("name,sigma", _cases())
def test_smoothing_matches_scipy_golden(golden, name, sigma):
    from srad_amd import metrics as M
    m = golden[f"{name}/maps"]
    want = golden[f"{name}/out_{sigma:g}"]
    src = torch.from_numpy(m).cuda()
    got, mx = M.smooth_maps(src, sigma, with_max=True)
    got = got.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert _bits_equal(got, want), (name, sigma, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    assert _bits_equal(src.cpu().numpy(), m)                                                     # the input is left alone
    mx = mx.cpu().numpy()
    for i in range(m.shape[0]):
        if np.isnan(want[i]).any():
            assert np.isnan(mx[i])
        else:
            assert mx[i] == want[i].max()
    assert _bits_equal(M.smooth_maps(src, sigma).cpu().numpy(), want)                           # without the maximum


@pytest.mark.parametrize("sigma", [4.0, 16.0])
def test_smoothing_1024px_matches_numpy_restatement(sigma):
    from srad_amd import metrics as M
    G = _generator()
    m = G.hashed_maps(2, 1024, 1024, 21)
    m[0, 500:540, 300:700] = 0.0
    want = G.smooth_ref(m, sigma)
    got, mx = M.smooth_maps(torch.from_numpy(m).cuda(), sigma, with_max=True)
    got = got.cpu().numpy()
    assert _bits_equal(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert np.isnan(mx[1].item()) and not np.isnan(mx[0].item()) and mx[0].item() == want[0].max()


def test_batch_invariance_and_repeatability():
    from srad_amd import metrics as M
    G = _generator()
    m = torch.from_numpy(G.hashed_maps(8, 77, 201, 5)).cuda()
    m = torch.nan_to_num(m, nan=0.25)                                    # image 1 of the generator holds a NaN
    for sigma in (1.0, 4.0, 8.0):
        batch, bmax = M.smooth_maps(m, sigma, with_max=True)
        again, amax = M.smooth_maps(m, sigma, with_max=True)
        assert torch.equal(batch.view(torch.int32), again.view(torch.int32)) and torch.equal(bmax, amax)
        for i in (0, 5, 7):
            alone, one_max = M.smooth_maps(m[i:i + 1].clone(), sigma, with_max=True)
            assert torch.equal(alone[0].view(torch.int32), batch[i].view(torch.int32)), (sigma, i)
            assert one_max[0].item() == bmax[i].item()


def test_image_maximum_and_radius_zero(golden):
    from srad_amd import metrics as M
    m = torch.from_numpy(golden["odd_45x63/maps"]).cuda()                # image 1 holds the NaN
    m3 = torch.cat([m, -m[:1].abs() - 0.5])                              # an all-negative image
    for sigma in (0.5, 2.0, 8.0):
        out, mx = M.smooth_maps(m3, sigma, with_max=True)
        nan = torch.isnan(mx).cpu().tolist()
        assert nan == [False, True, False], (sigma, nan)
        ref = out.amax((1, 2))
        assert mx[0].item() == ref[0].item() and mx[2].item() == ref[2].item() and mx[2].item() < 0
    # radius 0 (sigma < 0.125) copies, and sigma 0 returns the maps unchanged; the maximum comes from the same kernel
    for sigma in (0.0, 0.1):
        out, mx = M.smooth_maps(m3, sigma, with_max=True)
        assert _bits_equal(out.cpu().numpy(), m3.cpu().numpy())
        assert torch.isnan(mx).cpu().tolist() == [False, True, False]
        assert mx[0].item() == m3[0].max().item() and mx[2].item() == m3[2].max().item()
    same = M.smooth_maps(m3, 0.0)                                        # no launch: the maps as given
    assert same.data_ptr() == m3.data_ptr() and same.shape == m3.shape


def test_smooth_maps_value_errors():
    from srad_amd import metrics as M
    m = torch.zeros(2, 20, 30, device="cuda")
    with pytest.raises(ValueError, match="sigma"):
        M.smooth_maps(m, -1.0)
    with pytest.raises(ValueError, match=r"sigma = 5.2 .*radius 21.*20x30"):
        M.smooth_maps(m, 5.2)                                            # radius 21 > min(H, W) = 20
    assert M.smooth_maps(m, 5.0).shape == m.shape                        # radius 20 == min(H, W)
    big = torch.zeros(1, 300, 300, device="cuda")
    with pytest.raises(ValueError, match="radius 129"):
        M.smooth_maps(big, 32.2)                                         # radius 129 > 128
    assert M.smooth_maps(big, 32.0).shape == big.shape                   # radius 128
