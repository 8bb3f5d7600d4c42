"""GPU: metrics.gms_maps (srad_gms_maps) against the numpy restatement of tests/gms_ref.py.  The bar: every value equals the
restatement's float32 or is adjacent to it - about 20 correctly rounded float64 operations come before the single rounding
to float32, so the device can differ from numpy only where the float64 value lies within ~2^-48 of a rounding boundary.  The
count of unequal values is printed per case.  Shapes are the smallest at which each mechanism can fail: every tap reflecting
and every bilinear neighbour clamping (a 2 x 2 coarsest plane), odd plane sizes, a width that is no multiple of the wave,
several images, stacks that start at an odd byte."""
import numpy as np
import pytest
import torch

from tests import gms_ref as R

pytestmark = pytest.mark.gpu

# (n, H, W, C, levels)
CASES = [(2, 8, 8, 1, 1), (2, 16, 16, 1, 4), (2, 24, 40, 3, 1), (2, 24, 40, 3, 2), (2, 24, 40, 3, 3), (2, 64, 64, 3, 4),
         (2, 72, 200, 1, 4), (5, 128, 128, 1, 4)]


def _pair(shape, seed):
    rng = np.random.default_rng(seed)
    hr = rng.integers(0, 256, shape, dtype=np.uint8)
    sr = np.clip(hr.astype(np.int64) + rng.integers(-40, 41, shape), 0, 255).astype(np.uint8)
    sr[0] = rng.integers(0, 256, shape[1:], dtype=np.uint8)      # image 0: unrelated noise, the others: a degraded copy
    return sr, hr


def _gpu(sr, hr, levels):
    from srad_amd import metrics as M
    return M.gms_maps(torch.from_numpy(sr).cuda(), torch.from_numpy(hr).cuda(), levels).cpu().numpy()


def _ulps(a, b):
    """Distance in float32 steps between non-negative float32 arrays."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _check(got, want, tag):
    assert got.dtype == np.float32 and got.shape == want.shape
    d = _ulps(got, want)
    print(f"gms_maps {tag}: {int((d != 0).sum())} of {d.size} values differ from the restatement, max {int(d.max())} ulp")
    assert d.max() <= 1, (tag, int(d.max()))


@pytest.fixture(scope="module")
def random_cases():
    """{case: (sr, hr, restatement)} computed once."""
    out = {}
    for k, (n, H, W, C, L) in enumerate(CASES):
        sr, hr = _pair((n, H, W, C), 100 + k)
        out[n, H, W, C, L] = (sr, hr, R.gms_maps(sr, hr, L))
    return out


@pytest.mark.parametrize("case", CASES)
def test_random_pairs_match_the_restatement(random_cases, case):
    sr, hr, want = random_cases[case]
    got = _gpu(sr, hr, case[4])
    _check(got, want, str(case))
    assert (got >= 0).all() and (got < 1).all() and got.max() > 0
    # symmetric in (sr, hr), bit for bit; identical stacks give exact zeros
    assert np.array_equal(_gpu(hr, sr, case[4]).view(np.uint32), got.view(np.uint32))
    same = _gpu(sr, sr, case[4])
    assert not same.any() and not np.signbit(same).any()


@pytest.mark.parametrize("case", [(2, 16, 16, 1, 4), (2, 24, 40, 3, 3), (2, 72, 200, 1, 4)])
def test_views_that_start_at_an_odd_byte(random_cases, case):
    from srad_amd import metrics as M
    sr, hr, want = random_cases[case]
    views = []
    for a in (sr, hr):
        buf = torch.zeros(a.size + 1, dtype=torch.uint8, device="cuda")
        buf[1:] = torch.from_numpy(a).cuda().reshape(-1)
        views.append(buf[1:].view(a.shape))
        assert views[-1].data_ptr() % 2 == 1 and views[-1].is_contiguous()
    got = M.gms_maps(views[0], views[1], case[4]).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), _gpu(sr, hr, case[4]).view(np.uint32))
    _check(got, want, f"{case} from byte 1")


@pytest.mark.parametrize("C", [1, 3])
def test_one_pixel_changes_its_neighbourhood_only(C):
    rng = np.random.default_rng(5)
    hr = rng.integers(0, 256, (1, 24, 40, C), dtype=np.uint8)
    for y, x in ((0, 0), (11, 17), (23, 39), (1, 38)):
        sr = hr.copy()
        sr[0, y, x] ^= 0x80
        got = _gpu(sr, hr, 1)
        _check(got, R.gms_maps(sr, hr, 1), f"one pixel at {(y, x)}, C={C}")
        inside = np.zeros((24, 40), bool)
        inside[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
        assert got[0][inside].any() and not got[0][~inside].any(), (y, x)


@pytest.mark.parametrize("levels", [1, 4])
def test_extremes(levels):
    shape = (1, 32, 48, 3)
    black = np.zeros(shape, np.uint8)
    white = np.full(shape, 255, np.uint8)                      # the largest channel sums, and no edge in either stack
    assert not _gpu(white, black, levels).any()
    for C in (1, 3):
        step = np.zeros((1, 32, 48, C), np.uint8)
        step[:, :, 24:] = 255                                  # 0 on the left half, 255 on the right: the largest Gx
        got = _gpu(step, np.zeros_like(step), levels)
        _check(got, R.gms_maps(step, np.zeros_like(step), levels), f"step C={C} L={levels}")
        assert 0 < got.max() < 1 and not got[:, :, :8].any()


def test_batch_invariance_and_a_reused_workspace(random_cases):
    import ctypes as C
    from srad_amd import _lib as L
    sr, hr, want = random_cases[5, 128, 128, 1, 4]
    full = _gpu(sr, hr, 4)
    for i in (0, 3, 4):
        assert np.array_equal(_gpu(sr[i:i + 1], hr[i:i + 1], 4).view(np.uint32), full[i:i + 1].view(np.uint32)), i
    # two calls on one workspace (the second after another shape used it) give the same bits
    lib = L.lib()
    nb = C.c_size_t()
    L.check(lib.srad_gms_map_workspace_bytes(5, 128, 128, 4, C.byref(nb)))
    keep, wp, wb = L.ws_buffer(nb.value, "cuda")
    s, h = torch.from_numpy(sr).cuda(), torch.from_numpy(hr).cuda()
    outs = []
    for n in (5, 2, 5):
        out = torch.empty(n, 128, 128, device="cuda")
        L.check(lib.srad_gms_maps(L.dptr(s), L.dptr(h), n, 128, 128, 1, 4, L.dptr(out), wp, wb, L.current_stream_ptr()), "gms_maps")
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.uint32), full.view(np.uint32)) and np.array_equal(outs[2].view(np.uint32), full.view(np.uint32))
    assert np.array_equal(outs[1].view(np.uint32), full[:2].view(np.uint32))


def test_refusals():
    from srad_amd import metrics as M
    x = torch.zeros(1, 36, 64, 1, dtype=torch.uint8, device="cuda")
    for levels in (0, 5):
        with pytest.raises(ValueError, match="levels"):
            M.gms_maps(x, x, levels)
    with pytest.raises(ValueError, match="multiples of 8"):
        M.gms_maps(x, x, 4)
    assert M.gms_maps(x, x, 3).shape == (1, 36, 64)
    two = torch.zeros(1, 16, 16, 2, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="channels must be 1 or 3"):
        M.gms_maps(two, two, 1)
    with pytest.raises(RuntimeError, match="GPU only"):
        M.gms_maps(x.cpu(), x.cpu(), 1)
