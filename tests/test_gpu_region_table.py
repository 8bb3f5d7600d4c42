"""GPU: the region table (srad_region_table / metrics.region_table, csrc/kernels_region_table.hip) against the scipy tables of
tests/golden/regions_golden.npz and the numpy restatement of tests/regions_ref.py.  Every comparison is exact.  The shapes are
the smallest at which the kernel can go wrong: widths that are no multiple of the 32-pixel tile, regions across tile borders,
row and image ends, score ties, the largest region count, one region per image, none at all."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import regions_ref as R

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL = ["blobs", "corner", "borders", "wrap64", "spiral", "almost_full", "good_plus_one_bad", "zeros"]
DTYPES = dict(image=torch.int32, area=torch.int32, box=torch.int32, sum_y=torch.int64, sum_x=torch.int64, overlap=torch.int32,
              peak=torch.float32, peak_y=torch.int32, peak_x=torch.int32)


@pytest.fixture(scope="module")
def goldens():
    return np.load(os.path.join(GOLDEN_DIR, "pro_golden.npz")), np.load(os.path.join(GOLDEN_DIR, "regions_golden.npz"))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(m, s, o, cap):
    """srad_region_table straight from the C entry point: (records int32 [cap, 14], the three counts)."""
    from srad_amd import _lib as L
    from srad_amd import metrics as M
    n, H, W = m.shape
    rec = torch.full((max(cap, 1), 14), -7, dtype=torch.int32, device="cuda")
    counts = torch.empty(3, dtype=torch.int64, device="cuda")
    nb = C.c_size_t()
    L.check(L.lib().srad_region_table_workspace_bytes(n, H, W, C.byref(nb)))
    keep, wp, wb = M._ws_buffer(nb.value, m.device)
    L.check(L.lib().srad_region_table(L.dptr(m), L.dptr(s), L.dptr(o), n, H, W, L.dptr(rec), C.c_int64(cap), L.dptr(counts), wp, wb,
                                      L.current_stream_ptr()))
    torch.cuda.synchronize()
    return rec.cpu().numpy(), counts.tolist()


@pytest.mark.parametrize("case", SMALL)
def test_golden_cases_in_both_roles(goldens, case):
    from srad_amd import metrics as M
    pro, reg = goldens
    s, m = pro[f"{case}/s"], pro[f"{case}/m"] != 0
    pred = s.astype(np.float64) > float(reg["threshold"])
    for role, (a, b) in (("gt", (m, pred)), ("pred", (pred, m))):
        want = {k: reg[f"{case}/{role}/{k}"] for k in R.FIELDS + R.PEAK}
        want["n_regions"] = len(want["area"])
        got = M.region_table(_cuda(a), _cuda(s), _cuda(b))
        assert list(got) == list(R.FIELDS + R.PEAK) + ["n_regions"]
        for k, dt in DTYPES.items():
            assert got[k].is_cuda and got[k].dtype == dt and got[k].shape[0] == want["n_regions"], k
        R.assert_tables_equal(got, want, where=(case, role))
        plain = M.region_table(_cuda(a).bool())                    # no scores, no other mask; any mask dtype
        assert list(plain) == list(R.FIELDS) + ["n_regions"]
        R.assert_tables_equal(plain, dict(want, overlap=np.zeros_like(want["overlap"])), peak=False, where=(case, role, "plain"))


def test_lattice_of_single_pixels_and_the_capacity():
    """2 x 64 x 64, every other pixel of every other row: 2048 regions, the most this shape can hold."""
    from srad_amd import metrics as M
    m = np.zeros((2, 64, 64), np.uint8)
    m[:, ::2, ::2] = 1
    rng = np.random.RandomState(5)
    s = (np.round(rng.rand(2, 64, 64) * 8) / 8).astype(np.float32)
    want = R.region_table_ref(m, s, None)
    assert want["n_regions"] == 2048
    rec, counts = _raw(_cuda(m), _cuda(s), None, 8)
    assert counts == [2048, 0, 8]
    assert np.array_equal(rec[:8, 0], want["image"][:8]) and np.array_equal(rec[:8, 1], want["area"][:8])
    assert np.array_equal(rec[:8, 2:6], want["box"][:8]) and np.array_equal(rec[:8, 12], want["peak_y"][:8])
    assert np.array_equal(rec[:8, 11].view(np.float32), want["peak"][:8])
    rec0, counts0 = _raw(_cuda(m), _cuda(s), None, 0)              # no record at all: the counts alone
    assert counts0 == [2048, 0, 0] and (rec0 == -7).all()
    got = M.region_table(_cuda(m), _cuda(s), cap=8)                 # the wrapper repeats at the exact count
    R.assert_tables_equal(got, want, where="lattice")
    assert got["area"].shape[0] == 2048 and (got["area"] == 1).all()
    R.assert_tables_equal(M.region_table(_cuda(m), _cuda(s)), want, where="lattice, default capacity")
    R.assert_tables_equal(M.region_table(_cuda(m), _cuda(s), cap=2048), want, where="lattice, exact capacity")


def test_all_ones_mask_closed_forms():
    from srad_amd import metrics as M
    n, H, W = 2, 33, 65
    m = torch.ones(n, H, W, dtype=torch.uint8, device="cuda")
    s = torch.full((n, H, W), 0.25, device="cuda")
    o = torch.zeros(n, H, W, dtype=torch.uint8, device="cuda")
    o[1, 5:9, 60:] = 3
    got = M.region_table(m, s, o)
    assert got["n_regions"] == n
    assert got["image"].tolist() == [0, 1] and got["area"].tolist() == [H * W] * 2
    assert got["box"].tolist() == [[0, 0, H - 1, W - 1]] * 2
    assert got["sum_y"].tolist() == [W * H * (H - 1) // 2] * 2 and got["sum_x"].tolist() == [H * W * (W - 1) // 2] * 2
    assert got["overlap"].tolist() == [0, 20]
    assert got["peak"].tolist() == [0.25, 0.25] and got["peak_y"].tolist() == [0, 0] and got["peak_x"].tolist() == [0, 0]
    s[1, 20, 40] = s[1, 20, 41] = s[1, 32, 0] = 0.5                 # three equal maxima: the first in raster order
    s[0, 7, 7] = -0.0
    got = M.region_table(m, s, o)
    assert got["peak"].tolist() == [0.25, 0.5] and got["peak_y"].tolist() == [0, 20] and got["peak_x"].tolist() == [0, 40]
    z = torch.zeros(n, H, W, device="cuda")                         # -0.0 equals +0.0: the earlier pixel wins whatever its sign
    z[0, 0, 3] = -0.0
    z[1] = -0.0
    z[1, 4, 4] = 0.0
    got = M.region_table(m, z)
    assert got["peak"].tolist() == [0.0, 0.0] and got["peak_y"].tolist() == [0, 0] and got["peak_x"].tolist() == [0, 0]
    assert not torch.signbit(got["peak"]).any()
    neg = torch.full((n, H, W), -2.0, device="cuda")                # negative scores order as numbers do, -inf below all
    neg[0, 10, 10] = -1.0
    neg[1] = float("-inf")
    neg[1, 1, 64] = -3e38
    got = M.region_table(m, neg)
    assert got["peak"].tolist() == [-1.0, float(np.float32(-3e38))] and got["peak_y"].tolist() == [10, 1]
    assert got["peak_x"].tolist() == [10, 64]


def test_all_zero_mask():
    from srad_amd import metrics as M
    z = torch.zeros(3, 40, 50, dtype=torch.uint8, device="cuda")
    s = torch.rand(3, 40, 50, device="cuda")
    got = M.region_table(z, s, z)
    assert got["n_regions"] == 0
    for k, dt in DTYPES.items():
        assert got[k].dtype == dt and got[k].numel() == 0, k
    assert tuple(got["box"].shape) == (0, 4)
    assert M.region_table(z[0])["n_regions"] == 0                   # one [H, W] mask


def test_image_permutation_and_bit_identical_runs(goldens):
    from srad_amd import metrics as M
    pro, _ = goldens
    s, m = pro["blobs/s"], pro["blobs/m"]
    o = (s > 0.75).astype(np.uint8)
    perm = [3, 0, 4, 2, 1]
    a = M.region_table(_cuda(m), _cuda(s), _cuda(o))
    b = M.region_table(_cuda(m[perm]), _cuda(s[perm]), _cuda(o[perm]))
    assert a["n_regions"] == b["n_regions"] > 0
    img_a = a["image"].cpu().numpy()
    rows = np.concatenate([np.flatnonzero(img_a == src) for src in perm])   # the records of a, image by image in b's order
    for k in R.FIELDS[1:] + R.PEAK:
        assert torch.equal(b[k].cpu(), a[k].cpu()[torch.from_numpy(rows)]), k
    assert b["image"].tolist() == np.concatenate([[j] * int((img_a == src).sum()) for j, src in enumerate(perm)]).tolist()
    mt, st, ot = _cuda(m), _cuda(s), _cuda(o)
    rec1, c1 = _raw(mt, st, ot, 64)
    rec2, c2 = _raw(mt, st, ot, 64)
    assert c1 == c2 and rec1.tobytes() == rec2.tobytes()


def test_nan_scores(goldens):
    from srad_amd import metrics as M
    pro, _ = goldens
    s, m = pro["borders/s"].copy(), pro["borders/m"]
    outside = np.argwhere(m == 0)[::7]
    s[tuple(outside.T)] = np.nan                                    # a NaN outside every region is not looked at
    want = R.region_table_ref(m, s, None)
    assert want["n_nan"] == 0
    R.assert_tables_equal(M.region_table(_cuda(m), _cuda(s)), want, where="NaN outside")
    inside = np.argwhere(m != 0)[[0, 5, 6]]
    s[tuple(inside.T)] = np.nan
    with pytest.raises(ValueError, match="3 scores inside the regions are NaN"):
        M.region_table(_cuda(m), _cuda(s))
    want = R.region_table_ref(m, s, None)                           # counted, and never a peak
    rec, counts = _raw(_cuda(m), _cuda(s), None, 32)
    assert counts == [want["n_regions"], 3, want["n_regions"]]
    k = want["n_regions"]
    assert np.array_equal(rec[:k, 11].view(np.float32), want["peak"], equal_nan=True)
    assert np.array_equal(rec[:k, 12], want["peak_y"]) and np.array_equal(rec[:k, 13], want["peak_x"])
    one = np.zeros((1, 5, 5), np.uint8)                             # a region of NaN scores only: no peak
    one[0, 2, 2] = 1
    rec, counts = _raw(_cuda(one), _cuda(np.full((1, 5, 5), np.nan, np.float32)), None, 4)
    assert counts == [1, 1, 1] and np.isnan(rec[0, 11:12].view(np.float32)[0]) and rec[0, 12:14].tolist() == [-1, -1]


def test_wrapper_refusals():
    from srad_amd import metrics as M
    m = torch.ones(2, 8, 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="same shape"):
        M.region_table(m, torch.zeros(2, 8, 9, device="cuda"))
    with pytest.raises(ValueError, match="same shape"):
        M.region_table(m, None, torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="float32"):
        M.region_table(m, torch.zeros(2, 8, 8, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="non-empty"):
        M.region_table(torch.zeros(0, 8, 8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="cap"):
        M.region_table(m, cap=-1)


@pytest.mark.parametrize("case", ["blobs", "spiral", "zeros"])
def test_consistent_with_mask_regions_and_operating_point(goldens, case):
    from srad_amd import metrics as M
    pro, _ = goldens
    s, m = pro[f"{case}/s"], pro[f"{case}/m"]
    n, H, W = m.shape
    size, n_reg = M.mask_regions(_cuda(m))
    got = M.region_table(_cuda(m))
    assert got["n_regions"] == n_reg
    # the region's first pixel: the first member pixel of the top row of its box at or after x0 that belongs to it - found
    # from the reference's roots, and the size mask_regions writes there is the area
    firsts = [(i,) + root for i in range(n) for root in sorted(set(R.label_roots(m[i]).values()))]
    assert [int(size[f]) for f in firsts] == got["area"].tolist()
    assert [f[0] for f in firsts] == got["image"].tolist() and [f[1] for f in firsts] == got["box"][:, 0].tolist()
    for area in (1, 3):
        pred, img_pred, _ = M.operating_point(_cuda(s), 0.5, None, area)
        tab = M.region_table(pred, _cuda(s))
        per_image = np.bincount(tab["image"].cpu().numpy(), weights=tab["area"].cpu().numpy(), minlength=n).astype(np.int64)
        assert per_image.tolist() == img_pred.tolist()
        assert tab["n_regions"] == 0 or int(tab["area"].min()) >= area
        assert tab["n_regions"] == M.mask_regions(pred)[1]
