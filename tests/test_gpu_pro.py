"""GPU: region labelling (srad_mask_regions) and AU-PRO (srad_pixel_pro) against tests/golden/pro_golden.npz (scipy.ndimage
labels and the numpy restatement of the definition, written by tests/golden/make_pro_golden.py), against an in-test pure-Python
union-find labeller on random masks, and for bit-identical results across calls and image orders; constructed tie groups
(tests/helpers.py) put group heads and a headless tile on the scan's thread, tile and chunk boundaries.  No scipy or sklearn
here."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests.helpers import TIE_CHUNK_N, TIE_SMALL, pad_last_group, tie_chunk_lengths, tie_group_case

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL = ["blobs", "corner", "borders", "wrap64", "spiral", "almost_full", "good_plus_one_bad", "zeros"]


def _generator():
    spec = importlib.util.spec_from_file_location("make_pro_golden", os.path.join(GOLDEN_DIR, "make_pro_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "pro_golden.npz"))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _region_counts(m):
    """srad_mask_regions' count triple {n_regions, n_ok, n_defect}, straight from the C entry point."""
    from srad_amd import _lib as L
    from srad_amd import metrics as M
    mt = _cuda(m.astype(np.uint8))
    n, H, W = mt.shape
    size = torch.empty(n, H, W, dtype=torch.int32, device="cuda")
    counts = torch.empty(3, dtype=torch.int64, device="cuda")
    nb = C.c_size_t()
    L.check(L.lib().srad_mask_regions_workspace_bytes(n, H, W, C.byref(nb)))
    keep, wp, wb = M._ws_buffer(nb.value, mt.device)
    L.check(L.lib().srad_mask_regions(L.dptr(mt), n, H, W, L.dptr(size), L.dptr(counts), wp, wb, L.current_stream_ptr()))
    return counts.tolist()


@pytest.mark.parametrize("case", SMALL)
def test_region_sizes_match_golden(golden, case):
    from srad_amd import metrics as M
    m = golden[f"{case}/m"]
    size, R = M.mask_regions(_cuda(m))
    assert size.dtype == torch.int32 and tuple(size.shape) == m.shape
    assert np.array_equal(size.cpu().numpy().astype(np.int64), golden[f"{case}/sizes"].astype(np.int64))
    assert R == int(golden[f"{case}/counts"][0])
    assert _region_counts(m) == [int(v) for v in golden[f"{case}/counts"]]


@pytest.mark.parametrize("case", SMALL)
def test_curve_and_aupro_match_golden(golden, case):
    from srad_amd import metrics as M
    s, m = _cuda(golden[f"{case}/s"]), _cuda(golden[f"{case}/m"])
    fpr, pro = M.pro_curve(s, m)
    want_f, want_p = golden[f"{case}/fpr"], golden[f"{case}/pro"]
    assert len(fpr) == len(want_f)
    assert np.max(np.abs(fpr - want_f)) <= 1e-9 and np.max(np.abs(pro - want_p)) <= 1e-9
    for L, want in zip(golden[f"{case}/limits"], golden[f"{case}/aupro"]):
        got = M.aupro(s, m, float(L))
        assert abs(got - float(want)) <= 1e-9, (case, float(L), got, float(want))


def test_two_million_pixel_hashed_case(golden):
    from srad_amd import metrics as M
    G = _generator()
    n, H, W, salt = [int(v) for v in golden["large/args"]]
    s, m = G.hashed_case(n, H, W, salt)
    ck = golden["large/checksum"]
    assert s.astype(np.float64).sum() == ck[0] and float(m.sum()) == ck[1]
    st, mt = _cuda(s), _cuda(m)
    size, R = M.mask_regions(mt)
    z = size.cpu().numpy().astype(np.float64)
    assert float(z.sum()) == ck[2] and float((z ** 2).sum()) == ck[3]
    assert _region_counts(m) == [int(v) for v in golden["large/counts"]]
    fpr, pro = M.pro_curve(st, mt)
    assert len(fpr) == int(golden["large/n_points"])
    assert np.max(np.abs(fpr[::G.LARGE_STRIDE] - golden["large/fpr_every"])) <= 1e-9
    assert np.max(np.abs(pro[::G.LARGE_STRIDE] - golden["large/pro_every"])) <= 1e-9
    for L, want in zip(golden["large/limits"], golden["large/aupro"]):
        assert abs(M.aupro(st, mt, float(L)) - float(want)) <= 1e-9


def test_bit_identical_across_calls_and_image_order(golden):
    from srad_amd import metrics as M
    G = _generator()
    s, m = G.hashed_case(6, 96, 80, 5)
    perm = np.array([3, 0, 5, 1, 4, 2])

    def run(a, b):
        st, mt = _cuda(a), _cuda(b)
        fpr, pro = M.pro_curve(st, mt)
        return M.aupro(st, mt), M.aupro(st, mt, 0.05), fpr.tobytes(), pro.tobytes()
    first = run(s, m)
    assert run(s, m) == first
    assert run(s[perm], m[perm]) == first                                  # another image order: the same bits


def test_random_masks_against_python_union_find():
    from srad_amd import metrics as M
    G = _generator()
    rng = np.random.RandomState(77)
    for n, H, W, p in ((3, 20, 23, 0.3), (2, 70, 33, 0.45), (1, 5, 130, 0.5), (4, 33, 65, 0.2)):
        m = (rng.rand(n, H, W) < p).astype(np.uint8)
        s = (np.round(rng.rand(n, H, W) * 40) / 40 + 0.3 * m * rng.rand(n, H, W)).astype(np.float32)
        z, R = G.uf_sizes(m)
        size, r = M.mask_regions(_cuda(m))
        assert r == R and np.array_equal(size.cpu().numpy().astype(np.int64), z)
        fpr, pro = G.pro_curve_ref(s, z, R)
        gf, gp = M.pro_curve(_cuda(s), _cuda(m))
        assert len(gf) == len(fpr) and np.max(np.abs(gf - fpr)) <= 1e-9 and np.max(np.abs(gp - pro)) <= 1e-9
        for L in (0.3, 0.01, 1.0):
            assert abs(M.aupro(_cuda(s), _cuda(m), L) - G.aupro_ref(fpr, pro, L)) <= 1e-9


def test_refusals():
    from srad_amd import metrics as M
    rng = np.random.RandomState(1)
    m = np.zeros((2, 16, 16), np.uint8)
    m[1, 4:7, 4:9] = 1
    s = rng.rand(2, 16, 16).astype(np.float32)
    st, mt = _cuda(s), _cuda(m)
    bad = s.copy()
    bad[0, 3, 3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        M.aupro(_cuda(bad), mt)
    with pytest.raises(ValueError, match="no defect region"):
        M.aupro(st, _cuda(np.zeros_like(m)))
    with pytest.raises(ValueError, match="no ok pixel"):
        M.aupro(st, _cuda(np.ones_like(m)))
    with pytest.raises(ValueError, match="no defect region"):
        M.pro_curve(st, _cuda(np.zeros_like(m)))
    for L in (0.0, -0.3, 1.01, float("nan")):
        with pytest.raises(ValueError, match="fpr_limit"):
            M.aupro(st, mt, L)
    with pytest.raises(ValueError, match="same shape"):
        M.aupro(st[:, :8], mt)
    assert 0.0 <= M.aupro(st, mt) <= 1.0


def test_mask_dtypes_agree():
    from srad_amd import metrics as M
    rng = np.random.RandomState(4)
    m = rng.rand(3, 24, 40) < 0.25
    s = _cuda(rng.rand(3, 24, 40).astype(np.float32))
    ref = None
    for mm in (m, m.astype(np.int64) * 7, m.astype(np.uint8)):
        size, R = M.mask_regions(_cuda(mm))
        got = (size.cpu().numpy().tobytes(), R, M.aupro(s, _cuda(mm)), M.aupro(s, _cuda(mm), 0.1))
        ref = ref or got
        assert got == ref


def _rectangles(H, W, step_y, step_x, max_h, max_w):
    """A mask of non-touching axis-aligned rectangles on a (step_y, step_x) grid, and every pixel's region size; R."""
    assert max_h < step_y and max_w < step_x
    m, z, k = np.zeros((1, H, W), np.uint8), np.zeros((1, H, W), np.int64), 0
    for y0 in range(2, H - max_h, step_y):
        for x0 in range(3, W - max_w, step_x):
            h, w = 1 + (k * 37) % max_h, 1 + (k * 53) % max_w
            m[0, y0:y0 + h, x0:x0 + w] = 1
            z[0, y0:y0 + h, x0:x0 + w] = h * w
            k += 1
    return m, z, k


@pytest.mark.parametrize("case", ["small", "chunk"])
def test_constructed_tie_groups(case):
    from srad_amd import metrics as M
    G = _generator()
    if case == "small":
        H, W = 131, 159
        lengths = pad_last_group(TIE_SMALL, H * W)
        m, z, R = _rectangles(H, W, 23, 29, 17, 19)
    else:
        H, W = 1031, 1023
        lengths = tie_chunk_lengths()
        assert H * W == TIE_CHUNK_N
        m, z, R = _rectangles(H, W, 97, 101, 90, 95)
    s, _ = tie_group_case(lengths, descending=True, seed=3)
    s = s.reshape(1, H, W)
    fpr, pro = G.pro_curve_ref(s, z, R)
    st, mt = _cuda(s), _cuda(m)
    gf, gp = M.pro_curve(st, mt)
    assert len(gf) == len(lengths) + 2
    assert np.max(np.abs(gf - fpr)) <= 1e-9 and np.max(np.abs(gp - pro)) <= 1e-9
    for L in (0.3, 0.01, 1.0):
        assert abs(M.aupro(st, mt, L) - G.aupro_ref(fpr, pro, L)) <= 1e-9
