"""GPU: exact pixel-level ROC-AUC (srad_pixel_roc_auc: device radix sort + Mann-Whitney scan) against scikit-learn's
roc_auc_score (tests/golden/pixel_auc_golden.npz, written by tests/golden/make_pixel_auc_golden.py) and against a vectorised
numpy Mann-Whitney U.  Bar: 1e-12, and bit-identical results under permutation of the input and across calls.  Constructed
tie groups (tests/helpers.py) on the scan's thread, tile and chunk boundaries are compared as integers."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests.helpers import TIE_SMALL, tie_chunk_lengths, tie_group_case

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["continuous", "ties8", "signed_zeros", "negative", "all_equal", "perfect", "inverse", "n3", "odd_n"]


def _generator():
    spec = importlib.util.spec_from_file_location("make_pixel_auc_golden", os.path.join(GOLDEN_DIR, "make_pixel_auc_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "pixel_auc_golden.npz"))


def _auc(s, y):
    from srad_amd import metrics as M
    return M.pixel_roc_auc(torch.from_numpy(np.ascontiguousarray(s)).cuda(), torch.from_numpy(np.ascontiguousarray(y)).cuda())


def mann_whitney_counts(s, y):
    """(n_pos, n_neg, twice_U): twice_U = sum over tie groups g of pos_g * (2 * negatives below g + neg_g), in int64."""
    vals, inv = np.unique(s.astype(np.float64), return_inverse=True)
    pos = np.bincount(inv[y != 0], minlength=len(vals)).astype(np.int64)
    neg = np.bincount(inv[y == 0], minlength=len(vals)).astype(np.int64)
    below = np.concatenate([[0], np.cumsum(neg)[:-1]])
    return int(pos.sum()), int(neg.sum()), int(np.sum(pos * (2 * below + neg)))


def mann_whitney_auc(s, y):
    """twice_U / (2 * n_pos * n_neg)."""
    n_pos, n_neg, twice_u = mann_whitney_counts(s, y)
    return twice_u / (2.0 * n_pos * n_neg)


def _auc_raw(s, y):
    """srad_pixel_roc_auc's counts {n_pos, n_neg, n_nan, twice_U} and its double, straight from the C entry point."""
    from srad_amd import _lib as L
    from srad_amd import metrics as M
    st, yt = torch.from_numpy(np.ascontiguousarray(s)).cuda(), torch.from_numpy(np.ascontiguousarray(y)).cuda()
    counts = torch.empty(4, dtype=torch.int64, device="cuda")
    auc = torch.empty((), dtype=torch.float64, device="cuda")
    nb = C.c_size_t()
    L.check(L.lib().srad_pixel_auc_workspace_bytes(C.c_int64(len(s)), C.byref(nb)))
    keep, wp, wb = M._ws_buffer(nb.value, st.device)
    L.check(L.lib().srad_pixel_roc_auc(L.dptr(st), L.dptr(yt), C.c_int64(len(s)), L.dptr(counts), L.dptr(auc), wp, wb,
                                       L.current_stream_ptr()))
    return counts.tolist(), float(auc.item())


@pytest.mark.parametrize("case", CASES)
def test_matches_sklearn_golden(golden, case):
    got = _auc(golden[f"{case}/s"], golden[f"{case}/y"])
    assert abs(got - float(golden[f"{case}/auc"])) <= 1e-12, (case, got, float(golden[f"{case}/auc"]))


def test_fixture_values():
    g = np.load(os.path.join(GOLDEN_DIR, "pixel_auc_golden.npz"))
    assert float(g["all_equal/auc"]) == 0.5 and float(g["perfect/auc"]) == 1.0 and float(g["inverse/auc"]) == 0.0
    assert _auc(g["all_equal/s"], g["all_equal/y"]) == 0.5
    assert _auc(g["perfect/s"], g["perfect/y"]) == 1.0 and _auc(g["inverse/s"], g["inverse/y"]) == 0.0


def test_two_million_hashed_case(golden):
    n, salt = [int(v) for v in golden["large/args"]]
    s, y = _generator().hashed_case(n, salt)
    assert s.astype(np.float64).sum() == golden["large/checksum"][0] and float(y.sum()) == golden["large/checksum"][1]
    assert abs(_auc(s, y) - float(golden["large/auc"])) <= 1e-12


def test_three_million_vs_numpy_mann_whitney_and_order_independence():
    rng = np.random.default_rng(11)
    n = 3_000_017
    s = (rng.standard_normal(n) * 3).astype(np.float32)
    s[::7] = np.round(s[::7])                                     # many ties, -0.0 among them
    y = (rng.random(n) < 1 / (1 + np.exp(-s))).astype(np.uint8)
    want = mann_whitney_auc(s, y)
    a = _auc(s, y)
    assert abs(a - want) <= 1e-12, (a, want)
    assert _auc(s, y) == a                                        # bit-identical across calls
    p = rng.permutation(n)
    assert _auc(s[p], y[p]) == a                                  # ... and under a permutation of the input


def test_labels_of_any_dtype_and_shape():
    from srad_amd import metrics as M
    g = torch.Generator().manual_seed(1)
    s = torch.rand(3, 37, 29, generator=g)
    y = torch.rand(3, 37, 29, generator=g) < s
    a = M.pixel_roc_auc(s.cuda(), y.cuda())
    assert a == M.pixel_roc_auc(s.cuda(), y.to(torch.uint8).cuda()) == M.pixel_roc_auc(s.cuda(), (y.int() * 5).cuda())
    assert abs(a - mann_whitney_auc(s.numpy().ravel(), y.numpy().ravel())) <= 1e-12


def test_one_class_and_nan_raise():
    from srad_amd import metrics as M
    s = torch.rand(100, device="cuda")
    with pytest.raises(ValueError, match="Only one class present"):
        M.pixel_roc_auc(s, torch.ones(100, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="Only one class present"):
        M.pixel_roc_auc(s, torch.zeros(100, dtype=torch.uint8, device="cuda"))
    y = (torch.arange(100, device="cuda") % 2).to(torch.uint8)
    s[17] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        M.pixel_roc_auc(s, y)


@pytest.mark.parametrize("case", ["small", "chunk"])
def test_constructed_tie_groups_exact(case):
    s, y = tie_group_case(TIE_SMALL if case == "small" else tie_chunk_lengths(), descending=False, seed=3)
    n_pos, n_neg, twice_u = mann_whitney_counts(s, y)
    assert twice_u < 2 ** 53                                      # so the float division below is exact
    counts, auc = _auc_raw(s, y)
    assert counts == [n_pos, n_neg, 0, twice_u]
    assert auc == twice_u / (2.0 * n_pos * n_neg)


def test_constructed_tie_groups_with_nan_exact():
    s, y = tie_group_case(TIE_SMALL, descending=False, seed=3)
    bad = np.random.default_rng(5).choice(len(s), 37, replace=False)
    s[bad] = np.nan
    keep = ~np.isnan(s)
    n_pos, n_neg, twice_u = mann_whitney_counts(s[keep], y[keep])
    counts, _ = _auc_raw(s, y)
    assert counts == [n_pos, n_neg, 37, twice_u]
