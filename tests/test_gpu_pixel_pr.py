"""GPU: exact pixel-level precision-recall (srad_pixel_pr: the device radix sort and tie-group scan of the pixel AUC with a
precision-recall policy) against scikit-learn's numbers (tests/golden/pixel_pr_golden.npz, written by
tests/golden/make_pixel_pr_golden.py) and against that generator's numpy restatement, ``pr_ref``, which the generator checks
against sklearn.  Bars (DESIGN.md "Precision-recall"): AP within 1e-12, the curve's precision and recall within 1e-15 and its
thresholds bitwise, every count and the best-F1 point exactly, and bit-identical results under a permutation of the input.
Constructed tie groups put a group end and the next group's head on every boundary the scan carries across: a thread's 16 keys,
the scan tile (4096), the sort tile (8192) and the 256-tile chunk of the one-block tile scan."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests.helpers import TIE_SMALL, tie_chunk_lengths, tie_group_case

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_pixel_pr_golden", os.path.join(GOLDEN_DIR, "make_pixel_pr_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()
CASES = G.AUC_CASES + G.OWN_CASES
BOUNDARIES = (16, 4096, 8192, 256 * 4096)
SIZES = [1, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 8193, 256 * 4096 + 1]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "pixel_pr_golden.npz"))


@pytest.fixture(scope="module")
def inputs():
    return G.all_cases()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(f):
    return int(np.array([f], np.float32).view(np.uint32)[0])


def _raw(s, y):
    """(srad_pixel_pr's counts by name, its ap) through ``metrics._pixel_pr``, which refuses NaN and no positive."""
    from srad_amd import metrics as M
    c, ap, _ = M._pixel_pr(_cuda(s), _cuda(y), curve=False)
    return c, ap


def _check_against_ref(s, y, curve=True):
    """Everything ``pixel_pr`` and ``pr_curve`` return against the numpy restatement; returns the device's ap."""
    from srad_amd import metrics as M
    prec, rec, thr, tp, fp = G.pr_ref(s, y)
    k = G.best_point(tp, fp)
    P = int(tp[-1])
    c, ap = _raw(s, y)
    want = dict(n_pos=P, n_neg=len(s) - P, n_nan=0, n_points=len(thr), tp=int(tp[k]), fp=int(fp[k]), score_bits=_bits(thr[k]))
    assert c == want
    assert abs(ap - G.ap_ref(tp, fp)) <= 1e-12, (ap, G.ap_ref(tp, fp))
    r = M.pixel_pr(_cuda(s), _cuda(y))
    a, b = want["tp"], want["fp"]
    assert r["ap"] == ap and (r["tp"], r["fp"], r["fn"], r["n_pos"], r["n_neg"]) == (a, b, P - a, P, len(s) - P)
    assert (r["f1max"], r["precision"], r["recall"]) == (2 * a / (2 * a + b + P - a), a / (a + b), a / P)
    assert _bits(r["score"]) == want["score_bits"]
    assert r["threshold"] == float(np.nextafter(thr[k], np.float32(-np.inf)))
    if curve:
        got_p, got_r, got_t = M.pr_curve(_cuda(s), _cuda(y))
        assert got_p.dtype == got_r.dtype == np.float64 and got_t.dtype == np.float32 and len(got_t) == len(thr)
        assert np.array_equal(got_t.view(np.uint32), thr.view(np.uint32))
        assert np.abs(got_p - prec).max() <= 1e-15 and np.abs(got_r - rec).max() <= 1e-15
    return ap


@pytest.mark.parametrize("case", CASES)
def test_matches_sklearn_golden(golden, inputs, case):
    from srad_amd import metrics as M
    s, y = inputs[case]
    r = M.pixel_pr(_cuda(s), _cuda(y))
    print(f"{case}: ap {r['ap']!r}, sklearn {float(golden[f'{case}/ap'])!r}, |d| = {abs(r['ap'] - float(golden[f'{case}/ap'])):.1e}")
    assert abs(r["ap"] - float(golden[f"{case}/ap"])) <= 1e-12
    assert [r["tp"], r["fp"], _bits(r["score"])] == [int(v) for v in golden[f"{case}/best"]]
    got_p, got_r, got_t = M.pr_curve(_cuda(s), _cuda(y))
    assert len(got_t) == int(golden[f"{case}/n_points"])
    if f"{case}/thresholds" in golden:                            # sklearn's own arrays
        want_p, want_r, want_t = (golden[f"{case}/{k}"] for k in ("precision", "recall", "thresholds"))
    else:                                                         # the longer curves: the restatement the generator checked
        want_p, want_r, want_t = G.pr_ref(s, y)[:3]
    assert np.array_equal(got_t.view(np.uint32), want_t.view(np.uint32))
    assert np.abs(got_p - want_p).max() <= 1e-15 and np.abs(got_r - want_r).max() <= 1e-15


def test_no_negative_gives_ap_one(inputs):
    from srad_amd import metrics as M
    s, y = inputs["all_pos"]
    r = M.pixel_pr(_cuda(s), _cuda(y))
    assert r["ap"] == 1.0 and r["f1max"] == 1.0 and (r["tp"], r["fp"], r["fn"], r["n_neg"]) == (300, 0, 0, 0)
    assert r["score"] == float(s.min())                           # every point has precision 1; only the last has recall 1


def test_bit_identical_under_permutation_and_across_calls(inputs):
    rng = np.random.default_rng(4)
    for case in ("odd_n", "quant3pct", "f1_tie_far", "inf_zero"):
        s, y = inputs[case]
        first = _raw(s, y)
        assert _raw(s, y) == first
        for _ in range(2):
            p = rng.permutation(len(s))
            assert _raw(s[p], y[p]) == first, case


def boundary_lengths(n):
    """Tie-group lengths adding up to n with a group end at key b - 1 and a group head at key b for every b of BOUNDARIES
    below n; between the cuts the lengths cycle through 1, 3, 16, 7, 33, 2, so heads and ends also fall inside threads and some
    threads hold no head (tiles without one are in ``test_groups_across_the_boundaries_exact``)."""
    cycle, lengths, k, pos = (1, 3, 16, 7, 33, 2), [], 0, 0
    for cut in [b for b in BOUNDARIES if b < n] + [n]:
        while pos < cut:
            step = min(cycle[k % len(cycle)], cut - pos)
            lengths.append(step)
            pos += step
            k += 1
    assert sum(lengths) == n
    return lengths


@pytest.mark.parametrize("n", SIZES)
def test_boundary_sizes_exact(n):
    lengths = boundary_lengths(n)
    s, y = tie_group_case(lengths, descending=True, seed=n)
    y[np.argmax(s)] = 1                                           # a positive whatever the draw; n = 1 has nothing else
    ends = np.cumsum(lengths)
    for b in BOUNDARIES:
        assert b >= n or b in ends
    _check_against_ref(s, y)


@pytest.mark.parametrize("case", ["small", "chunk"])
def test_groups_across_the_boundaries_exact(case):
    """The lengths of the pixel AUC's test: groups that run across thread, tile and chunk boundaries, and tiles without a head."""
    s, y = tie_group_case(TIE_SMALL if case == "small" else tie_chunk_lengths(), descending=True, seed=3)
    _check_against_ref(s, y, curve=case == "small")


def test_three_percent_positives_200k():
    """The shape of the data: few positives, continuous and quantised scores."""
    rng = np.random.default_rng(17)
    n = 200_003
    y = (rng.random(n) < 0.03).astype(np.uint8)
    s = (rng.standard_normal(n) + 1.2 * y).astype(np.float32)
    _check_against_ref(s, y, curve=False)
    _check_against_ref(np.round(s * 16) / np.float32(16), y)


def test_nan_and_no_positive_raise():
    from srad_amd import metrics as M
    s = torch.rand(1000, device="cuda")
    y = (torch.arange(1000, device="cuda") % 7 == 0).to(torch.uint8)
    with pytest.raises(ValueError, match="No positive class"):
        M.pixel_pr(s, torch.zeros(1000, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="same number of elements"):
        M.pixel_pr(s, y[:999])
    with pytest.raises(ValueError, match="no elements"):
        M.pixel_pr(s[:0], y[:0])
    s[[17, 400, 999]] = float("nan")
    with pytest.raises(ValueError, match="pixel_pr: 3 of 1000 scores are NaN"):
        M.pixel_pr(s, y)
    with pytest.raises(ValueError, match="3 of 1000 scores are NaN"):
        M.pr_curve(s, y)


def test_nan_scores_are_left_out_of_the_counts():
    import ctypes as C
    from srad_amd import _lib as L
    from srad_amd import metrics as M
    s, y = tie_group_case(TIE_SMALL, descending=True, seed=3)
    bad = np.random.default_rng(5).choice(len(s), 37, replace=False)
    s[bad] = np.nan
    keep = ~np.isnan(s)
    _, _, thr, tp, fp = G.pr_ref(s[keep], y[keep])
    k = G.best_point(tp, fp)
    st, yt = _cuda(s), _cuda(y)
    counts = torch.empty(7, dtype=torch.int64, device="cuda")
    ap = torch.empty((), dtype=torch.float64, device="cuda")
    nb = C.c_size_t()
    L.check(L.lib().srad_pixel_pr_workspace_bytes(C.c_int64(len(s)), C.byref(nb)))
    ws_keep, wp, wb = M._ws_buffer(nb.value, st.device)
    L.check(L.lib().srad_pixel_pr(L.dptr(st), L.dptr(yt), C.c_int64(len(s)), L.dptr(counts), L.dptr(ap), None, None, None,
                                  C.c_int64(0), wp, wb, L.current_stream_ptr()))
    P = int(tp[-1])
    assert counts.tolist() == [P, int(keep.sum()) - P, 37, len(thr), int(tp[k]), int(fp[k]), _bits(thr[k])]
    assert abs(float(ap.item()) - G.ap_ref(tp, fp)) <= 1e-12


def test_labels_of_any_dtype_and_shape():
    from srad_amd import metrics as M
    g = torch.Generator().manual_seed(1)
    s = torch.rand(3, 37, 29, generator=g)
    y = torch.rand(3, 37, 29, generator=g) < s
    a = M.pixel_pr(s.cuda(), y.cuda())
    assert a == M.pixel_pr(s.cuda(), y.to(torch.uint8).cuda()) == M.pixel_pr(s.cuda(), (y.int() * 5).cuda())
    assert a == M.pixel_pr(s.double().cuda(), y.long().cuda())


def test_threshold_reproduces_the_best_point_at_the_operating_point():
    """``threshold`` is in the ``map > threshold`` convention of the operating point: the merged kernel, thresholding the same
    maps at it, counts the best point's tp / fp / fn."""
    from srad_amd import metrics as M
    rng = np.random.default_rng(8)
    masks = np.zeros((3, 45, 63), np.uint8)
    masks[0, 5:19, 7:30] = 1
    masks[2, 30:, 50:] = 1
    maps = (np.round((rng.standard_normal(masks.shape) + 1.5 * masks) * 4) / 4).astype(np.float32)      # ~30 distinct values
    r = M.pixel_pr(_cuda(maps), _cuda(masks))
    assert 0 < r["fp"] and 0 < r["fn"] and r["threshold"] < r["score"]
    assert int((maps == np.float32(r["score"])).sum()) > 100                                            # the best score is a tie group
    _, _, counts = M.operating_point(_cuda(maps), r["threshold"], _cuda(masks))
    assert (counts["tp"], counts["fp"], counts["fn"]) == (r["tp"], r["fp"], r["fn"])
    _, _, at_score = M.operating_point(_cuda(maps), r["score"], _cuda(masks))                           # '>' at s* itself drops the group
    assert at_score["tp"] + at_score["fp"] < r["tp"] + r["fp"]
    prec, rec, thr, tp, fp = G.pr_ref(maps, masks)
    k = G.best_point(tp, fp)
    assert (r["tp"], r["fp"], r["score"]) == (int(tp[k]), int(fp[k]), float(thr[k]))
