"""CPU: the cases of tests/test_gpu_score_paths.py can fail.  On their images a group of window sizes written to shifted
columns misses the oracle by far more than the 2e-6 bar, and so does an image written to its neighbour's slot across a chunk
boundary; numpy's "symmetric" padding instead of "reflect" moves the oracle far beyond the bar on at least one case of every
sweep kernel (the border handling is exercised); and the shapes take the sweep paths the cases name (``srad_score_plan``, a
host query)."""
import warnings

import numpy as np
import pytest

from oracle import scorer_ref as O
from tests.test_gpu_score_paths import (CASE_BY_NAME, CASES, CHUNK_CASES, SSIM_BAR, WS_GROUP, case_oracle, case_pairs,
                                        chunk_boundary_images, chunk_pair, oracle_ssim_of, plan_coverage)

SHIFT_GAP = 10 * SSIM_BAR


def test_cases_take_the_paths_they_name():
    from srad_amd import metrics as M
    for c in CASES:
        assert M.score_plan(c.n, c.H, c.W) == (c.kernel, c.n), c.name
    for cc in CHUNK_CASES:
        assert M.score_plan(cc.n, cc.H, cc.W) == (cc.kernel, cc.chunk), cc.name
    assert plan_coverage() == ({0, 1, 2}, 7, 2)
    with pytest.raises(RuntimeError, match="score_plan"):
        M.score_plan(0, 64, 64)


def _shift_gaps(v, windows):
    """For each launch group of ``windows`` (16 consecutive list entries) and each shift of one column to either side: the largest
    |oracle change| over the group's columns and the images, i.e. what a group written one column off would miss the oracle by.
    Also each later group against the columns of the first (a group written from column 0)."""
    n_ws = len(windows)
    out = []
    for g0 in range(0, n_ws, WS_GROUP):
        cols = range(g0, min(n_ws, g0 + WS_GROUP))
        for s in (-1, 1):
            d = [np.abs(v[:, j] - v[:, j + s]).max() for j in cols if 0 <= j + s < n_ws and windows[j] != windows[j + s]]
            if d:
                out.append(max(d))
        if g0 > 0:
            out.append(max(np.abs(v[:, j] - v[:, j - g0]).max() for j in cols))
    return out


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_shifted_window_groups_miss_the_oracle(name):
    """A window group written to shifted columns changes some (image, window) value by far more than the 2e-6 bar.  (Single
    neighbouring windows can score close where the SSIM-versus-window curve turns, so the guard is per group.)"""
    c = CASE_BY_NAME[name]
    keep = [k for k in range(c.n) if k not in c.identical]
    gaps = _shift_gaps(case_oracle(name)[keep], c.windows)
    print(f"{name}: smallest change of a shifted group {min(gaps):.2e}")
    assert min(gaps) > SHIFT_GAP, (name, gaps)


@pytest.mark.parametrize("cc", CHUNK_CASES, ids=[cc.name for cc in CHUNK_CASES])
def test_chunk_images_score_far_apart(cc):
    """The oracle columns of the chunk cases differ between the checked windows and between the images on either side of a
    chunk boundary: rows written to another image's slot or columns of another group cannot pass."""
    vals = {}
    for k in chunk_boundary_images(cc):
        sr, hr = chunk_pair(cc, k)
        vals[k] = np.array([oracle_ssim_of(sr, hr, cc.windows[j]) for j in cc.cols])
        assert np.abs(np.diff(vals[k])).min() > SHIFT_GAP, (cc.name, k, vals[k])
    ks = sorted(vals)
    for a, b in zip(ks, ks[1:]):
        assert np.abs(vals[a] - vals[b]).max() > SHIFT_GAP, (cc.name, a, b)


def _box_symmetric(x, ws):
    pad = ws // 2
    xp = np.pad(x.astype(np.float64), ((pad, pad), (pad, pad)), mode="symmetric")
    sat = np.zeros((xp.shape[0] + 1, xp.shape[1] + 1), dtype=np.float64)
    sat[1:, 1:] = xp.cumsum(0).cumsum(1)
    h, w = x.shape
    s = sat[ws:ws + h, ws:ws + w] - sat[:h, ws:ws + w] - sat[ws:ws + h, :w] + sat[:h, :w]
    return (s / float(ws * ws)).astype(np.float32)


def test_symmetric_padding_misses_the_bar_on_every_kernel(monkeypatch):
    """The oracle with "symmetric" padding (the edge sample repeated) differs from the real one by more than 100 x the SSIM bar on
    at least one case per sweep kernel."""
    worst = {}
    for c in CASES:
        if c.H * c.W > 1 << 18:
            continue
        sr, hr = case_pairs(c.name)
        ref = case_oracle(c.name)
        with monkeypatch.context() as m:
            m.setattr(O, "_box_fast", _box_symmetric)
            sym = np.array([[oracle_ssim_of(sr[k], hr[k], ws) for ws in c.windows] for k in range(c.n)])
        worst[c.kernel] = max(worst.get(c.kernel, 0.0), float(np.abs(sym - ref).max()))
    print(f"max |symmetric - reflect| per kernel: {worst}")
    assert set(worst) == {0, 1, 2} and min(worst.values()) > 100 * SSIM_BAR, worst


def test_val_oracle_has_no_value_when_the_shave_leaves_no_row():
    """W > 8, H <= 8: the reference shaves every row away; its PSNR is NaN and its SSIM raises (metrics.val_metrics refuses)."""
    rng = np.random.RandomState(0)
    s, h = (rng.uniform(0, 255, (1, 1, 8, 20)).astype(np.float32) for _ in range(2))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert np.isnan(O.psnr_torch_ref(s, h, 255.0))
    with pytest.raises(RuntimeError):
        O.ssim_torch_ref(s, h, 255.0)
    assert np.isfinite(O.psnr_torch_ref(s[:, :, :, :8], h[:, :, :, :8], 255.0))      # W = 8: no shave
