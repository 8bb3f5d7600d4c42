"""GPU: every path of the SSIM window sweep (srad_score_pairs, csrc/kernels_score.hip) against the oracle.

The host picks the sweep's evaluation kernel from the image shape (``metrics.score_plan``): the LDS sweep for power-of-two
widths 64..1024, the corner kernel with per-row waves for other multiples of 64 (and widths above 1024), the kernel for any
width otherwise.  Window sizes run in launches of up to 16 (``kWsGroup``), each writing its own columns, and the images in
chunks of 2^25 table points.  Each case below asserts the path it expects and compares every column with ``O.ssim_numpy`` on
structured non-square images (a smooth field, different content near each border, noise and planted defects).  The same shapes
go through the per-pixel anomaly maps, and the validation metrics through the shave and padding edges.

Bars are those of tests/test_gpu_scorer.py: SSIM 2e-6 absolute per (image, window size), MSE 1e-9 against a numpy fp32
restatement, PSNR 1e-5 (inf for identical images).  Every comparison prints its measured maximum."""
import functools
from typing import NamedTuple, Tuple

import numpy as np
import pytest
import torch

from oracle import scorer_ref as O

pytestmark = pytest.mark.gpu

SSIM_BAR, MSE_BAR, PSNR_BAR = 2e-6, 1e-9, 1e-5
WS_GROUP = 16                                     # window sizes per sweep launch (kWsGroup)


# ------------------------------------------------------------------ inputs
def make_pair(H: int, W: int, C: int = 1, seed: int = 0, defects: int = 3, identical: bool = False
              ) -> Tuple[np.ndarray, np.ndarray]:
    """One structured (sr, hr) u8 pair, each [H, W, C]: a smooth gradient / sine field with different content in a band along
    each border (stripes at the top, dots at the bottom, ripples on the left, a checkerboard contrast on the right), noise, and
    in SR a smooth contrast and brightness drift, more noise, a brightened bottom band, a darkened left band and ``defects`` planted rectangles, the first one in a
    corner.  ``identical`` returns SR = HR."""
    rng = np.random.RandomState(seed)
    yv = np.arange(H, dtype=np.float64)[:, None] / max(H - 1, 1)
    xv = np.arange(W, dtype=np.float64)[None, :] / max(W - 1, 1)
    f0, f1 = rng.uniform(1.0, 3.0, 2)
    base = np.broadcast_to(70 + 80 * yv + 50 * xv * (1 - yv) + 25 * np.sin(2 * np.pi * (f0 * xv + f1 * yv * yv)), (H, W)).copy()
    ii, jj = np.arange(H)[:, None], np.arange(W)[None, :]
    b = max(1, min(H, W) // 8)
    base[:b, :] += 30 * ((jj // 2) % 2)
    base[-b:, :] -= 25 * ((ii[-b:] + jj) % 3 == 0)
    base[:, :b] += 20 * np.cos(ii / 1.7)
    base[:, -b:] *= 0.8 + 0.4 * ((ii // 3 + jj[:, -b:] // 3) % 2)
    hr = base[:, :, None] + np.array([0.0, 12.0, -9.0])[:C] + rng.normal(0, 5, (H, W, C))
    gain = (1.0 + 0.25 * xv * yv)[:, :, None]                                   # contrast and brightness drift over the image
    sr = hr.mean() + (hr - hr.mean()) * gain + (14 * (yv - 0.5) + 10 * np.cos(3 * np.pi * xv))[:, :, None] \
        + rng.normal(0, 3, (H, W, C))
    sr[-b:] += 6
    sr[:, :b] *= 0.95
    for d in range(defects):
        h, w = rng.randint(1, max(1, H // 6) + 1), rng.randint(1, max(1, W // 6) + 1)
        if d == 0:
            y0, x0 = (0 if rng.rand() < 0.5 else H - h), (0 if rng.rand() < 0.5 else W - w)
        else:
            y0, x0 = rng.randint(0, H - h + 1), rng.randint(0, W - w + 1)
        sr[y0:y0 + h, x0:x0 + w] += (1 if rng.rand() < 0.5 else -1) * rng.uniform(25, 60)
    to_u8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)       # noqa: E731
    hr = to_u8(hr)
    return (hr.copy() if identical else to_u8(sr)), hr


def make_pairs(n: int, H: int, W: int, C: int = 1, seed: int = 0, identical=()) -> Tuple[np.ndarray, np.ndarray]:
    """n pairs of ``make_pair`` (image k from seed 1000 * seed + k) stacked to [n, H, W, C]; images in ``identical`` have SR = HR."""
    pairs = [make_pair(H, W, C, 1000 * seed + k, identical=k in identical) for k in range(n)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def f32(u8: np.ndarray) -> np.ndarray:
    return u8.astype(np.float32) / 255.0


def oracle_ssim_of(sr: np.ndarray, hr: np.ndarray, ws: int) -> float:
    """ssim_numpy(hr / 255, sr / 255, ws) as the evaluator calls it."""
    return O.ssim_numpy(f32(hr), f32(sr), ws)


def mse_ref(sr: np.ndarray, hr: np.ndarray) -> float:
    return float(np.mean((f32(sr) - f32(hr)) ** 2))


# ------------------------------------------------------------------ the cases
class Case(NamedTuple):
    name: str
    H: int
    W: int
    C: int
    n: int
    windows: tuple
    kernel: int              # metrics.score_plan's kernel: 0 LDS sweep, 1 corner kernel, 2 any width
    identical: tuple = ()    # images with SR = HR
    seed: int = 0


def _odd(lo, hi, step=2):
    return tuple(range(lo, hi + 1, step))


def _sweep(m, *extra):
    return tuple(O.sweep_window_sizes(m)) + tuple(extra)


CASES = [
    # LDS sweep: at W = 64 a workgroup covers 16 rows, so H = 2 and 20 leave a block partly empty; H = 1000 a partial last one
    Case("lds_2x64", 2, 64, 1, 3, (1, 2, 3), 0, seed=1),
    Case("lds_20x64_rgb", 20, 64, 3, 2, _odd(1, 39), 0, seed=2),
    Case("lds_1000x64", 1000, 64, 1, 2, (1, 3, 5, 11, 21, 31, 41, 51, 61, 63, 64, 65, 80, 100, 126, 127), 0, seed=3),
    Case("lds_256x256", 256, 256, 1, 3, _sweep(256), 0, identical=(2,), seed=4),
    Case("lds_96x256", 96, 256, 1, 2, _odd(1, 187, 6) + (191,), 0, seed=5),
    Case("lds_33x1024", 33, 1024, 1, 2, _odd(1, 65, 4), 0, seed=6),
    Case("lds_1024x1024", 1024, 1024, 1, 1, _sweep(1024), 0, seed=7),
    # corner kernel: multiples of 64 that are not a power of two, and W > 1024
    Case("rows_192x192", 192, 192, 1, 2, _sweep(192, 1, 383), 1, seed=8),
    Case("rows_320x192_rgb", 320, 192, 3, 2, (1, 3, 7, 11, 21, 41, 61, 81, 101, 121, 151, 181, 191, 193, 255, 321, 383), 1,
         identical=(1,), seed=9),
    Case("rows_32x320", 32, 320, 1, 2, _odd(1, 63, 4), 1, seed=10),
    Case("rows_128x1536", 128, 1536, 1, 1, (1, 3, 11, 33, 65, 127, 129, 255), 1, seed=11),
    # any width (256 x 96 is the transpose of lds_96x256)
    Case("any_256x96", 256, 96, 1, 2, _odd(1, 187, 6) + (191,), 2, seed=5),
    Case("any_65x65", 65, 65, 1, 3, _odd(1, 129, 8), 2, identical=(1,), seed=12),
    Case("any_200x127_rgb", 200, 127, 3, 2, _sweep(127, 1, 127, 253), 2, seed=13),
    Case("any_31x1000", 31, 1000, 1, 2, _odd(1, 61, 4), 2, seed=14),
]
CASE_BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def case_pairs(name: str) -> Tuple[np.ndarray, np.ndarray]:
    c = CASE_BY_NAME[name]
    if name == "any_256x96":                     # the transposed images of lds_96x256
        sr, hr = case_pairs("lds_96x256")
        return np.ascontiguousarray(sr.transpose(0, 2, 1, 3)), np.ascontiguousarray(hr.transpose(0, 2, 1, 3))
    return make_pairs(c.n, c.H, c.W, c.C, c.seed, c.identical)


@functools.lru_cache(maxsize=None)
def case_oracle(name: str) -> np.ndarray:
    """[n, len(windows)] oracle SSIM of a case."""
    c = CASE_BY_NAME[name]
    sr, hr = case_pairs(name)
    return np.array([[oracle_ssim_of(sr[k], hr[k], ws) for ws in c.windows] for k in range(c.n)])


class ChunkCase(NamedTuple):
    name: str
    n: int
    H: int
    W: int
    kernel: int
    chunk: int
    windows: tuple
    cols: tuple              # columns compared with the oracle, from both window groups
    seed: int


CHUNK_CASES = [
    ChunkCase("chunk_1024", 33, 1024, 1024, 0, 31, (1,) + tuple(O.sweep_window_sizes(1024)[::6]), (1, 9, 16), 20),
    ChunkCase("chunk_2048", 9, 2048, 2048, 1, 7, (1,) + tuple(O.sweep_window_sizes(2048)[::12]), (1, 9, 17), 21),
]


def chunk_boundary_images(cc: ChunkCase):
    """The images on either side of each chunk boundary, and the last one."""
    ks = set()
    for b in range(cc.chunk, cc.n, cc.chunk):
        ks |= {b - 1, b}
    return sorted(ks | {cc.n - 1})


def chunk_pair(cc: ChunkCase, k: int) -> Tuple[np.ndarray, np.ndarray]:
    return make_pair(cc.H, cc.W, 1, 1000 * cc.seed + k)


def plan_coverage():
    """(kernels, most window groups, most chunks) the case tables reach, from their sizes and score_plan."""
    from srad_amd import metrics as M
    kernels, groups, chunks = set(), 0, 0
    for c in CASES:
        k, ch = M.score_plan(c.n, c.H, c.W)
        kernels.add(k)
        groups = max(groups, -(-len(c.windows) // WS_GROUP))
        chunks = max(chunks, -(-c.n // ch))
    for cc in CHUNK_CASES:
        k, ch = M.score_plan(cc.n, cc.H, cc.W)
        kernels.add(k)
        groups = max(groups, -(-len(cc.windows) // WS_GROUP))
        chunks = max(chunks, -(-cc.n // ch))
    return kernels, groups, chunks


# ------------------------------------------------------------------ GPU helpers
def _score(sr: np.ndarray, hr: np.ndarray, windows):
    from srad_amd import metrics as M
    s, m, p = M.score_pairs(torch.from_numpy(np.ascontiguousarray(sr)).cuda(), torch.from_numpy(np.ascontiguousarray(hr)).cuda(),
                            list(windows))
    return s.cpu().numpy(), m.cpu().numpy(), p.cpu().numpy()


def _check_mse_psnr(tag, sr, hr, mse, psnr):
    ref_mse = np.array([mse_ref(s, h) for s, h in zip(sr, hr)])
    ref_psnr = np.array([O.psnr_numpy(f32(h), f32(s)) for s, h in zip(sr, hr)])
    d_mse = float(np.abs(mse - ref_mse).max())
    fin = np.isfinite(ref_psnr)
    assert np.array_equal(np.isinf(psnr), ~fin), (tag, psnr, ref_psnr)
    d_psnr = float(np.abs(psnr[fin] - ref_psnr[fin]).max()) if fin.any() else 0.0
    print(f"{tag}: max |mse - ref| {d_mse:.2e}, max |psnr - ref| {d_psnr:.2e}, identical pairs {int((~fin).sum())}")
    assert d_mse < MSE_BAR and d_psnr < PSNR_BAR, (tag, d_mse, d_psnr)


# ------------------------------------------------------------------ the sweep, case by case
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_sweep_matches_oracle(name):
    from srad_amd import metrics as M
    c = CASE_BY_NAME[name]
    assert M.score_plan(c.n, c.H, c.W) == (c.kernel, c.n), (name, M.score_plan(c.n, c.H, c.W))
    sr, hr = case_pairs(name)
    ssim, mse, psnr = _score(sr, hr, c.windows)
    assert ssim.shape == (c.n, len(c.windows))
    ref = case_oracle(name)
    d = np.abs(ssim - ref)
    worst = np.unravel_index(np.argmax(d), d.shape)
    print(f"{name} ({M.SCORE_KERNELS[c.kernel]}, {len(c.windows)} windows in {-(-len(c.windows) // WS_GROUP)} groups): "
          f"max |ssim - oracle| {d.max():.2e} at image {worst[0]}, ws {c.windows[worst[1]]}")
    assert d.max() < SSIM_BAR, (name, d.max(), worst)
    for k in c.identical:
        assert np.all(np.abs(ssim[k] - 1.0) < 1e-12), (name, k)
    _check_mse_psnr(name, sr, hr, mse, psnr)


@pytest.mark.parametrize("name", ["lds_96x256", "rows_192x192", "any_65x65"])
def test_window_order_and_duplicates_do_not_matter(name):
    """An unsorted window list with duplicates scores each window to the same bits as the sorted list: the LDS sweep derives its
    first table row and row ranges from each group's smallest and largest pad, and a window's arithmetic is the same in any group."""
    c = CASE_BY_NAME[name]
    sr, hr = case_pairs(name)
    shuffled = list(c.windows) + [c.windows[2], c.windows[-1]]
    np.random.RandomState(7).shuffle(shuffled)
    srt = sorted(set(shuffled))
    assert shuffled != sorted(shuffled) and len(shuffled) > WS_GROUP
    a, ma, pa = _score(sr, hr, shuffled)
    b, mb, pb = _score(sr, hr, srt)
    moved = sum(j // WS_GROUP != srt.index(w) // WS_GROUP for j, w in enumerate(shuffled))
    print(f"{name}: {len(shuffled)} windows, {moved} of them in another group than in the sorted list")
    for j, w in enumerate(shuffled):
        assert np.array_equal(a[:, j], b[:, srt.index(w)]), (name, j, w, a[:, j], b[:, srt.index(w)])
    assert np.array_equal(ma, mb) and np.array_equal(pa, pb)


def test_transposed_pair_lds_sweep_vs_any_width_kernel():
    """SSIM does not change when both images are transposed: 96 x 256 runs the LDS sweep, 256 x 96 the kernel for any width.  The
    LDS sweep rounds each map value to a multiple of 2^-24 before its exact integer sum; the difference stays far below the bar."""
    a, b = CASE_BY_NAME["lds_96x256"], CASE_BY_NAME["any_256x96"]
    assert a.windows == b.windows
    sa, _, _ = _score(*case_pairs(a.name), a.windows)
    sb, _, _ = _score(*case_pairs(b.name), b.windows)
    d = float(np.abs(sa - sb).max())
    print(f"LDS sweep 96x256 vs any-width kernel 256x96: max |difference| {d:.2e}")
    assert d < SSIM_BAR


# ------------------------------------------------------------------ image chunks
@pytest.mark.parametrize("cc", CHUNK_CASES, ids=[cc.name for cc in CHUNK_CASES])
def test_chunks_match_single_images_and_oracle(cc):
    """More images than one summed-area table chunk holds: every image scores the same bits as alone, the images on either
    side of each chunk boundary match the oracle at windows of both groups, and every MSE matches numpy."""
    from srad_amd import metrics as M
    assert M.score_plan(cc.n, cc.H, cc.W) == (cc.kernel, cc.chunk)
    assert M.score_plan(1, cc.H, cc.W) == (cc.kernel, 1)
    assert len(cc.windows) > WS_GROUP and {j // WS_GROUP for j in cc.cols} == {0, 1}
    pairs = [chunk_pair(cc, k) for k in range(cc.n)]
    sr = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    hr = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    ssim, mse, psnr = (t.cpu().numpy() for t in M.score_pairs(sr, hr, list(cc.windows)))
    for k in range(cc.n):
        one = [t.cpu().numpy() for t in M.score_pairs(sr[k:k + 1], hr[k:k + 1], list(cc.windows))]
        assert np.array_equal(one[0][0], ssim[k]) and one[1][0] == mse[k] and one[2][0] == psnr[k], (cc.name, k)
    worst = 0.0
    for k in chunk_boundary_images(cc):
        for j in cc.cols:
            ref = oracle_ssim_of(pairs[k][0], pairs[k][1], cc.windows[j])
            worst = max(worst, abs(ssim[k, j] - ref))
            assert abs(ssim[k, j] - ref) < SSIM_BAR, (cc.name, k, cc.windows[j], ssim[k, j], ref)
    print(f"{cc.name}: {cc.n} images in chunks of {cc.chunk}; max |ssim - oracle| {worst:.2e} at images "
          f"{chunk_boundary_images(cc)}, windows {[cc.windows[j] for j in cc.cols]}")
    _check_mse_psnr(cc.name, [p[0] for p in pairs], [p[1] for p in pairs], mse, psnr)


# ------------------------------------------------------------------ no windows, end to end
def test_empty_window_list_still_scores_mse_and_psnr():
    from srad_amd import metrics as M
    sr, hr = make_pairs(3, 40, 72, 3, seed=30, identical=(1,))
    s, m, p = M.score_pairs(torch.from_numpy(sr).cuda(), torch.from_numpy(hr).cuda(), [])
    assert tuple(s.shape) == (3, 0)
    _check_mse_psnr("no windows", sr, hr, m.cpu().numpy(), p.cpu().numpy())


def test_evaluate_pairs_non_square_vs_oracle():
    """The evaluator's whole sweep and three AUCs on a 192 x 320 test split (5 good, 7 bad pairs), as test_full_sweep_vs_oracle."""
    from srad_amd import metrics as M
    n_good, n_bad = 5, 7
    y = [0] * n_good + [1] * n_bad
    pairs = [make_pair(192, 320, 1, 40 + k, defects=0 if k < n_good else 3) for k in range(n_good + n_bad)]
    sr, hr = [p[0] for p in pairs], [p[1] for p in pairs]
    ref = O.evaluate_pairs(y, sr, hr)
    got = M.evaluate_pairs(y, torch.from_numpy(np.stack(sr)).cuda(), torch.from_numpy(np.stack(hr)).cuda())
    d_ssim = float(np.abs(np.array(got["scores_ssim"]) - np.array(ref["scores_ssim"])).max())
    d_mse = float(np.abs(np.array(got["scores_mse"]) - np.array(ref["scores_mse"])).max())
    d_sweep = float(np.abs(np.array(got["sweep_auc"]) - np.array(ref["sweep_auc"])).max())
    print(f"evaluate_pairs 192x320: best ws {got['best_ws']} (oracle {ref['best_ws']}), max |sweep auc| {d_sweep:.2e}, "
          f"max |ssim score| {d_ssim:.2e}, max |mse score| {d_mse:.2e}")
    assert got["window_sizes"] == ref["window_sizes"]
    assert got["best_ws"] == ref["best_ws"]
    assert d_sweep < 1e-12
    for k in ("auc_ssim", "auc_mse", "auc_psnr"):
        assert abs(got[k] - ref[k]) < 2e-3 and round(got[k], 3) == round(ref[k], 3), k
    assert d_ssim < 2e-6
    assert d_mse < 1e-9


# ------------------------------------------------------------------ anomaly maps at the same shapes
@pytest.mark.parametrize("H,W,C", [(192, 320, 1), (320, 192, 1), (65, 200, 1)])
def test_anomaly_maps_non_square(H, W, C):
    """Gray: the oracle's RGB luminance is a BLAS dot product whose rounding order is not fixed, and on these images a one-ulp
    luminance difference moves single ws = 3 map pixels by up to 1e-4 (RGB maps are compared at 64 px in test_gpu_anomaly_maps)."""
    from srad_amd import metrics as M
    from tests.test_gpu_anomaly_maps import map_oracle
    sr, hr = make_pairs(2, H, W, C, seed=50 + H)
    m = min(H, W)
    both = m + 3 if m % 2 == 0 else m + 2                   # the middle rows' windows hang over both edges of the short axis
    for ws in (1, 3, 11, O.sweep_window_sizes(m)[-1], both):
        got = M.anomaly_maps(torch.from_numpy(sr).cuda(), torch.from_numpy(hr).cuda(), ws).cpu().numpy()
        want = np.stack([map_oracle(s, h, ws) for s, h in zip(sr, hr)])
        d = np.abs(got.astype(np.float64) - want)
        print(f"anomaly maps {H}x{W}x{C} ws {ws}: mean |d| {d.mean():.2e}, max |d| {d.max():.2e}")
        assert d.mean() <= 1e-6 and d.max() <= 1e-4, (H, W, C, ws, d.mean(), d.max())


# ------------------------------------------------------------------ validation metrics
def _val_inputs(B, C, H, W, seed):
    """fp32 NCHW (sr, hr) on the 0..255 range, SR off the integer grid and a little outside the range (the SSIM clamps)."""
    sr, hr = make_pairs(B, H, W, C, seed=seed)
    rng = np.random.RandomState(seed)
    s = np.transpose(sr, (0, 3, 1, 2)).astype(np.float32) * np.float32(1.02) - np.float32(3.0) \
        + rng.normal(0, 0.7, (B, C, H, W)).astype(np.float32)
    h = np.transpose(hr, (0, 3, 1, 2)).astype(np.float32)
    return np.ascontiguousarray(s), np.ascontiguousarray(h)


@pytest.mark.parametrize("B,C,H,W", [(2, 3, 128, 96), (2, 1, 256, 256), (2, 1, 45, 31), (2, 1, 40, 8), (2, 1, 40, 9),
                                     (1, 3, 9, 20)])
def test_val_metrics_shapes(B, C, H, W):
    """Trainer.test's PSNR / SSIM: the 4-px shave applies when the WIDTH is above 8 (W = 8 keeps every pixel, W = 9 one column;
    H = 9 one row), zero padding around what is left."""
    from srad_amd import metrics as M
    s, h = _val_inputs(B, C, H, W, seed=60 + H + W)
    psnr, ssim = (t.cpu().numpy() for t in M.val_metrics(torch.from_numpy(s).cuda(), torch.from_numpy(h).cuda(), 255.0))
    rp = np.array([O.psnr_torch_ref(s[k:k + 1], h[k:k + 1], 255.0) for k in range(B)])
    rs = np.array([O.ssim_torch_ref(s[k:k + 1], h[k:k + 1], 255.0) for k in range(B)])
    dp, ds = float(np.abs(psnr - rp).max()), float(np.abs(ssim - rs).max())
    print(f"val metrics {B}x{C}x{H}x{W}: max |psnr - ref| {dp:.2e}, max |ssim - ref| {ds:.2e}")
    assert dp < 1e-4 and ds < 1e-6, (dp, ds)


@pytest.mark.parametrize("H,W", [(8, 20), (5, 9), (1, 30)])
def test_val_metrics_refuses_rows_shaved_away(H, W):
    """W > 8 and H <= 8: the shave leaves no row; the reference's PSNR is NaN and its SSIM raises, so the kernel refuses."""
    from srad_amd import metrics as M
    s, h = _val_inputs(1, 1, H, W, seed=70)
    with pytest.raises(RuntimeError, match="no rows left"):
        M.val_metrics(torch.from_numpy(s).cuda(), torch.from_numpy(h).cuda(), 255.0)


# ------------------------------------------------------------------ coverage of the cases above
def test_cases_reach_every_sweep_path():
    kernels, groups, chunks = plan_coverage()
    print(f"sweep paths reached: kernels {sorted(kernels)}, up to {groups} window groups, up to {chunks} chunks")
    assert kernels == {0, 1, 2} and groups > 1 and chunks > 1
