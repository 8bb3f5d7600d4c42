"""GPU: the exact radix select (srad_select_kth / metrics.select_kth / metrics.map_threshold) against numpy: the value of
ascending rank k is ``np.sort(v)[k]`` (a zero comes back as +0.0), with the counts of values below and equal to it.  Every
comparison is exact.  No scipy or sklearn here."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_pro_golden", os.path.join(GOLDEN_DIR, "make_pro_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(x):
    return np.array([x], np.float32).view(np.uint32)[0]


def _check(v, vt, srt, k):
    """select_kth(vt, k) against the sorted copy ``srt`` of the float32 array ``v``."""
    from srad_amd import metrics as M
    got, below, equal = M.select_kth(vt, k)
    want = srt[k]
    if want == 0.0:
        assert _bits(got) == 0, (k, got)                                    # +0.0, never -0.0
    else:
        assert _bits(got) == _bits(want), (k, got, want)
    lo, hi = np.searchsorted(srt, want, "left"), np.searchsorted(srt, want, "right")
    assert (below, equal) == (int(lo), int(hi - lo)), (k, got, below, equal, lo, hi)
    assert below <= k < below + equal


def _hashed_ranks(n, salt, count=5):
    return sorted({(salt * 2654435761 + j * 40503 * 7919) % n for j in range(count)})


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 8191, 8192, 8193, 3 * 8192 + 17, 78 * 64 * 64])
def test_lengths_and_ranks(n):
    rng = np.random.RandomState(n % 9973)
    v = (np.round(rng.rand(n) * 64) / 64).astype(np.float32)               # ties: 65 levels ...
    wild = rng.rand(n) < 0.3
    v[wild] = rng.randn(int(wild.sum())).astype(np.float32)                # ... and distinct values of both signs
    z = rng.rand(n) < 0.2
    v[z] = np.where(rng.rand(int(z.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    vt, srt = _cuda(v), np.sort(v)
    for k in sorted({0, n - 1, n // 2, *_hashed_ranks(n, n)}):
        _check(v, vt, srt, k)


def _structure_cases():
    rng = np.random.RandomState(5)
    out = {}
    out["all_equal"] = np.full(4096, 0.375, np.float32)
    last = (1.0 + np.arange(1024) * 2.0 ** -23).astype(np.float32)          # one exponent, top 13 mantissa bits equal:
    out["last_pass_decides"] = rng.permutation(np.tile(last, 4))            # only the low 10 key bits differ
    e = np.arange(-126, 128)
    p2 = np.concatenate([np.ldexp(1.0, e), -np.ldexp(1.0, e)]).astype(np.float32)   # distinct in the top 9 key bits
    out["first_pass_decides"] = rng.permutation(np.tile(p2, 5))
    tiny = np.array([1, 2, 3, 0x7FFFFF, 0x400000], np.uint32)
    sub = np.concatenate([tiny, tiny | np.uint32(0x80000000)]).view(np.float32)     # subnormals of both signs
    mix = np.concatenate([-rng.rand(900).astype(np.float32) * 1e3, rng.randn(900).astype(np.float32), np.tile(sub, 20),
                          np.full(150, 0.0, np.float32), np.full(150, -0.0, np.float32),
                          np.full(7, np.inf, np.float32), np.full(9, -np.inf, np.float32),
                          np.array([np.finfo(np.float32).max, np.finfo(np.float32).min, np.finfo(np.float32).tiny], np.float32)])
    out["mixed_signs_zeros_subnormals_inf"] = rng.permutation(mix)
    return out


@pytest.mark.parametrize("case", ["all_equal", "last_pass_decides", "first_pass_decides", "mixed_signs_zeros_subnormals_inf"])
def test_key_structure(case):
    v = _structure_cases()[case]
    n = len(v)
    vt, srt = _cuda(v), np.sort(v)
    ranks = {0, 1, n // 2, n - 2, n - 1, *_hashed_ranks(n, 17, 12)}
    if case == "mixed_signs_zeros_subnormals_inf":                          # the ends of the -inf, zero and +inf groups too
        for val in (-np.inf, 0.0, np.inf):
            lo, hi = int(np.searchsorted(srt, val, "left")), int(np.searchsorted(srt, val, "right"))
            ranks |= {max(lo - 1, 0), lo, hi - 1, min(hi, n - 1)}
    for k in sorted(ranks):
        _check(v, vt, srt, k)


def test_hashed_case_zero_group():
    G = _generator()
    s, _ = G.hashed_case(1, 64, 64, 3)
    v = s.ravel()
    vt, srt = _cuda(v), np.sort(v)
    lo, hi = int(np.searchsorted(srt, 0.0, "left")), int(np.searchsorted(srt, 0.0, "right"))
    assert hi - lo > 0.6 * len(v) and (np.signbit(v) & (v == 0)).any() and (~np.signbit(v) & (v == 0)).any()
    assert lo == 0 and hi < len(v)                                          # the scores are >= 0: nothing below the zeros here
    for k in (lo, hi - 1, hi):
        _check(v, vt, srt, k)
    w = v.copy()
    w[::5] -= np.float32(0.5)                                               # now values on both sides of the zero group
    wt, srt = _cuda(w), np.sort(w)
    lo, hi = int(np.searchsorted(srt, 0.0, "left")), int(np.searchsorted(srt, 0.0, "right"))
    assert 0 < lo < hi < len(w)
    for k in (lo - 1, lo, hi - 1, hi):
        _check(w, wt, srt, k)


def test_map_threshold_bounds_the_rate():
    from srad_amd import metrics as M
    G = _generator()
    s, m = G.hashed_case(2, 64, 64, 9)
    v = s[m == 0]
    vt = _cuda(v)
    for f in (0.01, 0.1, 0.3, 0.5, 0.999):
        t, achieved = M.map_threshold(vt, f)
        k = M.rank_for_rate(len(v), f)
        assert t == np.sort(v)[k] and t in v
        above = int((v > t).sum())
        assert above <= int(np.floor(f * len(v))) and abs(achieved - above / len(v)) <= 1e-12


def _raw(v, k):
    """srad_select_kth straight from the C entry point: (value bits, [n_nan, n_below, n_equal])."""
    from srad_amd import _lib as L
    from srad_amd import metrics as M
    vt = _cuda(v)
    value = torch.empty((), dtype=torch.float32, device="cuda")
    counts = torch.empty(3, dtype=torch.int64, device="cuda")
    nb = C.c_size_t()
    L.check(L.lib().srad_select_kth_workspace_bytes(C.c_int64(len(v)), C.byref(nb)))
    keep, wp, wb = M._ws_buffer(nb.value, vt.device)
    L.check(L.lib().srad_select_kth(L.dptr(vt), C.c_int64(len(v)), C.c_int64(k), L.dptr(value), L.dptr(counts), wp, wb,
                                    L.current_stream_ptr()))
    return int(value.cpu().numpy().view(np.uint32)), counts.tolist()


def test_nan_is_counted_and_refused():
    from srad_amd import metrics as M
    rng = np.random.RandomState(2)
    v = rng.rand(3000).astype(np.float32)
    v[[5, 77, 2999]] = np.nan
    v.view(np.uint32)[100] = 0xFFC00001                                     # a NaN with the sign bit and a payload
    clean = np.sort(v[~np.isnan(v)])
    bits, (n_nan, below, equal) = _raw(v, 1500)                             # NaN sort last: the finite ranks are unchanged
    lo, hi = int(np.searchsorted(clean, clean[1500], "left")), int(np.searchsorted(clean, clean[1500], "right"))
    assert n_nan == 4 and bits == _bits(clean[1500]) and (below, equal) == (lo, hi - lo)
    bits, (n_nan, below, equal) = _raw(v, 2998)                             # a rank among the NaN: the value is NaN
    assert n_nan == 4 and np.isnan(np.array([bits], np.uint32).view(np.float32)[0]) and (below, equal) == (2996, 0)
    with pytest.raises(ValueError, match="NaN"):
        M.select_kth(_cuda(v), 10)
    with pytest.raises(ValueError, match="NaN"):
        M.map_threshold(_cuda(v), 0.1)
    with pytest.raises(ValueError, match="rank"):
        M.select_kth(_cuda(clean), len(clean))
    with pytest.raises(ValueError):
        M.select_kth(_cuda(clean[:0]), 0)


def test_same_bits_on_every_call():
    G = _generator()
    s, _ = G.hashed_case(3, 96, 80, 5)
    v = s.ravel()
    for k in (0, len(v) // 3, int(0.8 * len(v)), len(v) - 1):
        assert _raw(v, k) == _raw(v, k)
