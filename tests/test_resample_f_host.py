"""CPU: the host half of the float32 resize (csrc/resample_coeffs_f.h behind srad_resample_ksize_f64 / srad_resample_coeffs_f64).
The library's double tables against an independent numpy restatement of Pillow's precompute_coeffs, on the bits; a pure-numpy
two-pass resize driven by the library's tables - sequential fp64 products and sums, rounded to float32 after each pass -
against ``Image.fromarray(a, mode='F').resize`` itself, compared as uint32; the argument errors of the three entry points
(srad_resize_f32 checks everything before it touches a device; the float functions take BILINEAR, the 8-bit ones keep refusing
it); and tests/host/resample_f_check.cpp, a stand-alone program that includes only the header, built with AddressSanitizer and
UndefinedBehaviorSanitizer (linked statically, nothing is preloaded) and run once.  Every comparison is an equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from tests.test_resample_host import _filter as _filter_u8
from tests.test_wgrad_queue_host import SANITIZE, _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "resample_f_check.cpp")
PAIRS = [(8, 20), (8, 31), (16, 5), (24, 7), (32, 70), (32, 300), (32, 257), (1024, 128), (5, 1), (1, 9), (7, 7)]
FILTERS = {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}
SHAPES = [((8, 8), (20, 31)), ((16, 24), (5, 7)), ((32, 32), (32, 70)), ((7, 9), (7, 9)), ((32, 32), (300, 257))]      # (H, W) -> (h, w)
SRAD_ERR_ARG = 1


def _filter(name, x):
    if name == "bilinear":
        x = np.abs(x)
        return np.where(x < 1.0, 1.0 - x, 0.0), 1.0
    return _filter_u8(name, x)


def numpy_coeffs_f(in_size, out_size, name):
    """Pillow's precompute_coeffs restated with numpy (float64 throughout): the taps divided by their sum, nothing else."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = _filter(name, np.zeros(1))[1] * fs
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coeffs = np.zeros((out_size, ksize), dtype=np.float64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = _filter(name, (np.arange(xmax) + xmin - center + 0.5) * (1.0 / fs))[0]
        ww = 0.0
        for v in w:                                           # the sum in index order, as the C loop
            ww += float(v)
        if ww != 0.0:
            w = w / ww
        coeffs[xx, :xmax] = w
        bounds[xx] = xmin, xmax
    return ksize, bounds, coeffs


def numpy_pass_f(a, axis, bounds, coeffs):
    """One pass along ``axis`` of the float32 array ``a`` [H,W]: per output one fp64 accumulator, the taps in index order, every
    product and every sum rounded on its own (numpy never fuses them), the result rounded to float32."""
    a = np.moveaxis(a, axis, 0).astype(np.float64)
    out = np.empty((len(bounds),) + a.shape[1:], dtype=np.float32)
    for xx, (xmin, xmax) in enumerate(bounds):
        ss = np.zeros(a.shape[1:], dtype=np.float64)
        for x in range(xmax):
            ss = ss + a[xmin + x] * coeffs[xx, x]
        out[xx] = ss.astype(np.float32)
    return np.moveaxis(out, 0, axis)


def numpy_resize_f(a, h, w, name):
    """``a`` float32 [H,W] -> [h,w] with the LIBRARY's tables: horizontal first, rounded to float32, then vertical; equal sizes skip."""
    from srad_amd import ops
    if a.shape[1] != w:
        a = numpy_pass_f(a, 1, *ops.resample_coeffs_f64(a.shape[1], w, name)[1:])
    if a.shape[0] != h:
        a = numpy_pass_f(a, 0, *ops.resample_coeffs_f64(a.shape[0], h, name)[1:])
    return a


def maps_f(shape, seed=0):
    """float32 [H,W] in about [-1, 1] with negative values, and values of magnitude 1e-6 on every third pixel."""
    rng = np.random.RandomState(seed)
    a = rng.uniform(-1.0, 1.0, shape)
    small = rng.uniform(-2e-6, 2e-6, shape)
    return np.where(np.arange(a.size).reshape(shape) % 3 == 0, small, a).astype(np.float32)


def pil_resize_f(a, h, w, name):
    """Pillow's mode-F resize of a float32 [H,W] map (a float32 array becomes a mode-F image)."""
    im = Image.fromarray(np.ascontiguousarray(a, dtype=np.float32))
    assert im.mode == "F"
    return np.asarray(im.resize((w, h), FILTERS[name]))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(FILTERS))
def test_library_tables_equal_the_numpy_restatement(name):
    from srad_amd import ops
    for in_size, out_size in PAIRS:
        ksize, bounds, coeffs = ops.resample_coeffs_f64(in_size, out_size, name)
        k2, b2, c2 = numpy_coeffs_f(in_size, out_size, name)
        assert ksize == k2 and coeffs.shape == (out_size, ksize) and coeffs.dtype == np.float64, (in_size, out_size)
        assert np.array_equal(bounds, b2), (in_size, out_size)
        assert np.array_equal(coeffs.view(np.uint64), c2.view(np.uint64)), (in_size, out_size, float(np.abs(coeffs - c2).max()))
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 0] + bounds[:, 1] <= in_size).all() and (bounds[:, 1] <= ksize).all()
        if name == "bilinear":
            assert (coeffs >= 0.0).all()                      # what keeps a resized map inside the range of its source


@pytest.mark.parametrize("name", sorted(FILTERS))
def test_resize_with_library_tables_equals_pil(name):
    for (H, W), (h, w) in SHAPES:
        a = maps_f((H, W), seed=H + w)
        assert (a < 0).any() and ((np.abs(a) < 3e-6) & (a != 0)).any()
        got, ref = numpy_resize_f(a, h, w, name), pil_resize_f(a, h, w, name)
        assert got.shape == ref.shape == (h, w) and got.dtype == ref.dtype == np.float32
        assert np.array_equal(bits(got), bits(ref)), (H, W, h, w, int((bits(got) != bits(ref)).sum()))


def test_argument_errors_without_gpu():
    from srad_amd import _lib as L, ops
    lib = L.lib()
    k = C.c_int(-1)
    assert lib.srad_resample_ksize_f64(1024, 128, 0, C.byref(k)) == 0 and k.value == 49
    assert lib.srad_resample_ksize_f64(40, 57, 1, C.byref(k)) == 0 and k.value == 5
    assert lib.srad_resample_ksize_f64(40, 57, 2, C.byref(k)) == 0 and k.value == 3          # BILINEAR is known here ...
    assert lib.srad_resample_ksize_f64(128, 32, 2, C.byref(k)) == 0 and k.value == 9
    assert lib.srad_resample_ksize(40, 57, 2, C.byref(k)) == SRAD_ERR_ARG and b"unknown filter" in lib.srad_last_error()      # ... and only here
    for args, text in (((0, 4, 2), b"not supported"), ((4, 0, 2), b"not supported"), ((4, 4, 3), b"unknown filter"), ((4, 4, -1), b"unknown filter"),
                       (((1 << 20) + 1, 4, 2), b"not supported")):
        k.value = -1
        assert lib.srad_resample_ksize_f64(*args, C.byref(k)) == SRAD_ERR_ARG and text in lib.srad_last_error() and k.value == -1, args
    assert lib.srad_resample_ksize_f64(4, 4, 2, None) == SRAD_ERR_ARG and b"null argument" in lib.srad_last_error()
    b, c = np.zeros((4, 2), np.int32), np.full((4, 5), 7.0)
    assert lib.srad_resample_coeffs_f64(8, 4, 2, None, c.ctypes.data) == SRAD_ERR_ARG and b"null argument" in lib.srad_last_error()
    assert lib.srad_resample_coeffs_f64(8, 4, 2, b.ctypes.data, None) == SRAD_ERR_ARG
    assert lib.srad_resample_coeffs_f64(8, 4, 5, b.ctypes.data, c.ctypes.data) == SRAD_ERR_ARG and b"unknown filter" in lib.srad_last_error()
    assert lib.srad_resample_coeffs_f64(0, 4, 2, b.ctypes.data, c.ctypes.data) == SRAD_ERR_ARG
    assert (c == 7.0).all() and (b == 0).all()                # a refused call writes nothing
    assert lib.srad_resample_coeffs_f64(8, 4, 2, b.ctypes.data, c.ctypes.data) == 0 and (c != 7.0).all()
    with pytest.raises(ValueError, match="resample filter"):
        ops.resample_coeffs_f64(8, 4, "nearest")
    assert ops.resample_coeffs_f64(8, 4)[0] == 5              # bilinear is the default
    with pytest.raises(ValueError, match="resample filter"):
        ops.resample_coeffs(8, 4, "bilinear")

    # srad_resize_f32: every refusal comes before a launch; the fake device pointers are never dereferenced
    src, dst, tmp, dev = 1 << 30, 2 << 30, 3 << 30, 1 << 20

    def table(in_size, out_size, ksize=None, bounds=None, dev_bounds=dev, dev_coeffs=dev):
        k_, b_, _ = ops.resample_coeffs_f64(in_size, out_size, "bilinear")
        b_ = b_ if bounds is None else bounds
        t = L.ResampleTableF(in_size, out_size, k_ if ksize is None else ksize, b_.ctypes.data, dev_bounds, dev_coeffs)
        t.keep = b_
        return t

    def call(src=src, n=2, H=16, W=12, dst=dst, h=4, w=6, xt="x", yt="y", tmp=tmp):
        xt = table(W, w) if isinstance(xt, str) else xt
        yt = table(H, h) if isinstance(yt, str) else yt
        return lib.srad_resize_f32(src, n, H, W, dst, h, w, xt, yt, tmp, None)

    def refused(text, **kw):
        assert call(**kw) == SRAD_ERR_ARG and text in lib.srad_last_error(), (kw, lib.srad_last_error())

    refused(b"null argument", src=None)
    refused(b"null argument", dst=None)
    refused(b"null argument", tmp=None)
    for kw in (dict(n=0), dict(H=0), dict(W=0), dict(h=0), dict(w=0)):
        refused(b"sizes must be >= 1", xt=None, yt=None, **kw)
    refused(b"resize_f32: the x table is missing", xt=None)
    refused(b"resize_f32: the y table is missing", yt=None)
    refused(b"null pointer in the x table", xt=table(12, 6, dev_bounds=None))
    refused(b"null pointer in the y table", yt=table(16, 4, dev_coeffs=None))
    refused(b"the x table is for 12 -> 5", xt=table(12, 5))
    refused(b"the y table is for 17 -> 4", yt=table(17, 4))
    refused(b"the x table is for", xt=table(12, 6, ksize=0))
    good = ops.resample_coeffs_f64(12, 6, "bilinear")[1]
    for row, col, value in ((5, 0, 12), (0, 0, -1), (3, 1, -2), (2, 1, 99), (5, 1, int(good[5, 1]) + 1)):
        bad = good.copy()
        bad[row, col] = value
        refused(b"the x table's bounds leave the source", xt=table(12, 6, bounds=bad))
    bad = ops.resample_coeffs_f64(16, 4, "bilinear")[1].copy()
    bad[3, 0] += 1
    refused(b"the y table's bounds leave the source", yt=table(16, 4, bounds=bad))
    n_src, n_dst, n_tmp = 4 * 2 * 16 * 12, 4 * 2 * 4 * 6, 4 * 2 * 16 * 6                    # bytes
    refused(b"dst overlaps src", dst=src + n_src - 4)
    refused(b"dst overlaps src", dst=src - n_dst + 4)
    refused(b"tmp overlaps src or dst", tmp=src + n_src - 4)
    refused(b"tmp overlaps src or dst", tmp=dst - n_tmp + 4)
    refused(b"tmp overlaps src or dst", tmp=dst + n_dst - 4)
    refused(b"dst overlaps src", dst=src, h=16, w=12, xt=None, yt=None)            # the copy too
    far = dict(src=1 << 40, dst=2 << 40, tmp=3 << 40)                               # room for 2^22 images between the fake pointers
    refused(b"more than one launch takes", n=1 << 22, **far)                        # n * H = 2^26 grid rows of 64 threads
    refused(b"more than one launch takes", n=1 << 22, W=6, xt=None, **far)          # n * h = 2^24 grid rows of 256 threads
    # srad_overlay_rgb checks its arguments before it launches, too
    def overlay(src=src, n=1, H=4, W=5, Cs=3, maps=dst, masks=tmp, lut=dev, scale=1.0, radius=1, rgb=(255, 0, 0), out=4 << 30):
        return lib.srad_overlay_rgb(src, n, H, W, Cs, maps, masks, lut, scale, radius, *rgb, out, None)

    for kw, text in ((dict(src=None), b"null argument"), (dict(maps=None), b"null argument"), (dict(masks=None), b"null argument"),
                     (dict(lut=None), b"null argument"), (dict(out=None), b"null argument"), (dict(n=0), b"sizes must be >= 1"),
                     (dict(H=0), b"sizes must be >= 1"), (dict(Cs=2), b"source channels"), (dict(Cs=4), b"source channels"),
                     (dict(radius=-1), b"contour radius"), (dict(radius=5), b"contour radius"), (dict(rgb=(256, 0, 0)), b"contour colour"),
                     (dict(rgb=(0, -1, 0)), b"contour colour"), (dict(scale=float("nan")), b"scale is NaN"),
                     (dict(out=src + 59), b"out overlaps an input"), (dict(out=dst - 59), b"out overlaps an input"),
                     (dict(out=tmp + 19), b"out overlaps an input"), (dict(out=dev + 1023), b"out overlaps an input")):
        assert overlay(**kw) == SRAD_ERR_ARG and text in lib.srad_last_error(), (kw, lib.srad_last_error())


def test_tables_and_passes_under_sanitizers(tmp_path):
    cxx = _compiler()
    version = subprocess.run(cxx + ["--version"], capture_output=True, text=True, timeout=60).stdout
    static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]       # clang links its runtimes statically by default
    exe = str(tmp_path / "resample_f_check")
    build = subprocess.run(cxx + ["-std=c++17", "-Wall", "-Wextra", "-Werror"] + SANITIZE + static + [SOURCE, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in run.stdout + run.stderr, run.stdout + run.stderr
    assert run.stdout.rstrip().endswith("resample_f_check: ok"), run.stdout
