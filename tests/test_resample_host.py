"""CPU: the host half of the device resize (csrc/resample_coeffs.h behind srad_resample_ksize / srad_resample_coeffs).
The library's tables against an independent numpy restatement of Pillow's precompute_coeffs + normalize_coeffs_8bpc; a numpy
resize driven by the library's tables against PIL.Image.resize itself, every pixel equal; the argument errors of the three entry
points (srad_resize_u8 checks everything before it touches a device); and tests/host/resample_check.cpp, a stand-alone program
that includes only the header, built with AddressSanitizer and UndefinedBehaviorSanitizer (linked statically, nothing is
preloaded) and run once."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from tests.test_wgrad_queue_host import SANITIZE, _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "resample_check.cpp")
PAIRS = [(1024, 128), (128, 32), (53, 17), (40, 57), (5, 1), (7, 7)]
FILTERS = {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC}
SRAD_ERR_ARG = 1


def _sinc(x):
    px = np.where(x == 0.0, 1.0, x * np.pi)
    return np.where(x == 0.0, 1.0, np.sin(px) / px)


def _filter(name, x):
    if name == "lanczos":
        return np.where((-3.0 <= x) & (x < 3.0), _sinc(x) * _sinc(x / 3), 0.0), 3.0
    a, x = -0.5, np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0)), 2.0


def numpy_coeffs(in_size, out_size, name):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc, restated with numpy (float64 throughout)."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = _filter(name, np.zeros(1))[1] * fs
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coeffs = np.zeros((out_size, ksize), dtype=np.int32)
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
        coeffs[xx, :xmax] = np.trunc(np.where(w < 0, -0.5, 0.5) + w * (1 << 22)).astype(np.int32)
        bounds[xx] = xmin, xmax
    return ksize, bounds, coeffs


def numpy_pass(a, axis, bounds, coeffs):
    """One pass of the resize along ``axis`` of the u8 array ``a`` [H,W,C] with int32 accumulators."""
    a = np.moveaxis(a, axis, 0).astype(np.int32)
    out = np.empty((len(bounds),) + a.shape[1:], dtype=np.uint8)
    for xx, (xmin, xmax) in enumerate(bounds):
        acc = (1 << 21) + np.tensordot(coeffs[xx, :xmax], a[xmin:xmin + xmax], axes=(0, 0))
        out[xx] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def numpy_resize(a, h, w, name):
    """``a`` u8 [H,W,C] -> [h,w,C] with the LIBRARY's tables: horizontal first, rounded to u8, then vertical; equal sizes skip."""
    from srad_amd import ops
    if a.shape[1] != w:
        a = numpy_pass(a, 1, *ops.resample_coeffs(a.shape[1], w, name)[1:])
    if a.shape[0] != h:
        a = numpy_pass(a, 0, *ops.resample_coeffs(a.shape[0], h, name)[1:])
    return a


def images(kind, shape, seed=0):
    rng = np.random.RandomState(seed)
    if kind == "random":
        return rng.randint(0, 256, shape).astype(np.uint8)
    if kind == "binary":
        return (rng.randint(0, 2, shape) * 255).astype(np.uint8)
    ramp = np.add.outer(np.arange(shape[0]) * 3, np.arange(shape[1]) * 5)
    return ((ramp[..., None] + 40 * np.arange(shape[2])) % 256).astype(np.uint8)


def pil_resize(a, h, w, name):
    """PIL.Image.resize of a u8 [H,W,C] image; 'L' for one channel, 'RGB' for three, channel by channel otherwise."""
    if a.shape[2] == 3:
        return np.asarray(Image.fromarray(a).resize((w, h), FILTERS[name]))
    return np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(a[:, :, c])).resize((w, h), FILTERS[name]))
                     for c in range(a.shape[2])], axis=2)


@pytest.mark.parametrize("name", sorted(FILTERS))
def test_library_tables_equal_the_numpy_restatement(name):
    from srad_amd import ops
    for in_size, out_size in PAIRS:
        ksize, bounds, coeffs = ops.resample_coeffs(in_size, out_size, name)
        k2, b2, c2 = numpy_coeffs(in_size, out_size, name)
        assert ksize == k2 and coeffs.shape == (out_size, ksize), (in_size, out_size)
        assert np.array_equal(bounds, b2), (in_size, out_size)
        assert np.array_equal(coeffs, c2), (in_size, out_size, int(np.abs(coeffs.astype(np.int64) - c2).max()))
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= in_size).all() and (bounds[:, 1] <= ksize).all()


@pytest.mark.parametrize("name", sorted(FILTERS))
@pytest.mark.parametrize("kind", ["random", "binary", "ramp"])
def test_resize_with_library_tables_equals_pil(name, kind):
    shapes = [((128, 128), (32, 32)), ((37, 53), (12, 17)), ((40, 40), (57, 57)), ((64, 48), (16, 48)), ((5, 5), (1, 1)), ((7, 7), (7, 7))]
    if name == "lanczos" and kind == "random":
        shapes.append(((1024, 1024), (128, 128)))
    for (H, W), (h, w) in shapes:
        for ch in (1, 3):
            a = images(kind, (H, W, ch), seed=H + ch)
            got, ref = numpy_resize(a, h, w, name), pil_resize(a, h, w, name)
            assert got.shape == ref.reshape(h, w, ch).shape and np.array_equal(got, ref.reshape(h, w, ch)), (H, W, h, w, ch)


def test_argument_errors_without_gpu():
    from srad_amd import _lib as L, ops
    lib = L.lib()
    k = C.c_int(-1)
    assert lib.srad_resample_ksize(1024, 128, 0, C.byref(k)) == 0 and k.value == 49
    assert lib.srad_resample_ksize(40, 57, 0, C.byref(k)) == 0 and k.value == 7
    assert lib.srad_resample_ksize(40, 57, 1, C.byref(k)) == 0 and k.value == 5
    for args, text in (((0, 4, 0), b"not supported"), ((4, 0, 0), b"not supported"), ((4, 4, 2), b"unknown filter"), ((4, 4, -1), b"unknown filter"),
                       (((1 << 20) + 1, 4, 0), b"not supported")):
        k.value = -1
        assert lib.srad_resample_ksize(*args, C.byref(k)) == SRAD_ERR_ARG and text in lib.srad_last_error() and k.value == -1, args
    assert lib.srad_resample_ksize(4, 4, 0, None) == SRAD_ERR_ARG and b"null argument" in lib.srad_last_error()
    b, c = np.zeros((4, 2), np.int32), np.zeros((4, 7), np.int32)
    assert lib.srad_resample_coeffs(8, 4, 0, None, c.ctypes.data) == SRAD_ERR_ARG and b"null argument" in lib.srad_last_error()
    assert lib.srad_resample_coeffs(8, 4, 0, b.ctypes.data, None) == SRAD_ERR_ARG
    assert lib.srad_resample_coeffs(8, 4, 5, b.ctypes.data, c.ctypes.data) == SRAD_ERR_ARG and b"unknown filter" in lib.srad_last_error()
    assert lib.srad_resample_coeffs(0, 4, 0, b.ctypes.data, c.ctypes.data) == SRAD_ERR_ARG
    with pytest.raises(ValueError, match="resample filter"):
        ops.resample_coeffs(8, 4, "nearest")

    # srad_resize_u8: every refusal comes before a launch; the fake device pointers are never dereferenced
    src, dst, tmp, dev = 1 << 30, 2 << 30, 3 << 30, 1 << 20

    def table(in_size, out_size, ksize=None, bounds=None, dev_bounds=dev, dev_coeffs=dev):
        k_, b_, _ = ops.resample_coeffs(in_size, out_size, "lanczos")
        b_ = b_ if bounds is None else bounds
        t = L.ResampleTable(in_size, out_size, k_ if ksize is None else ksize, b_.ctypes.data, dev_bounds, dev_coeffs)
        t.keep = b_
        return t

    def call(src=src, n=2, H=16, W=12, Cc=3, dst=dst, h=4, w=6, xt="x", yt="y", tmp=tmp):
        xt = table(W, w) if isinstance(xt, str) else xt
        yt = table(H, h) if isinstance(yt, str) else yt
        return lib.srad_resize_u8(src, n, H, W, Cc, dst, h, w, xt, yt, tmp, None)

    def refused(text, **kw):
        assert call(**kw) == SRAD_ERR_ARG and text in lib.srad_last_error(), (kw, lib.srad_last_error())

    refused(b"null argument", src=None)
    refused(b"null argument", dst=None)
    refused(b"null argument", tmp=None)
    for kw in (dict(n=0), dict(H=0), dict(W=0), dict(h=0), dict(w=0)):
        refused(b"sizes must be >= 1", xt=None, yt=None, **kw)
    refused(b"channels", Cc=0)
    refused(b"channels", Cc=5)
    refused(b"the x table is missing", xt=None)
    refused(b"the y table is missing", yt=None)
    refused(b"null pointer in the x table", xt=table(12, 6, dev_bounds=None))
    refused(b"null pointer in the y table", yt=table(16, 4, dev_coeffs=None))
    refused(b"the x table is for 12 -> 5", xt=table(12, 5))
    refused(b"the y table is for 17 -> 4", yt=table(17, 4))
    refused(b"the x table is for", xt=table(12, 6, ksize=0))
    good = ops.resample_coeffs(12, 6, "lanczos")[1]
    for row, col, value in ((5, 0, 12), (0, 0, -1), (3, 1, -2), (2, 1, 99), (5, 1, int(good[5, 1]) + 1)):
        bad = good.copy()
        bad[row, col] = value
        refused(b"the x table's bounds leave the source", xt=table(12, 6, bounds=bad))
    bad = ops.resample_coeffs(16, 4, "lanczos")[1].copy()
    bad[3, 0] += 1
    refused(b"the y table's bounds leave the source", yt=table(16, 4, bounds=bad))
    n_src, n_dst, n_tmp = 2 * 16 * 12 * 3, 2 * 4 * 6 * 3, 2 * 16 * 6 * 3
    refused(b"dst overlaps src", dst=src + n_src - 1)
    refused(b"dst overlaps src", dst=src - n_dst + 1)
    refused(b"tmp overlaps src or dst", tmp=src + n_src - 1)
    refused(b"tmp overlaps src or dst", tmp=dst - n_tmp + 1)
    refused(b"tmp overlaps src or dst", tmp=dst + n_dst - 1)
    refused(b"dst overlaps src", dst=src, h=16, w=12, xt=None, yt=None)            # the copy too


def test_tables_and_accumulators_under_sanitizers(tmp_path):
    cxx = _compiler()
    version = subprocess.run(cxx + ["--version"], capture_output=True, text=True, timeout=60).stdout
    static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]       # clang links its runtimes statically by default
    exe = str(tmp_path / "resample_check")
    build = subprocess.run(cxx + ["-std=c++17", "-Wall", "-Wextra", "-Werror"] + SANITIZE + static + [SOURCE, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in run.stdout + run.stderr, run.stdout + run.stderr
    assert run.stdout.rstrip().endswith("resample_check: ok"), run.stdout
