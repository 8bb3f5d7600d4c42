"""Writes tests/golden/map_smooth_golden.npz: float32 anomaly-map stacks and what
``scipy.ndimage.gaussian_filter(maps, (0, sigma, sigma), mode='reflect', truncate=4.0)`` makes of them.  srad_smooth_maps
(``metrics.smooth_maps``) must reproduce every output bit for bit, NaN positions included.

    python tests/golden/make_map_smooth_golden.py

Cases: sigma 0.5, 1, 2, 4 and 8; odd and non-square maps (45 x 63, 64 x 96, 127 x 128); maps whose radius equals min(H, W);
runs of exact zeros as real SSIM maps have; one image with a NaN pixel; signed maps whose sums cancel, on which the order of
the taps decides the fp32 result.  The maps are built from integer arithmetic only (no RNG
stream that could change between numpy versions).

``gaussian_weights_ref`` and ``smooth_ref`` are a plain numpy restatement of what scipy computes (DESIGN.md "Map smoothing") for
cases too large to store; they need no scipy, so the GPU tests import them from here."""
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "map_smooth_golden.npz")
# name: (n, H, W, salt, sigmas)
CASES = {
    "odd_45x63": (2, 45, 63, 1, (0.5, 1.0, 2.0, 4.0, 8.0)),
    "wide_64x96": (1, 64, 96, 2, (1.0, 8.0)),
    "odd_127x128": (1, 127, 128, 3, (4.0,)),
    "radius_eq_h_16x40": (2, 16, 40, 4, (4.0,)),          # r = 16 = H
    "radius_eq_w_40x24": (1, 40, 24, 5, (6.0,)),          # r = 24 = W
    "cancel_s2_64x64": (1, 64, 64, 6, (2.0,)),           # signed; centres cancel their taps (the order of the sum shows)
    "cancel_s4_64x64": (1, 64, 64, 7, (4.0,)),
}
SIGNED = ("cancel_s2_64x64", "cancel_s4_64x64")


def gaussian_weights_ref(sigma, truncate=4.0):
    """The half [r:] of scipy's _gaussian_kernel1d(sigma, 0, r), r = int(truncate * sigma + 0.5)."""
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return (phi / phi.sum())[r:]


def _pass(x, w, axis, inward=True):
    """One symmetric-filter pass along `axis` in scipy's arithmetic: fp64, acc = x*w0, then acc + (x[i-j] + x[i+j]) * w[j]
    for j = r down to 1 (scipy's loop starts at the farthest tap), each operation rounded on its own, half-sample reflection at
    the edges; the result rounded to fp32.  ``inward=False`` sums j = 1..r instead: the golden's signed cases tell the two
    apart."""
    x = np.moveaxis(np.asarray(x, np.float32).astype(np.float64), axis, -1)
    n, r = x.shape[-1], len(w) - 1
    assert r <= n, "more than one reflection"
    idx = np.arange(-r, n + r)
    idx = np.where(idx < 0, -idx - 1, np.where(idx >= n, 2 * n - 1 - idx, idx))
    e = x[..., idx]
    acc = e[..., r:r + n] * w[0]
    for j in (range(r, 0, -1) if inward else range(1, r + 1)):
        acc = acc + (e[..., r - j:r - j + n] + e[..., r + j:r + j + n]) * w[j]
    return np.moveaxis(acc.astype(np.float32), -1, axis)


def smooth_ref(maps, sigma, truncate=4.0, inward=True):
    """gaussian_filter(maps, (0, sigma, sigma), mode='reflect', truncate=truncate) of float32 maps [n, H, W], without scipy."""
    maps = np.asarray(maps, np.float32)
    if sigma <= 1e-15:
        return maps.copy()
    w = gaussian_weights_ref(sigma, truncate)
    return _pass(_pass(maps, w, 1, inward), w, 2, inward)


def hashed_maps(n, H, W, salt):
    """SSIM-like maps from integer hashing: a smooth bump field plus fine noise in [-0.05, 1.2], runs of exact zeros (whole
    row segments and blocks), and a NaN pixel in image 1 when there is one."""
    i = np.arange(n, dtype=np.int64)[:, None, None]
    y = np.arange(H, dtype=np.int64)[None, :, None]
    x = np.arange(W, dtype=np.int64)[None, None, :]
    h = (i * 73856093 + y * 19349663 + x * 83492791 + salt * 2654435761) % 1000003
    noise = (h % 4099).astype(np.float64) / 4099.0
    cy, cx = 0.3 * H + 0.1 * H * i, 0.6 * W - 0.05 * W * i
    bump = np.exp(-(((y - cy) / (0.2 * H)) ** 2 + ((x - cx) / (0.15 * W)) ** 2))
    m = (0.9 * bump + 0.25 * noise - 0.05).astype(np.float32)
    m[(h % 7 == 0) & (x % 11 < 5)] = 0.0                          # short runs of zeros along rows
    m[:, H // 2:H // 2 + max(1, H // 8), :W // 3] = 0.0          # a block of zeros
    m[:, :, -max(1, W // 10):] = 0.0                            # zero columns at the right edge
    if n > 1:
        m[1, H // 3, W // 4] = np.nan
    return m


def cancel_maps(n, H, W, salt, sigma):
    """Signed maps in [-1, 1) from integer hashing in which, every 2r + 3 rows, a pixel is set to minus the weighted sum of its
    vertical taps over the centre weight: there the H pass sums terms of ~1 to a result of ~1e-8, so the fp64 rounding of the
    sum, and with it the order of the taps, shows in the fp32 result.  A restatement that adds j = 1..r instead of r..1 differs
    from scipy on dozens of pixels per case."""
    i = np.arange(n, dtype=np.int64)[:, None, None]
    y = np.arange(H, dtype=np.int64)[None, :, None]
    x = np.arange(W, dtype=np.int64)[None, None, :]
    h = (i * 73856093 + y * 19349663 + x * 83492791 + salt * 2654435761) % 1000003
    m = ((h % 8191).astype(np.float64) / 4095.5 - 1.0).astype(np.float32)
    w = gaussian_weights_ref(sigma)
    r = len(w) - 1
    for c in range(r, H - r, 2 * r + 3):                       # centres far enough apart not to share taps
        side = sum(w[j] * (m[:, c - j].astype(np.float64) + m[:, c + j]) for j in range(1, r + 1))
        m[:, c] = (-side / w[0]).astype(np.float32)
    return m


def case_maps(name):
    n, H, W, salt, sigmas = CASES[name]
    return cancel_maps(n, H, W, salt, sigmas[0]) if name in SIGNED else hashed_maps(n, H, W, salt)


def main():
    from scipy import ndimage
    out = {}
    for name, (n, H, W, salt, sigmas) in CASES.items():
        m = case_maps(name)
        out[f"{name}/maps"] = m
        out[f"{name}/sigmas"] = np.asarray(sigmas, np.float64)
        for s in sigmas:
            assert int(4.0 * s + 0.5) <= min(H, W)
            ref = ndimage.gaussian_filter(m, (0, s, s), mode='reflect', truncate=4.0)
            assert ref.dtype == np.float32
            mine = smooth_ref(m, s)
            assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32)), (name, s)   # the restatement is scipy, bit for bit
            if name in SIGNED:                                   # and the order of the taps is visible in these cases
                outward = smooth_ref(m, s, inward=False)
                assert (outward.view(np.uint32) != ref.view(np.uint32)).sum() >= 20, (name, s)
            out[f"{name}/out_{s:g}"] = ref
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(CASES)} cases")


if __name__ == "__main__":
    main()
