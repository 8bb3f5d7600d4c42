"""The per-pixel map baseline restated in numpy (DESIGN.md "Baseline"), for the tests of srad_amd.baseline and its kernels:
float64 sums by an explicit loop over the images (never np.sum, whose pairwise order is not the definition's), the host
planes, the float32 apply, the float64 leave-one-out form, the per-image maximum under smooth_maps' rule - and ``literal``,
the same definitions once more as a per-pixel loop over Python floats (IEEE doubles, math.sqrt), which the restatement is
itself checked against at 5 x 7.  Also the synthetic band-and-blob case and the exact Mann-Whitney AUC the tests score it
with."""
import math

import numpy as np


def sums_ref(maps, s1=None, s2=None):
    """(s1, s2) float64 [H, W]: each starts at +0.0 (or at the given sums) and adds image by image, one rounding per add."""
    maps = np.asarray(maps, dtype=np.float32)
    s1 = np.zeros(maps.shape[1:], np.float64) if s1 is None else np.array(s1, dtype=np.float64)
    s2 = np.zeros(maps.shape[1:], np.float64) if s2 is None else np.array(s2, dtype=np.float64)
    with np.errstate(all="ignore"):
        for m in maps:
            x = m.astype(np.float64)
            s1 = s1 + x
            s2 = s2 + x * x                                   # the product of two floats is exact in double
    return s1, s2


def planes_ref(s1, s2, n, floor_rel):
    """dict(mean, var, pooled, floor, sd, mu32, inv32) of the definitions, numpy float64."""
    with np.errstate(all="ignore"):
        mean = s1 / n
        var = np.maximum(s2 - s1 * s1 / n, 0) / (n - 1)
        pooled = np.sqrt(var.mean())
        floor = floor_rel * pooled
        sd = np.maximum(np.sqrt(var), floor)
        return dict(mean=mean, var=var, pooled=float(pooled), floor=float(floor), sd=sd, mu32=np.float32(mean), inv32=np.float32(1.0 / sd))


def apply_ref(maps, mu32, inv32):
    """z = fl32(fl32(m - mu32) * inv32): numpy rounds every float32 operation on its own."""
    with np.errstate(all="ignore"):
        d = (np.asarray(maps, np.float32) - mu32[None]).astype(np.float32)
        return (d * inv32[None]).astype(np.float32)


def loo_ref(maps, s1, s2, n, floor):
    """The leave-one-out z-scores of maps that are part of the sums over n maps, in double, one rounding per operation."""
    with np.errstate(all="ignore"):
        x = np.asarray(maps, np.float32).astype(np.float64)
        a = s1[None] - x
        q = s2[None] - x * x
        mean_i = a / (n - 1)
        var_i = np.maximum(q - a * a / (n - 1), 0) / (n - 2)
        sd_i = np.maximum(np.sqrt(var_i), floor)
        return ((x - mean_i) / sd_i).astype(np.float32)


def max_ref(z):
    """Per-image maximum float32 [n]: NaN if any pixel of the image is NaN (np.max propagates it)."""
    with np.errstate(all="ignore"):
        return np.asarray(z, np.float32).reshape(len(z), -1).max(axis=1)


def same_bits(a, b):
    """Equal as bit patterns (so -0.0 is not +0.0), every NaN counting as one value: the payload of a NaN that an operation
    makes is the processor's choice."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(np.array_equal(nan_a, nan_b) and np.array_equal(a[~nan_a].view(u), b[~nan_b].view(u)))


def same_max(a, b):
    """Equal per-image maxima: NaN where the other has NaN, equal values elsewhere (a maximum of zero comes back as +0.0)."""
    a, b = np.asarray(a), np.asarray(b)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return bool(a.shape == b.shape and a.dtype == b.dtype and np.array_equal(nan_a, nan_b) and np.array_equal(a[~nan_a], b[~nan_b]))


def literal(maps, floor_rel):
    """The definitions as a per-pixel loop over Python floats: dict(s1, s2, mu32, inv32, floor, pooled, loo)."""
    maps = np.asarray(maps, dtype=np.float32)
    n, H, W = maps.shape
    s1, s2 = np.zeros((H, W)), np.zeros((H, W))
    var = np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            a, b = 0.0, 0.0
            for i in range(n):
                v = float(maps[i, y, x])
                a = a + v
                b = b + v * v
            s1[y, x], s2[y, x] = a, b
            var[y, x] = max(b - a * a / n, 0.0) / (n - 1)
    total = 0.0                                               # var.mean() is numpy's own sum: compared with a tolerance only
    for v in var.ravel():
        total += v
    pooled_loop = math.sqrt(total / (H * W))
    pooled = float(np.sqrt(var.mean()))
    floor = floor_rel * pooled
    mu32, inv32 = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    loo = np.zeros((n, H, W), np.float32)
    for y in range(H):
        for x in range(W):
            mu32[y, x] = np.float32(s1[y, x] / n)
            inv32[y, x] = np.float32(1.0 / max(math.sqrt(var[y, x]), floor))
            for i in range(n):
                v = float(maps[i, y, x])
                a, q = s1[y, x] - v, s2[y, x] - v * v
                mean_i = a / (n - 1)
                var_i = max(q - a * a / (n - 1), 0.0) / (n - 2)
                loo[i, y, x] = np.float32((v - mean_i) / max(math.sqrt(var_i), floor))
    return dict(s1=s1, s2=s2, mu32=mu32, inv32=inv32, floor=floor, pooled=pooled, pooled_loop=pooled_loop, loo=loo)


def auc(neg, pos):
    """The exact Mann-Whitney ROC-AUC of two score lists (ties count a half)."""
    neg, pos = np.asarray(neg, np.float64), np.asarray(pos, np.float64)
    twice = sum(2 * int((neg < p).sum()) + int((neg == p).sum()) for p in pos)
    return twice / (2.0 * len(neg) * len(pos))


def pixel_auc(scores, labels):
    """twice_U / (2 * n_pos * n_neg) of all pixels, in integers up to the one division."""
    s, y = np.asarray(scores, np.float64).ravel(), np.asarray(labels).ravel() != 0
    vals, inv = np.unique(s, return_inverse=True)
    pos = np.bincount(inv[y], minlength=len(vals)).astype(np.int64)
    neg = np.bincount(inv[~y], minlength=len(vals)).astype(np.int64)
    below = np.concatenate([[0], np.cumsum(neg)[:-1]])
    return int(np.sum(pos * (2 * below + neg))) / (2.0 * int(pos.sum()) * int(neg.sum()))


BAND_N = (12, 10, 10)                                         # calibration, good test and bad test maps


def band_and_blob(seed=0, hw=32):
    """(calib, good, bad, blob masks of bad) float32 maps [n, hw, hw]: baseline 0.5 on columns 0..3 and 0.05 elsewhere, every
    pixel times 1 + 0.2 U(-1, 1); each bad map carries a 3 x 3 blob of +0.15 in the quiet area.  The noisy band decides the raw
    map maximum; in sigmas of the per-pixel baseline the blob stands 30 sigmas out."""
    rng = np.random.default_rng(seed)
    base = np.full((hw, hw), 0.05)
    base[:, :4] = 0.5

    def draw(n):
        return (base[None] * (1.0 + 0.2 * rng.uniform(-1.0, 1.0, (n, hw, hw)))).astype(np.float32)
    calib, good, bad = draw(BAND_N[0]), draw(BAND_N[1]), draw(BAND_N[2])
    masks = np.zeros(bad.shape, np.uint8)
    for k in range(len(bad)):
        y, x = int(rng.integers(2, hw - 5)), int(rng.integers(6, hw - 5))
        bad[k, y:y + 3, x:x + 3] += np.float32(0.15)
        masks[k, y:y + 3, x:x + 3] = 1
    return calib, good, bad, masks
