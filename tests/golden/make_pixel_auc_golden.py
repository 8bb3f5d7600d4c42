"""Writes tests/golden/pixel_auc_golden.npz: pixel-level ROC-AUC cases and what ``sklearn.metrics.roc_auc_score`` returns for
them (the metric srad_pixel_roc_auc must reproduce to 1e-12).

    python tests/golden/make_pixel_auc_golden.py

Small cases are stored as arrays.  The ~2 M element case is stored as its generator's arguments: ``hashed_case`` builds it
from integer arithmetic only (no RNG stream that could change between numpy versions), and the test rebuilds it the same way;
its checksums are stored with it."""
import os

import numpy as np
from sklearn.metrics import roc_auc_score

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pixel_auc_golden.npz")
LARGE_N, LARGE_SALT = 2_000_003, 7


def hashed_case(n: int, salt: int):
    """float32 scores with ~64 k distinct values (many ties, both signs) and labels correlated with them, from a
    multiplicative hash of the index."""
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) & np.uint64(0xFFFFFFFF)
    h2 = ((h ^ (h >> np.uint64(13))) * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    s = ((h >> np.uint64(16)).astype(np.int64) - 32768).astype(np.float32) / np.float32(4096.0)
    y = ((h2 % np.uint64(1000)).astype(np.int64) < 300 + (s > 0) * 200).astype(np.uint8)
    return s, y


def cases():
    rng = np.random.RandomState(20)
    out = {}
    n = 10007
    out["continuous"] = (rng.standard_normal(n).astype(np.float32), (rng.rand(n) < 0.3).astype(np.uint8))
    y = (rng.rand(5000) < 0.4).astype(np.uint8)
    out["ties8"] = ((rng.randint(0, 8, 5000) + y * rng.randint(0, 3, 5000)).astype(np.float32) * np.float32(0.25), y)
    s = np.where(rng.rand(1000) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    s[rng.rand(1000) < 0.2] = np.float32(1.0)
    s[rng.rand(1000) < 0.2] = np.float32(-1.0)
    out["signed_zeros"] = (s, (rng.rand(1000) < 0.5).astype(np.uint8))
    y = (rng.rand(3000) < 0.5).astype(np.uint8)
    out["negative"] = ((-np.abs(rng.standard_normal(3000)) - 0.5 * y).astype(np.float32), y)
    out["all_equal"] = (np.full(777, 0.25, np.float32), (rng.rand(777) < 0.5).astype(np.uint8))
    y = (rng.rand(1000) < 0.5).astype(np.uint8)
    out["perfect"] = (np.where(y, 1.0 + rng.rand(1000), rng.rand(1000)).astype(np.float32), y)
    out["inverse"] = (np.where(y, rng.rand(1000), 1.0 + rng.rand(1000)).astype(np.float32), y.copy())
    out["n3"] = (np.array([0.1, 0.7, 0.3], np.float32), np.array([0, 1, 1], np.uint8))
    n = 3 * 8192 + 4097
    y = (rng.rand(n) < 0.2).astype(np.uint8)
    out["odd_n"] = ((rng.standard_normal(n) + y).astype(np.float32), y)
    return out


def main():
    data = {}
    for name, (s, y) in cases().items():
        data[f"{name}/s"], data[f"{name}/y"] = s, y
        data[f"{name}/auc"] = np.float64(roc_auc_score(y, s))
    s, y = hashed_case(LARGE_N, LARGE_SALT)
    data["large/args"] = np.array([LARGE_N, LARGE_SALT], np.int64)
    data["large/checksum"] = np.array([s.astype(np.float64).sum(), float(y.sum())])
    data["large/auc"] = np.float64(roc_auc_score(y, s))
    np.savez_compressed(OUT, **data)
    print({k: float(v) for k, v in data.items() if k.endswith("/auc")})


if __name__ == "__main__":
    main()
