"""Writes tests/golden/pro_golden.npz: AU-PRO cases (Bergmann et al., IJCV 2021) and what the definition in DESIGN.md "AU-PRO"
gives for them: the per-pixel region sizes (``scipy.ndimage.label`` with a 3 x 3 structure, per image), R, N_ok, the whole
per-region overlap curve and the normalised AU-PRO at several false-positive-rate limits.  srad_pixel_pro / srad_mask_regions
must reproduce them (sizes and counts exactly, curve and AU-PRO to 1e-9).

    python tests/golden/make_pro_golden.py

Small cases are stored as arrays.  The ~2 M pixel case is stored as its generator's arguments: ``hashed_case`` builds it from
integer arithmetic only (no RNG stream that could change between numpy versions) and the test rebuilds it the same way; its
checksums, sizes of its curve and every 97th curve point are stored with it.

``pro_curve_ref`` and ``aupro_ref`` are a plain numpy restatement of the definition, and ``uf_sizes`` a pure-Python labeller;
they need no scipy (only ``scipy_sizes`` does), so the tests import them from here."""
import os
from collections import Counter

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pro_golden.npz")
LIMITS = (0.3, 0.05, 1.0)
LARGE_ARGS = (8, 512, 512, 11)          # n, H, W, salt: 2,097,152 pixels
LARGE_STRIDE = 97


def scipy_sizes(masks):
    """Per-pixel region size (0 for ok pixels) and R of masks [n, H, W]: scipy.ndimage.label(m_i, np.ones((3, 3))) per image."""
    from scipy import ndimage
    sizes = np.zeros(masks.shape, np.int64)
    R = 0
    for i, m in enumerate(masks):
        lab, k = ndimage.label(m != 0, structure=np.ones((3, 3), int))
        cnt = np.bincount(lab.ravel(), minlength=k + 1)
        cnt[0] = 0
        sizes[i] = cnt[lab]
        R += k
    return sizes, R


def uf_sizes(masks):
    """The same as ``scipy_sizes`` without scipy: a dictionary union-find over each image's defect pixels (8-connectivity)."""
    masks = np.asarray(masks) != 0
    sizes = np.zeros(masks.shape, np.int64)
    R = 0
    for i in range(masks.shape[0]):
        pts = list(zip(*[a.tolist() for a in np.nonzero(masks[i])]))
        parent = {p: p for p in pts}

        def find(p):
            while parent[p] != p:
                parent[p] = parent[parent[p]]
                p = parent[p]
            return p
        for y, x in pts:
            for q in ((y, x - 1), (y - 1, x - 1), (y - 1, x), (y - 1, x + 1)):
                if q in parent:
                    a, b = find((y, x)), find(q)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
        roots = [find(p) for p in pts]
        cnt = Counter(roots)
        for (y, x), r in zip(pts, roots):
            sizes[i, y, x] = cnt[r]
        R += len(cnt)
    return sizes, R


def pro_curve_ref(scores, sizes, R):
    """The curve of the definition: every distinct score is a threshold, from the highest down (-0.0 == +0.0); a point counts
    every pixel with s >= t.  fpr = ok pixels / N_ok, pro = (1/R) sum over defect pixels of 1 / |region|, both clipped at 1;
    (0, 0) first and (1, 1) last.  Per-pixel region sizes carry all PRO needs: sum_r count_r / |r| = sum_p 1 / |r(p)|."""
    s = np.asarray(scores, np.float64).ravel()
    z = np.asarray(sizes, np.int64).ravel()
    ok = z == 0
    n_ok = int(ok.sum())
    vals, g = np.unique(s, return_inverse=True)           # ascending distinct values; -0.0 and +0.0 are one value
    g = g.ravel()
    ok_g = np.bincount(g[ok], minlength=len(vals))[::-1]
    w_g = np.bincount(g[~ok], weights=1.0 / z[~ok], minlength=len(vals))[::-1]
    fpr = np.minimum(1.0, np.cumsum(ok_g).astype(np.float64) / n_ok)
    pro = np.minimum(1.0, np.cumsum(w_g.astype(np.longdouble)).astype(np.float64) / R)
    return np.concatenate([[0.0], fpr, [1.0]]), np.concatenate([[0.0], pro, [1.0]])


def aupro_ref(fpr, pro, limit):
    """Trapezoids over consecutive points with fpr <= limit; if the limit is not a curve fpr, the segment that crosses it up to
    the limit with pro interpolated there; divided by the limit."""
    area = 0.0
    for k in range(1, len(fpr)):
        f0, p0, f1, p1 = fpr[k - 1], pro[k - 1], fpr[k], pro[k]
        if f1 <= limit:
            area += (f1 - f0) * (p0 + p1) * 0.5
        else:
            if f0 < limit:
                pl = p0 + (p1 - p0) * (limit - f0) / (f1 - f0)
                area += (limit - f0) * (p0 + pl) * 0.5
            break
    return area / limit


def _blobs(rng, n, H, W, k_big, k_small):
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        for k in range(k_big + k_small):
            r = rng.uniform(4, 9) if k < k_big else rng.uniform(0.5, 2.2)
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            m[i][(yy - cy) ** 2 + ((xx - cx) * rng.uniform(0.6, 1.6)) ** 2 <= r * r] = 1
    return m


def spiral(N):
    """A one-pixel-wide square spiral filling an N x N image, arms two pixels apart: one 8-connected region."""
    m = np.zeros((N, N), np.uint8)
    top, left, bottom, right = 0, 0, N - 1, N - 1
    while top <= bottom and left <= right:
        m[top, left:right + 1] = 1
        m[top:bottom + 1, right] = 1
        if bottom - top < 2 or right - left < 2:
            break
        m[bottom, left:right + 1] = 1
        m[top + 2:bottom + 1, left] = 1
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
        m[top - 1, left - 1] = 1                                   # the step from one ring into the next
    return m


def hashed_case(n, H, W, salt):
    """Large case from integer arithmetic: discs at hashed centres (a few large, many small) as the masks; scores on a grid of
    1/256 with ~70 % exact zeros (half of them -0.0), raised inside the discs."""
    idx = np.arange(n * H * W, dtype=np.uint64)
    h = (idx * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) & np.uint64(0xFFFFFFFF)
    h2 = ((h ^ (h >> np.uint64(13))) * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    m = np.zeros((n, H, W), np.uint8)
    yy, xx = np.mgrid[:H, :W]
    for i in range(n):
        for k in range(40):
            c = (i * 1000003 + k * 7919 + salt * 104729) * 2654435761 % (1 << 32)
            cy, cx = c % H, (c >> 9) % W
            r = 3 + (c >> 20) % 40 if k < 4 else 1 + (c >> 20) % 4
            m[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    q = (h2 % np.uint64(1000)).astype(np.int64)
    s = ((h >> np.uint64(20)).astype(np.int64) % 256).astype(np.float32) / np.float32(256.0)
    s = s + m.ravel().astype(np.float32) * np.float32(0.25) * ((h2 >> np.uint64(11)) % np.uint64(4)).astype(np.float32)
    s[q < 700] = np.float32(0.0)
    s[q < 350] = np.float32(-0.0)
    return s.reshape(n, H, W).astype(np.float32), m


def cases():
    rng = np.random.RandomState(31)
    out = {}
    m = _blobs(rng, 5, 40, 56, 2, 6)
    s = (np.round(rng.rand(*m.shape) * 16) / 16 + m * rng.randint(0, 3, m.shape) * 0.25).astype(np.float32)
    out["blobs"] = (s, m)
    m = np.zeros((1, 12, 12), np.uint8)
    m[0, 3, 3] = m[0, 4, 4] = 1                                    # touch only at a corner: one region with 8-connectivity
    m[0, 8:10, 7:10] = 1
    out["corner"] = (rng.rand(1, 12, 12).astype(np.float32), m)
    m = np.zeros((3, 37, 45), np.uint8)
    m[0, 0, 10:14] = 1                                             # the four borders
    m[0, 36, 20:25] = 1
    m[0, 15:18, 0] = 1
    m[0, 22:24, 44] = 1
    m[1, 5, 44] = m[1, 6, 0] = 1                                   # right end of row y, left end of row y + 1
    m[1, 36, 30:33] = 1                                            # bottom of image 1 ...
    m[2, 0, 30:33] = 1                                             # ... top of image 2
    m[2, 20, 44] = m[2, 21, 0] = m[2, 21, 1] = 1
    out["borders"] = ((np.round(rng.rand(3, 37, 45) * 64) / 64 + 0.5 * m).astype(np.float32), m)
    m = np.zeros((2, 64, 64), np.uint8)                            # the same at a width that is a whole number of 32-px tiles
    m[0, 31, 63] = m[0, 32, 0] = 1
    m[0, 63, 5:9] = 1
    m[1, 0, 5:9] = 1
    m[1, 40, 31:33] = 1
    m[1, 31, 32] = m[1, 32, 31] = 1
    out["wrap64"] = ((np.round(rng.rand(2, 64, 64) * 32) / 32 + 0.25 * m).astype(np.float32), m)
    m = spiral(128)[None]
    out["spiral"] = ((rng.rand(1, 128, 128) * 0.8 + 0.3 * m).astype(np.float32), m)
    m = np.ones((1, 50, 70), np.uint8)
    m[0, 17, 33] = 0
    out["almost_full"] = ((np.round(rng.rand(1, 50, 70) * 128) / 128).astype(np.float32), m)
    m = np.zeros((5, 33, 33), np.uint8)
    m[4] = _blobs(rng, 1, 33, 33, 1, 3)[0]
    out["good_plus_one_bad"] = ((rng.rand(5, 33, 33) + 0.4 * m).astype(np.float32), m)
    m = _blobs(rng, 3, 48, 48, 1, 5)
    s = (np.round(rng.rand(3, 48, 48) * 32) / 32 * (1 + m)).astype(np.float32)
    z = rng.rand(3, 48, 48) < 0.85
    s[z] = np.where(rng.rand(int(z.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    out["zeros"] = (s.astype(np.float32), m)
    return out


def _limits(fpr):
    """The default limits plus one equal to a curve point's fpr (no interpolation at it)."""
    inner = fpr[(fpr > 0.1) & (fpr < 0.9)]
    exact = float(inner[0]) if len(inner) else float(fpr[len(fpr) // 2])
    assert 0.0 < exact <= 1.0 and exact in set(fpr.tolist())
    return np.array(list(LIMITS) + [exact], np.float64)


def main():
    data = {}
    for name, (s, m) in cases().items():
        sizes, R = scipy_sizes(m)
        fpr, pro = pro_curve_ref(s, sizes, R)
        lim = _limits(fpr)
        data[f"{name}/s"], data[f"{name}/m"] = s, m
        data[f"{name}/sizes"] = sizes.astype(np.uint32)
        data[f"{name}/counts"] = np.array([R, int((m == 0).sum()), int((m != 0).sum())], np.int64)
        data[f"{name}/fpr"], data[f"{name}/pro"] = fpr, pro
        data[f"{name}/limits"] = lim
        data[f"{name}/aupro"] = np.array([aupro_ref(fpr, pro, L) for L in lim])
    s, m = hashed_case(*LARGE_ARGS)
    sizes, R = scipy_sizes(m)
    fpr, pro = pro_curve_ref(s, sizes, R)
    lim = _limits(fpr)
    data["large/args"] = np.array(LARGE_ARGS, np.int64)
    data["large/checksum"] = np.array([s.astype(np.float64).sum(), float(m.sum()), float(sizes.sum()),
                                       float((sizes.astype(np.float64) ** 2).sum())])
    data["large/counts"] = np.array([R, int((m == 0).sum()), int((m != 0).sum())], np.int64)
    data["large/n_points"] = np.int64(len(fpr))
    data["large/fpr_every"], data["large/pro_every"] = fpr[::LARGE_STRIDE], pro[::LARGE_STRIDE]
    data["large/limits"] = lim
    data["large/aupro"] = np.array([aupro_ref(fpr, pro, L) for L in lim])
    np.savez_compressed(OUT, **data)
    print({k: v.round(6).tolist() for k, v in data.items() if k.endswith("/aupro")})
    print({k: v.tolist() for k, v in data.items() if k.endswith("/counts")})


if __name__ == "__main__":
    main()
