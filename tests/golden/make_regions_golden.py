"""Writes tests/golden/regions_golden.npz: the region tables (DESIGN.md "Defect regions") that scipy gives for the small cases
of tests/golden/pro_golden.npz, in two roles each:

  <case>/gt/...    regions of the stored mask, peaks from the stored scores, ``other`` = the prediction ``scores > T``;
  <case>/pred/...  regions of that prediction, peaks from the stored scores, ``other`` = the stored mask.

    python tests/golden/make_regions_golden.py

Per image: ``scipy.ndimage.label(m, np.ones((3, 3)))`` numbers the regions (in the order of their first pixels in raster order),
``find_objects`` gives the boxes, ``sum`` the areas, coordinate sums and overlaps, ``maximum`` the peak and
``maximum_position`` where it is.  scipy does not say which of several equal maxima ``maximum_position`` returns, and the
definition wants the first in raster order with -0.0 equal to +0.0, so it is asked for the position of the maximum of a key
without ties: (rank of the score among the image's distinct scores) * H * W + (H * W - 1 - linear index).

Only the tables are stored; the masks and scores are read from pro_golden.npz.  The tests need no scipy."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "regions_golden.npz")
SMALL = ["blobs", "corner", "borders", "wrap64", "spiral", "almost_full", "good_plus_one_bad", "zeros"]
T = 0.5                                                            # the prediction of the swapped role: scores > T
FIELDS = ("image", "area", "box", "sum_y", "sum_x", "overlap", "peak", "peak_y", "peak_x")


def scipy_table(masks, scores, other):
    from scipy import ndimage
    n, H, W = masks.shape
    yy, xx = np.mgrid[:H, :W]
    cols = {k: [] for k in FIELDS}
    for i in range(n):
        lab, k = ndimage.label(masks[i] != 0, structure=np.ones((3, 3), int))
        if k == 0:
            continue
        idx = np.arange(1, k + 1)
        _, rank = np.unique(scores[i].astype(np.float64), return_inverse=True)      # -0.0 and +0.0 are one value
        key = rank.reshape(H, W).astype(np.int64) * (H * W) + (H * W - 1 - np.arange(H * W, dtype=np.int64).reshape(H, W))
        pos = ndimage.maximum_position(key, lab, idx)
        cols["image"] += [i] * k
        cols["area"] += np.rint(ndimage.sum(np.ones((H, W)), lab, idx)).astype(np.int64).tolist()
        cols["box"] += [(s[0].start, s[1].start, s[0].stop - 1, s[1].stop - 1) for s in ndimage.find_objects(lab)]
        cols["sum_y"] += np.rint(ndimage.sum(yy.astype(np.float64), lab, idx)).astype(np.int64).tolist()
        cols["sum_x"] += np.rint(ndimage.sum(xx.astype(np.float64), lab, idx)).astype(np.int64).tolist()
        cols["overlap"] += np.rint(ndimage.sum((other[i] != 0).astype(np.float64), lab, idx)).astype(np.int64).tolist()
        cols["peak"] += (np.asarray(ndimage.maximum(scores[i], lab, idx), np.float32) + np.float32(0.0)).tolist()
        cols["peak_y"] += [p[0] for p in pos]
        cols["peak_x"] += [p[1] for p in pos]
    dt = dict(sum_y=np.int64, sum_x=np.int64, peak=np.float32)
    out = {k: np.array(v, dt.get(k, np.int32)) for k, v in cols.items()}
    out["box"] = out["box"].reshape(-1, 4)
    return out


def main():
    pro = np.load(os.path.join(HERE, "pro_golden.npz"))
    data = {"threshold": np.float64(T)}
    for case in SMALL:
        s, m = pro[f"{case}/s"], pro[f"{case}/m"] != 0
        pred = s.astype(np.float64) > T
        for role, (a, b) in (("gt", (m, pred)), ("pred", (pred, m))):
            for k, v in scipy_table(a, s, b).items():
                data[f"{case}/{role}/{k}"] = v
        print(case, "regions:", len(data[f"{case}/gt/area"]), "predicted:", len(data[f"{case}/pred/area"]))
    np.savez_compressed(OUT, **data)


if __name__ == "__main__":
    main()
