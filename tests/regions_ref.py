"""A plain numpy restatement of the region table (DESIGN.md "Defect regions") for the tests: a dictionary union-find in the
manner of ``uf_sizes`` of tests/golden/make_pro_golden.py, whose links point to the smaller (y, x), so a root is its region's
first pixel in raster order; then one pass over each region's pixels.  No scipy, no GPU."""
import numpy as np

FIELDS = ("image", "area", "box", "sum_y", "sum_x", "overlap")
PEAK = ("peak", "peak_y", "peak_x")


def label_roots(mask):
    """{pixel (y, x): root (y, x)} of one image's 8-connected components; the root is the component's smallest (y, x)."""
    pts = list(zip(*[a.tolist() for a in np.nonzero(np.asarray(mask) != 0)]))
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
    return {p: find(p) for p in pts}


def region_table_ref(masks, scores=None, other=None):
    """The table of masks [n, H, W] as numpy arrays under FIELDS (+ PEAK with scores) and ``n_regions``; rows ordered by image
    and by each region's first pixel.  The peak is the largest score that is not NaN, -0.0 equal to +0.0, at the first pixel in
    raster order that has it; NaN and (-1, -1) for a region of NaN scores only.  ``n_nan``: NaN scores inside regions."""
    masks = np.asarray(masks)
    rows, n_nan = [], 0
    for i in range(masks.shape[0]):
        roots = label_roots(masks[i])
        members = {}
        for p in sorted(roots):                                # raster order within every region
            members.setdefault(roots[p], []).append(p)
        for root in sorted(members):
            ys = np.array([p[0] for p in members[root]], np.int64)
            xs = np.array([p[1] for p in members[root]], np.int64)
            row = dict(image=i, area=len(ys), box=(ys.min(), xs.min(), ys.max(), xs.max()), sum_y=ys.sum(), sum_x=xs.sum(),
                       overlap=int((np.asarray(other)[i, ys, xs] != 0).sum()) if other is not None else 0)
            if scores is not None:
                v = np.asarray(scores)[i, ys, xs].astype(np.float32)
                nan = np.isnan(v)
                n_nan += int(nan.sum())
                if nan.all():
                    row.update(peak=np.float32(np.nan), peak_y=-1, peak_x=-1)
                else:
                    k = int(np.argmax(np.where(nan, -np.inf, v)))      # the first of equal maxima; -0.0 == +0.0
                    row.update(peak=v[k] + np.float32(0.0), peak_y=ys[k], peak_x=xs[k])
            rows.append(row)
    out = dict(image=np.array([r["image"] for r in rows], np.int32), area=np.array([r["area"] for r in rows], np.int32),
               box=np.array([r["box"] for r in rows], np.int32).reshape(-1, 4),
               sum_y=np.array([r["sum_y"] for r in rows], np.int64), sum_x=np.array([r["sum_x"] for r in rows], np.int64),
               overlap=np.array([r["overlap"] for r in rows], np.int32))
    if scores is not None:
        out.update(peak=np.array([r["peak"] for r in rows], np.float32), peak_y=np.array([r["peak_y"] for r in rows], np.int32),
                   peak_x=np.array([r["peak_x"] for r in rows], np.int32))
    out["n_regions"], out["n_nan"] = len(rows), n_nan
    return out


def assert_tables_equal(got, want, peak=True, where=""):
    """Every field of ``want`` (numpy) equals ``got`` (GPU tensors or numpy), exactly; a NaN peak equals a NaN peak."""
    assert int(got["n_regions"]) == int(want["n_regions"]), (where, got["n_regions"], want["n_regions"])
    for k in FIELDS + (PEAK if peak else ()):
        g = got[k]
        g = g.cpu().numpy() if hasattr(g, "cpu") else np.asarray(g)
        w = np.asarray(want[k])
        assert g.shape == w.shape, (where, k, g.shape, w.shape)
        assert np.array_equal(g.astype(w.dtype), w, equal_nan=(k == "peak")), (where, k, g[:8], w[:8])
