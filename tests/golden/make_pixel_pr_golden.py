"""Writes tests/golden/pixel_pr_golden.npz: precision-recall cases and what scikit-learn (1.7.2) returns for them - the numbers
srad_pixel_pr and srad_average_precision must reproduce: ``average_precision_score`` to 1e-12, the points of
``precision_recall_curve`` to 1e-15 with bitwise thresholds, and the best-F1 point exactly.

    python tests/golden/make_pixel_pr_golden.py

The cases named in ``AUC_CASES`` take their scores and labels from tests/golden/pixel_auc_golden.npz and are not stored again;
the others are stored as arrays.  Per case: ``ap`` (sklearn), ``best`` = (tp, fp, float32 bits of the score) of the best-F1
point and ``n_points``; the curve (``precision``, ``recall``, ``thresholds``: sklearn's arrays reversed to run from the highest
score down, without the (1, 0) end point it appends, and with a -0.0 threshold written as +0.0, which is what the device decodes
from its keys) is stored where it has at most ``CURVE_MAX`` points.  For longer curves, and for the large cases the GPU test
builds from a seed, the tests use ``pr_ref``, the numpy restatement below, which is checked here against sklearn on every case.

The best point is not sklearn's to give: float F1 values can tie (or fail to) spuriously, so ``best_point`` compares
F1 = 2 tp / (tp + fp + P) as fractions of Python integers; of equal F1 values the highest threshold wins.

sklearn refuses infinite scores.  The ranking is all that the metrics see, so ``sklearn_curve`` hands it the ``inf_zero`` case
with +-inf replaced by +-FLT_MAX, which no other score of the case equals, and writes the two thresholds back."""
import math
import os
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pixel_pr_golden.npz")
AUC_CASES = ["continuous", "ties8", "signed_zeros", "negative", "all_equal", "perfect", "inverse", "n3", "odd_n"]
OWN_CASES = ["quant3pct", "inf_zero", "single_pos", "all_pos", "one_score", "n1", "f1_tie", "f1_tie_far"]
CURVE_MAX = 4096


def pr_ref(s, y):
    """(precision f64, recall f64, thresholds f32, tp i64, fp i64) with one point per distinct score from the highest down
    (-0.0 == +0.0, written +0.0): the point of score t is "predict iff score >= t"."""
    s = np.asarray(s, np.float32).ravel() + np.float32(0.0)                # -0.0 + 0.0 = +0.0
    y = np.asarray(y).ravel() != 0
    order = np.argsort(-s.astype(np.float64), kind="stable")
    ss, yy = s[order], y[order]
    ends = np.r_[np.nonzero(ss[1:] != ss[:-1])[0], len(ss) - 1]
    tp = np.cumsum(yy, dtype=np.int64)[ends]
    fp = ends + 1 - tp
    with np.errstate(invalid="ignore"):
        return tp / (tp + fp), tp / tp[-1], ss[ends], tp, fp


def ap_ref(tp, fp):
    """sum_k (R_k - R_k-1) P_k = (1 / P) sum_k (tp_k - tp_k-1) tp_k / (tp_k + fp_k), each term rounded once, summed exactly."""
    d = np.diff(np.r_[0, tp])
    return math.fsum((d * tp / (tp + fp)).tolist()) / int(tp[-1])


def best_point(tp, fp):
    """Index of the highest F1 = 2 tp / (tp + fp + P), exactly; the first (highest threshold) of equal ones."""
    P = int(tp[-1])
    best, best_f = 0, Fraction(-1)
    for k, (a, b) in enumerate(zip(tp.tolist(), fp.tolist())):
        f = Fraction(2 * a, a + b + P)
        if f > best_f:
            best, best_f = k, f
    return best


def own_cases():
    rng = np.random.RandomState(31)
    out = {}
    n = 12000
    y = (rng.rand(n) < 0.03).astype(np.uint8)
    out["quant3pct"] = ((np.round((rng.standard_normal(n) + 1.5 * y) * 8) / 8).astype(np.float32), y)     # ~60 distinct scores
    s = np.where(rng.rand(600) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    s[rng.rand(600) < 0.3] = np.float32(2.5)
    s[rng.rand(600) < 0.3] = np.float32(-1e-40)                                                             # a denormal
    s[[7, 99, 300]], s[[11, 12, 500]] = np.float32(np.inf), np.float32(-np.inf)
    out["inf_zero"] = (s, (rng.rand(600) < 0.4).astype(np.uint8))
    y = np.zeros(500, np.uint8)
    y[123] = 1
    out["single_pos"] = (rng.standard_normal(500).astype(np.float32), y)
    out["all_pos"] = ((rng.randint(0, 40, 300) / 8).astype(np.float32), np.ones(300, np.uint8))
    out["one_score"] = (np.full(400, -3.5, np.float32), (rng.rand(400) < 0.1).astype(np.uint8))
    out["n1"] = (np.array([0.25], np.float32), np.array([1], np.uint8))
    # P = 2: (tp 1, fp 0) has F1 2/3 and so has (tp 2, fp 2); the higher threshold, score 3, is the answer
    out["f1_tie"] = (np.array([3, 2, 2, 2, 1, 1, 1], np.float32), np.array([1, 1, 0, 0, 0, 0, 0], np.uint8))
    # P = 400, shuffled: (tp 100, fp 0) has F1 200 / 500 = 2/5 and so has (tp 200, fp 400), 400 / 1000; the last point has 1/4
    s = np.concatenate([np.full(100, 9.0), np.full(500, 5.0), np.full(2200, 1.0)]).astype(np.float32)
    y = np.concatenate([np.ones(100), np.r_[np.ones(100), np.zeros(400)], np.r_[np.ones(200), np.zeros(2000)]]).astype(np.uint8)
    p = rng.permutation(len(s))
    out["f1_tie_far"] = (s[p], y[p])
    return out


def all_cases():
    g = np.load(os.path.join(HERE, "pixel_auc_golden.npz"))
    out = {c: (g[f"{c}/s"], g[f"{c}/y"]) for c in AUC_CASES}
    out.update(own_cases())
    return out


def sklearn_curve(s, y):
    """(ap, precision, recall, thresholds) of sklearn, the curve from the highest score down without the appended (1, 0)."""
    from sklearn.metrics import average_precision_score, precision_recall_curve
    big = np.finfo(np.float32).max
    assert not np.any(np.abs(s[np.isfinite(s)]) == big)
    finite = np.clip(s, -big, big)
    p, r, t = precision_recall_curve(y, finite)
    t = t[::-1] + np.float32(0.0)
    t[t == big], t[t == -big] = np.float32(np.inf), np.float32(-np.inf)
    return float(average_precision_score(y, finite)), p[-2::-1], r[-2::-1], t


def main():
    data, own = {}, set(OWN_CASES)
    for name, (s, y) in all_cases().items():
        prec, rec, thr, tp, fp = pr_ref(s, y)
        ap, sk_p, sk_r, sk_t = sklearn_curve(s, y)
        assert len(sk_t) == len(thr) and sk_t.dtype == np.float32 and np.array_equal(sk_t.view(np.uint32), thr.view(np.uint32)), name
        assert np.abs(sk_p - prec).max() <= 1e-15 and np.abs(sk_r - rec).max() <= 1e-15, name
        assert abs(ap - ap_ref(tp, fp)) <= 1e-15, (name, ap, ap_ref(tp, fp))
        k = best_point(tp, fp)
        if name in own:
            data[f"{name}/s"], data[f"{name}/y"] = s, y
        data[f"{name}/ap"] = np.float64(ap)
        data[f"{name}/best"] = np.array([tp[k], fp[k], int(thr[k:k + 1].view(np.uint32)[0])], np.int64)
        data[f"{name}/n_points"] = np.int64(len(thr))
        if len(thr) <= CURVE_MAX:
            data[f"{name}/precision"], data[f"{name}/recall"], data[f"{name}/thresholds"] = sk_p.copy(), sk_r.copy(), sk_t.copy()
        print(f"{name}: n={len(s)} points={len(thr)} ap={ap:.6f} |ap - restatement|={abs(ap - ap_ref(tp, fp)):.1e} "
              f"best tp={tp[k]} fp={fp[k]} score={thr[k]!r}")
    assert int(data["f1_tie/best"][0]) == 1 and int(data["f1_tie_far/best"][0]) == 100             # the ties are pinned
    np.savez_compressed(OUT, **data)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
