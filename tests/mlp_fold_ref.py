"""numpy restatement of a Swin block's folded second-half weight (csrc/mlp_fold.h), shared by the host and the
GPU tests:  adjust(x1 + fc2(h) + b2) = [A | A W2] [x1 | h] + (A b2 + b_a).  Everything in float64; callers round."""
import numpy as np

SHAPES = [(180, 360, 32), (212, 424, 32), (244, 488, 32), (276, 276, 32), (308, 308, 180)]      # (d, hidden, adjust outputs) of DRCT-L


def cdiv(a, b):
    return (a + b - 1) // b


def up256(n):
    return cdiv(n, 256) * 256


def layout(d, m, no):
    """Byte offsets of a block's region, in the order of mlp_fold.h's MlpFoldLayout, and kf = the columns of Wf."""
    kc, kcm = cdiv(d, 32), cdiv(m, 32)
    kf = 32 * (kc + kcm)
    sizes = [("w2", d * m * 4), ("b2", d * 4), ("a", no * d * 4), ("ba", no * 4), ("wf", no * kf * 4), ("pack", cdiv(no, 128) * 128 * kf * 2),
             ("bias", no * 4)]
    off, out = 0, {}
    for name, nbytes in sizes:
        out[name] = off
        off += up256(nbytes)
    out["bytes"] = off
    out["kf"] = kf
    out["kc32"] = 32 * kc
    return out


def compose(w2, b2, a, ba):
    """(Wf [no, kf], bf [no]) in float64 from fc2.weight [d, m], fc2.bias [d], adjust.weight [no, d], adjust.bias [no]."""
    w2, b2, a, ba = (np.asarray(t, dtype=np.float64) for t in (w2, b2, a, ba))
    d, m = w2.shape
    no = a.shape[0]
    lay = layout(d, m, no)
    wf = np.zeros((no, lay["kf"]))
    wf[:, :d] = a
    wf[:, lay["kc32"]:lay["kc32"] + m] = a @ w2
    return wf, a @ b2 + ba


def padding_mask(d, m, no):
    """True where Wf holds padding (columns [d, 32 KC) and [32 KC + m, kf))."""
    lay = layout(d, m, no)
    mask = np.ones((no, lay["kf"]), dtype=bool)
    mask[:, :d] = False
    mask[:, lay["kc32"]:lay["kc32"] + m] = False
    return mask
