"""CPU: the host side of the folded Swin-block second half (csrc/mlp_fold.h): the region layout the library
reports against its numpy restatement for DRCT-L's five block shapes, the launch-plan override's id, and the symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import mlp_fold_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1


def lib_layout(d, m, no):
    from srad_amd import _lib as L
    off = (C.c_size_t * 8)()
    kf = C.c_int()
    assert L.lib().srad_op_mlp_fold_layout(d, m, no, off, C.byref(kf)) == 0
    return dict(zip(("w2", "b2", "a", "ba", "wf", "pack", "bias", "bytes"), [int(v) for v in off])), kf.value


@pytest.mark.parametrize("d,m,no", MR.SHAPES + [(168, 360, 32), (180, 360, 28), (32, 32, 4)])
def test_layout_matches_the_restatement(d, m, no):
    from srad_amd import _lib as L
    got, kf = lib_layout(d, m, no)
    ref = MR.layout(d, m, no)
    assert kf == ref["kf"] == 32 * ((d + 31) // 32 + (m + 31) // 32) and kf % 32 == 0
    for k in got:
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert all(v % 256 == 0 for v in got.values())
    assert L.lib().srad_op_mlp_fold_scratch_bytes(d, m, no) == got["bytes"]
    # the regions follow one another without overlap, in the header's order, and the pack holds 128-row-padded tiles of 1 KB
    order = ["w2", "b2", "a", "ba", "wf", "pack", "bias", "bytes"]
    sizes = [d * m * 4, d * 4, no * d * 4, no * 4, no * kf * 4, (no + 127) // 128 * 128 * kf * 2, no * 4]
    for a, b, n in zip(order, order[1:], sizes):
        assert got[a] + n <= got[b], (a, b)
    assert sizes[5] % 1024 == 0


def test_known_sizes_of_the_five_shapes():
    """Wf's column counts and the per-model source bytes the documents quote (DRCT-L: 12 RDGs)."""
    kfs = [lib_layout(*s)[1] for s in MR.SHAPES]
    assert kfs == [32 * (6 + 12), 32 * (7 + 14), 32 * (8 + 16), 32 * (9 + 9), 32 * (10 + 10)]
    src = sum(4 * (d * m + d + no * d + no) for d, m, no in MR.SHAPES) * 12
    assert src == 25485696                                     # 24.3 MiB of fp32 sources
    total = sum(lib_layout(*s)[0]["bytes"] for s in MR.SHAPES) * 12
    print("DRCT-L: sources", src, "bytes, regions", total, "bytes")
    assert src < total < 2 * src


def test_restatement_composes_the_algebra():
    """adjust(x1 + fc2(h) + b2) == Wf [x1 | h] + bf in float64, on the padded layout, with zero padding."""
    rng = np.random.default_rng(0)
    d, m, no = 44, 72, 12
    w2, b2, a, ba = rng.standard_normal((d, m)), rng.standard_normal(d), rng.standard_normal((no, d)), rng.standard_normal(no)
    x1, h = rng.standard_normal((5, d)), rng.standard_normal((5, m))
    wf, bf = MR.compose(w2, b2, a, ba)
    lay = MR.layout(d, m, no)
    k = np.zeros((5, lay["kf"]))
    k[:, :d] = x1
    k[:, lay["kc32"]:lay["kc32"] + m] = h
    ref = (x1 + h @ w2.T + b2) @ a.T + ba
    assert np.abs(k @ wf.T + bf - ref).max() < 1e-12
    assert not wf[MR.padding_mask(d, m, no)].any() and wf[~MR.padding_mask(d, m, no)].all()


def test_override_id_round_trips():
    from srad_amd import _lib as L, ops
    lib = L.lib()
    i = ops.PLAN_PATHS["fc2_chain"]
    assert i == 48 and "fc2_chain" not in ops.PATHS and lib.srad_get_path_override(i) == 0
    assert lib.srad_set_path_override(i, 1) == 0 and lib.srad_get_path_override(i) == 1
    assert lib.srad_get_path_override(ops.PLAN_PATHS["ends_chain"]) == 0          # independent of the other ranges
    assert lib.srad_set_path_override(i, 0) == 0 and lib.srad_get_path_override(i) == 0
    with ops.path_override(fc2_chain=True):
        assert lib.srad_get_path_override(i) == 1
    assert lib.srad_get_path_override(i) == 0
    for unknown in list(range(33, 48)) + [49, 18, 31]:
        assert lib.srad_set_path_override(unknown, 1) == ERR_ARG and lib.srad_get_path_override(unknown) == -1


def test_symbols_declared_bound_and_exported():
    from srad_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srad.h")).read(), flags=re.S)
    lib = L.lib()
    for name in ("srad_op_mlp_fold_scratch_bytes", "srad_op_mlp_fold_layout", "srad_op_mlp_fold_compose", "srad_swin_block_fold_supported",
                 "srad_op_swin_block_folded"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in L.exported_symbols() and hasattr(lib, name), name
    assert "SRAD_PATH_FC2_CHAIN = 48" in text and "SRAD_PATH_PLAN3_END = 49" in text and "SRAD_PATH_PLAN2_END = 33" in text
    n = lib.srad_prof_num_classes()
    assert lib.srad_prof_class_name(n - 1).decode() == "body_end"                 # no new profiler class
