"""CPU: the host side of fc2 folded into the adjust conv in mlp_block: which launches have a folded form
(`srad_mlp_block_fold_supported`), the stage counts of the chain and of its folded form (`MlpChain` / `MlpFoldChain`,
csrc/swin_tiles.h) against the document's table, and the symbols."""
import ctypes as C
import os
import re

import pytest

from tests import mlp_fold_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (d, hidden, adjust outputs) -> (chain stages, folded stages): DESIGN.md 5k's table
STAGES = {(180, 360, 32): (10, 6), (212, 424, 32): (11, 7), (244, 488, 32): (11, 7), (276, 276, 32): (20, 13), (308, 308, 180): (22, 18)}


def supported(T, d, m, no, precision="bf16"):
    from srad_amd import _lib as L
    return bool(L.lib().srad_mlp_block_fold_supported(L.PRECISIONS[precision], T, d, m, no))


@pytest.mark.parametrize("d,m,no", MR.SHAPES)
@pytest.mark.parametrize("T", [64, 256, 4096, 8192, 65536])
def test_table_shapes_fold_at_every_tile_height_that_fits(d, m, no, T):
    """16-row tiles below 8192 rows, 32-row tiles from there, 64-row tiles from 32768: every one has a folded instance except
    64 rows at d = 244, whose folded tile [64][32 (8 + 16) + 16] bf16 does not fit the LDS next to the attention tile."""
    lds = (64 * 400 + 64 * (32 * ((d + 31) // 32 + (m + 31) // 32) + 16)) * 2 + (2560 + 64 * 16) * 4
    want = not (T >= 32768 and lds > 160 * 1024)
    assert (lds > 160 * 1024) == (d == 244)
    assert supported(T, d, m, no) == want


def test_what_has_no_folded_form():
    assert supported(64, 168, 360, 32) and supported(64, 180, 360, 28)          # the same-key shape, a part-filled column tile
    for no in (36, 64, 128):                                                     # one column group, more than two column tiles
        assert not supported(64, 180, 360, no)
    assert supported(64, 308, 308, 132)
    assert not supported(64, 180, 360, 32, "fp32") and not supported(64, 180, 360, 32, "bf16x3")
    assert not supported(72, 180, 360, 32)                                       # rows: whole 16-row tiles
    assert not supported(64, 180, 512, 32)                                       # not a shape of the fused second half


@pytest.mark.parametrize("d,m,no", MR.SHAPES)
def test_stage_counts_match_the_table(d, m, no):
    from srad_amd import _lib as L
    chain, folded = C.c_int(), C.c_int()
    assert L.lib().srad_mlp_block_stage_counts(d, m, no, C.byref(chain), C.byref(folded)) == 0
    assert (chain.value, folded.value) == STAGES[(d, m, no)]
    # the same numbers from the geometry: 128-column groups x 8-chunk k groups per phase; adjF is ONE k-split stage for <= 32
    # outputs, else column groups x k groups of the joined k range
    cdiv = MR.cdiv
    kc, kcm = cdiv(d, 32), cdiv(m, 32)
    gd, gm, gn, kgd, kgm = cdiv(d, 128), cdiv(m, 128), cdiv(no, 128), cdiv(kc, 8), cdiv(kcm, 8)
    assert chain.value == gd * kgd + gm * kgd + gd * kgm + gn * kgd
    assert folded.value == gd * kgd + gm * kgd + (1 if no <= 32 else gn * cdiv(kc + kcm, 8))
    if no <= 32:
        assert cdiv(kc + kcm, 4) <= 8                                            # a k part fits one register set


def test_stage_counts_of_a_width_without_a_folded_form():
    from srad_amd import _lib as L
    chain, folded = C.c_int(), C.c_int()
    assert L.lib().srad_mlp_block_stage_counts(180, 360, 64, C.byref(chain), C.byref(folded)) == 0
    assert (chain.value, folded.value) == (10, 0)
    assert L.lib().srad_mlp_block_stage_counts(180, 512, 32, C.byref(chain), C.byref(folded)) != 0


def test_symbols_declared_bound_and_exported():
    from srad_amd import _lib as L, ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srad.h")).read(), flags=re.S)
    lib = L.lib()
    for name in ("srad_mlp_block_fold_supported", "srad_op_mlp_block_folded", "srad_mlp_block_stage_counts"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in L.exported_symbols() and hasattr(lib, name), name
    assert callable(ops.mlp_block_folded) and callable(ops.mlp_block_fold_supported)
    n = lib.srad_prof_num_classes()
    assert lib.srad_prof_class_name(n - 1).decode() == "body_end"                 # no new profiler class
