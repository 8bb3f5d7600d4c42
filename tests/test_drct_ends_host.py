"""CPU: the host side of the DRCT body-end launch (csrc/kernels_drct_ends.hip) - the rule that selects it, the
refusals the op entry point makes before any launch, the ends_chain override id, and the new symbols."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F32, BF16X3 = 1, 0, 2
ERR_ARG = 1


def test_rule_truth_table():
    """bf16; E % 4 == 0; E <= 192; F == 64; C in {1, 3}; H, W >= 1; B * H * ceil(W / 16) <= CUs - on a CU count passed in."""
    from srad_amd import _lib as L, ops
    ok = lambda *a: bool(L.lib().srad_drct_ends_supported_cus(*a))
    assert ok(BF16, 180, 64, 1, 4, 32, 32, 256)                       # the benchmark: 4 * 32 * 2 = 256 tiles, one round
    assert not ok(BF16, 180, 64, 1, 4, 32, 32, 255)
    assert not ok(BF16, 180, 64, 1, 8, 32, 32, 256)                   # the anomaly-eval batch: two rounds
    assert ok(BF16, 180, 64, 3, 1, 8, 8, 256) and ok(BF16, 180, 64, 1, 1, 1, 1, 1)
    assert ok(BF16, 180, 64, 1, 1, 16, 33, 48) and not ok(BF16, 180, 64, 1, 1, 16, 33, 47)   # ceil(33 / 16) = 3 tiles per row
    assert not ok(F32, 180, 64, 1, 1, 8, 8, 256) and not ok(BF16X3, 180, 64, 1, 1, 8, 8, 256)
    assert ok(BF16, 192, 64, 1, 1, 8, 8, 256) and not ok(BF16, 196, 64, 1, 1, 8, 8, 256) and not ok(BF16, 182, 64, 1, 1, 8, 8, 256)
    assert ok(BF16, 4, 64, 1, 1, 8, 8, 256) and not ok(BF16, 0, 64, 1, 1, 8, 8, 256)
    assert not ok(BF16, 180, 32, 1, 1, 8, 8, 256) and not ok(BF16, 180, 128, 1, 1, 8, 8, 256)
    assert not ok(BF16, 180, 64, 2, 1, 8, 8, 256) and not ok(BF16, 180, 64, 4, 1, 8, 8, 256)
    assert not ok(BF16, 180, 64, 1, 0, 8, 8, 256) and not ok(BF16, 180, 64, 1, 1, 0, 8, 256) and not ok(BF16, 180, 64, 1, 1, 8, 0, 256)
    assert not ok(BF16, 180, 64, 1, 1 << 20, 1 << 10, 1 << 10, 256)   # the tile count does not wrap
    assert ops.drct_ends_supported("bf16", 180, 64, 1, 4, 32, 32, cus=256) and not ops.drct_ends_supported("fp32", 180, 64, 1, 4, 32, 32, cus=256)
    # without a device the library assumes 256 CUs; with one it asks: either way a single tile passes
    assert ops.drct_ends_supported("bf16", 180, 64, 1, 1, 1, 16)


def test_op_entry_point_refuses_before_any_launch():
    """Null pointers, E > 192, E % 4, F != 64, misaligned rows and a short scratch: refused on the host, pointers never
    dereferenced."""
    from srad_amd import _lib as L
    lib = L.lib()
    fake, odd = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 4)
    nb = lib.srad_op_drct_ends_scratch_bytes(180, 64)
    assert nb == 12 * 54 * 1024 + 4 * 54 * 1024

    def body(x=fake, ldx=308, E=180, F=64, feat0=fake, c2=fake, scratch=fake, bytes_=nb, w1=fake):
        return lib.srad_op_drct_body_end(x, ldx, 1, 8, 8, E, F, fake, fake, w1, fake, feat0, fake, fake, c2, scratch, C.c_size_t(bytes_), None)

    for call in (lambda: body(x=None), lambda: body(w1=None), lambda: body(feat0=None), lambda: body(c2=None), lambda: body(scratch=None)):
        assert call() == ERR_ARG and b"null argument" in lib.srad_last_error()
    for call in (lambda: body(E=196), lambda: body(E=182), lambda: body(E=0)):
        assert call() == ERR_ARG and b"multiple of 4, at most 192" in lib.srad_last_error()
    assert body(F=32) == ERR_ARG and b"F = 32 must be 64" in lib.srad_last_error()
    for call in (lambda: body(ldx=306), lambda: body(ldx=176), lambda: body(x=odd), lambda: body(feat0=odd), lambda: body(c2=odd)):
        assert call() == ERR_ARG and b"16-byte aligned" in lib.srad_last_error()
    for call in (lambda: body(bytes_=1024), lambda: body(scratch=C.c_void_p((1 << 20) + 16))):
        assert call() == ERR_ARG and b"scratch" in lib.srad_last_error()


def test_override_id_round_trips():
    from srad_amd import _lib as L, ops
    lib = L.lib()
    i = ops.PLAN_PATHS["ends_chain"]
    assert i == 32 and lib.srad_get_path_override(i) == 0
    assert lib.srad_set_path_override(i, 1) == 0 and lib.srad_get_path_override(i) == 1
    assert lib.srad_get_path_override(ops.PLAN_PATHS["tail_chain"]) == 0          # independent of its neighbour
    assert lib.srad_set_path_override(i, 0) == 0 and lib.srad_get_path_override(i) == 0
    with ops.path_override(ends_chain=True):
        assert lib.srad_get_path_override(i) == 1
    assert lib.srad_get_path_override(i) == 0
    for unknown in (18, 19, 31, 33):                                              # the first range still ends at 18
        assert lib.srad_set_path_override(unknown, 1) == ERR_ARG and lib.srad_get_path_override(unknown) == -1


def test_symbols_declared_bound_and_exported():
    from srad_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srad.h")).read(), flags=re.S)
    lib = L.lib()
    for name in ("srad_drct_ends_supported", "srad_drct_ends_supported_cus", "srad_op_drct_ends_scratch_bytes", "srad_op_drct_body_end"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in L.exported_symbols() and hasattr(lib, name), name
    assert "SRAD_PATH_ENDS_CHAIN = 32" in text and "SRAD_PATH_END = 18" in text and "SRAD_PATH_PLAN2_END = 33" in text
    n = lib.srad_prof_num_classes()
    names = [lib.srad_prof_class_name(k).decode() for k in range(n)]
    assert names[-1] == "body_end" and names[-2] == "tail_fold" and "layout" in names
