"""CPU: the C-ABI library loads without a GPU and exports every symbol include/srad.h declares; the
product path refuses to run without the HIP engine (no CPU fallback)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "srad.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(srad_[a-z0-9_]+)\s*\(", text)))


def test_header_and_bindings_agree():
    from srad_amd import _lib
    hdr = _header_symbols()
    assert len(hdr) >= 35
    assert hdr == _lib.exported_symbols(), set(hdr) ^ set(_lib.exported_symbols())


def test_library_exports_every_declared_symbol():
    from srad_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build libsrad.so first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = _lib.lib()                       # dlopen works without a GPU; raises on a missing symbol
    for name in _header_symbols():
        assert hasattr(lib, name), name
    assert lib.srad_version() >= 100
    assert lib.srad_last_error() is not None


def test_argument_errors_without_gpu():
    """Host-side validation paths that need no device."""
    import ctypes as C
    from srad_amd import _lib as L
    lib = L.lib()
    h = C.c_void_p()
    bad = L.DrctConfig(2, 32, 8, 4, 180, 12, 6, 32, 64, 2.0, 1.0, 0, 0)         # in_chans = 2
    assert lib.srad_drct_create(C.byref(bad), C.byref(h)) != 0
    assert b"in_chans" in lib.srad_last_error()
    ok = L.DrctConfig(1, 32, 8, 4, 180, 12, 6, 32, 64, 2.0, 1.0, 1, 0)
    assert lib.srad_drct_create(C.byref(ok), C.byref(h)) == 0
    assert lib.srad_drct_num_params(h) == 916 + 0 or lib.srad_drct_num_params(h) > 900
    nb = C.c_size_t()
    assert lib.srad_drct_workspace_bytes(h, 4, 30, 32, C.byref(nb)) != 0        # not a multiple of the window
    assert b"multiple of the window" in lib.srad_last_error()
    assert lib.srad_drct_workspace_bytes(h, 4, 32, 32, C.byref(nb)) == 0 and nb.value > 0
    f = C.c_double()
    assert lib.srad_drct_flops(h, 1, 32, 32, C.byref(f)) == 0
    assert abs(f.value / 1e9 - 60.39) < 0.4                                      # 60.39 GFLOP / image
    lib.srad_drct_destroy(h)
    dn = L.DrnConfig(3, 4, 40, 20, 0.2, 255.0, 0, 0)
    assert lib.srad_drn_create(C.byref(dn), C.byref(h)) == 0
    assert lib.srad_drn_num_params(h) == 664
    assert lib.srad_drn_flops(h, 1, 64, 64, C.byref(f)) == 0
    assert abs(f.value / 1e9 - 199.51) < 1.5                                     # 199.51 GFLOP / 256^2 RGB image
    lib.srad_drn_destroy(h)
    # srad_op_gemm_plan is host code: the launcher's decision for srad_op_gemm's arguments, pointers never dereferenced
    plan, fake = L.GemmPlan(), C.c_void_p(1 << 20)
    args = [L.PREC_BF16, fake, 180, 1, 1, 12293, 180, fake, 100, 1, 1, fake, None, None, 0, 0.0, 1.0, None, 0, fake, 100, 0, 0, fake,
            C.c_size_t(lib.srad_op_gemm_scratch_bytes(L.PREC_BF16, 100, 180, 1)), None]
    assert lib.srad_op_gemm_plan(*args, C.byref(plan)) == 0
    assert (L.GEMM_FAMILIES[plan.family], plan.BM, plan.BN, plan.CPS, plan.grid_x, plan.grid_y) == ("tiled", 64, 64, 4, 2, 193)
    assert lib.srad_op_gemm_plan(*args, None) != 0 and b"null argument" in lib.srad_last_error()
    args[1] = None
    assert lib.srad_op_gemm_plan(*args, C.byref(plan)) != 0 and b"null argument" in lib.srad_last_error()
    # srad_op_wgrad_plan / srad_op_wgrad_deferred_plan: the weight-gradient launchers' decisions, host code as well
    wp = L.WgradPlan()
    wargs = [L.PREC_BF16, fake, 84, 0, 0, fake, 84, 0, 1, 17, 23, 80, 80, 80, 80, 0, 0, 9, 1, None]
    assert lib.srad_op_wgrad_plan(*wargs, C.byref(wp)) == 0
    assert (L.WGRAD_FAMILIES[wp.family[0]], wp.CONV, wp.launches, wp.ksplit[0], wp.rows_per[0], wp.grid[0]) == ("w80", 1, 1, 2, 256, 18)
    wargs[0] = L.PREC_F32
    assert lib.srad_op_wgrad_plan(*wargs, C.byref(wp)) == 0 and L.WGRAD_FAMILIES[wp.family[0]] == "tile64" and (wp.tn[0], wp.tc[0]) == (2, 2)
    assert lib.srad_op_wgrad_plan(*wargs, None) != 0 and b"null argument" in lib.srad_last_error()
    wargs[1] = None
    assert lib.srad_op_wgrad_plan(*wargs, C.byref(wp)) != 0 and b"null argument" in lib.srad_last_error()
    st = L.WqStep()
    st.kind = L.WQ_WGRAD_DEFERRED
    for j, v in enumerate([180, 0, 180, 1, 1000, 180, 180, 0]):
        st.i[j] = v
    for j in range(3):
        st.p[j] = 1 << 20
    assert lib.srad_op_wgrad_deferred_plan(L.PREC_BF16, C.byref(st), 1, C.byref(wp)) == 0
    assert (L.WGRAD_FAMILIES[wp.family[0]], wp.FULL[0], wp.XH[0], wp.YH[0], wp.ksplit[0], wp.nblk[0]) == ("multi", 0, 1, 0, 4, 36)
    st.kind = L.WQ_WGRAD
    assert lib.srad_op_wgrad_deferred_plan(L.PREC_BF16, C.byref(st), 1, C.byref(wp)) != 0 and b"not a deferred" in lib.srad_last_error()
    assert lib.srad_op_wgrad_deferred_plan(L.PREC_BF16, None, 1, C.byref(wp)) != 0
    # srad_op_wgrad_ex checks before it launches: real extents beyond the stored ones are refused without a device
    assert lib.srad_op_wgrad_ex(L.PREC_F32, fake, 8, 0, fake, 8, 1, 1, 16, 4, 4, 5, 4, 0, 0, 1, 1, None, 1.0, fake, None, fake, None) != 0
    assert b"bad real extents" in lib.srad_last_error()
    auc = C.c_double()
    y = (C.c_int32 * 4)(0, 0, 1, 1)
    s = (C.c_double * 4)(0.1, 0.4, 0.35, 0.8)
    assert lib.srad_roc_auc(y, s, 4, C.byref(auc)) == 0 and abs(auc.value - 0.75) < 1e-15


def test_wgrad_queue_script_argument_errors_without_gpu():
    """srad_op_wgrad_queue_script checks its budget, every step kind and every step's pointers before it launches anything."""
    import ctypes as C
    from srad_amd import _lib as L
    lib = L.lib()
    SRAD_ERR_ARG = 1
    ws, ws_bytes = C.c_void_p(1 << 20), 1 << 16              # never dereferenced: every call below fails in the checks
    fake = 1 << 12
    n, why = C.c_int(-1), (C.c_int * 4)()

    def call(steps, budget=1024, workspace=ws, n_out=C.byref(n)):
        arr = (L.WqStep * max(1, len(steps)))(*steps)
        return lib.srad_op_wgrad_queue_script(L.PREC_F32, arr if steps else None, len(steps), budget, workspace, ws_bytes, n_out, why, 4, None)

    def step(kind, ptrs=()):
        st = L.WqStep()
        st.kind = kind
        for j, v in enumerate(ptrs):
            st.p[j] = v
        return st

    flush = step(L.WQ_FLUSH)
    assert call([flush], budget=ws_bytes // 4 + 1) == SRAD_ERR_ARG and b"does not fit the workspace" in lib.srad_last_error()
    assert call([flush], budget=0) == SRAD_ERR_ARG
    assert call([flush, step(7)]) == SRAD_ERR_ARG and b"step 1: unknown step kind 7" in lib.srad_last_error()
    assert call([step(0)]) == SRAD_ERR_ARG and b"unknown step kind" in lib.srad_last_error()
    assert call([]) == SRAD_ERR_ARG and b"null argument" in lib.srad_last_error()
    assert call([flush], workspace=None) == SRAD_ERR_ARG and b"null argument" in lib.srad_last_error()
    assert call([flush], n_out=None) == SRAD_ERR_ARG and b"null argument" in lib.srad_last_error()
    assert call([flush], workspace=C.c_void_p((1 << 20) + 16)) == SRAD_ERR_ARG and b"256-byte aligned" in lib.srad_last_error()
    for kind, nptr in ((L.WQ_WGRAD, 3), (L.WQ_WGRAD_DEFERRED, 3), (L.WQ_ATTN_BWD, 5)):
        for missing in range(nptr):                          # each required pointer in turn
            ptrs = [None if j == missing else fake for j in range(nptr)]
            assert call([flush, step(kind, ptrs)]) == SRAD_ERR_ARG and b"step 1: null argument" in lib.srad_last_error(), (kind, missing)
    for missing in (0, 1, 2, 4):                             # LayerNorm: dxn, x, gamma, out (dres, dgamma, dbeta are optional)
        ptrs = [None if j == missing else fake for j in range(5)]
        assert call([step(L.WQ_LN_BWD, ptrs)]) == SRAD_ERR_ARG and b"step 0: null argument" in lib.srad_last_error(), missing
    assert n.value == -1                                     # nothing was reported by a call that failed
    h = C.c_void_p()
    ok = L.DrctConfig(1, 32, 8, 4, 180, 12, 6, 32, 64, 2.0, 1.0, 1, 0)
    assert lib.srad_drct_create(C.byref(ok), C.byref(h)) == 0
    assert lib.srad_drct_train_set_wgrad_budget(h, 1 << 20) == 0
    assert lib.srad_drct_train_set_wgrad_budget(h, (1 << 20) + 4) == SRAD_ERR_ARG and b"multiple of 512" in lib.srad_last_error()
    assert lib.srad_drct_train_set_wgrad_budget(h, lib.srad_op_wgrad_workspace_bytes() + 512) == SRAD_ERR_ARG
    assert lib.srad_drct_train_set_wgrad_budget(h, 0) == SRAD_ERR_ARG
    assert lib.srad_drct_train_set_wgrad_budget(None, 512) == SRAD_ERR_ARG
    lib.srad_drct_destroy(h)


def test_path_overrides_ignore_the_environment():
    """Kernel paths follow shape and precision, plus the explicit overrides of srad_set_path_override: a fresh process with
    an old A/B switch in its environment starts with every override off; set / get round-trip; an unknown path is an error."""
    import subprocess
    import sys
    child = r"""
import ctypes as C
from srad_amd import _lib as L, ops
lib = L.lib()
assert [lib.srad_get_path_override(i) for i in ops.PATHS.values()] == [0, 0, 0, 0]
for i in ops.PATHS.values():
    assert lib.srad_set_path_override(i, 1) == 0 and lib.srad_get_path_override(i) == 1
    assert lib.srad_set_path_override(i, 0) == 0 and lib.srad_get_path_override(i) == 0
with ops.path_override(unfused_blocks=True, upconv_one_gemm=True):
    assert [lib.srad_get_path_override(i) for i in ops.PATHS.values()] == [1, 0, 0, 1]
assert [lib.srad_get_path_override(i) for i in ops.PATHS.values()] == [0, 0, 0, 0]
SRAD_ERR_ARG = 1
assert lib.srad_set_path_override(len(ops.PATHS), 1) == SRAD_ERR_ARG and b"unknown path" in lib.srad_last_error()
assert lib.srad_set_path_override(-1, 1) == SRAD_ERR_ARG
assert lib.srad_get_path_override(len(ops.PATHS)) == -1
print("ok")
"""
    env = dict(os.environ, SRAD_NO_FUSE="1", SRAD_NO_LN_QKV="1", SRAD_ATTN_F32IN="1", SRAD_NO_UPCONV_SPLIT="1")
    r = subprocess.run([sys.executable, "-c", child], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_no_cpu_fallback():
    from srad_amd import metrics, ops
    with pytest.raises(RuntimeError, match="GPU only"):
        metrics.to_u8_hwc(torch.zeros(1, 1, 4, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.layernorm(torch.zeros(4, 8), torch.zeros(8), torch.zeros(8))


def test_state_dict_surface_matches_reference_names():
    """make_model-compatible modules expose exactly the reference's state-dict keys and shapes."""
    from srad_amd import spec as S
    from srad_amd.nets import DRCT, DRN

    class O1:
        n_colors, img_size, window_size, upscale = 1, 32, 8, 4
        embed_dim, depths, num_heads, mlp_ratio, img_range = 180, (6,) * 12, (6,) * 12, 2, 1.0
        upsampler, resi_connection = "pixelshuffle", "1conv"
    m = DRCT(O1())
    sd = m.state_dict()
    sp = S.drct_spec(S.DRCTConfig())
    assert list(sd.keys()) == list(sp.keys()) and len(sd) == 1000
    assert all(tuple(sd[k].shape) == tuple(v[0]) for k, v in sp.items())
    assert sum(p.numel() for p in m.parameters()) == 27382021

    class O2:
        n_colors, n_blocks, n_feats, negval, rgb_range, scale = 3, 40, 20, 0.2, 255, [2, 4]
    sd = DRN(O2()).state_dict()
    sp = S.drn_spec(S.DRNConfig.for_scale(4, 3))
    assert list(sd.keys()) == list(sp.keys()) and len(sd) == 664


def test_no_kernel_uses_scratch():
    """Every gfx950 kernel of the shipped library keeps its state in registers: a private-memory (scratch) allocation in the
    code object's metadata means a register array was spilled or indexed dynamically - a silent 4x on the 64-row mlp_block
    instances once (tools/check_scratch.py)."""
    import importlib.util
    so = os.path.join(ROOT, "anomaly-detection-super-resolution_amd", "libsrad.so")
    if not os.path.exists(so) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    spec = importlib.util.spec_from_file_location("check_scratch", os.path.join(ROOT, "tools", "check_scratch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    found, total = mod.kernels_with_scratch(so)
    assert total > 200, total
    assert not found, found
