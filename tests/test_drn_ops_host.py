"""CPU: what tests/test_gpu_drn_ops.py relies on, checked without a GPU.  The launch plan of the RCAB tail kernels
(srad_drn_ca_plan: slices per image and NI) over the case table must reach every path the table claims, so a later retuning
of ca_slices or of the NI thresholds fails here instead of quietly un-covering a kernel instance; the srad_op_drn_* entries
refuse bad arguments before any launch; the test's own fp64 references agree with autograd and with torch's bicubic."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import drn_ops_ref as R


def test_ca_plan_reaches_every_claimed_path():
    from srad_amd import ops
    got = {case: ops.drn_ca_plan(case[1], case[2]) for case in R.CA_CASES}
    assert got == R.CA_CASES, {k: (v, R.CA_CASES[k]) for k, v in got.items() if v != R.CA_CASES[k]}
    combos = set(got.values())
    # every slice count with every NI it is claimed with: 1 and 8 slices with the short items, 8 / 64 / 128 with 10 and the loop
    assert combos >= {(1, 5), (8, 5), (8, 10), (8, 0), (64, 5), (64, 10), (64, 0), (128, 10), (128, 0)}
    assert {s for s, _ in combos} == {1, 8, 64, 128} and {n for _, n in combos} == {0, 5, 10}
    # a slice that starts at or past the image's end: its workgroups have no items (items <= 0)
    past = [(B, hw, Cc) for (B, hw, Cc), (s, _) in got.items() if (s - 1) * -(-hw // s) >= hw]
    assert (2, 1025, 80) in past
    hw, s = 1025, 64
    assert sum(1 for k in range(s) if k * -(-hw // s) >= hw) == 3
    for case in R.NCHUNK_CASES + R.STORAGE_CASES:
        assert case in R.CA_CASES
    assert {R.CA_CASES[c] for c in R.STORAGE_CASES} == {(8, 10), (64, 0), (128, 10), (64, 5)}     # the storage instances at all three NI


def test_ca_plan_thresholds():
    """The boundaries themselves: the first image size of every slice count, the last item count of every NI."""
    from srad_amd import ops
    assert [ops.drn_ca_plan(hw, 80)[0] for hw in (1, 63, 64, 1023, 1024, 16383, 16384, 1 << 20)] == [1, 1, 8, 8, 64, 64, 128, 128]
    assert ops.drn_ca_plan(63, 80) == (1, 5) and ops.drn_ca_plan(63, 512) == (1, 0)      # 63 * 20 = 1260 | 63 * 128 = 8064
    assert ops.drn_ca_plan(64 * 64, 80) == (64, 5) and ops.drn_ca_plan(64 * 65, 80) == (64, 10)     # 64 * 20 = 1280 | 65 * 20
    assert ops.drn_ca_plan(64 * 128, 80) == (64, 10) and ops.drn_ca_plan(64 * 128 + 1, 80) == (64, 0)   # 2560 | 2580


def test_drn_op_entries_refuse_bad_arguments_without_gpu():
    """Null pointers, C % 4 != 0, C < 16, C > 512, nchunk outside 1 .. 256, C * C/16 > 4096 for ca_bwd: all before any launch."""
    from srad_amd import _lib as L
    lib = L.lib()
    ERR = 1
    p = C.c_void_p(1 << 20)                    # never dereferenced: every call below fails in the checks
    sl, ni = C.c_int(), C.c_int()

    def pool_dot(Cc=80, nchunk=32, r=p, part=p):
        return lib.srad_op_drn_pool_dot(None, r, 0, 1, 64, Cc, nchunk, part, None)

    def scale_add(Cc=80, nchunk=32, miss=-1, ldx=None, rh=0, xh=0):
        a = [None if i == miss else p for i in range(8)]
        return lib.srad_op_drn_ca_scale_add(a[0], nchunk, 1, 64, Cc, a[1], a[2], a[3], a[4], a[5], rh, a[6], xh, Cc if ldx is None else ldx,
                                            a[7], 0, None, None, None)

    def apply_bwd(Cc=80, nchunk=32, miss=-1):
        a = [None if i == miss else p for i in range(8)]
        return lib.srad_op_drn_ca_apply_bwd(a[0], a[1], a[2], nchunk, a[3], 1, 64, Cc, a[4], a[5], a[6], a[7], 0, None)

    def ca_bwd(Cc=80, nchunk=32, miss=-1):
        a = [None if i == miss else p for i in range(11)]
        return lib.srad_op_drn_ca_bwd(a[0], nchunk, a[1], a[2], 1, 64, Cc, a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], None)

    for fn in (pool_dot, scale_add, apply_bwd, ca_bwd):
        for bad_c in (82, 12, 8, 516, 1024):
            assert fn(Cc=bad_c) == ERR and b"multiple of 4 in 16 .. 512" in lib.srad_last_error(), (fn.__name__, bad_c)
        for bad_n in (0, -1, 257):
            assert fn(nchunk=bad_n) == ERR and b"nchunk" in lib.srad_last_error(), (fn.__name__, bad_n)
    assert pool_dot(r=None) == ERR and pool_dot(part=None) == ERR and b"null argument" in lib.srad_last_error()
    for fn, n in ((scale_add, 8), (apply_bwd, 8), (ca_bwd, 11)):
        for miss in range(n):
            assert fn(miss=miss) == ERR and b"null argument" in lib.srad_last_error(), (fn.__name__, miss)
    assert ca_bwd(Cc=272) == ERR and b"do not fit" in lib.srad_last_error()          # 272 * 17 = 4624
    assert scale_add(ldx=82) == ERR and scale_add(ldx=76) == ERR and b"ldx" in lib.srad_last_error()
    assert scale_add(xh=1) == ERR and b"only with a bf16 r" in lib.srad_last_error()
    assert lib.srad_drn_ca_plan(64, 80, None, C.byref(ni)) == ERR and lib.srad_drn_ca_plan(64, 82, C.byref(sl), C.byref(ni)) == ERR
    assert lib.srad_drn_ca_plan(0, 80, C.byref(sl), C.byref(ni)) == ERR
    # the image-end and gradient-plumbing kernels
    assert lib.srad_op_drn_bicubic(None, 1, 3, 4, 4, 4, p, p, p, None, None) == ERR and b"null argument" in lib.srad_last_error()
    assert lib.srad_op_drn_bicubic(p, 1, 2, 4, 4, 4, p, p, p, None, None) == ERR and b"1 or 3 channels" in lib.srad_last_error()
    assert lib.srad_op_drn_affine_to_nchw(p, 4, 1, 4, 16, p, p, p, None) == ERR and b"1 or 3 channels" in lib.srad_last_error()
    assert lib.srad_op_drn_affine_to_nchw(p, 2, 1, 3, 16, p, p, p, None) == ERR
    assert lib.srad_op_drn_affine_to_nchw(p, 4, 1, 3, 16, p, p, None, None) == ERR and b"null argument" in lib.srad_last_error()
    assert lib.srad_op_drn_affine_bwd(p, p, p, 4, None, 1, 3, 16, p, p, p, None) == ERR and b"exactly one layout" in lib.srad_last_error()
    assert lib.srad_op_drn_affine_bwd(None, None, p, 4, None, 1, 3, 16, p, p, p, None) == ERR
    assert lib.srad_op_drn_affine_bwd(p, None, p, 4, None, 1, 2, 16, p, p, p, None) == ERR and b"1 or 3 channels" in lib.srad_last_error()
    assert lib.srad_op_drn_zero_upsample(p, None, 1, 3, 3, 12, None) == ERR and lib.srad_op_drn_zero_upsample(p, p, 1, 3, 3, 10, None) == ERR
    assert lib.srad_op_drn_add_cols(p, 12, None, 12, 5, 12, None) == ERR and lib.srad_op_drn_add_cols(p, 8, p, 12, 5, 12, None) == ERR
    rows = C.c_int(-1)
    assert lib.srad_op_conv_pool(L.PREC_F32, None, None, None, 1, 8, 8, 82, None, None, C.byref(rows), None, 0, None) == ERR
    assert lib.srad_op_conv_pool(L.PREC_F32, None, None, None, 1, 8, 8, 80, None, None, None, None, 0, None) == ERR
    assert lib.srad_op_conv_pool(L.PREC_F32, p, p, p, 1, 8, 8, 80, p, None, C.byref(rows), p, 1 << 30, None) == ERR     # no pool_part
    assert b"null argument" in lib.srad_last_error() and rows.value == -1


def test_conv_pool_eligibility_query():
    """The shapes test_gpu_drn_ops.py expects on the conv epilogue, and the network tests that are to reach it, are eligible;
    small ones are not.  Host only: the tile choice is a function of the shape and the precision."""
    from srad_amd import ops
    assert ops.conv_pool_rows(6, 64, 64, 80, "fp32") == 64 and ops.conv_pool_rows(6, 64, 64, 80, "bf16x3") == 64      # 64-row tiles
    assert ops.conv_pool_rows(3, 64, 64, 80, "fp32") == 64                                   # 64 x 64 tiles, two column tiles: 384
    assert ops.conv_pool_rows(2, 64, 64, 80, "fp32") == 0                                    # 256 tiles < 384: 32-row tiles
    assert ops.conv_pool_rows(2, 64, 64, 160, "fp32") == 64 and ops.conv_pool_rows(1, 64, 64, 160, "fp32") == 0
    assert ops.conv_pool_rows(6, 64, 64, 40, "fp32") == 64 and ops.conv_pool_rows(5, 64, 64, 40, "fp32") == 0
    assert ops.conv_pool_rows(11, 64, 48, 80, "bf16") == 24                                  # 128-row tiles of the tiled GEMM
    assert ops.conv_pool_rows(8, 64, 48, 80, "bf16") == 48                                   # 64-row tiles
    assert ops.conv_pool_rows(2, 64, 64, 80, "bf16") == 32                                   # W % 32 == 0: the 80-channel kernel
    assert ops.conv_pool_rows(1, 8, 8, 80, "fp32") == 0 and ops.conv_pool_rows(2, 32, 32, 80, "fp32") == 0


@pytest.mark.parametrize("case", list(R.CA_CASES))
def test_ca_reference_matches_autograd_and_fp32_restatement(case):
    """The fp64 CALayer restatement against autograd of torch's own modules' functions on the same data (conv2d 1x1 on the
    adaptive average pool), forward and d/dr; and the fp32 restatement stays 4x under the 1e-5 bar, so that bar holds."""
    B, hw, Cc = case
    d = R.ca_inputs(B, hw, Cc, from_r=True)
    y, gate, pool, pre = R.ca_tail64(d["part"], hw, d["w1"], d["b1"], d["w2"], d["b2"], d["r"], d["x"])
    assert float(pre.abs().min()) > 1e-3
    H = W = None
    for h in range(int(hw ** 0.5), 0, -1):
        if hw % h == 0:
            H, W = h, hw // h
            break
    r4 = d["r"].double().reshape(B, H, W, Cc).permute(0, 3, 1, 2).clone().requires_grad_(True)
    x4 = d["x"].double().reshape(B, H, W, Cc).permute(0, 3, 1, 2)
    a = F.adaptive_avg_pool2d(r4, 1)
    a = F.relu(F.conv2d(a, d["w1"].double()[:, :, None, None], d["b1"].double()))
    a = torch.sigmoid(F.conv2d(a, d["w2"].double()[:, :, None, None], d["b2"].double()))
    out = r4 * a + x4
    g = torch.randn(B * hw, Cc, generator=torch.Generator().manual_seed(hw))
    (out * g.double().reshape(B, H, W, Cc).permute(0, 3, 1, 2)).sum().backward()
    ymod = out.detach().permute(0, 2, 3, 1).reshape(B * hw, Cc)
    # the partial rows are fp32 roundings of the true chunk sums: the means agree to n * 2^-24
    assert float((y - ymod).abs().max() / ymod.abs().max()) < 1e-6
    bw = R.ca_backward64(d["r"], d["x"], g, B, hw, d["w1"], d["b1"], d["w2"], d["b2"])
    drmod = r4.grad.permute(0, 2, 3, 1).reshape(B * hw, Cc)
    assert float((bw["dr"] - drmod).abs().max() / drmod.abs().max()) < 1e-12
    y32, gate32 = R.ca_tail32(d["part"], hw, d["w1"], d["b1"], d["w2"], d["b2"], d["r"], d["x"])
    e_y = float((y32.double() - y).abs().max() / y.abs().max())
    e_g = float((gate32.double() - gate).abs().max() / gate.abs().max())
    print(f"{case}: fp32 restatement y {e_y:.2e} gate {e_g:.2e}, min |pre| {float(pre.abs().min()):.2e}")
    assert e_y < R.BAR32 / 4 and e_g < R.BAR32 / 4


@pytest.mark.parametrize("B,Cc,H,W,scale", [(2, 3, 5, 7, 4), (1, 1, 1, 9, 2), (1, 3, 4, 4, 8), (3, 1, 6, 1, 8)])
def test_bicubic_formula_is_torch_bicubic(B, Cc, H, W, scale):
    x = torch.rand(B, Cc, H, W, generator=torch.Generator().manual_seed(H * W), dtype=torch.float64)
    ref = F.interpolate(x, scale_factor=scale, mode="bicubic", align_corners=False)
    assert float((R.bicubic_kernel64(x, scale) - ref).abs().max()) < 1e-14
