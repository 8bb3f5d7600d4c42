"""The case table, inputs, fp64 reference and per-element checker of the tiled GEMM (csrc/kernels_gemm.hip), shared by
tests/test_gpu_gemm_tiles.py (GPU) and tests/test_gemm_ref_host.py (CPU).  Plain torch, device-agnostic: the GPU tests run the
reference in fp64 on the GPU, the host tests on the CPU.  Nothing here reads another project: the operation is written down
from its definition (include/srad.h, srad_op_gemm).

The operation, in this order
    A[m, tap, c]  row gather of x [rows, ldx]: identity (ntaps = 1), or the 3x3 window (pad 1, stride 1 | 2) of pixel m of a
                  [B, Hi, Wi] NHWC image, zero outside the image
    LayerNorm     optional, over the Cin channels of a row, biased variance, eps 1e-5, then * gamma + beta
    pre = sum_k A[m, k] w[n, k] + bias[n]
    y = act(pre) * alpha + residual[m, n]           act: none | erf-GELU | LeakyReLU(slope) | ReLU
    store         plain: out[m, out_offset + n]; PixelShuffle(2): column n = 4 c + 2 dy + dx of pixel (b, oy, ox) goes to row
                  (b, 2 oy + dy, 2 ox + dx) of a [B, 2 Ho, 2 Wo] image, column out_offset + c
and S[m, n] = sum_k |A[m, k]| |w[n, k]| + |bias[n]|, the magnitude every accumulation bound is stated in.

The bound of element (m, n).  u = 2^-24 is the unit round-off of fp32; everything is first order in u.

  Operands.  In bf16 mode x and w are generated bf16-representable, so the kernel's conversion is exact; a bf16 x bf16 product
  is exact in fp32.  fp32 mode multiplies with an fma (v_mfma_f32_16x16x4_f32), one rounding per term.

  Accumulation.  K = ntaps * Cp terms (Cp = Cin rounded up to 32: the padding is zero-filled but still added) and the bias are
  summed in fp32 in an order the test does not know (MFMA-internal trees, chunk order), and the MFMA's internal adds may
  truncate (relative error below 2^-23 instead of 2^-24 per add).  Any order of n adds of terms t_i has error at most
  n * 2^-23 * sum |t_i|:
        e_acc = K * 2^-23 * S
  Split-bf16 (bf16x3) takes unrounded fp32 operands as hi + lo bf16 terms and computes hi.hi + hi.lo + lo.hi.  What is lost is
  the lo.lo product and the residue of each two-term split, three terms of relative size 2^-18 each in the issue's accounting
  of the format (2^-9 per bf16 rounding):
        e_split = 3 * 2^-18 * (S - |bias|)
  (A worst-case reading of bf16 - 8 significant bits, half-spacing 2^-8 of the binade - would give 3 * 2^-16 and 3 K adds; the
  tighter figures are the ones enforced here, and the observed errors stay far inside them because the terms do not conspire.)

  LayerNorm (n = Cin <= 320 channels, fp32): the kernel forms s = sum x, ss = sum x^2, mean = s / n, var = max(ss / n - mean^2, 0),
  rs = rsqrtf(var + eps), v = (x - mean) * rs * gamma + beta.  With A1 = sum |x| / n and E2 = sum x^2 / n (exact values):
        |d mean| <= n u A1                                  n - 1 adds in any order and one division
        |d E2|   <= (n + 1) u E2                            n squares, n - 1 adds, one division, all terms positive
        |d var|  <= (n + 1) u E2 + 2 |mean| n u A1 + 3 u E2  <= (3 n + 4) u E2        since |mean| <= A1 <= sqrt(E2)
        rho      = |d rs| / rs <= (3 n + 4) u E2 / (2 (var + eps)) + 2^-22 + 2 u      (rsqrtf taken as good to 2 ulp)
        |d xhat| <= rs |d mean| + |xhat| (rho + 2 u)
        |d v|    <= |gamma| |d xhat| + 2 u |xhat gamma| + u |v|
  The first term of |d xhat| is the same for every channel of a row: the error of the mean is absolute, in units of the row's
  max |xhat|, not relative per element - a small xhat carries the same error as a large one.  The GEMM turns it into
        e_ln[m, n] = sum_k |d v|[m, k] |w[n, k]|
  In bf16 mode the reference rounds v to bf16 as the kernel does, but from the exact value: where the two fp32-close values
  straddle a rounding boundary the rounded operands differ.  The issue's allowance for that is one bf16 rounding of every
  operand, e_flip = 2^-9 * (S - |bias|).

  pre-activation:  e_pre = e_acc + e_split (bf16x3) + e_ln + e_flip (LayerNorm, bf16)

  Activation.  none, ReLU: Lipschitz 1, exact.  LeakyReLU(slope <= 1): Lipschitz 1, one rounding u |act|.  erf-GELU
  0.5 x (1 + erf(x / sqrt 2)): max |gelu'| < 1.13 scales e_pre; computing it costs the rounding of x / sqrt 2 (moves erf by
  at most 0.49 u), the device erff, the rounding of 1 + erf (<= 2 u) and two multiplications:
        e_act = 1.13 e_pre + 0.5 |x| (E_ERF + 3 u) + 2 u |gelu(x)|
  E_ERF is the absolute error of the device erff.  The ROCm math documentation is not installed next to the toolchain this was
  written with, so it was measured once on an MI355X (float32 erf element-wise against fp64 over 2^24 arguments, uniform in
  [-4.5, 4.5] plus 2^21 log-spaced ones of both signs down to 1e-30): the maximum was ERFF_MEASURED_ABS = 1.456 * 2^-24
  (below), and E_ERF is twice that.  The kernel's own GELU, fed exact pre-activations through an identity weight, then used
  0.45 of the activation term.

  Epilogue.  * alpha and + residual are one fp32 rounding each:
        e = |alpha| e_act + 2 u (|alpha act(pre)| + |residual|)

The buffer rule.  The checker gets the WHOLE output buffer, allocated with a row stride above out_offset + N and slack rows,
pre-filled with NaN: every element the operation defines must be finite and within its bound, every other one still NaN.
x has a row stride above Cin and the residual one above N, with NaN in the columns the operation does not define either: a
kernel that reads them poisons its output."""
import collections
import functools
import math

import torch

U32 = 2.0 ** -24
ACT_NONE, ACT_GELU, ACT_LRELU, ACT_RELU = 0, 1, 2, 3
LN_EPS = 1e-5
GELU_LIP = 1.13
# measured on an MI355X (see above): max |erff(x) - erf(x)| = 8.68e-08 = 1.456 * 2^-24 (at x = -0.9716; 1.49 ulp at most, near
# x = 0.0035); E_ERF is twice the measured value
ERFF_MEASURED_ABS = 1.456 * 2.0 ** -24
E_ERF = 2 * ERFF_MEASURED_ABS

PRECS = ("fp32", "bf16", "bf16x3")

Case = collections.namedtuple(
    "Case", "name prec M N Cin ntaps stride B H W ln act slope alpha residual out_offset ps bias plan")
Plan = collections.namedtuple("Plan", "BM BN CPS LN CONV SPECIAL")


def _case(name, prec, N, Cin, plan, *, M=0, conv=None, stride=1, ln=False, epi="plain", ps=False):
    act, slope, alpha, residual, off = {
        "plain": (ACT_NONE, 0.0, 1.0, False, 0),
        "gelu": (ACT_GELU, 0.0, 1.0, False, 0),
        "lrelu_res": (ACT_LRELU, 0.2, 0.75, True, 0),
        "offset": (ACT_NONE, 0.0, 1.0, False, 8),
        "relu": (ACT_RELU, 0.0, 1.0, False, 4),
    }[epi]
    if conv is None:
        B, H, W, ntaps = 1, 1, M, 1
    else:
        (B, H, W), ntaps = conv, 9
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        M = B * Ho * Wo
    return Case(f"{name}-{prec}", prec, M, N, Cin, ntaps, stride, B, H, W, ln, act, slope, alpha, residual, off, ps, True, plan)


def cps(prec, bm, bn, ln=False, conv=False):
    """K chunks per stage the cases expect (the issue's statement: 4 instead of 8 for bf16 at 64x64, and for the conv gather at
    64x80 and 128x80 too; fp32 and split-bf16 stage 4)."""
    if prec != "bf16":
        return 4
    if ln:
        return 8
    if conv:
        return 4 if (bm, bn) in ((64, 64), (64, 80), (128, 80)) else 8
    return 4 if (bm, bn) == (64, 64) else 8


# tile -> (N, M) of the smallest linear problem that selects it; the plan assertion of every test is the judge
M128 = 383 * 128 + 6          # 384 row tiles of 128, the last one holds 6 rows
LINEAR_TILES = {
    (128, 16): (12, M128),
    (128, 32): (20, M128),
    (32, 32): (20, 77),                     # 3 tiles: fewer than the 8 XCDs (q = 0 in the tile remap)
    (128, 80): (72, 255 * 128 + 5),         # bf16 only
    (64, 80): (72, 383 * 64 + 8),           # below 255 * 128 rows, so bf16 stays off 128x80
    (64, 64): (100, 192 * 64 + 5),          # 193 x 2 = 386 tiles, 386 % 8 = 2
    (32, 64): (180, 4100),                  # 129 x 3 = 387 tiles
    "fall": (180, 77),                      # 32x32 fall-through, 3 x 6 = 18 tiles
}
# the same tiles through the 3x3 gather: (N, (B, H, W)) with no friendly factor in H, W or H * W
CONV_TILES = {
    (128, 16): (12, (1, 211, 233)),
    (128, 32): (20, (1, 211, 233)),
    (32, 32): (20, (1, 7, 11)),
    (128, 80): (72, (1, 181, 181)),
    (64, 80): (72, (1, 157, 157)),
    (64, 64): (100, (1, 109, 113)),         # 193 x 2 tiles
    (32, 64): (180, (1, 59, 71)),           # 131 x 3 tiles
    "fall": (180, (1, 7, 11)),
}


def _tile(key):
    return (32, 32) if key == "fall" else key


def _tname(key):
    return "fall32x32" if key == "fall" else "%dx%d" % key


def linear_cases():
    out = []
    for key, (N, M) in LINEAR_TILES.items():
        bm, bn = _tile(key)
        for prec in PRECS:
            if key == (128, 80) and prec != "bf16":
                continue
            plan = Plan(bm, bn, cps(prec, bm, bn), False, False, False)
            for Cin in (36, 180):
                for epi in ("plain", "gelu", "lrelu_res", "offset"):
                    out.append(_case(f"lin-{_tname(key)}-c{Cin}-{epi}", prec, N, Cin, plan, M=M, epi=epi))
    for prec in PRECS:                                   # 17 K chunks: full stages plus one chunk under CPS 4 and 8
        N, M = LINEAR_TILES[(64, 64)]
        out.append(_case("lin-64x64-c520-plain", prec, N, 520, Plan(64, 64, cps(prec, 64, 64), False, False, False), M=M))
    return out


def ln_cases():
    out = []
    for key in ((32, 32), (64, 64), (32, 64), "fall"):
        N, M = LINEAR_TILES[key]
        bm, bn = _tile(key)
        for prec in PRECS:
            for Cin, epi in ((180, "gelu"), (320, "plain")):
                plan = Plan(bm, bn, cps(prec, bm, bn, ln=True), True, False, False)
                out.append(_case(f"ln-{_tname(key)}-c{Cin}-{epi}", prec, N, Cin, plan, M=M, ln=True, epi=epi))
    return out


def conv_cases():
    out = []
    for key, (N, img) in CONV_TILES.items():
        bm, bn = _tile(key)
        for prec in PRECS:
            if key == (128, 80) and prec != "bf16":
                continue
            plan = Plan(bm, bn, cps(prec, bm, bn, conv=True), False, True, False)
            out.append(_case(f"conv-{_tname(key)}-c36-relu", prec, N, 36, plan, conv=img, epi="relu"))
    # the real fall-back of the 80-channel conv kernel: width 182 is no multiple of 32
    out.append(_case("conv-128x80-c80-w182", "bf16", 80, 80, Plan(128, 80, 4, False, True, False), conv=(1, 180, 182)))
    for prec in PRECS:
        c = cps(prec, 64, 64, conv=True)
        out.append(_case("conv-64x64-stride2", prec, 100, 36, Plan(64, 64, c, False, True, False), conv=(1, 217, 225), stride=2,
                         epi="lrelu_res"))
        out.append(_case("conv-64x64-shuffle", prec, 100, 36, Plan(64, 64, c, False, True, True), conv=(1, 109, 113), ps=True,
                         epi="offset"))
        out.append(_case("conv-128x16-shuffle", prec, 12, 36, Plan(128, 16, cps(prec, 128, 16, conv=True), False, True, True),
                         conv=(1, 211, 233), ps=True))
    return out


def all_cases():
    return linear_cases() + ln_cases() + conv_cases()


def determinism_cases():
    N, M = LINEAR_TILES[(64, 64)]
    return [_case("det-64x64-c180", prec, N, 180, Plan(64, 64, cps(prec, 64, 64), False, False, False), M=M, epi="lrelu_res")
            for prec in PRECS]


# ---------------------------------------------------------------------------------------------- inputs

def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def geometry(c):
    """(Ho, Wo, rows of x, ldx, ldr, ldy, rows of out)."""
    if c.ntaps == 9:
        Ho, Wo = (c.H - 1) // c.stride + 1, (c.W - 1) // c.stride + 1
        xrows = c.B * c.H * c.W
    else:
        Ho, Wo, xrows = 1, c.M, c.M
    ldx = c.Cin + 12                                      # row stride != Cin, a multiple of 4 floats
    ldr = c.N + 5
    ncol = c.N // 4 if c.ps else c.N
    ldy = c.out_offset + ncol + 7
    orows = (4 * c.M if c.ps else c.M) + 3                # slack rows
    return Ho, Wo, xrows, ldx, ldr, ldy, orows


@functools.lru_cache(maxsize=4)
def _raw(xrows, ldx, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(xrows, ldx, generator=g)


def make_inputs(c, seed=0):
    """CPU fp32 tensors of a case: x [xrows, ldx] (NaN beyond Cin), w, bias, gamma / beta, residual [M, ldr] (NaN beyond N).
    bf16 mode: x and w bf16-representable (LayerNorm cases: x only, the normalised operand is the kernel's to round)."""
    Ho, Wo, xrows, ldx, ldr, ldy, orows = geometry(c)
    g = torch.Generator().manual_seed(1000 + seed)
    x = _raw(xrows, ldx, seed).clone()
    if c.ln:
        x = x * 1.5 + 0.75                                # a mean the LayerNorm has to take out
    w = torch.randn(c.N, c.Cin, c.ntaps, generator=g) / math.sqrt(c.Cin * c.ntaps)
    if c.prec == "bf16":
        x, w = bf16_round(x), bf16_round(w)
    x[:, c.Cin:] = float("nan")
    t = {"x": x, "w": w.reshape(c.N, c.Cin, 3, 3) if c.ntaps == 9 else w.reshape(c.N, c.Cin)}
    t["bias"] = torch.randn(c.N, generator=g) * 0.5
    if c.ln:
        t["g"] = 1.0 + 0.3 * torch.randn(c.Cin, generator=g)
        t["b"] = 0.2 * torch.randn(c.Cin, generator=g)
    if c.residual:
        r = torch.randn(c.M, ldr, generator=g)
        r[:, c.N:] = float("nan")
        t["r"] = r
    return t


# ---------------------------------------------------------------------------------------------- the operation in fp64

def gather(c, x):
    """A [M, ntaps, Cin] from x [xrows, >= Cin] (any dtype)."""
    x = x[:, :c.Cin]
    if c.ntaps == 1:
        return x.reshape(c.M, 1, c.Cin)
    img = x.reshape(c.B, c.H, c.W, c.Cin)
    img = torch.nn.functional.pad(img, (0, 0, 1, 1, 1, 1))
    Ho, Wo = (c.H - 1) // c.stride + 1, (c.W - 1) // c.stride + 1
    taps = []
    for ky in range(3):
        for kx in range(3):
            taps.append(img[:, ky:ky + (Ho - 1) * c.stride + 1:c.stride, kx:kx + (Wo - 1) * c.stride + 1:c.stride, :])
    return torch.stack(taps, dim=3).reshape(c.M, 9, c.Cin)


def weight_rows(c, w):
    """w [N, Cin] or [N, Cin, 3, 3] -> [N, ntaps, Cin], tap = 3 ky + kx."""
    return w.reshape(c.N, c.Cin, c.ntaps).permute(0, 2, 1)


def store(c, vals, fill=float("nan"), swap_dxdy=False):
    """vals [M, N] -> the whole output buffer [orows, ldy], `fill` where the operation defines nothing."""
    Ho, Wo, xrows, ldx, ldr, ldy, orows = geometry(c)
    buf = torch.full((orows, ldy), fill, dtype=vals.dtype, device=vals.device)
    if not c.ps:
        buf[:c.M, c.out_offset:c.out_offset + c.N] = vals
        return buf
    C4 = c.N // 4
    v = vals.reshape(c.B, Ho, Wo, C4, 2, 2)               # n = 4 c + 2 dy + dx
    if swap_dxdy:
        v = v.transpose(4, 5)
    v = v.permute(0, 1, 4, 2, 5, 3).reshape(c.B * 2 * Ho * 2 * Wo, C4)     # [b, oy, dy, ox, dx, c]
    buf[:4 * c.M, c.out_offset:c.out_offset + C4] = v
    return buf


def act64(c, pre):
    if c.act == ACT_GELU:
        return 0.5 * pre * (1.0 + torch.erf(pre * 0.7071067811865476))
    if c.act == ACT_LRELU:
        return torch.where(pre > 0, pre, pre * c.slope)
    if c.act == ACT_RELU:
        return torch.relu(pre)
    return pre


Ref = collections.namedtuple("Ref", "expect bound y S")


def reference(c, t, device="cpu"):
    """fp64 reference and per-element bound of a case: Ref(expect, bound) are whole output buffers (NaN / 0 outside the
    operation's elements); y, S the [M, N] result and magnitude."""
    f64 = lambda a: a.to(device=device, dtype=torch.float64)
    A = gather(c, f64(t["x"]))
    Wr = f64(weight_rows(c, t["w"]))
    K = c.ntaps * ((c.Cin + 31) // 32 * 32)
    dv = None
    if c.ln:
        n = c.Cin
        a = A[:, 0, :]
        mean = a.mean(1, keepdim=True)
        A1 = a.abs().mean(1, keepdim=True)
        E2 = (a * a).mean(1, keepdim=True)
        var = ((a - mean) ** 2).mean(1, keepdim=True)
        rs = 1.0 / torch.sqrt(var + LN_EPS)
        xhat = (a - mean) * rs
        gam, bet = f64(t["g"]), f64(t["b"])
        v = xhat * gam + bet
        dmean = n * U32 * A1
        rho = (3 * n + 4) * U32 * E2 / (2 * (var + LN_EPS)) + 2.0 ** -22 + 2 * U32
        dxhat = rs * dmean + xhat.abs() * (rho + 2 * U32)
        dv = gam.abs() * dxhat + 2 * U32 * (xhat * gam).abs() + U32 * v.abs()
        if c.prec == "bf16":
            v = bf16_round(v)
        A = v.reshape(c.M, 1, n)
    A2, W2 = A.reshape(c.M, -1), Wr.reshape(c.N, -1)
    bias = f64(t["bias"]) if c.bias else torch.zeros(c.N, dtype=torch.float64, device=device)
    pre = A2 @ W2.t() + bias
    Saw = A2.abs() @ W2.abs().t()
    S = Saw + bias.abs()
    e = K * 2.0 ** -23 * S
    if c.prec == "bf16x3":
        e = e + 3 * 2.0 ** -18 * Saw
    if c.ln:
        e = e + dv @ W2.abs().t()
        if c.prec == "bf16":
            e = e + 2.0 ** -9 * Saw
    a64 = act64(c, pre)
    if c.act == ACT_GELU:
        e = GELU_LIP * e + 0.5 * pre.abs() * (E_ERF + 3 * U32) + 2 * U32 * a64.abs()
    elif c.act == ACT_LRELU:
        e = e + U32 * a64.abs()
    y = a64 * c.alpha
    e = abs(c.alpha) * e + 2 * U32 * y.abs()
    if c.residual:
        r = f64(t["r"])[:, :c.N]
        y = y + r
        e = e + 2 * U32 * r.abs()
    return Ref(store(c, y), store(c, e, fill=0.0), y, S)


def check(c, out, ref):
    """Every element the operation defines is finite and within its bound, every other element of the buffer is still NaN.
    Returns the largest |err| / bound."""
    out = out.to(device=ref.expect.device, dtype=torch.float64)
    assert out.shape == ref.expect.shape, (c.name, out.shape, ref.expect.shape)
    defined = ~torch.isnan(ref.expect)
    touched = ~torch.isnan(out)
    stray = touched & ~defined
    assert not bool(stray.any()), f"{c.name}: {int(stray.sum())} elements written outside the output, first at {stray.nonzero()[0].tolist()}"
    missing = defined & ~torch.isfinite(out)
    assert not bool(missing.any()), f"{c.name}: {int(missing.sum())} output elements not finite, first at {missing.nonzero()[0].tolist()}"
    err = torch.where(defined, (out - ref.expect).abs(), torch.zeros_like(out))
    ratio = torch.where(defined, err / ref.bound.clamp_min(1e-300), torch.zeros_like(out))
    worst = float(ratio.max())
    if worst > 1.0:
        at = (ratio == ratio.max()).nonzero()[0].tolist()
        raise AssertionError(f"{c.name}: {int((ratio > 1).sum())} elements outside their bound; worst at {at}: got {float(out[tuple(at)])!r} "
                             f"expected {float(ref.expect[tuple(at)])!r}, |err| = {worst:.3g} x bound {float(ref.bound[tuple(at)]):.3g}")
    return worst


# ---------------------------------------------------------------------------------------------- float32 emulation (host tests)

MUTATIONS = ("drop_last4", "dup_last_row", "bias_last_col", "bf16_acc_once", "swap_row_blocks", "swap_dxdy", "write_past_n")


def emulate(c, t, mutation=None, seed=0):
    """The operation as a float32 program: operands rounded as the mode rounds them, fp32 accumulation over K in a shuffled
    order, fp32 epilogue.  Returns the whole output buffer.  `mutation` plants one of MUTATIONS."""
    assert mutation is None or mutation in MUTATIONS
    g = torch.Generator().manual_seed(77 + seed)
    A = gather(c, t["x"].float())
    Wr = weight_rows(c, t["w"].float())
    if c.ln:
        a = A[:, 0, :]
        n = c.Cin
        mean = a.sum(1, keepdim=True) / n
        var = ((a * a).sum(1, keepdim=True) / n - mean * mean).clamp_min(0)
        v = (a - mean) * torch.rsqrt(var + torch.tensor(LN_EPS)) * t["g"] + t["b"]
        if c.prec == "bf16":
            v = bf16_round(v)
        A = v.reshape(c.M, 1, n)
    if mutation == "drop_last4":
        A = A.clone()
        A[:, :, c.Cin - 4:] = 0
    A2, W2 = A.reshape(c.M, -1).contiguous(), Wr.reshape(c.N, -1).contiguous()
    if c.prec == "bf16x3":
        Ah, Wh = bf16_round(A2), bf16_round(W2)
        Al, Wl = bf16_round(A2 - Ah), bf16_round(W2 - Wh)
    perm = torch.randperm(A2.shape[1], generator=g)
    acc = torch.zeros(c.M, c.N)
    for i in range(0, len(perm), 12):
        k = perm[i:i + 12]
        if c.prec == "bf16x3":
            acc = acc + Al[:, k] @ Wh[:, k].t()
            acc = acc + Ah[:, k] @ Wl[:, k].t()
            acc = acc + Ah[:, k] @ Wh[:, k].t()
        else:
            acc = acc + A2[:, k] @ W2[:, k].t()
    if mutation == "bf16_acc_once":         # ONE accumulator: among the large positive ones (no ReLU hides it), the one a bf16 rounding moves most
        d = (bf16_round(acc) - acc).abs() / (acc.abs() + 1e-30)
        d = torch.where(acc > 0.5 * acc.max(), d, torch.zeros_like(d))
        m, n_ = divmod(int(d.argmax()), c.N)
        acc[m, n_] = bf16_round(acc[m, n_])
    bias = t["bias"].clone()
    pre = acc + bias
    if mutation == "bias_last_col":
        pre[:, c.N - 1] = acc[:, c.N - 1]
    if c.act == ACT_GELU:
        a = 0.5 * pre * (1.0 + torch.erf(pre * 0.70710678118654752440))
    elif c.act == ACT_LRELU:
        a = torch.where(pre > 0, pre, pre * c.slope)
    elif c.act == ACT_RELU:
        a = torch.relu(pre)
    else:
        a = pre
    y = a * c.alpha
    if c.residual:
        y = y + t["r"][:, :c.N]
    if mutation == "dup_last_row":                        # the last valid row of the last M tile computed from its neighbour
        y[c.M - 1] = y[c.M - 2]
    if mutation == "swap_row_blocks":
        y = y.clone()
        y[0:32], y[32:64] = y[32:64].clone(), y[0:32].clone()
    buf = store(c, y, swap_dxdy=mutation == "swap_dxdy")
    if mutation == "write_past_n":
        ncol = c.N // 4 if c.ps else c.N
        buf[0, c.out_offset + ncol] = 1.0
    return buf
