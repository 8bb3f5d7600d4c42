"""The case table, inputs, references and checkers of the weight-gradient kernels (csrc/kernels_wgrad.hip), shared by
tests/test_gpu_wgrad_paths.py (GPU) and tests/test_wgrad_ref_host.py (CPU).  Plain torch, device-agnostic; nothing here reads
another project: the operation is written down from its definition (csrc/wgrad_queue.h, WgradParams).

The operation
    dW[n, c, tap] += alpha * sum_m rs[m // rps] * dY[m, ycol0 + n] * A(X)[m, tap, c]          n < n_real, c < cin_real
    db[n]         += alpha * sum_m rs[m // rps] * dY[m, ycol0 + n]
    A             identity (one tap), or the 3x3 gather of pixel m of a [B, Hi, Wi] NHWC image: pad 1, stride 1 | 2, zero
                  outside the image
    channels      X stores Cin >= cin_real channels (a multiple of 4).  With groups (grp_pad > 0) stored channel g grp_pad + r,
                  r < grp_real, is real channel g grp_real + r and the other stored channels are padding; without, the real
                  channels are the first cin_real.  dY stores N >= n_real columns from column ycol0 of its rows.

Two tiers.

  Exact.  dY, X in {+-1, +-2, +-3}, rs in {0, 1, 2}, alpha in {0.5, 1, 2}, prior dW / db contents integers |v| <= 1000.  Every
  operand is bf16- and fp32-representable, every product an integer, and every partial sum in ANY order an integer of size at
  most 9 * 2 * M.  Integers below 2^24 are exact in fp32 (half-integers, alpha = 0.5, below 2^23), so with
        CAP:  alpha * 18 * M + 1000  <  2^24    (2^23 for alpha = 0.5)          asserted per case by check_cap
  the kernel's fp32 result is BIT-IDENTICAL to the integer reference whatever the precision mode, operand storage, split,
  wave order or reduce order.  The reference sums in float64, where integers below 2^53 are exact (int64 matmul is not
  available on every device); the result is checked to be integral and compared as fp32 bits.

  Rounding.  dY, X ~ N(0, 1), rs in {0, 1 / 0.7}.  The reference forms the operands as the kernel does - a = fp32(dY * rs), one
  deterministic fp32 multiply; in bf16 mode a and x rounded to bf16 (round to nearest even); db sums the unrounded a, or the
  bf16 value where dY is stored as bf16 - and then sums in float64.  With u = 2^-24 and S = sum_m |a| |b| (db: sum_m |a|):
    * products: bf16 x bf16 is exact in fp32; fp32 mode rounds each product once (u |a b|)
    * accumulation: the M row terms of an element are added in fp32 in an order the test does not know (MFMA-internal trees
      that may truncate: relative 2^-23 per add), then the four waves of a workgroup (2 or 3 adds), then ksplit partial tiles.
      n adds in any order lose at most n * 2^-23 * sum |t_i|.  T = M + ksplit + 4 covers the row terms, the cross-wave and
      cross-split adds and the product rounding:      e_acc = T * 2^-23 * S
    * store: dst = prior + v * alpha is two fp32 roundings:      e_st = 2 u (|alpha * sum| + |prior|)
  bound = e_acc + e_st.  No measured constant enters.  The sum's error is scaled by alpha with the sum; the checker takes
  min(1, alpha) * e_acc, never more than e_acc as stated.  (conv9 has no row splits: its ksplit is the number of workgroups.)

Buffers.  Operands sit in wider row-major buffers (ldx > Cin, ldy > ycol0 + N, multiples of 4); every column the operation does
not define - outside the layer's block, pad channels of a group, channels past cin_real / n_real - holds NaN.  The exception is
a deferred layer, whose launch may take the mask-free body: that one reads clamped columns of the layer's own block by design,
so the columns beside the block hold a finite integer that would break exactness if it were used.  dW / db are the middle of
larger buffers: the defined part holds the prior integers, GUARD floats of NaN before and after must be bit-unchanged."""
import collections
import math
import zlib

import torch

U32 = 2.0 ** -24
GUARD = 64
ALIEN = 7.0                       # finite filler beside a deferred layer's column block

# ------------------------------------------------------------------------------------------------------------------
# Case table.  Every case names the plan it was built for: family, CONV and ksplit (conv9: NT, cpw, nchunks too; groups: the
# launch families, FULL flags and per-layer ksplit).  The shapes are the smallest that reach the path; where the plan query
# disagreed with a first guess the shape was changed and the comment says so.
# ------------------------------------------------------------------------------------------------------------------
_F = ("name route prec family conv ksplit ntaps stride B H W N Cin n_real cin_real grp_real grp_pad ycol0 ldy ldx xcol0 "
      "alpha prior rs storage rounding extra")
Case = collections.namedtuple("Case", _F)


def _case(name, prec, family, ksplit, N, Cin, *, M=0, B=1, H=0, W=0, ntaps=1, stride=1, n_real=None, cin_real=None, grp_real=0,
          grp_pad=0, ycol0=0, alpha=1.0, prior=False, rs=False, storage="f32", rounding=False, route="op", xcol0=0, ldx=None,
          ldy=None, extra=None):
    if ntaps == 1 and stride == 1 and H == 0:
        B, H, W = 1, 1, M
    conv = ntaps == 9 or stride != 1
    return Case(name, route, prec, family, conv, ksplit, ntaps, stride, B, H, W, N, Cin, N if n_real is None else n_real,
                Cin if cin_real is None else cin_real, grp_real, grp_pad, ycol0, ycol0 + N + 4 if ldy is None else ldy,
                xcol0 + Cin + 4 if ldx is None else ldx, xcol0, alpha, prior, rs, storage, rounding, extra or {})


def out_hw(c):
    pad, k = (1, 3) if c.ntaps == 9 else (0, 1)
    return (c.H + 2 * pad - k) // c.stride + 1, (c.W + 2 * pad - k) // c.stride + 1


def rows(c):
    Ho, Wo = out_hw(c)
    return c.B * Ho * Wo


PRECS = ("fp32", "bf16")
KR = {"fp32": 4, "bf16": 32}


def tile64_linear_cases():
    out = []
    for prec, M1 in (("fp32", 30), ("bf16", 200)):
        for N, Cin in ((4, 36), (68, 132), (64, 64)):                  # one partial tile; a partial second tile on both axes; whole
            out.append(_case(f"lin-{prec}-M{M1}-{N}x{Cin}", prec, "tile64", 1, N, Cin, M=M1))
        # split-K with a ragged last split
        out.append(_case(f"lin-{prec}-M1000-ragged", prec, "tile64", 32 if prec == "fp32" else 4, 68, 132, M=1000, rounding=True))
        # rounding the row ranges up to whole steps leaves splits empty: ksplit below the power of two (M = 1030: 4 -> 3 splits of
        # 384 rows in bf16; fp32, 16-row steps: M = 1030 -> 32 splits of 48 rows would be 22)
        out.append(_case(f"lin-{prec}-M1030-empty-splits", prec, "tile64", 22 if prec == "fp32" else 3, 64, 64, M=1030))
        # one row past a whole step, 4 KR k + 1
        step = 4 * KR[prec]
        out.append(_case(f"lin-{prec}-step-plus-1", prec, "tile64", 2, 68, 36, M=4 * step + 1))
        # alpha, prior contents, per-sample factor with rps = 52 (no multiple of a wave step), dY from column 4
        out.append(_case(f"lin-{prec}-alpha-prior-rs-ycol", prec, "tile64", 2 if prec == "bf16" else 6, 68, 36, B=5, H=1, W=52,
                         alpha=0.5, prior=True, rs=True, ycol0=4))
    return out


def tile64_conv_cases():
    out = []
    geoms = (("2x5x7", 2, 5, 7, 1),          # odd sizes; 35 pixels per image: the 8-row lane group of rows 32 .. 39 straddles two images
             ("1x15x11s2", 1, 15, 11, 2),    # stride 2, both output sizes odd: the last window hangs over the border
             ("3x4x4", 3, 4, 4, 1))          # 16 pixels per image: an image ends with a lane group, the raster carry runs into bb
    for prec in PRECS:
        for g, B, H, W, s in geoms:
            for Cin, N in ((4, 180), (36, 4)):
                # fp32 steps are 16 rows: these 48 to 70 output pixels are two row splits there, one in bf16 (128-row steps)
                out.append(_case(f"conv-{prec}-{g}-{Cin}to{N}", prec, "tile64", 2 if prec == "fp32" else 1, N, Cin, B=B, H=H, W=W, ntaps=9,
                                 stride=s))
    # 80 -> 80 in fp32 mode must stay on the 64-wide tiles
    out.append(_case("conv-fp32-2x5x7-80to80-not-w80", "fp32", "tile64", 2, 80, 80, B=2, H=5, W=7, ntaps=9))
    return out


def real_extent_cases():
    """The n < n_real && c < cin_real / srad_real_channel stores, in the kernel's direct store (ksplit 1) and in the reduce."""
    out = []
    for prec in PRECS:
        # fp32 (16-row steps) stores directly up to 32 rows only: (2, 4, 4); (2, 5, 7) is two splits there.  bf16 (128-row steps):
        # (2, 5, 7) stores directly, (2, 20, 24) = 960 rows are four splits
        small, big = (dict(B=2, H=4, W=4), dict(B=2, H=5, W=7)) if prec == "fp32" else (dict(B=2, H=5, W=7), dict(B=2, H=20, W=24))
        for tag, geo, ks in (("direct", small, 1), ("reduce", big, 2 if prec == "fp32" else 4)):
            out.append(_case(f"real-{prec}-{tag}-head-cin3of4", prec, "tile64", ks, 36, 4, cin_real=3, ntaps=9, prior=True, **geo))
            out.append(_case(f"real-{prec}-{tag}-tail-n3of4", prec, "tile64", ks, 4, 36, n_real=3, ntaps=9, prior=True, **geo))
            out.append(_case(f"real-{prec}-{tag}-groups-2x6in8", prec, "tile64", ks, 36, 16, cin_real=12, grp_real=6, grp_pad=8,
                             ntaps=9, prior=True, alpha=2.0, **geo))
        for tag, M, ks in (("direct", 30 if prec == "fp32" else 200, 1), ("reduce", 1000, 32 if prec == "fp32" else 4)):
            out.append(_case(f"real-{prec}-{tag}-n66of68", prec, "tile64", ks, 68, 132, M=M, n_real=66, prior=True))
    return out


def w80_cases():
    return [
        _case("w80-lin-M130", "bf16", "w80", 1, 80, 80, M=130),
        _case("w80-lin-M1000", "bf16", "w80", 4, 80, 80, M=1000, rounding=True),
        # 32 splits: the eight-deep unrolled loop of the square-tile reduce (from 29 partials), which conv9's 23 workgroups do not reach
        _case("w80-lin-M8192-32-splits", "bf16", "w80", 32, 80, 80, M=8192),
        _case("w80-lin-M130-ycol4-wide", "bf16", "w80", 1, 80, 80, M=130, ycol0=4, ldy=96, ldx=100, alpha=2.0, prior=True),
        _case("w80-conv-1x5x7", "bf16", "w80", 1, 80, 80, B=1, H=5, W=7, ntaps=9),
        _case("w80-conv-1x17x23", "bf16", "w80", 2, 80, 80, B=1, H=17, W=23, ntaps=9, rounding=True),
        # width 33 is no multiple of 32 and 594 pixels are below 8192: stays on w80; the fifth-channel loads at an image edge
        _case("w80-conv-2x9x33", "bf16", "w80", 2, 80, 80, B=2, H=9, W=33, ntaps=9, prior=True),
    ]


def conv9_cases():
    """Operands as column blocks of wider buffers, as the existing strided-operand test lays them out: X is columns [C, 2 C) of
    rows of 2 C, dY columns [4, 4 + C) of rows of C + 8.  Both shapes have 68 chunks in 23 workgroups of cpw = 3: the last
    workgroup's range is short (2 chunks)."""
    out = []
    # (1, 67, 128): the last row chunk holds 3 of 4 rows.  (2, 66, 64): a row chunk ends an image with 2 rows.
    for C, g in ((4, 0), (16, 1), (20, 0), (36, 1), (64, 0), (76, 1), (80, 0), (80, 1)):
        B, H, W = ((1, 67, 128), (2, 66, 64))[g]
        out.append(_case(f"conv9-C{C}-{B}x{H}x{W}", "bf16", "conv9", 23, C, C, B=B, H=H, W=W, ntaps=9, ycol0=4, ldy=C + 8, xcol0=C,
                         ldx=2 * C, prior=C in (36, 80), alpha=2.0 if C == 36 else 1.0, rounding=(C, g) == (80, 1),
                         extra=dict(NT=min(5, (C + 15) // 16), cpw=3, nchunks=68)))
    return out


def conv9h_cases():
    """wgrad_conv9_kernel<5, YH, XH> through ops.wgrad_conv9_bf16: bf16 dY, fp32 or bf16 X, contiguous [M, 80], fresh outputs."""
    out = []
    for B, H, W in ((1, 67, 128), (2, 66, 64)):
        for st in ("yh", "yh+xh"):
            out.append(_case(f"conv9h-{st}-{B}x{H}x{W}", "bf16", "conv9", 23, 80, 80, B=B, H=H, W=W, ntaps=9, ldy=80, ldx=80, storage=st,
                             route="conv9h", extra=dict(NT=5, cpw=3, nchunks=68)))
    return out


def op_cases():
    return tile64_linear_cases() + tile64_conv_cases() + real_extent_cases() + w80_cases() + conv9_cases() + conv9h_cases()


# A deferred group: layers (M, N, Cin, storage, rps) queued one after the other and sent as the shared launch(es).
Group = collections.namedtuple("Group", "name prec layers families full ksplits alpha prior rounding")
SHAPES5 = ((32, 180), (540, 180), (180, 360), (4, 36), (68, 132))         # N x Cin


def group_cases():
    def five(M, storages, rps=256):
        return tuple((M[i] if isinstance(M, tuple) else M, n, c, storages[i], 0 if storages[i] == "xh+yh" else rps)
                     for i, (n, c) in enumerate(SHAPES5))
    out = []
    # one layer, rows that are not whole 128-row steps: the masked body, per storage
    for st in ("f32", "xh", "xh+yh"):
        out.append(Group(f"one-M1000-{st}", "bf16", ((1000, 180, 180, st, 0 if st == "xh+yh" else 250),), ("multi",), (False,), (4,),
                         0.5, True, False))
    # one layer, whole steps but a per-sample factor that changes inside a 32-row wave step: masked as well
    for st in ("f32", "xh"):
        out.append(Group(f"one-M1024-rps100-{st}", "bf16", ((1024, 68, 132, st, 100),), ("multi",), (False,), (4,), 1.0, True, False))
    # one layer the plan proves FULL
    for st, fam in (("f32", "multi"), ("xh", "multi"), ("xh+yh", "multi_hh")):
        out.append(Group(f"one-M1024-full-{st}", "bf16", ((1024, 180, 180, st, 0 if st == "xh+yh" else 256),), (fam,), (True,), (4,),
                         2.0, True, False))
    mixed = ("xh", "xh+yh", "f32", "xh", "xh+yh")
    out.append(Group("five-mixed-full", "bf16", five(1024, mixed), ("multi",), (True,), (4, 4, 4, 4, 4), 0.5, True, True))
    out.append(Group("five-all-hh", "bf16", five((1024, 512, 1024, 256, 1024), ("xh+yh",) * 5), ("multi_hh",), (True,), (4, 2, 4, 1, 4),
                     1.0, True, False))
    out.append(Group("five-one-ragged", "bf16", five((1024, 1024, 1000, 1024, 1024), mixed), ("multi",), (False,), (4, 4, 4, 4, 4),
                     1.0, True, False))
    out.append(Group("five-fp32", "fp32", five(1024, ("f32",) * 5, rps=100), ("multi",), (False,), (32, 8, 8, 32, 32), 2.0, True, False))
    six = five(1024, mixed) + ((1000, 68, 132, "xh", 250),)
    out.append(Group("six-two-launches", "bf16", six, ("multi", "multi"), (True, False), (4, 4, 4, 4, 4, 4), 1.0, True, False))
    return out


# ------------------------------------------------------------------------------------------------------------------
# Plans from shapes alone (no GPU): what the table is checked against on the host; the GPU tests ask with their real tensors.
# ------------------------------------------------------------------------------------------------------------------
def plan_of_case(c, ops):
    M = rows(c) if not c.conv else 0
    return ops.wgrad_plan_shape(c.prec, c.N, c.Cin, M=M, ntaps=c.ntaps, stride=c.stride, B=c.B, H=c.H, W=c.W, ldy=c.ldy, ldx=c.ldx,
                                ycol0=c.ycol0, n_real=c.n_real, cin_real=c.cin_real, grp_real=c.grp_real, grp_pad=c.grp_pad,
                                row_scale=c.rs, dy_bf16="yh" in c.storage, x_bf16="xh" in c.storage)


def assert_case_plan(c, p):
    tn, tc = ((c.N + 63) // 64, (c.Cin + 63) // 64) if c.family == "tile64" else (1, 1)
    lay = p.layers[0]
    got = (p.families, p.conv, p.precision, lay.ksplit, lay.tn, lay.tc, lay.YH, lay.XH, p.launches)
    want = ((c.family,), c.conv, c.prec, c.ksplit, tn, tc, "yh" in c.storage, "xh" in c.storage, 1)
    assert got == want, f"{c.name}: built for {want}, the launcher plans {got}"
    M = rows(c)
    if c.family == "conv9":
        assert (p.NT, p.cpw, p.nchunks) == (c.extra["NT"], c.extra["cpw"], c.extra["nchunks"]), f"{c.name}: {p}"
        assert p.nchunks % p.cpw != 0 and p.grids == (c.ksplit,) and p.reduce_tiles > 0
    else:
        taps_tiles = tn * tc * c.ntaps
        assert p.grids == (taps_tiles * c.ksplit,) and lay.nblk == p.grids[0], f"{c.name}: {p}"
        assert (p.reduce_tiles > 0) == (c.ksplit > 1)
        step = 128 if c.family == "w80" else 4 * KR[c.prec]
        assert lay.rows_per % step == 0 and lay.rows_per * (c.ksplit - 1) < M <= lay.rows_per * c.ksplit, f"{c.name}: {p}"


def assert_group_plan(g, p):
    assert (p.families, p.full, p.precision, p.launches) == (g.families, g.full, g.prec, len(g.families)), f"{g.name}: {p}"
    assert tuple(l.ksplit for l in p.layers) == g.ksplits, f"{g.name}: {p}"
    end = {}
    for i, ((M, N, Cin, st, rps), l) in enumerate(zip(g.layers, p.layers)):
        assert l.launch == i // 5
        assert l.nblk == ((N + 63) // 64) * ((Cin + 63) // 64) * l.ksplit, f"{g.name} layer {i}: {l}"
        assert l.blk0 == (end.get(l.launch, 0) + 7) // 8 * 8, f"{g.name} layer {i}: block range does not start at the next multiple of 8"
        assert (l.XH, l.YH) == ("xh" in st, "yh" in st)
        end[l.launch] = l.blk0 + l.nblk
    assert p.grids == tuple(end[j] for j in range(p.launches))
    assert p.reduce_tiles == sum(((N + 63) // 64) * ((Cin + 63) // 64) for (M, N, Cin, st, rps), l in zip(g.layers, p.layers) if l.ksplit > 1)


# ------------------------------------------------------------------------------------------------------------------
# Problems: one layer's buffers and parameters, whatever the route.  `Layer` is what the references and the emulation take.
# ------------------------------------------------------------------------------------------------------------------
Layer = collections.namedtuple("Layer", "name prec ntaps stride B H W N Cin n_real cin_real grp_real grp_pad ycol0 xcol0 alpha rps "
                                        "yh xh dy x rs dw db dw0 db0")


def _gen(name, tier):
    return torch.Generator().manual_seed(zlib.crc32(f"{name}/{tier}".encode()))


def _values(shape, g, tier):
    if tier == "exact":
        mag = torch.randint(1, 4, shape, generator=g).float()
        return mag * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)
    return torch.randn(shape, generator=g)


def real_columns(n_real_c, grp_real, grp_pad):
    """stored channel of every real input channel"""
    if grp_pad <= 0:
        return list(range(n_real_c))
    return [(r // grp_real) * grp_pad + r % grp_real for r in range(n_real_c)]


def _make_layer(name, tier, prec, *, ntaps, stride, B, H, W, N, Cin, n_real, cin_real, grp_real, grp_pad, ycol0, xcol0, ldy, ldx, alpha,
                prior, rs_entries, rps, yh, xh, filler, guard=True):
    g = _gen(name, tier)
    pad, k = (1, 3) if ntaps == 9 else (0, 1)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    M, xrows = B * Ho * Wo, B * H * W
    dy = torch.full((M, ldy), filler)
    dy[:, ycol0:ycol0 + n_real] = _values((M, n_real), g, tier)
    x = torch.full((xrows, ldx), filler)
    cols = torch.tensor(real_columns(cin_real, grp_real, grp_pad)) + xcol0
    x[:, cols] = _values((xrows, cin_real), g, tier)
    if math.isfinite(filler):                       # a deferred layer: every stored channel is real there (n_real = N, cin_real = Cin)
        assert n_real == N and cin_real == Cin and grp_pad == 0
    rs = None
    if rs_entries:
        if tier == "exact":
            rs = torch.randint(0, 3, (rs_entries,), generator=g).float()
            rs[:3] = torch.tensor([2.0, 0.0, 1.0])[:rs_entries]
        else:
            rs = torch.floor(0.7 + torch.rand(rs_entries, generator=g)) / 0.7
    if yh:
        dy = dy.to(torch.bfloat16)
    if xh:
        x = x.to(torch.bfloat16)
    G = GUARD if guard else 0
    nw, nb = n_real * cin_real * ntaps, n_real
    dw = torch.full((nw + 2 * G,), float("nan"))
    db = torch.full((nb + 2 * G,), float("nan"))
    if prior:
        dw[G:G + nw] = torch.randint(-1000, 1001, (nw,), generator=g).float()
        db[G:G + nb] = torch.randint(-1000, 1001, (nb,), generator=g).float()
    else:
        dw[G:G + nw] = 0.0
        db[G:G + nb] = 0.0
    return Layer(name, prec, ntaps, stride, B, H, W, N, Cin, n_real, cin_real, grp_real, grp_pad, ycol0, xcol0, alpha, rps, yh, xh,
                 dy, x, rs, dw, db, dw.clone(), db.clone())


def make_case_layer(c, tier):
    Ho, Wo = out_hw(c)
    return _make_layer(c.name, tier, c.prec, ntaps=c.ntaps, stride=c.stride, B=c.B, H=c.H, W=c.W, N=c.N, Cin=c.Cin, n_real=c.n_real,
                       cin_real=c.cin_real, grp_real=c.grp_real, grp_pad=c.grp_pad, ycol0=c.ycol0, xcol0=c.xcol0, ldy=c.ldy, ldx=c.ldx,
                       alpha=c.alpha, prior=c.prior, rs_entries=c.B if c.rs else 0, rps=Ho * Wo, yh="yh" in c.storage,
                       xh="xh" in c.storage, filler=float("nan"), guard=c.route != "conv9h")


def make_group_layers(g, tier):
    out = []
    for i, (M, N, Cin, st, rps) in enumerate(g.layers):
        out.append(_make_layer(f"{g.name}/{i}", tier, g.prec, ntaps=1, stride=1, B=1, H=1, W=M, N=N, Cin=Cin, n_real=N, cin_real=Cin,
                               grp_real=0, grp_pad=0, ycol0=0, xcol0=0, ldy=N + 4, ldx=Cin + 8, alpha=g.alpha, prior=g.prior,
                               rs_entries=(M + rps - 1) // rps if rps else 0, rps=rps or M, yh="yh" in st, xh="xh" in st, filler=ALIEN))
    return out


def to_device(l, dev):
    return l._replace(**{k: (None if getattr(l, k) is None else getattr(l, k).to(dev)) for k in ("dy", "x", "rs", "dw", "db", "dw0", "db0")})


def dw_view(l, buf=None):
    G = (l.dw.numel() - l.n_real * l.cin_real * l.ntaps) // 2
    buf = l.dw if buf is None else buf
    return buf[G:buf.numel() - G].view(l.n_real, l.cin_real, l.ntaps)


def db_view(l, buf=None):
    G = (l.db.numel() - l.n_real) // 2
    buf = l.db if buf is None else buf
    return buf[G:buf.numel() - G]


def layer_rows(l):
    pad, k = (1, 3) if l.ntaps == 9 else (0, 1)
    Ho, Wo = (l.H + 2 * pad - k) // l.stride + 1, (l.W + 2 * pad - k) // l.stride + 1
    return l.B * Ho * Wo, Ho, Wo


def check_cap(l):
    """The exact tier's premise: every partial sum, the scaled sum and the result are exactly representable in fp32."""
    M, _, _ = layer_rows(l)
    cap = 2.0 ** 23 if l.alpha == 0.5 else 2.0 ** 24
    assert l.alpha in (0.5, 1.0, 2.0) and max(1.0, l.alpha) * 18 * M + 1000 < cap, f"{l.name}: sums of {M} rows can pass {cap}"
    for t in (l.dy, l.x):
        v = t.float()
        v = v[torch.isfinite(v)]
        assert bool(((v == v.round()) & (v.abs() <= max(3.0, ALIEN))).all())
    return max(1.0, l.alpha) * 18 * M + 1000


# ------------------------------------------------------------------------------------------------------------------
# The gather and the references
# ------------------------------------------------------------------------------------------------------------------
def gather_index(l, device, swap_taps=False):
    """[M, ntaps] row of X each tap of output row m reads, -1 outside the image"""
    M, Ho, Wo = layer_rows(l)
    m = torch.arange(M, device=device)
    if l.ntaps == 1 and l.stride == 1:
        return m[:, None]
    b, rem = m // (Ho * Wo), m % (Ho * Wo)
    oy, ox = rem // Wo, rem % Wo
    pad = 1 if l.ntaps == 9 else 0
    cols = []
    for tap in range(l.ntaps):
        ky, kx = (tap // 3, tap % 3) if l.ntaps == 9 else (0, 0)
        if swap_taps:
            ky, kx = kx, ky
        iy, ix = oy * l.stride - pad + ky, ox * l.stride - pad + kx
        inside = (iy >= 0) & (iy < l.H) & (ix >= 0) & (ix < l.W)
        cols.append(torch.where(inside, (b * l.H + iy) * l.W + ix, torch.full_like(m, -1)))
    return torch.stack(cols, 1)


def _operands(l, dtype, tier):
    """a [M, n_real] and xr [rows, cin_real] as the kernel forms them, in `dtype`; ab: the a the bias sums"""
    M, _, _ = layer_rows(l)
    dev = l.dy.device
    a = l.dy[:, l.ycol0:l.ycol0 + l.n_real].float()
    if l.rs is not None:
        a = a * l.rs[torch.arange(M, device=dev) // l.rps][:, None]              # one fp32 multiply
    cols = torch.tensor(real_columns(l.cin_real, l.grp_real, l.grp_pad), device=dev) + l.xcol0
    xr = l.x[:, cols].float()
    ab = a
    if l.prec == "bf16":
        a, xr = a.to(torch.bfloat16).float(), xr.to(torch.bfloat16).float()
    return a.to(dtype), xr.to(dtype), ab.to(dtype)


def reference(l, tier):
    """(dW, db, S_w, S_b) in float64: prior + alpha * sums, and the magnitude sums of the bound"""
    a, xr, ab = _operands(l, torch.float64, tier)
    idx = gather_index(l, a.device)
    dW = torch.empty(l.n_real, l.cin_real, l.ntaps, dtype=torch.float64, device=a.device)
    S = torch.empty_like(dW)
    for tap in range(l.ntaps):
        src = idx[:, tap]
        A = xr[src.clamp_min(0)] * (src >= 0).to(torch.float64)[:, None]
        dW[:, :, tap] = a.t() @ A
        S[:, :, tap] = a.abs().t() @ A.abs()
    sb, Sb = ab.sum(0), ab.abs().sum(0)
    return (dw_view(l, l.dw0).double() + l.alpha * dW, db_view(l, l.db0).double() + l.alpha * sb, S, Sb)


def _guards_ok(buf, buf0, n):
    G = (buf.numel() - n) // 2
    if G == 0:
        return True
    a, b = buf.view(torch.int32), buf0.view(torch.int32)
    return torch.equal(a[:G], b[:G]) and torch.equal(a[-G:], b[-G:])


def check_exact(l, ref=None):
    """The kernel's dW / db (in l.dw / l.db) against the integer reference: bit-equal, guard bands bit-unchanged."""
    dW, db, _, _ = reference(l, "exact") if ref is None else ref
    assert bool((dW * 2 == (dW * 2).round()).all()) and float(dW.abs().max()) < 2.0 ** 24, f"{l.name}: the reference itself is not exact"
    got_w, got_b = dw_view(l), db_view(l)
    want_w, want_b = dW.float(), db.float()
    assert bool((want_w.double() == dW).all()) and bool((want_b.double() == db).all())
    assert _guards_ok(l.dw, l.dw0, got_w.numel()), f"{l.name}: dW's guard band was written"
    assert _guards_ok(l.db, l.db0, got_b.numel()), f"{l.name}: db's guard band was written"
    if not torch.equal(got_w.contiguous().view(torch.int32), want_w.contiguous().view(torch.int32)):
        bad = (got_w != want_w) | torch.isnan(got_w)
        n, c, t = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError(f"{l.name}: dW differs from the integer reference in {int(bad.sum())} of {bad.numel()} elements, first at "
                             f"[n={n}, c={c}, tap={t}]: {float(got_w[n, c, t])} instead of {float(want_w[n, c, t])}")
    if not torch.equal(got_b.contiguous().view(torch.int32), want_b.contiguous().view(torch.int32)):
        bad = (got_b != want_b) | torch.isnan(got_b)
        n = int(bad.nonzero()[0])
        raise AssertionError(f"{l.name}: db differs from the integer reference in {int(bad.sum())} elements, first at [n={n}]: "
                             f"{float(got_b[n])} instead of {float(want_b[n])}")


def check_bound(l, ksplit, ref=None):
    """The rounding tier: every element finite and within its bound, guards untouched.  Returns the largest |err| / bound."""
    dW, db, S, Sb = reference(l, "rounding") if ref is None else ref
    M, _, _ = layer_rows(l)
    T = M + ksplit + 4
    got_w, got_b = dw_view(l).double(), db_view(l).double()
    assert _guards_ok(l.dw, l.dw0, got_w.numel()) and _guards_ok(l.db, l.db0, got_b.numel()), f"{l.name}: a guard band was written"
    assert bool(torch.isfinite(got_w).all()) and bool(torch.isfinite(got_b).all()), f"{l.name}: non-finite gradient"
    pw, pb = dw_view(l, l.dw0).double(), db_view(l, l.db0).double()
    bw = T * 2.0 ** -23 * min(1.0, l.alpha) * S + 2 * U32 * ((dW - pw).abs() + pw.abs())
    bb = T * 2.0 ** -23 * min(1.0, l.alpha) * Sb + 2 * U32 * ((db - pb).abs() + pb.abs())
    rw = float(((got_w - dW).abs() / bw.clamp_min(1e-300)).max())
    rb = float(((got_b - db).abs() / bb.clamp_min(1e-300)).max())
    assert rw <= 1.0, f"{l.name}: dW is {rw:.3f} of its bound"
    assert rb <= 1.0, f"{l.name}: db is {rb:.3f} of its bound"
    return max(rw, rb)


# ------------------------------------------------------------------------------------------------------------------
# A float32 emulation of the operation (CPU): rows in a shuffled order, cut into `ksplit` ranges at random points, every range
# summed in fp32 into a partial tile, the partials summed in fp32, dst = prior + v * alpha - what any correct kernel may do.
# `mutation` plants one of the bugs the exact tier has to catch (tests/test_wgrad_ref_host.py).
# ------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("drop_last_row_of_split", "duplicate_row", "border_pixel_inside", "swap_ky_kx", "carry_ox_over_image", "ignore_row_scale_once",
             "alpha_on_prior", "skip_prior", "write_row_n_real", "pad_column_as_real", "layer_unreduced", "partial_to_bf16")


def emulate(l, tier, ksplit=3, mutation=None, seed=0):
    """Writes the emulated result into l.dw / l.db (CPU tensors).  Returns True if the mutation found a place to apply."""
    g = torch.Generator().manual_seed(seed + 17)
    M, Ho, Wo = layer_rows(l)
    applied = False
    lm = l
    if mutation == "ignore_row_scale_once" and l.rs is not None:
        k = int((l.rs != 1).nonzero()[0]) if bool((l.rs != 1).any()) else -1
        if k >= 0:
            rs = l.rs.clone(); rs[k] = 1.0
            lm, applied = l._replace(rs=rs), True
    if mutation == "pad_column_as_real" and l.grp_pad > l.grp_real:
        applied = True
    a, xr, ab = _operands(lm, torch.float32, tier)
    if mutation == "pad_column_as_real" and applied:                    # real channel grp_real - 1 of group 0 reads the pad slot beside it
        xr = xr.clone(); xr[:, l.grp_real - 1] = l.x[:, l.xcol0 + l.grp_real].float()
    idx = gather_index(l, a.device, swap_taps=mutation == "swap_ky_kx" and l.ntaps == 9)
    applied |= mutation == "swap_ky_kx" and l.ntaps == 9
    if mutation == "border_pixel_inside" and bool((idx < 0).any()):
        m, tap = [int(v) for v in (idx < 0).nonzero()[len((idx < 0).nonzero()) // 2]]
        ok = idx[m][idx[m] >= 0]
        idx[m, tap], applied = ok[0], True                              # the clamped neighbour instead of zero
    if mutation == "carry_ox_over_image" and l.ntaps == 9 and l.B > 1:
        # the first pixel of image 1 is taken for row Ho of image 0: taps with ky = 0 read image 0's last row, the others nothing
        m0, pad = Ho * Wo, 1
        for tap in range(9):
            iy, ix = Ho * l.stride - pad + tap // 3, 0 - pad + tap % 3
            idx[m0, tap] = iy * l.W + ix if (0 <= iy < l.H and 0 <= ix < l.W) else -1
        applied = True
    perm = torch.randperm(M, generator=g)
    cuts = sorted(torch.randint(0, M + 1, (max(0, ksplit - 1),), generator=g).tolist())
    bounds = [0] + cuts + [M]
    dW = torch.zeros(l.n_real, l.cin_real, l.ntaps)
    dbs = torch.zeros(l.n_real)
    for k in range(len(bounds) - 1):
        sel = perm[bounds[k]:bounds[k + 1]]
        if k == len(bounds) - 2 and len(sel) > 1:
            if mutation == "drop_last_row_of_split":
                sel, applied = sel[:-1], True
            if mutation == "duplicate_row":
                sel, applied = torch.cat([sel, sel[-1:]]), True
        part = torch.zeros_like(dW)
        for tap in range(l.ntaps):
            src = idx[sel, tap]
            A = xr[src.clamp_min(0)] * (src >= 0).float()[:, None]
            part[:, :, tap] = a[sel].t() @ A
        if mutation == "partial_to_bf16" and k == len(bounds) - 2:
            part, applied = part.to(torch.bfloat16).float(), True
        dW += part
        dbs += ab[sel].sum(0)
    pw, pb = dw_view(l, l.dw0), db_view(l, l.db0)
    if mutation == "layer_unreduced":
        return True
    if mutation == "alpha_on_prior":
        rw, rb, applied = (pw + dW) * l.alpha, (pb + dbs) * l.alpha, True
    elif mutation == "skip_prior":
        rw, rb, applied = dW * l.alpha, dbs * l.alpha, True
    else:
        rw, rb = pw + dW * l.alpha, pb + dbs * l.alpha
    dw_view(l).copy_(rw)
    db_view(l).copy_(rb)
    if mutation == "write_row_n_real" and l.n_real < l.N:               # tile row n_real goes to the memory behind the tensor
        G = (l.dw.numel() - rw.numel()) // 2
        l.dw[G + rw.numel():G + rw.numel() + l.cin_real * l.ntaps] = 1.0
        applied = True
    return applied
