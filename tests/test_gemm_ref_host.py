"""CPU: (1) the GEMM plan query reproduces the tile selection the launcher had before the plan existed, over a grid of
(precision, M, N, LayerNorm, conv); (2) the reference and checker of tests/gemm_ref.py hold what they promise: a float32
emulation of the operation stays inside the derived bound at every case of the GPU table, and every planted kernel bug is
caught.  No GPU: the plan query is host code, the emulation plain torch."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as G  # noqa: E402

# ---------------------------------------------------------------------------------------------- the plan


def old_rule(prec, M, N, ln, conv):
    """Transcription of launch_prec / launch_cfg as they stood before srad_op_gemm_plan: (BM, BN, CPS)."""
    def tiles(bm, bn):
        return ((M + bm - 1) // bm) * ((N + bn - 1) // bn)
    if not ln and N <= 16 and tiles(128, 16) >= 384:
        t = (128, 16)
    elif not ln and N <= 32 and tiles(128, 32) >= 384:
        t = (128, 32)
    elif N <= 32:
        t = (32, 32)
    elif prec == "bf16" and not ln and 64 < N <= 80 and tiles(128, 80) >= 256:
        t = (128, 80)
    elif not ln and 64 < N <= 80 and tiles(64, 80) >= 384:
        t = (64, 80)
    elif tiles(64, 64) >= 384:
        t = (64, 64)
    elif tiles(32, 64) >= 384:
        t = (32, 64)
    else:
        t = (32, 32)
    default = 8 if prec == "bf16" else 4
    if conv:
        c = 4 if prec == "bf16" and t in ((64, 64), (64, 80), (128, 80)) else default
    elif ln:
        c = default
    else:
        c = 4 if prec == "bf16" and t == (64, 64) else default
    return t + (c,)


def old_family(prec, N, Cin, B, H, W, ps):
    """The kernels srad_launch_gemm tried before the tiled one, for a 3x3 stride-1 conv with bias, no activation, no residual."""
    M = B * H * W
    if prec != "bf16":
        return "tiled"
    if not ps and Cin == 80 and N == 80 and H % 4 == 0 and W % 32 == 0 and M >= 128 * 64:
        return "conv80"
    if ps and N == 320 and Cin == 80 and H % 4 == 0 and W % 32 == 0 and M >= 128 * 64:
        return "conv80x4"
    n4 = (N + 3) // 4
    if not ps and Cin <= 8 and Cin * 4 * n4 <= 320 and n4 in (1, 5, 10, 20) and M >= 32768:
        return "thin"
    if not ps and 1 <= N <= 4 and Cin in (40, 80) and W % 16 == 0 and M >= 32768:
        return "tail"
    return "tiled"


# row counts around every threshold of the rule: 384 tiles of 128 / 64 / 32 rows, 256 of 128, and their halves and thirds for
# problems with 2 or 3 column tiles
_MS = sorted({1, 31, 32, 33, 77, 4100} | {k * bm + d for bm in (32, 64, 128) for k in (127, 128, 191, 192, 255, 256, 383, 384)
                                          for d in (-1, 0, 1)})
_NS = (1, 3, 12, 16, 17, 20, 32, 33, 64, 65, 72, 80, 81, 100, 128, 129, 180, 192, 193, 540)


def test_plan_reproduces_the_old_tile_rule():
    from srad_amd import ops
    n = 0
    for prec in G.PRECS:
        for ln in (False, True):
            for N in _NS:
                for M in _MS:
                    p = ops.gemm_plan_shape(prec, M, N, 180, ln=ln)
                    bm, bn, c = old_rule(prec, M, N, ln, False)
                    want = ("tiled", bm, bn, c, ln, False, False, ((N + bn - 1) // bn, (M + bm - 1) // bm), 1)
                    assert tuple(p) == want, (prec, M, N, ln, p, want)
                    n += 1
    assert n == 3 * 2 * len(_NS) * len(_MS)


_IMGS = ((1, 7, 11), (1, 64, 128), (1, 180, 182), (2, 128, 128), (1, 157, 157), (1, 181, 181), (1, 211, 233), (1, 256, 192), (3, 109, 113))


def test_plan_reproduces_the_old_conv_dispatch():
    """3x3 convs: the kernel family in front of the tiled GEMM, and behind it the same tile rule with the conv K-stage depth."""
    from srad_amd import ops
    seen = set()
    for prec in G.PRECS:
        for (B, H, W) in _IMGS:
            for N, Cin, ps in [(n, c, False) for n in (3, 4, 12, 20, 40, 72, 80, 100, 180) for c in (4, 8, 36, 40, 80)] + \
                              [(320, 80, True), (100, 36, True), (12, 36, True), (320, 36, True)]:
                p = ops.gemm_plan_shape(prec, 0, N, Cin, ntaps=9, B=B, H=H, W=W, pixel_shuffle=ps)
                fam = old_family(prec, N, Cin, B, H, W, ps)
                seen.add(fam)
                assert p.family == fam, (prec, B, H, W, N, Cin, ps, p)
                if fam == "tiled":
                    bm, bn, c = old_rule(prec, B * H * W, N, False, True)
                    assert tuple(p)[1:] == (bm, bn, c, False, True, ps, ((N + bn - 1) // bn, (B * H * W + bm - 1) // bm), 1), (prec, N, Cin, p)
                else:
                    assert p.launches == (4 if fam == "conv80x4" else 1) and p.grid == (0, 0)
            for (N, Cin) in ((100, 36), (20, 36)):             # stride 2: the conv gather at a quarter of the rows
                p = ops.gemm_plan_shape(prec, 0, N, Cin, ntaps=9, stride=2, B=B, H=H, W=W)
                M = B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)
                assert tuple(p)[:7] == ("tiled",) + old_rule(prec, M, N, False, True) + (False, True, False), (prec, B, H, W, p)
    assert seen == {"tiled", "conv80", "conv80x4", "thin", "tail"}


def test_plan_refuses_what_the_launch_refuses():
    from srad_amd import ops
    with pytest.raises(RuntimeError, match="up to 320 channels"):
        ops.gemm_plan_shape("bf16", 77, 20, 324, ln=True)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.gemm_plan_shape("fp32", 77, 20, 38)
    with pytest.raises(RuntimeError, match="pixel-shuffle"):
        ops.gemm_plan_shape("fp32", 0, 10, 36, ntaps=9, B=1, H=8, W=8, pixel_shuffle=True)
    assert ops.gemm_plan_shape("bf16", G.M128, 20, 180, ln=True)[:3] == ("tiled", 32, 32)     # LayerNorm never takes a 128-row tile


def test_every_case_names_the_plan_it_gets():
    """The case table of the GPU tests against the plan query: every tile, K-stage depth and variant the issue lists is there."""
    from srad_amd import ops
    got = set()
    for c in G.all_cases() + G.determinism_cases():
        p = ops.gemm_plan_shape(c.prec, c.M, c.N, c.Cin, ntaps=c.ntaps, stride=c.stride, B=c.B, H=c.H, W=c.W, ln=c.ln, act=c.act,
                                residual=c.residual, pixel_shuffle=c.ps)
        assert p.family == "tiled" and G.Plan(*p[1:7]) == c.plan, (c.name, p)
        got.add((c.prec,) + tuple(c.plan))
    for prec in G.PRECS:
        for tile in ((128, 16), (128, 32), (32, 32), (64, 80), (64, 64), (32, 64)) + (((128, 80),) if prec == "bf16" else ()):
            for conv in (False, True):
                assert (prec,) + tile + (G.cps(prec, *tile, conv=conv), False, conv, False) in got, (prec, tile, conv)
        for tile in ((32, 32), (64, 64), (32, 64)):
            assert (prec,) + tile + (G.cps(prec, *tile, ln=True), True, False, False) in got
    assert ("bf16", 128, 80, 4, False, True, False) in got and ("bf16", 64, 64, 4, False, True, True) in got


# ---------------------------------------------------------------------------------------------- reference and checker

_CASES = G.all_cases()


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(c):
        if c.name not in cache:
            cache.clear()                                 # one case at a time: the large ones hold a few hundred MB
            t = G.make_inputs(c)
            cache[c.name] = (t, G.reference(c, t))
        return cache[c.name]
    return get


def test_emulation_is_inside_the_bound_at_every_case(refs):
    """The reference alone stays inside the bound: float32 arithmetic in another order is not a kernel bug."""
    worst = {}
    for c in _CASES:
        t, ref = refs(c)
        r = G.check(c, G.emulate(c, t), ref)
        worst[c.prec] = max(worst.get(c.prec, 0.0), r)
    print("largest |err| / bound of the float32 emulation:", worst)
    assert all(v <= 1.0 for v in worst.values())


def _by_name(name):
    (c,) = [c for c in _CASES if c.name == name]
    return c


# one no-LayerNorm case per precision and path kind (mutations that need more than one 32-row block use M >= 64)
_MUT_CASES = ["lin-32x64-c36-plain-fp32", "lin-32x64-c180-offset-bf16", "lin-32x64-c180-lrelu_res-bf16x3", "conv-32x64-c36-relu-bf16",
              "lin-fall32x32-c36-gelu-fp32"]
_GENERAL = [m for m in G.MUTATIONS if m != "swap_dxdy"]


@pytest.mark.parametrize("name", _MUT_CASES)
@pytest.mark.parametrize("mutation", _GENERAL)
def test_checker_catches(refs, name, mutation):
    c = _by_name(name)
    t, ref = refs(c)
    with pytest.raises(AssertionError):
        G.check(c, G.emulate(c, t, mutation=mutation), ref)


@pytest.mark.parametrize("name", ["conv-64x64-shuffle-bf16", "conv-128x16-shuffle-fp32"])
@pytest.mark.parametrize("mutation", ["swap_dxdy", "write_past_n", "dup_last_row"])
def test_checker_catches_on_pixel_shuffle(refs, name, mutation):
    c = _by_name(name)
    t, ref = refs(c)
    assert G.check(c, G.emulate(c, t), ref) <= 1.0
    with pytest.raises(AssertionError):
        G.check(c, G.emulate(c, t, mutation=mutation), ref)


def test_checker_wants_nan_outside_and_finite_inside(refs):
    c = _by_name("lin-fall32x32-c36-plain-fp32")
    t, ref = refs(c)
    good = G.emulate(c, t)
    assert G.check(c, good, ref) <= 1.0
    bad = good.clone()
    bad[c.M, 0] = 0.0                                     # a slack row
    with pytest.raises(AssertionError, match="outside the output"):
        G.check(c, bad, ref)
    bad = good.clone()
    bad[5, c.out_offset + 3] = float("nan")               # an element never written
    with pytest.raises(AssertionError, match="not finite"):
        G.check(c, bad, ref)
    bad = good.clone()
    bad[5, c.out_offset + 3] = float("inf")
    with pytest.raises(AssertionError, match="not finite"):
        G.check(c, bad, ref)
