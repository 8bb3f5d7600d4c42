"""CPU: the weight-gradient case table against the launcher's own plan query, and the teeth of tests/wgrad_ref.py.

The plan query (ops.wgrad_plan_shape / ops.wgrad_deferred_plan) is host code: every case of the table is asked here, so a
retune of the split rules fails on a machine without a GPU already.  A float32 emulation of the operation, with a shuffled
summation order and random split points, has to pass both tiers of the reference; every planted mutation of it has to fail
the exact tier."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_ref as R  # noqa: E402

OP_CASES = R.op_cases()
GROUPS = R.group_cases()
BY_NAME = {c.name: c for c in OP_CASES}
GROUP_BY_NAME = {g.name: g for g in GROUPS}


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("c", OP_CASES, ids=_ids(OP_CASES))
def test_case_plans_are_as_tabled(c):
    from srad_amd import ops
    R.assert_case_plan(c, R.plan_of_case(c, ops))


@pytest.mark.parametrize("g", GROUPS, ids=_ids(GROUPS))
def test_group_plans_are_as_tabled(g):
    from srad_amd import ops
    R.assert_group_plan(g, ops.wgrad_deferred_plan(g.layers, g.prec))


def test_table_reaches_every_family_and_variant():
    fams = {(c.family, c.prec, c.conv, c.ksplit > 1) for c in OP_CASES}
    for prec in R.PRECS:
        for conv in (False, True):
            for split in (False, True):
                assert ("tile64", prec, conv, split) in fams, (prec, conv, split)
    for conv in (False, True):
        for split in (False, True):
            assert ("w80", "bf16", conv, split) in fams
    assert {c.extra["NT"] for c in OP_CASES if c.family == "conv9" and c.route == "op"} == {1, 2, 3, 4, 5}
    assert {c.storage for c in OP_CASES if c.route == "conv9h"} == {"yh", "yh+xh"}
    launches = {(g.prec, f, full) for g in GROUPS for f, full in zip(g.families, g.full)}
    assert launches == {("bf16", "multi", True), ("bf16", "multi", False), ("bf16", "multi_hh", True), ("fp32", "multi", False)}


def test_plan_of_the_older_deferred_test():
    """tests/test_gpu_bwd_ops.py::test_wgrad_linear_deferred: all six of its shapes, M = 1536 included, are whole 128-row steps
    with rps = 256 - the mask-free body in every storage (the all-bf16 storage on the lean kernel)."""
    from srad_amd import ops
    for M, N, K in ((2048, 540, 180), (1024, 180, 360), (2048, 32, 180), (1024, 360, 244), (3072, 128, 64), (1536, 180, 180)):
        for st, fam in (("f32", "multi"), ("xh", "multi"), ("xh+yh", "multi_hh")):
            p = ops.wgrad_deferred_plan([(M, N, K, st, 0 if st == "xh+yh" else 256)], "bf16")
            assert (p.families, p.full) == ((fam,), (True,)), (M, N, K, st, p)
            assert p.layers[0].rows_per * p.layers[0].ksplit == M
    p = ops.wgrad_deferred_plan([(1536, 180, 180, "xh", 256)], "bf16")
    assert (p.layers[0].ksplit, p.layers[0].rows_per) == (4, 384)


def test_plan_refusals():
    from srad_amd import ops
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.wgrad_plan_shape("bf16", 30, 36, M=100)
    with pytest.raises(RuntimeError, match="bad real extents"):
        ops.wgrad_plan_shape("bf16", 32, 36, M=100, n_real=33)
    with pytest.raises(RuntimeError, match="bad channel groups"):
        ops.wgrad_plan_shape("bf16", 32, 16, M=100, cin_real=12, grp_real=6, grp_pad=10)
    with pytest.raises(RuntimeError, match="bf16 operand storage"):
        ops.wgrad_plan_shape("bf16", 80, 80, ntaps=9, B=1, H=8, W=32, dy_bf16=True)          # below 8192 pixels: not conv9
    with pytest.raises(RuntimeError, match="1 to 6"):
        ops.wgrad_deferred_plan([(1024, 32, 36, "xh", 0)] * 7, "bf16")
    with pytest.raises(RuntimeError, match="bf16 MFMA path"):
        ops.wgrad_deferred_plan([(1024, 32, 36, "xh", 0)], "fp32")


@pytest.mark.parametrize("c", OP_CASES, ids=_ids(OP_CASES))
def test_emulation_passes_both_tiers(c):
    l = R.make_case_layer(c, "exact")
    assert R.check_cap(l) < 2.0 ** 24
    R.emulate(l, "exact", ksplit=5, seed=len(c.name))
    R.check_exact(l)
    if c.rounding:
        l = R.make_case_layer(c, "rounding")
        R.emulate(l, "rounding", ksplit=c.ksplit)
        assert R.check_bound(l, c.ksplit) <= 1.0


@pytest.mark.parametrize("g", GROUPS, ids=_ids(GROUPS))
def test_emulation_passes_both_tiers_groups(g):
    for tier in ("exact",) + (("rounding",) if g.rounding else ()):
        for l, ks in zip(R.make_group_layers(g, tier), g.ksplits):
            R.emulate(l, tier, ksplit=ks)
            if tier == "exact":
                R.check_cap(l)
                R.check_exact(l)
            else:
                assert R.check_bound(l, ks) <= 1.0


# which cases a mutation is planted in: ones where it has a place to act
PLANT = {
    "drop_last_row_of_split": ("lin-bf16-M1000-ragged", "conv9-C80-2x66x64"),
    "duplicate_row": ("lin-fp32-M1000-ragged", "w80-conv-1x17x23"),
    "border_pixel_inside": ("conv-bf16-2x5x7-4to180", "w80-conv-2x9x33", "conv9-C4-1x67x128"),
    "swap_ky_kx": ("conv-fp32-1x15x11s2-36to4", "conv9-C20-1x67x128"),
    "carry_ox_over_image": ("conv-bf16-2x5x7-36to4", "conv-bf16-3x4x4-4to180", "conv9-C16-2x66x64"),
    "ignore_row_scale_once": ("lin-fp32-alpha-prior-rs-ycol", "lin-bf16-alpha-prior-rs-ycol"),
    "alpha_on_prior": ("lin-bf16-alpha-prior-rs-ycol", "real-bf16-reduce-groups-2x6in8"),
    "skip_prior": ("lin-fp32-alpha-prior-rs-ycol", "conv9-C36-2x66x64"),
    "write_row_n_real": ("real-fp32-direct-tail-n3of4", "real-bf16-reduce-n66of68"),
    "pad_column_as_real": ("real-fp32-direct-groups-2x6in8", "real-bf16-reduce-groups-2x6in8"),
    "partial_to_bf16": ("lin-bf16-M1000-ragged",),
}


@pytest.mark.parametrize("mutation,name", [(m, n) for m, names in PLANT.items() for n in names])
def test_planted_mutation_fails_the_exact_tier(mutation, name):
    c = BY_NAME[name]
    l = R.make_case_layer(c, "exact")
    assert R.emulate(l, "exact", ksplit=4, mutation=mutation), f"{mutation} found no place to act in {name}"
    with pytest.raises(AssertionError, match=name):
        R.check_exact(l)
    if mutation == "partial_to_bf16":                       # the class of bug the rounding tier is for
        l = R.make_case_layer(c, "rounding")
        assert R.emulate(l, "rounding", ksplit=4, mutation=mutation)
        with pytest.raises(AssertionError, match="of its bound"):
            R.check_bound(l, c.ksplit)


def test_unreduced_layer_of_a_group_fails_the_exact_tier():
    g = GROUP_BY_NAME["five-mixed-full"]
    layers = R.make_group_layers(g, "exact")
    for i, l in enumerate(layers):
        R.emulate(l, "exact", ksplit=g.ksplits[i], mutation="layer_unreduced" if i == 2 else None)
    for i, l in enumerate(layers):
        if i == 2:
            with pytest.raises(AssertionError, match="differs from the integer reference"):
                R.check_exact(l)
        else:
            R.check_exact(l)


def test_every_mutation_is_planted():
    assert set(PLANT) | {"layer_unreduced"} == set(R.MUTATIONS)


def test_nan_filler_reaches_no_defined_element_and_guards_are_checked():
    """An emulation that reads one column beside the block, or writes one float past the tensor, fails."""
    c = BY_NAME["lin-bf16-alpha-prior-rs-ycol"]
    l = R.make_case_layer(c, "exact")
    R.emulate(l._replace(ycol0=l.ycol0 - 1), "exact")
    with pytest.raises(AssertionError):
        R.check_exact(l)
    l = R.make_case_layer(c, "exact")
    R.emulate(l, "exact")
    l.db[R.GUARD - 1] = 0.0
    with pytest.raises(AssertionError, match="guard band"):
        R.check_exact(l)
    assert torch.isnan(l.dy.float()).any() and torch.isnan(l.x.float()).any()
