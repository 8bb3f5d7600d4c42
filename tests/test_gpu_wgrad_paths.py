"""GPU: every launch path of the weight-gradient kernels (csrc/kernels_wgrad.hip) against the references of
tests/wgrad_ref.py.

Every case first asks the launcher's plan query which kernel its very tensors take and asserts the family, variant flags and
row splits the case table states: a retune of the split rules fails here instead of turning a case into a test of another
kernel.  Every case then runs the exact tier - small-integer operands, so the fp32 result has to be bit-identical to the
integer reference whatever the precision, storage, split or reduce order, and one dropped row or one wrong border pixel fails
with certainty - with NaN in every operand column the operation does not define and NaN guard bands around dW and db.  The
cases marked `rounding` also run N(0, 1) operands against a derived per-element bound.

The largest |err| / bound seen per kernel family is printed when the module finishes (pytest -s).  The module stops launching
after a device error."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

_WORST = {}
_DEVICE_ERROR = []
OP_CASES = R.op_cases()
GROUPS = R.group_cases()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield torch.device("cuda:0")
    if _WORST:
        print("\nlargest |err| / bound per family: " + ", ".join(f"{k} {v[0]:.2e} ({v[1]})" for k, v in sorted(_WORST.items())))


def _guarded(name, fn):
    """A device error ends the module: nothing more is launched on a card that may have faulted."""
    if _DEVICE_ERROR:
        pytest.exit(f"stopped after a device error in {_DEVICE_ERROR[0]}", returncode=3)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except RuntimeError:
        _DEVICE_ERROR.append(name)
        raise


def _note(family, ratio, name):
    print(f"{name}: |err| / bound {ratio:.2e}")
    if ratio > _WORST.get(family, (0.0, ""))[0]:
        _WORST[family] = (ratio, name)


def _op_kwargs(c, l):
    kw = dict(ntaps=c.ntaps, stride=c.stride, precision=c.prec, n_real=c.n_real, cin_real=c.cin_real, grp_real=c.grp_real,
              grp_pad=c.grp_pad, ycol0=c.ycol0, row_scale=l.rs)
    if c.conv or c.rs:
        kw.update(B=c.B, H=c.H, W=c.W)
    return kw


def _run_op(c, tier, dev, check_plan):
    from srad_amd import ops
    l = R.to_device(R.make_case_layer(c, tier), dev)
    if c.route == "conv9h":
        if check_plan:
            R.assert_case_plan(c, ops.wgrad_plan(l.dy, l.x, 80, 80, ntaps=9, B=c.B, H=c.H, W=c.W, precision="bf16"))
        dw, db = _guarded(c.name, lambda: ops.wgrad_conv9_bf16(l.dy, l.x, B=c.B, H=c.H, W=c.W))
        return l._replace(dw=dw.reshape(-1), db=db)          # fresh, zeroed outputs without guard bands (l.dw0 / l.db0 are zero)
    dy, x = l.dy, l.x[:, c.xcol0:c.xcol0 + c.Cin]
    kw = _op_kwargs(c, l)
    if check_plan:
        R.assert_case_plan(c, ops.wgrad_plan(dy, x, c.N, c.Cin, **kw))
    _guarded(c.name, lambda: ops.wgrad(dy, x, c.N, c.Cin, alpha=c.alpha, dw=R.dw_view(l), db=R.db_view(l), **kw))
    return l


@pytest.mark.parametrize("c", OP_CASES, ids=[c.name for c in OP_CASES])
def test_immediate_paths(dev, c):
    """wgrad_kernel<fp32 | bf16, linear | conv> with direct stores and through the reduce, the real-extent and group stores,
    wgrad80_kernel, wgrad_conv9_kernel<NT> and its bf16-storage variants, the square-tile reduce."""
    l = _run_op(c, "exact", dev, True)
    R.check_cap(l)
    R.check_exact(l)
    if c.rounding:
        l = _run_op(c, "rounding", dev, False)
        _note(c.family, R.check_bound(l, c.ksplit), c.name)


def _run_group(g, tier, dev, check_plan):
    from srad_amd import ops
    layers = [R.to_device(l, dev) for l in R.make_group_layers(g, tier)]
    steps = [ops.wq_wgrad_deferred(l.dy[:, :l.N], l.x[:, :l.Cin], R.dw_view(l).view(l.N, l.Cin), R.db_view(l), row_scale=l.rs,
                                   rps=l.rps if l.rs is not None else 0, alpha=l.alpha) for l in layers]
    plan = ops.wgrad_deferred_plan(steps, g.prec)
    if check_plan:
        R.assert_group_plan(g, plan)
    _guarded(g.name, lambda: ops.wgrad_queue_script(steps, precision=g.prec))
    return layers, plan


@pytest.mark.parametrize("g", GROUPS, ids=[g.name for g in GROUPS])
def test_deferred_groups(dev, g):
    """wgrad_multi_kernel<fp32>, <bf16, FULL> and <bf16, !FULL> with their per-layer storage branches, wgrad_multi_hh_kernel;
    five layers of different shapes in one launch (block ranges from multiples of 8, padding blocks between them) and the
    launch a sixth layer triggers."""
    layers, _ = _run_group(g, "exact", dev, True)
    for l in layers:
        R.check_cap(l)
        R.check_exact(l)
    if g.rounding:
        layers, plan = _run_group(g, "rounding", dev, False)
        for l, lp in zip(layers, plan.layers):
            _note(plan.families[lp.launch], R.check_bound(l, lp.ksplit), l.name)


def test_two_launches_are_bit_equal(dev):
    c = next(c for c in OP_CASES if c.name == "conv9-C80-2x66x64")
    a = _run_op(c, "rounding", dev, False)
    b = _run_op(c, "rounding", dev, False)
    assert torch.equal(a.dw.view(torch.int32), b.dw.view(torch.int32)) and torch.equal(a.db.view(torch.int32), b.db.view(torch.int32))
