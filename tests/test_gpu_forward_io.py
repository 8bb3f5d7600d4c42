"""GPU: the DRCT inference forward reads the caller's input and writes a fresh output with graph replay on.  Only the launches
between the one that reads x and the one that writes y are recorded (csrc/drct.hip), so a new input or output pointer neither
recaptures nor costs a copy, and every output is the eager forward's, bit for bit."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8, 8), (2, 1, 16, 8)]          # the smallest legal inputs at window 8: one window, and 2 x (2 x 1) windows
PRECISIONS = ["bf16", "fp32"]


def _cfg_sd(seed=5):
    from srad_amd import spec as S
    cfg = S.DRCTConfig(n_rdg=1)
    return cfg, S.synth_state(S.drct_spec(cfg), seed=seed, cfg=cfg)


def _build(precision, use_graph, sd=None):
    from tests.test_gpu_drct import build
    cfg, sd0 = _cfg_sd()
    return build(cfg, sd0 if sd is None else sd, precision, use_graph)


@functools.lru_cache(maxsize=None)
def _models(precision):
    """(graph off, graph on) with the same weights; shared by the tests that do not change them"""
    return _build(precision, False), _build(precision, True)


def _fresh_inputs(shape, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(shape, generator=g).cuda() for _ in range(n)]      # a new allocation and new contents each


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES)
def test_fresh_inputs_replay_without_copies_or_recapture(shape, precision):
    eager, graph = _models(precision)
    base = graph.graph_captures()
    xs = _fresh_inputs(shape, 5, seed=sum(shape))
    assert len({x.data_ptr() for x in xs}) == 5
    with torch.no_grad():
        want = [eager(x).cpu() for x in xs]
        outs, kept = [], []
        for x in xs:                                             # eager, capture, replay, replay, replay
            outs.append(graph(x))
            kept.append(outs[-1].cpu())
    assert not torch.equal(want[0], want[1])                     # different inputs did give different images
    for i in range(5):
        assert torch.equal(kept[i], want[i]), i                  # graph on == graph off, for this call's input
        assert torch.equal(outs[i].cpu(), kept[i]), i            # ... and no later call wrote over an earlier output
    assert len({o.data_ptr() for o in outs}) == 5                # five live outputs, five buffers
    assert graph.graph_captures() == base + 1                    # one capture, whatever x and y were
    # another shape: one eager run, one capture; then back to replaying
    other = (shape[0], 1, shape[3] + 8, shape[2])
    ys = _fresh_inputs(other, 3, seed=7)
    with torch.no_grad():
        for y in ys:
            assert torch.equal(graph(y).cpu(), eager(y).cpu())
    assert graph.graph_captures() == base + 2


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fp16_and_non_contiguous_inputs(precision):
    eager, graph = _models(precision)
    x = _fresh_inputs((2, 1, 8, 16), 1, seed=3)[0]
    xt = x.transpose(2, 3)                                       # [2, 1, 16, 8], not contiguous
    xh = _fresh_inputs((2, 1, 16, 8), 1, seed=4)[0].half()
    assert not xt.is_contiguous()
    with torch.no_grad():
        for _ in range(3):                                       # through the eager run, the capture and a replay
            assert torch.equal(graph(xt).cpu(), eager(xt.contiguous()).cpu())
            assert torch.equal(graph(xh).cpu(), eager(xh.float()).cpu())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_set_param_between_replays_reaches_the_next_output(precision):
    """A changed parameter - one read by the recorded launches, one folded into a Swin block's second half, one folded into the
    output end (the launch after the graph) - is repacked, and its fold rebuilt, before anything of the next call is launched."""
    cfg, sd = _cfg_sd()
    m = _build(precision, True, sd)
    xs = _fresh_inputs(SHAPES[1], 6, seed=11)
    with torch.no_grad():
        before = [m(x).cpu() for x in xs[:3]]
        n = m.graph_captures()
        assert n == 1
        m.get_parameter("conv_first.bias").add_(0.05)
        m.get_parameter("layers.0.swin2.mlp.fc2.weight").mul_(1.25)
        m.get_parameter("conv_last.weight").mul_(0.5)
        after = [m(x).cpu() for x in xs[3:]] + [m(xs[0]).cpu()]
        fresh = _build(precision, False, {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()})
        want = [fresh(x).cpu() for x in xs[3:]] + [fresh(xs[0]).cpu()]
    assert m.graph_captures() == n                               # the same graph went on replaying
    for got, ref in zip(after, want):
        assert torch.equal(got, ref)
    assert not torch.equal(after[-1], before[0])
