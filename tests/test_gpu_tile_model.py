"""GPU: ``Model`` with tiled inference on (DESIGN.md "Tiled inference").  The oracle is the composition the definition names:
the gather restatement, the PLAIN network on the same chunks of ``tile_batch`` tiles, the blend restatement
(tests/test_tile_host.py).  Every comparison is ``torch.equal``."""
import numpy as np
import pytest
import torch

from tests import helpers
from tests.test_gpu_self_ensemble import _lr, composed
from tests.test_tile_host import axis_rule, blend_ref, gather_ref

pytestmark = pytest.mark.gpu


def _drct_model(tile=8, overlap=2, blend="mean", self_ensemble=False):
    from srad_amd import options as Opt
    from srad_amd import spec as S
    from srad_amd.model import Model
    opt = Opt.build_opt('drct', 'grid', 64, 4)                # the tiny config of tests/test_gpu_self_ensemble.py: window 4, one RDG
    opt.use_graph, opt.depths, opt.num_heads = False, (6,), (6,)
    opt.self_ensemble, opt.drop_path_rate = self_ensemble, 0.0
    if tile:
        opt.tile, opt.tile_overlap, opt.tile_blend = tile, overlap, blend
    cfg = S.DRCTConfig(in_chans=1, img_size=16, window_size=4, upscale=4, n_rdg=1)
    sd = S.synth_state(S.drct_spec(cfg), seed=9, gain=0.7, cfg=cfg)
    m = Model(opt, None)
    m.get_model().load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.eval()


def tiled(net, x, T, O, g, blend, step):
    """The definition around ``net``: gather, ``net`` on chunks of ``step`` tiles, blend output by output at its own scale."""
    B, _, h, w = x.shape
    tiles = torch.from_numpy(gather_ref(x.cpu().numpy(), T, O, g)).cuda()
    ty = tiles.shape[2]
    ys = [net(tiles[i:i + step]) for i in range(0, tiles.shape[0], step)]
    many = isinstance(ys[0], (list, tuple))
    outs = []
    for j in range(len(ys[0]) if many else 1):
        y = torch.cat([c[j] if many else c for c in ys])
        outs.append(torch.from_numpy(blend_ref(y.cpu().numpy(), B, h, w, T, O, g, y.shape[2] // ty, blend)).cuda())
    return outs if many else outs[0]


def _default_step(ty, tx):
    return max(1, min(64, 65536 // (ty * tx)))                 # evaluate._auto_batch on the tile's LR pixels


@pytest.mark.parametrize("blend", ["mean", "feather"])
def test_drct_any_size_is_the_definition(blend):
    m = _drct_model(8, 2, blend)
    assert m.model.granule == m.model.window_size == 4 and (m.tile, m.tile_overlap, m.tile_blend, m.tile_batch) == (8, 2, blend, 0)
    x = _lr((1, 1, 22, 30))                                   # not a multiple of the window: 4 x 5 = 20 tiles
    assert len(axis_rule(22, 8, 2, 4)[3]) * len(axis_rule(30, 8, 2, 4)[3]) == 20
    with torch.no_grad():
        with pytest.raises(ValueError, match="multiple of the window"):
            m.model(x)                                        # the plain network still refuses the size
        for step in (7, 0):                                   # 7 + 7 + 6 tiles, and the default (one chunk of 20)
            m.tile_batch = step
            got = m(x)
            want = tiled(m.model, x, 8, 2, 4, blend, step or _default_step(8, 8))
            assert tuple(got.shape) == (1, 1, 22 * 4, 30 * 4) and not got.requires_grad
            assert torch.equal(got, want), (step, float((got - want).abs().max()))
        assert _default_step(8, 8) == 64


def test_one_tile_without_padding_is_the_plain_forward():
    m = _drct_model(16, 0)
    x = _lr((2, 1, 16, 16))
    with torch.no_grad():
        assert torch.equal(m(x), m.model(x))
        m.tile_blend = "feather"
        assert torch.equal(m(x), m.model(x))


def test_tile_zero_makes_no_tile_call(monkeypatch):
    from srad_amd import ops
    m = _drct_model(0)
    for name in ("tile_plan", "tile_gather", "tile_blend"):
        monkeypatch.setattr(ops, name, helpers.must_not_be_called(name, "tile = 0 is the path without tiles"))
    monkeypatch.setattr(m, "forward_tiled", helpers.must_not_be_called("forward_tiled", "tile = 0 is the path without tiles"))
    x = _lr((2, 1, 16, 16))
    with torch.no_grad():
        assert torch.equal(m(x), m.model(x))
        assert torch.equal(m.forward_x8(x), composed(m.model, x))


def test_settings_are_refused_when_the_model_is_made():
    for kw, what in ((dict(tile=6), "granule"), (dict(tile=8, overlap=8), "overlap"), (dict(tile=8, blend="median"), "tile_blend"),
                     (dict(tile=4096, overlap=1024), "4094")):
        with pytest.raises(ValueError, match=what):
            _drct_model(**kw)


def test_drn_blends_every_output_at_its_own_scale():
    from srad_amd import options as Opt
    from srad_amd.model import Model
    opt = Opt.build_opt('drn-l', 'grid', 64, 4)
    opt.n_blocks, opt.use_graph = 2, False
    opt.tile, opt.tile_overlap, opt.tile_blend = 8, 3, "feather"
    m = Model(opt, None).eval()
    assert m.model.granule == 1
    x = _lr((1, 1, 13, 21))
    m.tile_batch = 5
    with torch.no_grad():
        got, want = m(x), tiled(m.model, x, 8, 3, 1, "feather", 5)
    assert isinstance(got, list) and len(got) == 3 == len(want)
    for j in range(3):
        assert tuple(got[j].shape) == (1, 1, 13 * 2 ** j, 21 * 2 ** j)
        assert torch.equal(got[j], want[j]), (j, float((got[j] - want[j]).abs().max()))


def test_self_ensemble_runs_the_tiled_network():
    m = _drct_model(8, 2, "mean", self_ensemble=True)
    m.tile_batch = 7
    net = lambda t: tiled(m.model, t, 8, 2, 4, "mean", 7)    # every member tiled with its own plan
    for shape in ((1, 1, 16, 16), (1, 1, 10, 14)):
        x = _lr(shape)
        with torch.no_grad():
            got, want = m(x), composed(net, x)
        assert tuple(got.shape) == (1, 1, 4 * shape[2], 4 * shape[3])
        assert torch.equal(got, want), float((got - want).abs().max())


def test_training_mode_ignores_the_flag(monkeypatch):
    m = _drct_model(8, 2)
    x = _lr((2, 1, 16, 16))
    with torch.no_grad():
        tiled_out = m(x)
        plain = m.model(x)
    assert not torch.equal(tiled_out, plain)                  # in eval mode the flag is not ignored
    m.train()
    monkeypatch.setattr(m, "forward_tiled", helpers.must_not_be_called("forward_tiled", "training mode ignores the tile setting"))
    y = m(x)
    assert y.requires_grad and tuple(y.shape) == (2, 1, 64, 64)
    m.eval()
