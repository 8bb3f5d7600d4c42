"""CPU: the bf16-rounding reference (tests/grad_ref.py) and its per-tensor checker, tested before they judge the engine.
 * with the rounding replaced by the identity, the hand-written backward formulas of ``bf16_matmuls()`` equal plain autograd;
 * one corrupted tensor at a time - the kinds of wiring mistake a flat cosine cannot see - is reported, alone;
 * ``oracle.sr_ref.F`` is torch.nn.functional again after the context, also after an exception."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import sr_ref as R
from srad_amd import spec as S
from tests import grad_ref as G
from tests.helpers import DRN_GAIN

KEEP_P = 0.7


@functools.lru_cache(maxsize=None)
def _drct_case():
    """One RDG, window 8, gray x2, B = 2 at 16 x 16: the 89 parameter tensors of the DropPath test of test_gpu_train.py."""
    cfg = S.DRCTConfig(in_chans=1, img_size=16, window_size=8, upscale=2, n_rdg=1)
    sd = S.synth_state(S.drct_spec(cfg), seed=77, gain=1.0, cfg=cfg)
    gen = torch.Generator().manual_seed(1)
    keep = torch.floor(KEEP_P + torch.rand(2 * cfg.n_rdg * 5, 2, generator=gen)) / KEEP_P
    return cfg, sd, keep


def _drct_images(seed):
    return S.synth_image("tr", (2, 1, 16, 16), seed=seed), S.synth_image("tr/hr", (2, 1, 32, 32), seed=seed + 1)


def _drct_run(seed, emulate, keep=None, rnd=G.bf16_round):
    cfg, sd, keep0 = _drct_case()
    x, hr = _drct_images(seed)
    keep = keep0 if keep is None else keep
    out, loss, dx, grads = G.oracle_grads(G.drct_l1(cfg, hr, G.keeps_of(keep, cfg.n_rdg)), sd, x, emulate, rnd)
    return G.as_tensors(out, dx, grads)


@functools.lru_cache(maxsize=None)
def _drct_exact_and_pairs():
    exact = _drct_run(5, False)
    pairs = [(_drct_run(5, True), exact)] + [(_drct_run(s, True), _drct_run(s, False)) for s in (15, 25)]
    return exact, pairs


def _drn_run(emulate, rnd):
    cfg = S.DRNConfig(n_colors=3, scale=4, n_blocks=2, n_feats=20)
    sds = {"": S.synth_state(S.drn_spec(cfg), seed=31, gain=DRN_GAIN, cfg=cfg)}
    for i in range(cfg.phase):
        sds[f"dual{i}."] = S.synth_state(S.dual_spec(cfg), seed=131 + i, gain=DRN_GAIN, cfg=cfg)
    B, H = 2, 8
    lrs = [S.synth_image(f"drn_tr/lr{i}", (B, 3, H << i, H << i), seed=6 + i) for i in range(cfg.phase)]
    hr = S.synth_image("drn_tr/hr", (B, 3, H * 4, H * 4), seed=9)
    out, loss, dx, grads = G.oracle_grads(G.drn_composite(cfg, lrs, hr), sds, lrs[0], emulate, rnd)
    return G.as_tensors(out, dx, grads)


def _assert_same(got, want):
    assert sorted(got) == sorted(want)
    for n, w in want.items():
        scale = float(w.abs().max())
        assert scale > 0, n
        err = float((got[n] - w).abs().max())
        assert err <= 1e-6 * scale, (n, err, scale)


def test_identity_rounding_equals_plain_autograd_drct():
    want = _drct_exact_and_pairs()[0]
    cfg, sd, _ = _drct_case()
    assert sorted(want) == sorted([k for k, v in sd.items() if v.dtype.kind == "f" and "attn_mask" not in k] +["<out0>", "<dx>"])      # 89 parameters, the output, dx
    _assert_same(_drct_run(5, True, rnd=lambda t: t), want)


def test_identity_rounding_equals_plain_autograd_drn_with_dual_models():
    """The stride-2 and the bias-free convolutions (DownBlock, in the net and as the dual models), the 1 x 1 convolutions of the
    channel attention on a 1 x 1 image, and the 1 x 1 MeanShift layers."""
    want = _drn_run(False, None)
    assert any(n.startswith("dual1.dual_module.0.0") for n in want) and "down.0.dual_module.0.0.weight" in want
    _assert_same(_drn_run(True, lambda t: t), want)


def test_bf16_rounding_moves_every_gradient_a_little_and_skips_1x1_inputs():
    """The emulation is not the identity: every tensor moves, by a bf16-sized amount (so the bars exist and are far below the cap
    for DRCT); a convolution on a 1 x 1 image is left in fp32."""
    exact, pairs = _drct_exact_and_pairs()
    rep = G.per_tensor_report(exact, exact, pairs)
    assert all(0 < r["e_emu"] for r in rep.values())
    assert max(r["e_emu"] for r in rep.values()) < G.BAR_CAP / G.BAR_FACTOR, max(rep.items(), key=lambda t: t[1]["e_emu"])
    assert not G.left_out(rep) and not G.failures(rep)
    x, w = torch.randn(2, 5, 1, 1), torch.randn(7, 5, 1, 1)
    with G.bf16_matmuls():
        assert torch.equal(R.F.conv2d(x, w), F.conv2d(x, w))
        assert not torch.equal(R.F.conv2d(x.expand(2, 5, 2, 2), w), F.conv2d(x.expand(2, 5, 2, 2), w))


def _flat_cos(a, b, names):
    u = torch.cat([a[n].reshape(-1) for n in names]).double()
    v = torch.cat([b[n].reshape(-1) for n in names]).double()
    return float((u * v).sum() / (u.norm() * v.norm()))


def _corruptions(exact):
    """{label: {name: corrupted gradient}}: one wiring mistake each."""
    L0 = "layers.0."
    c = {}
    c["bias gradient zeroed"] = {L0 + "swin2.mlp.fc1.bias": torch.zeros_like(exact[L0 + "swin2.mlp.fc1.bias"])}
    c["norm1.weight from norm2"] = {L0 + "swin2.norm1.weight": exact[L0 + "swin2.norm2.weight"].clone()}
    c["qkv weight doubled"] = {L0 + "swin3.attn.qkv.weight": 2 * exact[L0 + "swin3.attn.qkv.weight"]}
    c["proj weight transposed"] = {L0 + "swin1.attn.proj.weight": exact[L0 + "swin1.attn.proj.weight"].t().contiguous()}
    t1, t4 = L0 + "swin1.attn.relative_position_bias_table", L0 + "swin4.attn.relative_position_bias_table"
    assert tuple(exact[t1].shape) == tuple(exact[t4].shape) == (225, 6)
    c["tables of swin1 and swin4 exchanged"] = {t1: exact[t4].clone(), t4: exact[t1].clone()}
    # DropPath: the MLP branch's factor of one kept sample of swin3 left off (1 instead of 1 / keep_prob), oracle rerun
    cfg, sd, keep = _drct_case()
    row = 2 * 2 + 1                                              # block index 2 (swin3), MLP branch
    b = int(torch.nonzero(keep[row] > 0)[0])
    other = keep.clone()
    other[row, b] = 1.0
    name = L0 + "swin3.mlp.fc2.weight"
    c["DropPath factor left off one sample"] = {name: _drct_run(5, False, keep=other)[name]}
    return c


def test_checker_flags_each_corrupted_tensor_alone_where_the_flat_cosine_sees_nothing():
    exact, pairs = _drct_exact_and_pairs()
    params = [n for n in exact if not n.startswith("<")]
    cases = _corruptions(exact)
    assert len(cases) == 6
    for label, changed in cases.items():
        got = dict(exact)
        got.update(changed)
        for n, t in changed.items():
            assert not torch.equal(t, exact[n]), (label, n)
        rep = G.per_tensor_report(got, exact, pairs)
        cos = _flat_cos(got, exact, params)
        print(f"{label}: flat cosine {cos:.8f}, flagged {[(n, round(rep[n]['e_eng'], 3), round(rep[n]['bar'], 4)) for n in G.failures(rep)]}")
        assert sorted(G.failures(rep)) == sorted(changed), (label, G.failures(rep))
        assert cos > 0.99, (label, cos)                          # the bar the bf16 engine tests had: it passes all six
        with pytest.raises(AssertionError):
            G.assert_report(rep, 0.0, label)


def test_left_out_tensors_are_counted_and_still_held_to_a_cosine():
    exact, pairs = _drct_exact_and_pairs()
    name = "layers.0.swin1.attn.relative_position_bias_table"
    noisy = dict(pairs[0][0])
    noisy[name] = pairs[0][1][name] * 1.2                        # e_emu 0.2: 4 x 0.2 is past the cap
    rep = G.per_tensor_report(exact, exact, [(noisy, pairs[0][1])] + pairs[1:])
    assert G.left_out(rep) == [name] and rep[name]["bar"] == G.BAR_CAP and not G.failures(rep)
    G.assert_report(rep, 0.05, "one of 91 tensors left out")
    with pytest.raises(AssertionError):
        G.assert_report(rep, 0.0, "none may be left out")
    for wrong in (-exact[name], exact[name] * float("nan")):     # left out of the bar, not out of the test
        got = dict(exact)
        got[name] = wrong
        assert G.failures(G.per_tensor_report(got, exact, [(noisy, pairs[0][1])] + pairs[1:])) == [name]


def test_oracle_functional_is_restored():
    assert R.F is F
    with G.bf16_matmuls():
        assert R.F is not F and R.F.gelu is F.gelu
    assert R.F is F
    with pytest.raises(ZeroDivisionError):
        with G.bf16_matmuls():
            1 / 0
    assert R.F is F
