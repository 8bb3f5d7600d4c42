"""GPU: the guarded Adam step (DESIGN.md "Guarded step") from the kernels up to the command line: the fp64 norm against
numpy, detection of a single inf / NaN anywhere in the buffer, the bits of an applied step against the unguarded kernels,
clipping against ``clip_grad_norm_`` + ``torch.optim.Adam``, the applied-step count, and the same through ``FusedAdam``,
the two graphed steps, data parallelism and ``main``."""
import math
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_train import _write_grid_class, build_train

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 1e-4, 0.9, 0.999, 1e-8
INF = float("inf")
FULL_PASS = 4096 * 256                       # threads of the capped grid: Adam's stride in floats, the norm pass's in float4s
SIZES = [1, 255, 257, FULL_PASS + 257]
PAST_A_PASS = 4 * FULL_PASS + 257             # a ragged tail behind one full pass of the norm kernel's 16-byte loads
UNROLLED = 17 * FULL_PASS + 259               # > 12 FULL_PASS floats: the four-loads-in-flight loop runs, then both remainders


def _dev(t, pad=0):
    """``t`` on the GPU, ``pad`` floats behind the allocation's (256-byte) alignment."""
    buf = torch.empty(t.numel() + pad, device="cuda")
    buf[pad:].copy_(t)
    return buf[pad:]


def _guard(sizes, max_norm=None):
    from srad_amd.train import GradGuard
    return GradGuard(sizes, "cuda", (B1, B2), max_norm)


def _hyper(lr=LR, gs=1.0):
    return torch.tensor([lr, 0.0, 0.0, gs], dtype=torch.float32).cuda()


def _f32(v):
    return float(np.float32(v))


# ---------------------------------------------------------------- 1: the norm
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("n", SIZES + [UNROLLED])
def test_norm_one_tensor_matches_numpy_fp64_and_repeats(n, pad):
    from srad_amd.train import guard_reference
    g = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000 + pad))
    gd = _dev(g, pad)
    assert gd.data_ptr() % 16 == 4 * pad
    want = guard_reference(g.numpy(), grad_scale=0.5)[0]
    bits = []
    for _ in range(2):
        guard = _guard([n])
        guard.run([gd], _hyper(gs=0.5))
        st = guard.stats()
        print("n", n, "pad", pad, "last_norm", st["last_norm"], "numpy", want, "rel", abs(st["last_norm"] - want) / want)
        assert abs(st["last_norm"] - want) <= 1e-9 * want
        assert (st["applied"], st["skipped"], st["clipped"]) == (1, 0, 0) and int(guard.apply_flag[0]) == 1
        bits.append(guard.state.cpu())
    assert torch.equal(bits[0], bits[1])


@pytest.mark.parametrize("pads", [(0, 0, 0), (1, 3, 2)])
def test_norm_three_uneven_tensors_into_one_partial_buffer(pads):
    from srad_amd.train import guard_reference
    sizes = [255, FULL_PASS + 257, 1]
    gen = torch.Generator().manual_seed(11)
    host = [torch.randn(n, generator=gen) * (k + 1) for k, n in enumerate(sizes)]
    devs = [_dev(t, p) for t, p in zip(host, pads)]
    want = guard_reference([t.numpy() for t in host])[0]
    bits = []
    for _ in range(2):
        guard = _guard(sizes)
        assert guard.slots == [1, 4096, 1] and guard.nbytes == 64 + 8 * 4098
        guard.ws[64:].fill_(0xFF)                              # NaN patterns: every slot must be written, none may be added to
        guard.run(devs, _hyper())
        st = guard.stats()
        print("pads", pads, "last_norm", st["last_norm"], "numpy", want, "rel", abs(st["last_norm"] - want) / want)
        assert abs(st["last_norm"] - want) <= 1e-9 * want and st["applied"] == 1
        bits.append(guard.state.cpu())
    assert torch.equal(bits[0], bits[1])
    # every tensor counts: one tensor less, another norm
    guard = _guard(sizes[:2])
    guard.run(devs[:2], _hyper())
    assert abs(guard.stats()["last_norm"] - guard_reference([t.numpy() for t in host[:2]])[0]) <= 1e-9 * want
    assert guard.stats()["last_norm"] != st["last_norm"]


# ---------------------------------------------------------------- 2: detection, and a skipped step touches nothing
def _adam_inputs(n, seed, pad=0):
    g = torch.Generator().manual_seed(seed)
    p, m, ema = (torch.randn(n, generator=g) for _ in range(3))
    v = torch.rand(n, generator=g) * 1e-2
    return [_dev(t, pad) for t in (p, m, v, ema)]


def _guarded_step(guard, bufs, grad, ema_on, wd=0.0, hyper=None, decay=0.999):
    """guard -> guarded Adam through the C ABI, as ``FusedAdam._guarded`` issues them."""
    from srad_amd import _lib as L
    lib, s = L.lib(), L.current_stream_ptr()
    p, m, v, ema = bufs
    hyper = _hyper() if hyper is None else hyper
    guard.run([grad], hyper)
    if ema_on:
        rc = lib.srad_adam_ema_guarded_step(L.dptr(p), L.dptr(grad), L.dptr(m), L.dptr(v), L.dptr(ema), p.numel(), B1, B2, EPS, wd,
                                            decay, L.dptr(guard.ws), s)
    else:
        rc = lib.srad_adam_guarded_step(L.dptr(p), L.dptr(grad), L.dptr(m), L.dptr(v), p.numel(), B1, B2, EPS, wd, L.dptr(guard.ws), s)
    L.check(rc, "guarded adam")
    torch.cuda.synchronize()                                  # hyper stays alive until the finalize has read it


@pytest.mark.parametrize("bad", [INF, -INF, float("nan")])
@pytest.mark.parametrize("n,pad", [(257, 0), (257, 1), (PAST_A_PASS, 0), (PAST_A_PASS, 1)])
def test_one_nonfinite_element_anywhere_skips_the_step_bit_for_bit(n, pad, bad):
    clean = torch.randn(n, generator=torch.Generator().manual_seed(5)) * 0.1
    for ema_on in (True, False):
        bufs = _adam_inputs(n, seed=21, pad=pad)
        before = [t.clone() for t in bufs]
        guard = _guard([n], max_norm=1.0)
        positions = [0, n // 2, n - 1] + ([4 * FULL_PASS - 1, 4 * FULL_PASS] if n > 4 * FULL_PASS else [])
        for k, at in enumerate(positions):                    # first, middle, last (the ragged tail), both sides of a full pass
            g = clean.clone()
            g[at] = bad
            _guarded_step(guard, bufs, _dev(g, pad), ema_on, wd=1e-4)
            st = guard.stats()
            assert int(guard.apply_flag[0]) == 0 and (st["applied"], st["skipped"], st["clipped"]) == (0, k + 1, 0), (at, st)
            assert not math.isfinite(st["last_norm"])
            for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "ema"), bufs, before):
                assert torch.equal(a, b), (name, at, ema_on)
        _guarded_step(guard, bufs, _dev(clean, pad), ema_on, wd=1e-4)     # the same guard applies the next clean step
        assert int(guard.apply_flag[0]) == 1 and guard.stats()["applied"] == 1
        assert not torch.equal(bufs[0], before[0]) and torch.equal(bufs[3], before[3]) != ema_on


@pytest.mark.parametrize("bad", [INF, float("nan")])
def test_detection_in_the_unrolled_loop(bad):
    """Positions that the four-loads-in-flight loop reads (one per load of the trip), the single-load loop and the tail."""
    n = UNROLLED
    g = _dev(torch.ones(n) * 1e-3)
    guard = _guard([n])
    for k, at in enumerate([0, 4 * FULL_PASS + 5, 8 * FULL_PASS + 6, 12 * FULL_PASS + 7, 16 * FULL_PASS + 9, n - 1]):
        g[at] = bad
        guard.run([g], _hyper())
        g[at] = 1e-3
        assert int(guard.apply_flag[0]) == 0 and guard.stats()["skipped"] == k + 1, at
    guard.run([g], _hyper())
    st = guard.stats()
    assert int(guard.apply_flag[0]) == 1 and abs(st["last_norm"] - 1e-3 * math.sqrt(n)) <= 1e-6 * st["last_norm"]


@pytest.mark.parametrize("n", [257, FULL_PASS + 257])
def test_huge_finite_gradients_are_applied_not_skipped(n):
    """3e38 squared overflows fp32; the fp64 squares do not, so the norm is finite and the step is taken (and clipped)."""
    from srad_amd.train import guard_reference
    g = torch.full((n,), 3e38)
    g[1::2] = -3e38
    g[0] = 1.0
    bufs = _adam_inputs(n, seed=2)
    before = [t.clone() for t in bufs]
    guard = _guard([n], max_norm=1.0)
    _guarded_step(guard, bufs, _dev(g), ema_on=True)
    st = guard.stats()
    want = guard_reference(g.numpy())[0]
    assert int(guard.apply_flag[0]) == 1 and (st["applied"], st["skipped"], st["clipped"]) == (1, 0, 1)
    assert math.isfinite(st["last_norm"]) and abs(st["last_norm"] - want) <= 1e-9 * want
    assert all(bool(torch.isfinite(t).all()) for t in bufs) and not torch.equal(bufs[0], before[0])


# ---------------------------------------------------------------- 3: an applied step carries the unguarded kernels' bits
def _plain_dev_step(bufs, grad, ema_on, wd, hyper, decay=0.999):
    from srad_amd import _lib as L
    lib, s = L.lib(), L.current_stream_ptr()
    p, m, v, ema = bufs
    if ema_on:
        rc = lib.srad_adam_ema_step_dev(L.dptr(p), L.dptr(grad), L.dptr(m), L.dptr(v), L.dptr(ema), p.numel(), B1, B2, EPS, wd, decay,
                                        L.dptr(hyper), s)
    else:
        rc = lib.srad_adam_step_dev(L.dptr(p), L.dptr(grad), L.dptr(m), L.dptr(v), p.numel(), B1, B2, EPS, wd, L.dptr(hyper), s)
    L.check(rc, "adam dev")
    torch.cuda.synchronize()


def _neighbours(x):
    x = np.float32(x)
    return {float(x), float(np.nextafter(x, np.float32(-np.inf))), float(np.nextafter(x, np.float32(np.inf)))}


def _host_corrections(t):
    b1, b2 = _f32(B1), _f32(B2)                               # FusedAdam.hyper(): fp64 from the fp32 betas
    return 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)


@pytest.mark.parametrize("max_norm", [None, 1e9])             # coef == 1 both ways: no clipping, and a norm below the bound
@pytest.mark.parametrize("ema_on", [True, False])
@pytest.mark.parametrize("n,pad", [(257, 1), (FULL_PASS + 257, 0)])
def test_applied_step_has_the_bits_of_the_unguarded_kernels(n, pad, ema_on, max_norm):
    gen = torch.Generator().manual_seed(8)
    grads = [_dev(torch.randn(n, generator=gen) * 0.1, pad) for _ in range(3)]
    for wd in (0.0, 1e-4):
        for gs in (1.0, 0.5):
            mine, twin = _adam_inputs(n, seed=31, pad=pad), _adam_inputs(n, seed=31, pad=pad)
            start = mine[0].clone()
            guard = _guard([n], max_norm)
            for t in (1, 2, 3):
                _guarded_step(guard, mine, grads[t - 1], ema_on, wd=wd, hyper=_hyper(gs=gs))
                rec = guard.record.clone()
                c1, c2 = _host_corrections(t)
                assert float(rec[0]) == _f32(LR) and float(rec[3]) == _f32(gs), (t, rec)      # coef == 1 exactly
                assert float(rec[1]) in _neighbours(c1) and float(rec[2]) in _neighbours(c2), (t, rec, c1, c2)
                _plain_dev_step(twin, grads[t - 1], ema_on, wd, rec)
                for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "ema"), mine, twin):
                    assert torch.equal(a, b), (name, n, ema_on, wd, gs, t)
            assert not torch.equal(mine[0], start) and guard.stats()["clipped"] == 0
            assert torch.equal(mine[3], _adam_inputs(n, seed=31, pad=pad)[3]) != ema_on


def test_bias_corrections_at_step_1000():
    n = 300
    guard = _guard([n])
    guard.state[:8].view(torch.int64)[0] = 999                # applied
    mine, twin = _adam_inputs(n, seed=4), _adam_inputs(n, seed=4)
    g = _dev(torch.randn(n, generator=torch.Generator().manual_seed(1)))
    _guarded_step(guard, mine, g, ema_on=False)
    rec = guard.record.clone()
    c1, c2 = _host_corrections(1000)
    print("t = 1000: device", float(rec[1]), float(rec[2]), "host", _f32(c1), _f32(c2))
    assert guard.stats()["applied"] == 1000
    assert float(rec[1]) in _neighbours(c1) and float(rec[2]) in _neighbours(c2)
    _plain_dev_step(twin, g, False, 0.0, rec)
    assert all(torch.equal(a, b) for a, b in zip(mine, twin))


# ---------------------------------------------------------------- 4: clipping
@pytest.mark.parametrize("n", [4099, FULL_PASS + 257])
def test_clipping_matches_clip_grad_norm_and_torch_adam(n):
    """norm = 10 max_norm on every one of four steps; the bar is the plain-Adam test's, 5e-6 absolute at lr 1e-4."""
    from srad_amd.train import guard_reference
    max_norm = 0.5
    gen = torch.Generator().manual_seed(77)
    bufs = _adam_inputs(n, seed=6)
    bufs[1].zero_(), bufs[2].zero_()                          # torch.optim.Adam starts from zero moments
    ref = torch.nn.Parameter(bufs[0].clone())
    topt = torch.optim.Adam([ref], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=0)
    guard = _guard([n], max_norm)
    for it in range(4):
        g = torch.randn(n, generator=gen)
        g = _dev(g * (10.0 * max_norm / float(g.double().norm())))
        _guarded_step(guard, bufs, g, ema_on=False)
        ref.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_([ref], max_norm)
        assert abs(float(total) - 10.0 * max_norm) < 1e-4 and abs(guard.stats()["last_norm"] - 10.0 * max_norm) < 1e-5
        coef = guard_reference(g.cpu().numpy(), max_norm=max_norm)[1]      # the fp64 reference of tests/test_grad_guard_host.py
        assert abs(coef - 0.1) < 1e-6 and float(guard.record[3]) in _neighbours(coef), (float(guard.record[3]), coef)
        topt.step()
        diff = float((bufs[0] - ref.detach()).abs().max())
        print("step", it, "max |guarded - clip_grad_norm_ + torch Adam|", diff)
        assert diff < 5e-6, (it, diff)
    st = guard.stats()
    assert (st["applied"], st["skipped"], st["clipped"]) == (4, 0, 4)


# ---------------------------------------------------------------- 5: the bias correction counts applied steps
@pytest.mark.parametrize("ema_on", [True, False])
def test_clean_poisoned_clean_equals_clean_clean(ema_on):
    from srad_amd.train import guard_reference_run
    n = FULL_PASS + 257
    gen = torch.Generator().manual_seed(13)
    g1, g2 = (_dev(torch.randn(n, generator=gen) * 0.1) for _ in range(2))
    poisoned = g1.clone()
    poisoned[n - 2] = float("nan")
    mine, twin = _adam_inputs(n, seed=17), _adam_inputs(n, seed=17)
    guard, tguard = _guard([n], 1.0), _guard([n], 1.0)
    for g in (g1, poisoned, g2):
        _guarded_step(guard, mine, g, ema_on, wd=1e-4)
    for g in (g1, g2):
        _guarded_step(tguard, twin, g, ema_on, wd=1e-4)
    for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "ema"), mine, twin):
        assert torch.equal(a, b), name
    st, tst = guard.stats(), tguard.stats()
    assert (st["applied"], st["skipped"]) == (2, 1) and (tst["applied"], tst["skipped"]) == (2, 0)
    assert st["clipped"] == tst["clipped"] == 2 and st["last_norm"] == tst["last_norm"]
    assert guard_reference_run([1.0, float("nan"), 1.0]) [:2] == (2, 1)
    assert torch.equal(guard.record, tguard.record)           # the third attempt was corrected as step 2


# ---------------------------------------------------------------- 6: FusedAdam, eager and graphed
def _poisoned(x):
    bad = x.clone()
    bad[0, 0, 3, 3] = INF
    return bad


def _snapshot(m, opt):
    return [t.clone() for t in (m.flat_params, opt.exp_avg, opt.exp_avg_sq, m.flat_ema)]


def test_poisoned_batch_really_gives_nonfinite_gradients_and_ruins_an_unguarded_run():
    """The contrast: l1_grad maps a NaN difference to a zero seed, so this is asserted and not assumed."""
    from srad_amd.train import FusedAdam, train_step
    from tests.test_gpu_ema import _tiny_drct
    make, x, hr = _tiny_drct()
    m = make()
    opt = FusedAdam(m, lr=LR, ema_decay=0.999)
    train_step(m, x, hr, opt)
    assert bool(torch.isfinite(m.flat_grads).all()) and bool(torch.isfinite(m.flat_params).all())
    train_step(m, _poisoned(x), hr, opt)
    assert not bool(torch.isfinite(m.flat_grads).all())
    assert not bool(torch.isfinite(m.flat_params).all()) and not bool(torch.isfinite(m.flat_ema).all())


@pytest.mark.parametrize("graphed", [False, True])
def test_fused_adam_skips_a_poisoned_batch_eager_and_graphed(graphed):
    from srad_amd.train import FusedAdam, GraphedTrainStep, train_step
    from tests.test_gpu_ema import _tiny_drct
    make, x, hr = _tiny_drct()
    m, twin = make(), make()
    opt, topt = (FusedAdam(mm, lr=LR, ema_decay=0.999, max_grad_norm=1e3) for mm in (m, twin))
    if graphed:
        step, tstep = GraphedTrainStep(m, opt, warmup=2), GraphedTrainStep(twin, topt, warmup=2)
    else:
        step, tstep = (lambda a, b: train_step(m, a, b, opt)), (lambda a, b: train_step(twin, a, b, topt))
    warm = 3 if graphed else 1                                # graphed: two eager warm-up steps, the capture and its first replay
    for i in range(warm):
        step(x + i, hr)
        tstep(x + i, hr)
    if graphed:
        assert len(step._graphs) == 1
    before = _snapshot(m, opt)
    step(_poisoned(x), hr)                                    # graphed: a replay
    for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "ema"), _snapshot(m, opt), before):
        assert torch.equal(a, b), name
    st = opt.guard_stats()
    assert (st["applied"], st["skipped"]) == (warm, 1) and not math.isfinite(st["last_norm"])
    assert opt.step_count == warm + 1                         # the host counts attempts
    step(x + warm, hr)                                        # the next clean step: as if the poisoned batch had never come
    tstep(x + warm, hr)
    for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "ema"), _snapshot(m, opt), _snapshot(twin, topt)):
        assert torch.equal(a, b), name
    assert not torch.equal(m.flat_params, before[0])
    st, tst = opt.guard_stats(), topt.guard_stats()
    assert (st["applied"], st["skipped"]) == (warm + 1, 1) and (tst["applied"], tst["skipped"]) == (warm + 1, 0)
    assert st["last_norm"] == tst["last_norm"] and math.isfinite(st["last_norm"]) and st["last_norm"] > 0
    if graphed:
        assert len(step._graphs) == 1 and len(tstep._graphs) == 1
    # the state dict carries the guard only in this mode, and restores the applied count
    sd = opt.state_dict()
    assert list(sd) == ["step", "exp_avg", "exp_avg_sq", "lr", "ema", "ema_decay", "guard_state"]
    fresh = FusedAdam(make(), lr=LR, ema_decay=0.999, skip_nonfinite=True)
    assert fresh.guard.max_norm == INF and fresh.guard_stats()["applied"] == 0
    fresh.load_state_dict(sd)
    assert fresh.guard_stats() == st and fresh.step_count == warm + 2
    plain = FusedAdam(make(), lr=LR)
    assert list(plain.state_dict()) == ["step", "exp_avg", "exp_avg_sq", "lr"] and plain.guard is None
    with pytest.raises(RuntimeError):
        plain.guard_stats()


def test_guarded_eager_and_graphed_steps_share_one_arithmetic():
    """With clipping active on every step, graphed replays and eager steps give the same bits."""
    from srad_amd.train import FusedAdam, GraphedTrainStep, train_step
    from tests.test_gpu_ema import _tiny_drct
    make, x, hr = _tiny_drct()
    m, twin = make(), make()
    opt, topt = (FusedAdam(mm, lr=LR, max_grad_norm=1e-3) for mm in (m, twin))
    step = GraphedTrainStep(m, opt, warmup=2)
    for i in range(5):
        if i == 4:                                            # a scheduler step between replays reaches the guard through set4
            opt.param_groups[0]["lr"] = topt.param_groups[0]["lr"] = 0.5 * LR
        step(x + i, hr)
        train_step(twin, x + i, hr, topt)
        assert torch.equal(m.flat_params, twin.flat_params), i
    st = opt.guard_stats()
    assert st == topt.guard_stats() and (st["applied"], st["clipped"]) == (5, 5) and len(step._graphs) == 1


# ---------------------------------------------------------------- 7: DRN-L with its dual models
def test_drn_guards_on_every_optimizer_graphed_equals_eager():
    from srad_amd.train import FusedAdam, GraphedDrnTrainStep, TensorAdam, drn_train_step, guard_reference
    from tests.helpers import rel_err
    from tests.test_gpu_drn_train import _setup
    runs = []
    for mode in ("eager", "graph"):
        cfg, sd, duals, lrs, hr, m, dms = _setup(4, 1, 2, 20, 1, 4, 4)
        opt = FusedAdam(m, lr=LR, weight_decay=1e-8, max_grad_norm=0.05)
        dopts = [TensorAdam(dm.parameters(), lr=LR, weight_decay=1e-8, max_grad_norm=0.05) for dm in dms]
        lr_t, hr_t = [torch.from_numpy(a).cuda() for a in lrs], torch.from_numpy(hr).cuda()
        step = (GraphedDrnTrainStep(m, dms, opt, dopts, warmup=2) if mode == "graph"
                else (lambda a, b: drn_train_step(m, dms, a, b, opt, dopts)))
        losses = [float(step([t + 0.5 * i for t in lr_t], hr_t)) for i in range(4)]
        stats = [o.guard_stats() for o in [opt] + dopts]
        if mode == "eager":                                   # the gradients of the last step are still there
            for dm, o, st in zip(dms, dopts, stats[1:]):
                parts = [p.grad.detach().cpu().numpy() for p in dm.parameters()]
                assert len(parts) >= 2
                want = guard_reference(parts)[0]
                print("dual last_norm", st["last_norm"], "numpy over", [a.size for a in parts], want)
                assert abs(st["last_norm"] - want) <= 1e-9 * want
                assert st["last_norm"] > guard_reference(parts[0])[0]          # one norm over all of them, not over the first
            want = guard_reference(m.flat_grads.cpu().numpy())[0]
            assert abs(stats[0]["last_norm"] - want) <= 1e-9 * want
        runs.append((losses, m.flat_params.clone(), [p.detach().clone() for dm in dms for p in dm.parameters()], stats))
        if mode == "graph":
            assert len(step._graphs) == 1
            assert "guard_state" in dopts[0].state_dict() and "guard_state" not in TensorAdam(dms[0].parameters()).state_dict()
    (le, pe, de, se), (lg, pg, dg, sg) = runs
    assert max(abs(a - b) / abs(a) for a, b in zip(le, lg)) < 1e-5
    assert rel_err(pg.cpu().numpy(), pe.cpu().numpy()) < 1e-5
    for a, b in zip(de, dg):
        assert rel_err(b.cpu().numpy(), a.cpu().numpy()) < 1e-5
    for a, b in zip(se, sg):
        assert (a["applied"], a["skipped"]) == (b["applied"], b["skipped"]) == (4, 0)
        assert abs(a["last_norm"] - b["last_norm"]) <= 1e-4 * a["last_norm"]
    assert se[0]["clipped"] == sg[0]["clipped"] == 4          # the SR net's norm is far above 0.05


# ---------------------------------------------------------------- 8: data parallel
DP_MAX_NORM = 1e-2


def _dp_worker(rank, world, port, cfg_tuple, seed, x, hr, q):
    import struct
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from srad_amd import spec as S
    from srad_amd.train import FusedAdam, GradReducer, train_step
    cfg = S.DRCTConfig(*cfg_tuple)
    sd = S.synth_state(S.drct_spec(cfg), seed=seed, gain=1.0, cfg=cfg)
    m = build_train(cfg, sd, "fp32")
    opt = FusedAdam(m, lr=LR, max_grad_norm=DP_MAX_NORM)
    red = GradReducer().attach(m)
    xs, hs = torch.from_numpy(x[rank::world]).cuda(), torch.from_numpy(hr[rank::world]).cuda()
    train_step(m, xs, hs, opt, red)
    torch.cuda.synchronize()
    st = opt.guard_stats()
    q.put((rank, struct.pack("d", st["last_norm"]), st, m.flat_params.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_guarded_step_two_ranks_equals_one_rank_on_the_full_batch():
    import socket
    import struct
    import torch.multiprocessing as mp
    from srad_amd import spec as S
    from srad_amd.train import FusedAdam, train_step
    cfg_tuple = (1, 16, 8, 2, 180, 2)        # in_chans, img_size, window, upscale, embed_dim, n_rdg
    cfg = S.DRCTConfig(*cfg_tuple)
    x = S.synth_image("dp", (4, 1, 16, 16), seed=5)
    hr = S.synth_image("dp/hr", (4, 1, 32, 32), seed=6)
    sd = S.synth_state(S.drct_spec(cfg), seed=9, gain=1.0, cfg=cfg)
    m = build_train(cfg, sd, "fp32")
    opt = FusedAdam(m, lr=LR, max_grad_norm=DP_MAX_NORM)
    train_step(m, torch.from_numpy(x).cuda(), torch.from_numpy(hr).cuda(), opt)
    g_ref, p_ref, st_ref = m.flat_grads.cpu().numpy(), m.flat_params.cpu().numpy(), opt.guard_stats()
    assert st_ref["clipped"] == 1 and st_ref["last_norm"] > 10 * DP_MAX_NORM
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, cfg_tuple, 9, x, hr, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in procs:
        r, bits, st, pp = q.get(timeout=300)
        res[r] = (bits, st, pp)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][0] == res[1][0]                             # the same norm bits on both ranks: the same decision, no collective
    assert res[0][1] == res[1][1] and (res[0][1]["applied"], res[0][1]["clipped"]) == (1, 1)
    norm = struct.unpack("d", res[0][0])[0]
    assert abs(norm - st_ref["last_norm"]) < 2e-4 * st_ref["last_norm"]      # grad_scale = 1 / world is inside the norm
    big = np.abs(g_ref) > 1e-3 * np.abs(g_ref).max()          # as the unguarded test: where the gradient is clearly non-zero
    assert np.abs(res[0][2] - p_ref)[big].max() < 2e-5
    assert np.array_equal(res[0][2], res[1][2])


# ---------------------------------------------------------------- 9: the command line
def test_cli_train_with_and_without_the_guard(tmp_path):
    from srad_amd import main as Mn
    from srad_amd import options as Opt
    from srad_amd.train import FusedAdam
    from tests.test_gpu_ema import _tiny_drct
    data = str(tmp_path / "data")
    _write_grid_class(tmp_path / "data", n_test=(2, 2))
    base = ["--model-type", "drct", "--classe", "grid", "--resolution", "128", "--scale", "4", "--epochs", "1", "--batch-size", "4",
            "--data-root", data]

    def run(save, extra):
        opt = Mn.build_train_opt(Opt.parse_train_args(base + ["--save-dir", str(tmp_path / save)] + extra))
        opt.depths, opt.num_heads, opt.test_every, opt.print_every = (6, 6), (6, 6), 3, 1       # 2 RDG, 3 steps per epoch
        Mn.train_drct(opt)
        read = lambda f: open(os.path.join(opt.save, f)).read()
        return opt, read("log.txt"), read("config.txt"), torch.load(os.path.join(opt.save, "optimizer.pt"))

    opt, log, cfg, osd = run("on", ["--grad-clip", "0.5", "--skip-nonfinite"])
    assert opt.grad_clip == 0.5 and opt.skip_nonfinite is True
    lines = [l for l in log.splitlines() if "[L1: " in l]
    assert len(lines) == 3 and all("[grad norm: " in l for l in lines), lines
    assert all(float(l.split("[grad norm: ")[1].split("]")[0]) > 0 for l in lines)
    assert log.count("Guarded steps: ") == 1 and " skipped (non-finite gradients) of 3" in log
    assert "grad_clip: 0.5" in cfg and "skip_nonfinite: True" in cfg
    assert osd["step"] == 3 and osd["guard_state"].numel() == 32
    make, _, _ = _tiny_drct()
    other = FusedAdam(make(), lr=LR, max_grad_norm=0.5)
    sd = other.state_dict()
    sd["guard_state"] = osd["guard_state"]
    other.load_state_dict(sd)
    st = other.guard_stats()
    assert (st["applied"], st["skipped"]) == (3, 0) and st["last_norm"] > 0
    assert f"{st['last_norm']:.4e}" in lines[-1]

    opt, log, cfg, osd = run("off", [])
    assert "grad_clip" not in cfg and "skip_nonfinite" not in cfg
    assert "grad norm" not in log and "Guarded steps" not in log and log.count("[L1: ") == 3
    assert list(osd) == ["step", "exp_avg", "exp_avg_sq", "lr"]
