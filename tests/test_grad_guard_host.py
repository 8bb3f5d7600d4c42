"""CPU: the guarded step's public surface without a GPU (DESIGN.md "Guarded step") - ``--grad-clip`` / ``--skip-nonfinite`` and
their YAML keys, the five C entry points (exported, and every refusal made before a launch), the optimizers' keywords, and
the numpy fp64 reference of norm, coef and applied count that the GPU tests compare against."""
import ctypes as C
import inspect
import math
import os
import types

import numpy as np
import pytest

SRAD_ERR_ARG = 1
INF = float("inf")


# ---------------------------------------------------------------- flags, YAML keys
def test_flags_are_off_by_default_and_leave_no_field():
    from srad_amd import options as Opt
    from srad_amd.main import build_train_opt
    t = Opt.parse_train_args([])
    assert t.grad_clip is None and t.skip_nonfinite is False
    for model_type in ('drct', 'drn-l'):
        off = build_train_opt(Opt.parse_train_args(['--model-type', model_type]))
        assert 'grad_clip' not in vars(off) and 'skip_nonfinite' not in vars(off)      # config.txt lists vars(opt)
        on = build_train_opt(Opt.parse_train_args(['--model-type', model_type, '--grad-clip', '0.5']))
        assert on.grad_clip == 0.5 and 'skip_nonfinite' not in vars(on)
        on = build_train_opt(Opt.parse_train_args(['--model-type', model_type, '--skip-nonfinite']))
        assert on.skip_nonfinite is True and 'grad_clip' not in vars(on)
        on = build_train_opt(Opt.parse_train_args(['--model-type', model_type, '--grad-clip', '2', '--skip-nonfinite']))
        assert on.grad_clip == 2.0 and on.skip_nonfinite is True


def test_grad_clip_parsing_from_the_command_line_and_a_config_file(tmp_path):
    from srad_amd import options as Opt
    from srad_amd.main import build_train_opt
    assert Opt.parse_train_args(['--grad-clip', '1e-3']).grad_clip == 1e-3
    assert Opt.parse_train_args(['--grad-clip', 'inf']).grad_clip == INF                 # "no clipping", as max_norm = +inf
    for bad in ('0', '-1', '-0.0', 'nan', 'x'):
        with pytest.raises(SystemExit):
            Opt.parse_train_args(['--grad-clip', bad])
    on = tmp_path / 'on.yaml'
    on.write_text("grad_clip: 0.25\nskip_nonfinite: true\n")
    a = Opt.parse_train_args(['--config', str(on)])
    assert a.grad_clip == 0.25 and a.skip_nonfinite is True
    opt = build_train_opt(a)
    assert opt.grad_clip == 0.25 and opt.skip_nonfinite is True
    assert Opt.parse_train_args(['--config', str(on), '--grad-clip', '3']).grad_clip == 3.0      # command line wins
    for bad in ('0', '0.0', '-2', '.nan'):
        cfg = tmp_path / 'bad.yaml'
        cfg.write_text(f"grad_clip: {bad}\n")
        with pytest.raises(SystemExit):
            Opt.parse_train_args(['--config', str(cfg)])


def test_make_optimizers_pass_the_guard_only_with_the_flags():
    from srad_amd import trainer as T
    seen = []

    class Spy:
        def __init__(self, model, **kw):
            seen.append(kw)

    class Dual:
        def parameters(self):
            return []
    real_f, real_t, T.FusedAdam, T.TensorAdam = T.FusedAdam, T.TensorAdam, Spy, Spy
    try:
        base = dict(lr=1e-4, beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.0)
        for extra in (dict(), dict(grad_clip=0.5), dict(skip_nonfinite=True), dict(grad_clip=2.0, skip_nonfinite=True)):
            T.make_optimizer(types.SimpleNamespace(**base, **extra), object())
            T.make_dual_optimizer(types.SimpleNamespace(**base, **extra), [Dual()])
    finally:
        T.FusedAdam, T.TensorAdam = real_f, real_t
    guard = lambda kw: {k: v for k, v in kw.items() if k in ('max_grad_norm', 'skip_nonfinite')}
    want = [{}, {'max_grad_norm': 0.5}, {'skip_nonfinite': True}, {'max_grad_norm': 2.0, 'skip_nonfinite': True}]
    assert [guard(kw) for kw in seen[0::2]] == want and [guard(kw) for kw in seen[1::2]] == want


def test_optimizer_signatures():
    from srad_amd.train import FusedAdam, TensorAdam
    for cls in (FusedAdam, TensorAdam):
        sig = inspect.signature(cls.__init__).parameters
        assert sig['max_grad_norm'].default is None and sig['skip_nonfinite'].default is False
        assert hasattr(cls, 'guard_stats')
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            TensorAdam([], max_grad_norm=bad)
        with pytest.raises(ValueError):
            FusedAdam(object(), max_grad_norm=bad)


# ---------------------------------------------------------------- C entry points: every refusal comes before a launch
NAMES = ("srad_grad_guard_workspace", "srad_grad_guard_partials", "srad_grad_guard_finalize", "srad_adam_guarded_step",
         "srad_adam_ema_guarded_step")


def test_symbols_are_declared_bound_and_exported():
    from srad_amd import _lib as L
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "srad.h")).read()
    for name in NAMES:
        assert name + "(" in header and name in L.exported_symbols() and hasattr(L.lib(), name), name


def test_workspace_size_follows_the_adam_grid():
    from srad_amd import _lib as L
    lib = L.lib()
    s, b = C.c_int(), C.c_size_t()
    for n, slots in ((1, 1), (255, 1), (256, 1), (257, 2), (4096 * 256, 4096), (4096 * 256 + 257, 4096), (1 << 33, 4096)):
        assert lib.srad_grad_guard_workspace(n, C.byref(s), C.byref(b)) == 0
        assert (s.value, b.value) == (slots, 64 + 8 * slots), n
    assert lib.srad_grad_guard_workspace(5, None, C.byref(b)) == 0 and b.value == 72
    for n in (0, -3):
        assert lib.srad_grad_guard_workspace(n, C.byref(s), C.byref(b)) == SRAD_ERR_ARG
    assert lib.srad_grad_guard_workspace(5, None, None) == SRAD_ERR_ARG


def test_argument_errors_without_gpu():
    from srad_amd import _lib as L
    lib = L.lib()
    n = 1000                                                   # 4 slots: the workspace needs 64 + 32 bytes
    p, g, m, v, ema, hyper, ws = (C.c_void_p(k << 20) for k in (1, 2, 3, 4, 5, 6, 7))     # never dereferenced
    err = lambda: lib.srad_last_error()

    def partials(g=g, n=n, ws=ws, nbytes=96, first=0):
        return lib.srad_grad_guard_partials(g, n, ws, nbytes, first, None)

    def finalize(ws=ws, nbytes=96, slots=4, hyper=hyper, max_norm=1.0):
        return lib.srad_grad_guard_finalize(ws, nbytes, slots, hyper, 0.9, 0.999, max_norm, None)

    def plain(p=p, g=g, m=m, v=v, n=n, ws=ws):
        return lib.srad_adam_guarded_step(p, g, m, v, n, 0.9, 0.999, 1e-8, 0.0, ws, None)

    def with_ema(p=p, g=g, m=m, v=v, ema=ema, n=n, ws=ws, decay=0.999):
        return lib.srad_adam_ema_guarded_step(p, g, m, v, ema, n, 0.9, 0.999, 1e-8, 0.0, decay, ws, None)

    # null pointers and n <= 0
    for kw in (dict(g=None), dict(ws=None), dict(n=0), dict(n=-5)):
        assert partials(**kw) == SRAD_ERR_ARG and b"grad_guard_partials: bad argument" in err(), kw
    for kw in (dict(ws=None), dict(hyper=None)):
        assert finalize(**kw) == SRAD_ERR_ARG and b"grad_guard_finalize: bad argument" in err(), kw
    for name, call in (("adam_guarded_step", plain), ("adam_ema_guarded_step", with_ema)):
        for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(ws=None), dict(n=0), dict(n=-5)):
            assert call(**kw) == SRAD_ERR_ARG and f"{name}: bad argument".encode() in err(), (name, kw)
    # max_norm
    for bad in (0.0, -0.0, -1.0, -INF, float("nan")):
        assert finalize(max_norm=bad) == SRAD_ERR_ARG and b"max_norm must be > 0" in err(), bad
    # a workspace smaller than the slots named, a negative slot, no slots, a misaligned workspace
    assert partials(nbytes=95) == SRAD_ERR_ARG and b"workspace too small" in err()
    assert partials(nbytes=96, first=1) == SRAD_ERR_ARG and b"workspace too small" in err()
    assert partials(nbytes=0) == SRAD_ERR_ARG and b"workspace too small" in err()
    assert partials(first=-1) == SRAD_ERR_ARG and b"negative" in err()
    assert finalize(nbytes=95) == SRAD_ERR_ARG and b"workspace too small" in err()
    assert finalize(slots=5) == SRAD_ERR_ARG and b"workspace too small" in err()
    assert finalize(slots=0) == SRAD_ERR_ARG and b"n_slots must be positive" in err()
    odd = C.c_void_p((7 << 20) + 8)
    for call in (partials, finalize, plain, with_ema):
        assert call(ws=odd) == SRAD_ERR_ARG and b"16-byte aligned" in err()
    # the workspace against the buffers the guard itself reads
    assert partials(ws=C.c_void_p((2 << 20) + 4 * n - 16), nbytes=96) == SRAD_ERR_ARG and b"overlaps the gradients" in err()
    assert partials(g=C.c_void_p((7 << 20) + 92)) == SRAD_ERR_ARG and b"overlaps the gradients" in err()
    assert finalize(hyper=C.c_void_p((7 << 20) + 80)) == SRAD_ERR_ARG and b"overlaps dev_hyper" in err()
    # the state and record (the first 64 bytes) against every Adam buffer: one shared float / byte range at either end
    for name, call, bufs in (("adam_guarded_step", plain, (1, 2, 3, 4)), ("adam_ema_guarded_step", with_ema, (1, 2, 3, 4, 5))):
        for base in bufs:
            for off in (0, 4 * n - 16, -48):
                assert call(ws=C.c_void_p((base << 20) + off)) == SRAD_ERR_ARG, (name, base, off)
                assert f"{name}: the guard state overlaps another buffer".encode() in err(), (name, base, off)
    # ... and what the unguarded EMA step refuses
    assert with_ema(ema=None) == SRAD_ERR_ARG and b"adam_ema_guarded_step: null ema" in err()
    for bad in (1.0, -0.1, float("nan")):
        assert with_ema(decay=bad) == SRAD_ERR_ARG and b"ema_decay must be in [0, 1)" in err()
    assert with_ema(ema=p) == SRAD_ERR_ARG and b"ema overlaps another buffer" in err()


# ---------------------------------------------------------------- the fp64 reference the GPU tests reuse
def test_reference_norm_coef_and_counts():
    from srad_amd.train import guard_reference, guard_reference_run
    g = np.array([3.0, -4.0], np.float32)
    norm, coef, apply = guard_reference(g)
    assert (norm, coef, apply) == (5.0, 1.0, True)                                        # max_norm = inf: exactly 1
    norm, coef, apply = guard_reference(g, grad_scale=0.5, max_norm=1.0)
    assert norm == 2.5 and apply and coef == 1.0 / (2.5 + 1e-6)
    assert guard_reference(g, max_norm=5.0)[1] == 5.0 / (5.0 + 1e-6)                       # clip_grad_norm_ clips at the bound itself
    assert guard_reference(g, max_norm=6.0)[1] == 1.0
    assert guard_reference([g[:1], g[1:]])[0] == 5.0                                      # several tensors, one norm
    big = np.full(1000, 3e38, np.float32)                                                 # fp32 squares would overflow: fp64 does not
    norm, coef, apply = guard_reference(big)
    assert apply and math.isclose(norm, 3e38 * math.sqrt(1000.0), rel_tol=1e-6) and coef == 1.0
    assert guard_reference(np.zeros(7, np.float32)) == (0.0, 1.0, True)
    for bad in (np.inf, -np.inf, np.nan):
        for at in (0, 3, 6):
            x = np.ones(7, np.float32)
            x[at] = bad
            norm, coef, apply = guard_reference(x, max_norm=1.0)
            assert not apply and coef is None and not math.isfinite(norm)
    both = np.array([np.inf, np.nan], np.float32)
    assert not guard_reference(both)[2]
    assert guard_reference_run([1.0, INF, 2.0], max_norm=1.5) == (2, 1, 1)
    assert guard_reference_run([1.0, float('nan'), 2.0]) == (2, 1, 0)
    assert guard_reference_run([]) == (0, 0, 0)
