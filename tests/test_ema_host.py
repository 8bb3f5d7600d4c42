"""CPU: the weight EMA's public surface without a GPU (DESIGN.md "Weight EMA") - the ``--ema`` / ``--ema-decay`` flags and
their YAML keys in both parsers, the evaluator's checkpoint choice under ``--ema``, the two C entry points beside
``srad_adam_step`` (exported, and every refusal made before a launch), and ``FusedAdam``'s new keyword."""
import ctypes as C
import inspect
import os
import types

import pytest

SRAD_ERR_ARG = 1
_EVAL_ARGV = ['--run-dir', 'some_run']


# ---------------------------------------------------------------- flags, YAML keys
def test_flag_is_off_by_default_in_both_parsers():
    from srad_amd import options as Opt
    from srad_amd.main import build_train_opt
    t = Opt.parse_train_args([])
    assert t.ema is False and t.ema_decay is None
    assert Opt.parse_train_args(['--ema']).ema is True
    assert Opt.parse_eval_args(_EVAL_ARGV).ema is False
    assert Opt.parse_eval_args(_EVAL_ARGV + ['--ema']).ema is True
    for model_type in ('drct', 'drn-l'):
        off = build_train_opt(Opt.parse_train_args(['--model-type', model_type]))
        assert not getattr(off, 'ema', False)
        assert 'ema' not in vars(off)                          # config.txt lists vars(opt): a run without the flag writes today's file
        on = build_train_opt(Opt.parse_train_args(['--model-type', model_type, '--ema']))
        assert on.ema is True and on.ema_decay == 0.999        # DRCT's field; the DRN option set has none and gets the same default
        on = build_train_opt(Opt.parse_train_args(['--model-type', model_type, '--ema', '--ema-decay', '0.9']))
        assert on.ema is True and on.ema_decay == 0.9
    assert 'ema_decay' not in vars(build_train_opt(Opt.parse_train_args(['--model-type', 'drn-l'])))


def test_yaml_keys_and_decay_parsing(tmp_path):
    from srad_amd import options as Opt
    from srad_amd.main import build_train_opt
    on = tmp_path / 'on.yaml'
    on.write_text("ema: true\nema_decay: 0.95\n")
    a = Opt.parse_train_args(['--config', str(on)])
    assert a.ema is True and a.ema_decay == 0.95
    opt = build_train_opt(a)
    assert opt.ema is True and opt.ema_decay == 0.95
    assert Opt.parse_train_args(['--config', str(on), '--ema-decay', '0.5']).ema_decay == 0.5      # command line wins
    assert Opt.parse_eval_args(_EVAL_ARGV + ['--config', str(on)]).ema is True
    assert Opt.parse_train_args(['--ema-decay', '0']).ema_decay == 0.0
    for bad in ('1', '-0.1', 'nan', '1.5'):
        with pytest.raises(SystemExit):
            Opt.parse_train_args(['--ema', '--ema-decay', bad])
    for bad in ('1.0', '-0.1', '.nan'):                        # a value from a config file gets the same check
        cfg = tmp_path / 'bad.yaml'
        cfg.write_text(f"ema_decay: {bad}\n")
        with pytest.raises(SystemExit):
            Opt.parse_train_args(['--config', str(cfg)])


def test_make_optimizer_passes_the_decay_only_with_the_flag():
    from srad_amd import trainer as T
    seen = []

    class Spy:
        def __init__(self, model, **kw):
            seen.append(kw)
    real, T.FusedAdam = T.FusedAdam, Spy
    try:
        base = dict(lr=1e-4, beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.0)
        T.make_optimizer(types.SimpleNamespace(**base, ema_decay=0.999), object())      # DRCT's option set: the field alone is not the flag
        T.make_optimizer(types.SimpleNamespace(**base, ema=True, ema_decay=0.9), object())
        T.make_optimizer(types.SimpleNamespace(**base, ema=True), object())              # DRN: no field
    finally:
        T.FusedAdam = real
    assert 'ema_decay' not in seen[0]
    assert seen[1]['ema_decay'] == 0.9 and seen[2]['ema_decay'] == 0.999


def test_evaluator_refuses_ema_with_an_explicit_checkpoint(capsys):
    from srad_amd import options as Opt
    with pytest.raises(SystemExit):
        Opt.parse_eval_args(['--ema', '--checkpoint', 'f.pt'])
    assert "--ema and --checkpoint exclude each other" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        Opt.parse_eval_args(['--run-dir', 'r', '--ema', '--checkpoint', 'f.pt'])


# ---------------------------------------------------------------- resolve_checkpoint
def test_resolve_checkpoint(tmp_path):
    from srad_amd.evaluate import resolve_checkpoint
    run = tmp_path / 'run'
    (run / 'model').mkdir(parents=True)

    def args(ema, run_dir=str(run), checkpoint=''):
        return types.SimpleNamespace(ema=ema, run_dir=run_dir, checkpoint=checkpoint)

    def touch(*names):
        for f in os.listdir(run / 'model'):
            os.remove(run / 'model' / f)
        for n in names:
            (run / 'model' / n).write_bytes(b'')

    path = lambda n: os.path.join(str(run), 'model', n)
    touch('model_best.pt', 'model_latest.pt', 'model_ema_best.pt', 'model_ema_latest.pt')
    assert resolve_checkpoint(args(True)) == path('model_ema_best.pt')                  # best before latest
    assert resolve_checkpoint(args(False)) == path('model_best.pt')                     # the raw files when the flag is absent
    touch('model_best.pt', 'model_latest.pt', 'model_ema_latest.pt')
    assert resolve_checkpoint(args(True)) == path('model_ema_latest.pt')
    assert resolve_checkpoint(args(False)) == path('model_best.pt')
    touch('model_latest.pt', 'model_ema_best.pt', 'model_ema_latest.pt')
    assert resolve_checkpoint(args(False)) == path('model_latest.pt')
    touch('model_ema_best.pt', 'model_ema_latest.pt')                                   # the EMA files only under --ema
    with pytest.raises(FileNotFoundError):
        resolve_checkpoint(args(False))
    touch('model_best.pt', 'model_latest.pt')                                           # no silent fall-back to the raw weights
    for a in (args(True), args(True, run_dir='')):
        with pytest.raises(FileNotFoundError) as e:
            resolve_checkpoint(a)
        assert 'model_ema_best.pt' in str(e.value) and 'model_ema_latest.pt' in str(e.value)
    assert resolve_checkpoint(args(False, checkpoint='f.pt')) == 'f.pt'
    assert resolve_checkpoint(types.SimpleNamespace(run_dir=str(run), checkpoint='')) == path('model_best.pt')   # an older namespace


# ---------------------------------------------------------------- C entry points: every refusal comes before a launch
def test_symbols_are_declared_bound_and_exported():
    from srad_amd import _lib as L
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "srad.h")).read()
    for name in ("srad_adam_ema_step", "srad_adam_ema_step_dev"):
        assert name + "(" in header and name in L.exported_symbols() and hasattr(L.lib(), name), name


def test_argument_errors_without_gpu():
    from srad_amd import _lib as L
    lib = L.lib()
    n = 1000
    p, g, m, v, ema, hyper = (C.c_void_p(k << 20) for k in (1, 2, 3, 4, 5, 6))     # never dereferenced: every call below fails in the checks
    err = lambda: lib.srad_last_error()

    def host(p=p, g=g, m=m, v=v, ema=ema, n=n, step=1, decay=0.999):
        return lib.srad_adam_ema_step(p, g, m, v, ema, n, 1e-4, 0.9, 0.999, 1e-8, 0.0, step, 1.0, decay, None)

    def dev(p=p, g=g, m=m, v=v, ema=ema, n=n, decay=0.999, hyper=hyper):
        return lib.srad_adam_ema_step_dev(p, g, m, v, ema, n, 0.9, 0.999, 1e-8, 0.0, decay, hyper, None)

    for name, call in (("adam_ema_step", host), ("adam_ema_step_dev", dev)):
        assert call(ema=None) == SRAD_ERR_ARG and f"{name}: null ema".encode() in err(), name
        for bad in (1.0, 1.5, -0.1, -1e-30, float("nan"), float("inf")):
            assert call(decay=bad) == SRAD_ERR_ARG and f"{name}: ema_decay must be in [0, 1)".encode() in err(), (name, bad)
        # one shared float at either end of each of the four other buffers
        for other, base in (("params", 1), ("grads", 2), ("exp_avg", 3), ("exp_avg_sq", 4)):
            for off in (0, 4 * (n - 1), -4 * (n - 1)):
                assert call(ema=C.c_void_p((base << 20) + off)) == SRAD_ERR_ARG, (name, other, off)
                assert f"{name}: ema overlaps another buffer".encode() in err(), (name, other, off)
        # the existing refusals
        for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=0), dict(n=-5)):
            assert call(**kw) == SRAD_ERR_ARG and f"{name}: bad argument".encode() in err(), (name, kw)
    assert host(step=0) == SRAD_ERR_ARG and b"step counts from 1" in err()
    assert dev(hyper=None) == SRAD_ERR_ARG and b"adam_ema_step_dev: bad argument" in err()


# ---------------------------------------------------------------- the Python keyword
def test_fused_adam_signature_default():
    from srad_amd.train import FusedAdam, TensorAdam
    assert inspect.signature(FusedAdam.__init__).parameters['ema_decay'].default is None
    assert 'ema_decay' not in inspect.signature(TensorAdam.__init__).parameters      # the dual models keep no average
