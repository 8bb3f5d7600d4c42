"""CPU: the self-ensemble's public surface without a GPU - the ``--self-ensemble`` flag and its YAML key, the new keyword of
the evaluator's functions, the argument checks of the two C entry points - and the member table of DESIGN.md
"Self-ensemble" restated in torch (``members`` / ``back_mean``, the oracle of tests/test_gpu_self_ensemble.py) against a
literal index loop."""
import ctypes as C
import inspect

import torch

SRAD_ERR_ARG = 1


# ---------------------------------------------------------------- DESIGN.md "Self-ensemble" in torch
def transform(x: torch.Tensor, t: int) -> torch.Tensor:
    """Member t of x [..., H, W]: T^(t>>2 & 1)( h^(t>>1 & 1)( v^(t & 1)(x) ) ); v flips W, h flips H, T swaps H and W."""
    if t & 1:
        x = x.flip(-1)
    if t & 2:
        x = x.flip(-2)
    if t & 4:
        x = x.transpose(-1, -2)
    return x.contiguous()


def members(x: torch.Tensor) -> list:
    return [transform(x, t) for t in range(8)]


def back(y: torch.Tensor, t: int) -> torch.Tensor:
    """z_t = v^(t & 1)( h^(t>>1 & 1)( T^(t>>2 & 1)(y_t) ) )."""
    if t & 4:
        y = y.transpose(-1, -2)
    if t & 2:
        y = y.flip(-2)
    if t & 1:
        y = y.flip(-1)
    return y.contiguous()


def back_mean(ys) -> torch.Tensor:
    """(((z_0 + z_1) + z_2) + ... + z_7) * 0.125 of the eight member outputs: an explicit loop of seven fp32 additions."""
    acc = back(ys[0], 0)
    for t in range(1, 8):
        acc = acc + back(ys[t], t)
    return acc * 0.125


def test_member_table_against_an_index_loop():
    H, W = 3, 4
    x = torch.arange(H * W, dtype=torch.float32).reshape(1, 1, H, W)
    ms = members(x)
    # the list forward_x8 builds: for tf in 'v', 'h', 't': lst += [tf(e) for e in lst]
    lst = [x]
    for tf in (lambda e: e.flip(-1), lambda e: e.flip(-2), lambda e: e.transpose(-1, -2)):
        lst = lst + [tf(e) for e in lst]
    for t in range(8):
        assert torch.equal(ms[t], lst[t].contiguous()), t
    for t in range(8):
        fw, fh, tr = t & 1, (t >> 1) & 1, (t >> 2) & 1
        assert tuple(ms[t].shape) == ((1, 1, W, H) if tr else (1, 1, H, W))
        for r in range(H):
            for c in range(W):
                rr, cc = (H - 1 - r if fh else r), (W - 1 - c if fw else c)      # where x[r][c] lands in h(v(x)) ...
                i, j = (cc, rr) if tr else (rr, cc)                               # ... and after the swap
                assert float(ms[t][0, 0, i, j]) == float(x[0, 0, r, c]), (t, r, c)
    # the back-transform undoes each member, and its order matters: on members 5 and 6 the swapped order is another image
    for t in range(8):
        assert torch.equal(back(ms[t], t), x), t
    assert not torch.equal(transform(ms[5], 5), x) and not torch.equal(transform(ms[6], 6), x)
    # eight independent outputs: out[r][c] sums y_t at the position x[r][c] went to, in member order
    g = torch.Generator().manual_seed(5)
    ys = [torch.randn(ms[t].shape, generator=g) for t in range(8)]
    out = back_mean(ys)
    for r in range(H):
        for c in range(W):
            acc = None
            for t in range(8):
                rr, cc = (H - 1 - r if t & 2 else r), (W - 1 - c if t & 1 else c)
                v = ys[t][0, 0, cc, rr] if t & 4 else ys[t][0, 0, rr, cc]
                acc = v if acc is None else acc + v
            assert float(out[0, 0, r, c]) == float(acc * 0.125), (r, c)
    small = torch.randint(-8, 9, (2, 3, 5, 7)).float()
    assert torch.equal(back_mean(members(small)), small)                           # eight equal values sum exactly


# ---------------------------------------------------------------- flag, YAML key, keyword
_EVAL_ARGV = ['--checkpoint', 'x.pt']


def test_flag_parses_and_defaults_to_false(tmp_path):
    from srad_amd import options as Opt
    assert Opt.parse_eval_args(_EVAL_ARGV).self_ensemble is False
    assert Opt.parse_eval_args(_EVAL_ARGV + ['--self-ensemble']).self_ensemble is True
    on, off = tmp_path / 'on.yaml', tmp_path / 'off.yaml'
    on.write_text("self_ensemble: true\n")
    off.write_text("self_ensemble: false\n")
    assert Opt.parse_eval_args(_EVAL_ARGV + ['--config', str(on)]).self_ensemble is True
    assert Opt.parse_eval_args(_EVAL_ARGV + ['--config', str(off)]).self_ensemble is False
    assert Opt.parse_eval_args(_EVAL_ARGV + ['--config', str(off), '--self-ensemble']).self_ensemble is True   # command line wins
    # main.py's parser and the option object Trainer.test reads
    assert Opt.parse_train_args([]).self_ensemble is False
    assert Opt.parse_train_args(['--self-ensemble']).self_ensemble is True
    assert Opt.parse_train_args(['--config', str(on)]).self_ensemble is True
    from srad_amd.main import build_train_opt
    for model_type in ('drct', 'drn-l'):
        assert build_train_opt(Opt.parse_train_args(['--model-type', model_type])).self_ensemble is False
        assert build_train_opt(Opt.parse_train_args(['--model-type', model_type, '--self-ensemble'])).self_ensemble is True
    assert Opt.DRN().self_ensemble is False and Opt.DRCT().self_ensemble is False and Opt.build_opt('drct', 'grid', 64, 4).self_ensemble is False


def test_evaluator_functions_take_the_keyword():
    from srad_amd import evaluate as E
    from srad_amd.model import Model
    for fn in (E.evaluate_on_test, E.super_resolve_u8):
        p = inspect.signature(fn).parameters['self_ensemble']
        assert p.default is False, fn.__name__
    assert callable(Model.forward_x8)


# ---------------------------------------------------------------- C entry points: every refusal comes before a launch
def test_argument_errors_without_gpu():
    from srad_amd import _lib as L
    lib = L.lib()
    x, a, b, out = (C.c_void_p(v << 20) for v in (1, 2, 3, 4))          # never dereferenced: every call below fails in the checks

    def inputs(x=x, B=2, Cc=1, H=5, W=7, a=a, b=b):
        return lib.srad_ensemble_inputs(x, B, Cc, H, W, a, b, None)

    def mean(a=a, b=b, B=2, Cc=1, H=5, W=7, out=out):
        return lib.srad_ensemble_mean(a, b, B, Cc, H, W, out, None)

    for name, call, ptrs in (("ensemble_inputs", inputs, ("x", "a", "b")), ("ensemble_mean", mean, ("a", "b", "out"))):
        for p in ptrs:
            assert call(**{p: None}) == SRAD_ERR_ARG and f"{name}: null argument".encode() in lib.srad_last_error(), (name, p)
        for dim in ("B", "Cc", "H", "W"):
            for bad in (0, -3):
                assert call(**{dim: bad}) == SRAD_ERR_ARG, (name, dim, bad)
                assert f"{name}: sizes must be positive".encode() in lib.srad_last_error(), (name, dim, bad)
        # B*C*H*W*8 < 2^31: 2^28 elements is the first size over it, whichever dimension carries it
        for shape in ((1, 1, 1 << 14, 1 << 14), (1 << 28, 1, 1, 1), (1, 1, 1, 1 << 28), (1 << 16, 1 << 16, 1 << 16, 1 << 16),
                      (2, 1, (1 << 31) - 1, 1)):
            assert call(**dict(zip(("B", "Cc", "H", "W"), shape))) == SRAD_ERR_ARG, (name, shape)
            assert b"does not fit 32-bit offsets" in lib.srad_last_error(), (name, shape)
    n = 2 * 1 * 5 * 7 * 4                                                # bytes of x / out; a and b are 4 n each
    base = 1 << 20
    at = lambda off: C.c_void_p(base + off)
    for kw in (dict(x=at(0), a=at(n - 4)), dict(x=at(4 * n - 4), a=at(0)), dict(x=at(0), b=at(n - 4)), dict(x=at(4 * n - 4), b=at(0)),
               dict(a=at(0), b=at(4 * n - 4)), dict(a=at(4), b=at(0))):
        assert inputs(**kw) == SRAD_ERR_ARG and b"ensemble_inputs: the outputs overlap" in lib.srad_last_error(), kw
    for kw in (dict(out=at(0), a=at(n - 4)), dict(out=at(4 * n - 4), a=at(0)), dict(out=at(0), b=at(n - 4)), dict(out=at(4 * n - 4), b=at(0)),
               dict(out=at(0), a=at(0), b=at(4 * n))):                    # the last: a square stack with out on its first member
        assert mean(**kw) == SRAD_ERR_ARG and b"ensemble_mean: out overlaps an input" in lib.srad_last_error(), kw
