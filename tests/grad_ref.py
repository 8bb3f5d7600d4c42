"""CPU only: a bf16-rounding restatement of the oracle's GEMMs, and the per-tensor gradient checker built on it.

``bf16_matmuls()`` swaps the name ``F`` inside ``oracle.sr_ref`` for an object whose ``linear`` and ``conv2d`` round to bf16
exactly the operands a bf16 MFMA GEMM rounds (forward: x and w; data gradient: dy and w; weight gradient: dy and x), with fp32
accumulation, an fp32 bias and an fp32 bias gradient from the unrounded dy.  Everything else of the oracle runs as it is, so the
distance between such a run and the plain one is what bf16 operands alone cost each gradient tensor: the yardstick
``per_tensor_report`` holds the engine's bf16 mode to ("bf16 gradients, tensor by tensor").
``oracle/sr_ref.py`` is not edited."""
import contextlib
import re

import numpy as np
import torch
import torch.nn.functional as F

from oracle import sr_ref as R

BAR_FACTOR = 4.0      # engine error allowed per tensor, in units of the emulation's own error (DESIGN.md derives the 4)
BAR_CAP = 0.5         # relative L2: a wrong sign, a missing term of equal size, a factor 2, a transposed square matrix all exceed it
LEFT_OUT_COS = 0.5    # a tensor whose bar would pass the cap is left out of the bar, but still held to this cosine


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype)      # round to nearest even


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, rnd):
        xr, wr = rnd(x), rnd(w)
        ctx.save_for_backward(xr, wr)
        ctx.rnd, ctx.has_bias = rnd, b is not None
        return F.linear(xr, wr, b)

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        dyr = ctx.rnd(dy)
        n, k = wr.shape
        dx = dyr @ wr
        dw = dyr.reshape(-1, n).t() @ xr.reshape(-1, k)
        db = dy.reshape(-1, n).sum(0) if ctx.has_bias else None
        return dx, dw, db, None


class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, padding, rnd):
        if x.shape[-2:] == (1, 1):       # the channel-attention squeeze / excite: fp32 FMAs in the engine, not an MFMA GEMM
            rnd = _identity
        xr, wr = rnd(x), rnd(w)
        ctx.save_for_backward(xr, wr)
        ctx.rnd, ctx.has_bias, ctx.stride, ctx.padding = rnd, b is not None, stride, padding
        return F.conv2d(xr, wr, b, stride=stride, padding=padding)

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        dyr = ctx.rnd(dy)
        dx, dw, _ = _conv_backward(dyr, xr, wr, ctx.stride, ctx.padding, [True, True, False])
        db = _conv_backward(dy, xr, wr, ctx.stride, ctx.padding, [False, False, True])[2] if ctx.has_bias else None
        return dx, dw, db, None, None, None


def _conv_backward(dy, x, w, stride, padding, which):
    """(conv2d_input, conv2d_weight, dy.sum((0, 2, 3))) of torch.nn.grad for the asked ones, from the one routine those go to, in
    one call.  Called so, the fp32 sums run in the order of torch's own convolution backward; two calls, or a plain sum for the
    bias, are another order of the same sums - 1e-6 away on a small tensor far upstream (a relative-position table), which is
    the whole tolerance of the identity test."""
    pair = lambda v: [v, v] if isinstance(v, int) else list(v)
    return torch.ops.aten.convolution_backward(dy, x, w, [w.shape[0]], pair(stride), pair(padding), [1, 1], False, [0, 0], 1, which)


def _identity(t):
    return t


class _RoundedF:
    """torch.nn.functional, except ``linear`` and ``conv2d`` (the two calls every GEMM of the oracle goes through)."""

    def __init__(self, rnd):
        self._rnd = rnd

    def __getattr__(self, name):
        return getattr(F, name)

    def linear(self, x, w, bias=None):
        return _Linear.apply(x, w, bias, self._rnd)

    def conv2d(self, x, w, bias=None, stride=1, padding=0):
        return _Conv2d.apply(x, w, bias, stride, padding, self._rnd)


@contextlib.contextmanager
def bf16_matmuls(rnd=bf16_round):
    """For the duration, ``oracle.sr_ref.F`` rounds GEMM operands with ``rnd`` (the identity: a test of the backward formulas)."""
    before = R.F
    R.F = _RoundedF(rnd)
    try:
        yield
    finally:
        R.F = before


# ------------------------------------------------------------------ oracle runs
def leaf_state(sd):
    """A state dict (numpy or torch values) as fresh autograd leaves; integer buffers stay as they are."""
    out = {}
    for k, v in sd.items():
        t = torch.from_numpy(np.asarray(v)).clone() if not isinstance(v, torch.Tensor) else v.detach().clone()
        out[k] = t.requires_grad_(t.dtype == torch.float32)
    return out


def oracle_grads(forward, sd, x, emulate, rnd=bf16_round):
    """One oracle forward + backward.  ``sd``: a state dict, or {prefix: state dict} for a model with satellites (DRN and its
    dual models: {"": drn, "dual0.": ..}); ``forward(leaves, x_leaf) -> (output tensor or list of them, scalar loss)`` gets the
    leaves in the same form.  Returns (outputs, loss, dx, {prefix + name: grad}), all detached.  A float entry of the state that
    the oracle never reads (the attn_mask buffers: it computes its own) has no gradient and is not listed; the callers look every
    parameter of the engine up by name."""
    nested = all(isinstance(v, dict) for v in sd.values())
    leaves = {p: leaf_state(s) for p, s in sd.items()} if nested else leaf_state(sd)
    xr = torch.from_numpy(np.asarray(x)).clone().requires_grad_(True)
    with (bf16_matmuls(rnd) if emulate else contextlib.nullcontext()):
        out, loss = forward(leaves, xr)
        loss.backward()
    grads = {}
    for p, s in (leaves.items() if nested else [("", leaves)]):
        for k, t in s.items():
            if t.grad is not None:
                grads[p + k] = t.grad.detach()
    out = [o.detach() for o in out] if isinstance(out, (list, tuple)) else out.detach()
    return out, float(loss.detach()), None if xr.grad is None else xr.grad.detach(), grads


def drct_l1(cfg, hr, keeps=None):
    """``forward`` of ``oracle_grads`` for DRCT under nn.L1Loss against ``hr``; ``keeps`` as ``R.drct_forward`` takes them."""
    hr = torch.from_numpy(np.asarray(hr))

    def forward(sdt, xr):
        out = R.drct_forward(sdt, xr, cfg, keeps=keeps)
        return out, F.l1_loss(out, hr)
    return forward


def drn_composite(cfg, lrs, hr):
    """``forward`` of ``oracle_grads`` for DRN-L with its dual models under the reference's composite loss; the leaves are
    {"": drn state, "dual0.": .., ..}, ``lrs`` the LR pyramid coarse to fine (lrs[0] is the input)."""
    lrs = [torch.from_numpy(np.asarray(a)) for a in lrs]
    hr = torch.from_numpy(np.asarray(hr))

    def forward(leaves, xr):
        sr = R.drn_forward(leaves[""], xr, cfg)
        sr2lr = [R.dual_forward(leaves[f"dual{i}."], sr[i - cfg.phase], cfg) for i in range(cfg.phase)]
        return sr, R.drn_total_loss(sr, lrs, hr, sr2lr)
    return forward


def keeps_of(keep, n_rdg):
    """[2 * n_rdg * 5, B] DropPath factors (the engine's ``keep_scale_override`` layout) as ``R.drct_forward``'s ``keeps``."""
    return [[(keep[2 * (i * 5 + k)], keep[2 * (i * 5 + k) + 1]) for k in range(5)] for i in range(n_rdg)]


def as_tensors(out, dx, grads):
    """One dict for the checker: the parameter gradients plus the output(s) and dx as further tensors."""
    d = dict(grads)
    for i, o in enumerate(out if isinstance(out, (list, tuple)) else [out]):
        d[f"<out{i}>"] = o
    if dx is not None:
        d["<dx>"] = dx
    return d


# ------------------------------------------------------------------ the checker
def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def per_tensor_report(engine, exact, emulated_list):
    """{name: dict(e_eng, e_emu, bar, cos, left_out, finite)} over the tensors of ``exact``.
    ``emulated_list``: [(emulated, exact of the same inputs)] - the emulated runs differ in the seed of the input and target
    images, and each is measured against the plain oracle on ITS images (the first pair may share ``exact``).
    e_emu = max over the pairs of |emulated - exact| / |exact|, bar = BAR_FACTOR * e_emu; a bar above BAR_CAP leaves the tensor
    out (the reference itself is ill-conditioned there)."""
    rep = {}
    for name, ex in exact.items():
        eng = engine[name]
        assert tuple(eng.shape) == tuple(ex.shape), (name, tuple(eng.shape), tuple(ex.shape))
        e_emu = max(_rel_l2(emu[name], own[name]) for emu, own in emulated_list)
        a, b = eng.detach().double().cpu().reshape(-1), ex.detach().double().reshape(-1)
        finite = bool(torch.isfinite(a).all())
        cos = float((a * b).sum() / (a.norm() * b.norm()).clamp_min(1e-300)) if finite else float("nan")
        bar = BAR_FACTOR * e_emu
        rep[name] = dict(e_eng=_rel_l2(eng, ex) if finite else float("inf"), e_emu=e_emu, bar=min(bar, BAR_CAP), cos=cos,
                         left_out=bar > BAR_CAP, finite=finite)
    return rep


def failures(report):
    """Names of the tensors that miss their bar (or, left out of it, are not finite or have a cosine <= LEFT_OUT_COS)."""
    bad = []
    for name, r in report.items():
        ok = r["finite"] and (r["cos"] > LEFT_OUT_COS if r["left_out"] else r["e_eng"] <= r["bar"])
        if not ok:
            bad.append(name)
    return bad


def left_out(report):
    return [n for n, r in report.items() if r["left_out"]]


def tensor_class(name):
    """layers.0.swin3.attn.qkv.weight -> swin.attn.qkv.weight; up_blocks.1.0.body.2.bias -> up_blocks.body.#.bias (the
    position inside a Sequential stays: it tells the layers of one block apart)."""
    name = re.sub(r"^layers\.\d+\.", "", name)
    name = re.sub(r"^(swin|adjust)\d+", r"\1", name)
    name = re.sub(r"^(up_blocks|down|dual)\.?\d+\.(\d+\.)?", r"\1.", name)
    return name


def class_lines(report):
    """One line per tensor class: the worst e_eng / e_emu of the class and the tensor that has it."""
    worst = {}
    for name, r in report.items():
        ratio = r["e_eng"] / max(r["e_emu"], 1e-300)
        c = tensor_class(name)
        if c not in worst or ratio > worst[c][0]:
            worst[c] = (ratio, name, r)
    return [f"  {c:44s} e_eng / e_emu {ratio:6.2f}  ({name}: e_eng {r['e_eng']:.3e}, e_emu {r['e_emu']:.3e}, bar {r['bar']:.3e}"
            f"{', LEFT OUT' if r['left_out'] else ''})" for c, (ratio, name, r) in sorted(worst.items())]


def assert_report(report, max_left_out_frac, label=""):
    """Every tensor within min(BAR_FACTOR * e_emu, BAR_CAP); at most ``max_left_out_frac`` of the tensors left out."""
    print(f"{label}: {len(report)} tensors, worst e_eng / e_emu per class")
    for line in class_lines(report):
        print(line)
    out = left_out(report)
    for n in out:
        print(f"  left out of the bar: {n} (e_emu {report[n]['e_emu']:.3e}; engine e_eng {report[n]['e_eng']:.3e}, cosine {report[n]['cos']:.4f})")
    assert len(out) <= max_left_out_frac * len(report), \
        (label, "left out of the bar", [(n, report[n]["e_emu"]) for n in out])
    bad = failures(report)
    assert not bad, (label, [(n, {k: report[n][k] for k in ("e_eng", "e_emu", "bar", "cos")}) for n in bad])
