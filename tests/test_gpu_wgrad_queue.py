"""GPU: the split-K gradient queue (WgradQueue) under pressure.  Every weight gradient, LayerNorm dgamma / dbeta and attention
bias-table gradient of a backward pass reserves workspace from one queue and is summed by wgrad_reduce_kernel; when the batch
(12 items) or the workspace is full the queue flushes itself in the middle of the pass.  The operator tests give every op a
fresh queue and 256 MiB, so they never reach that flush.  Here scripts of the engines' calls run through ONE queue
(srad_op_wgrad_queue_script) with a workspace budget chosen from the needs the code computes, so that the flush lands at the
reservation the case names; the reported flush reasons are asserted, so a case cannot silently exercise another path.

Every case that succeeds is held to two things:
 1. every output is bit-identical to the same script with the whole workspace (split counts depend on the shape alone and
    each item is summed in a fixed order: only the flush positions differ);
 2. every output matches a float64 torch reference of its operation within the bar tests/test_gpu_bwd_ops.py applies to that
    operation and precision.
All outputs start from non-zero values (the reduce does +=)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EXPLICIT, BATCH, WS = 0, 1, 2
WG_TS = 64 * 64 + 64                 # floats of one partial tile (kernels_wgrad.hip)

# operand shapes of the small cases of tests/test_gpu_bwd_ops.py
LINEAR = {"linA": (77, 308, 180), "linB": (1000, 212, 32), "linC": (4096, 180, 540)}          # M, K, N
LAYERNORM = {"lnA": (37, 64), "lnB": (1000, 308)}                                             # rows, C
ATTN = {"att8": dict(ws=8, shift=4, B=1, H=8, W=24, d=48, heads=2), "att4": dict(ws=4, shift=2, B=2, H=8, W=12, d=180, heads=6)}
CONV = dict(B=1, H=64, W=128, C=16)  # the smallest shape the nine-tap kernel takes (8192 pixels, W % 32 == 0); bf16 mode


def cdiv(a, b):
    return (a + b - 1) // b


# ---- workspace needs in floats, as the launchers compute them -------------------------------------------------------------
def tiled_need(M, N, Cin, prec, ntaps=1, wg_target=512):
    """plan_wgrad: 64 x 64 tiles x split count; 0 when the layer is not split (no partials, no reduce item)."""
    tiles = cdiv(N, 64) * cdiv(Cin, 64) * ntaps
    kr = 32 if prec == "bf16" else 4
    kmax = cdiv(M, 8 * kr)
    target = min(cdiv(wg_target, tiles), kmax)
    ks = 1
    while ks * 2 <= kmax and ks * 10 <= target * 7:
        ks *= 2
    rows_per = cdiv(cdiv(M, ks), 4 * kr) * 4 * kr
    ks = cdiv(M, rows_per)
    return tiles * ks * WG_TS if ks > 1 else 0


def linear_need(name, prec, deferred=False):
    M, K, N = LINEAR[name]
    return tiled_need(M, N, K, prec, wg_target=144 if deferred else 512)


def ln_need(name):
    return cdiv(LAYERNORM[name][0], 16) * 640            # one row [dgamma 320 | dbeta 320] per 16-row workgroup


def attn_need(name):
    a = ATTN[name]
    return a["B"] * (a["H"] // a["ws"]) * (a["W"] // a["ws"]) * (2 * a["ws"] - 1) ** 2 * a["heads"]   # one table row per window


def conv_need(prec):
    B, H, W, Cc = CONV["B"], CONV["H"], CONV["W"], CONV["C"]
    if prec != "bf16":
        return tiled_need(B * H * W, Cc, Cc, prec, ntaps=9)
    nchunks = B * cdiv(H, 4) * (W // 32)                   # launch_wgrad_conv9
    ks = max(1, min(int(4.0 * math.sqrt(nchunks) + 0.5), 256, nchunks))
    ks = cdiv(nchunks, cdiv(nchunks, ks))
    return 9 * ks * (Cc * Cc + Cc)


def need_of(op, prec):
    kind = op.rstrip("'")
    if kind.startswith("defer:"):
        return linear_need(kind[6:], prec, deferred=True)
    if kind in LINEAR:
        return linear_need(kind, prec)
    if kind in LAYERNORM:
        return ln_need(kind)
    if kind in ATTN:
        return attn_need(kind)
    assert kind == "conv"
    return conv_need(prec)


def items_of(op, prec):
    kind = op.rstrip("'")
    if kind in LAYERNORM:
        return 2
    return 1 if need_of(op, prec) > 0 else 0


# ---- operands and float64 references, built once ---------------------------------------------------------------------------
def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def bank():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from oracle import sr_ref as R
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(20)
    bank = {}
    for name, (M, K, N) in LINEAR.items():
        x = torch.randn(M, K + 8, generator=g)[:, :K]
        dy = torch.randn(M, N + 4, generator=g)[:, :N]
        bank[name] = dict(x=x.to(dev), dy=dy.to(dev), dw=dy.double().t() @ x.double(), db=dy.double().sum(0),
                          dw0=torch.randn(N, K, generator=g), db0=torch.randn(N, generator=g))
    for name, (rows, Cc) in LAYERNORM.items():
        x = (torch.randn(rows, Cc + 4, generator=g) * 2 + 0.3)[:, :Cc].double().clone().requires_grad_(True)
        gam = torch.randn(Cc, generator=g).double().requires_grad_(True)
        bet = torch.randn(Cc, generator=g).double().requires_grad_(True)
        dy, dres, prev = (torch.randn(rows, Cc, generator=g) for _ in range(3))
        F.layer_norm(x, (Cc,), gam, bet, 1e-5).backward(dy.double())
        xd = torch.zeros(rows, Cc + 4, device=dev)
        xd[:, :Cc] = x.detach().float().to(dev)
        bank[name] = dict(x=xd[:, :Cc], dxn=dy.to(dev), gamma=gam.detach().float().to(dev), dres=dres.to(dev), out0=prev,
                          out=x.grad + dres.double() + prev.double(), dg=gam.grad, db=bet.grad,
                          dg0=torch.randn(Cc, generator=g), db0=torch.randn(Cc, generator=g))
    for name, a in ATTN.items():
        ws, shift, B, H, W, d, heads = (a[k] for k in ("ws", "shift", "B", "H", "W", "d", "heads"))
        T, n, hd = B * H * W, ws * ws, d // heads
        qkv = (torch.randn(T, 3 * d, generator=g) * 0.7).double().requires_grad_(True)
        table = (torch.randn((2 * ws - 1) ** 2, heads, generator=g) * 0.5).double().requires_grad_(True)
        dout = torch.randn(T, d, generator=g)
        x = torch.roll(qkv.view(B, H, W, 3 * d), shifts=(-shift, -shift), dims=(1, 2))
        xw = R.window_partition(x, ws).view(-1, n, 3, heads, hd).permute(2, 0, 3, 1, 4)
        o = R.attention_from_qkv(xw[0] * hd ** -0.5, xw[1], xw[2], table, ws, R.calculate_mask(H, W, ws, shift).double())
        o = R.window_reverse(o.transpose(1, 2).reshape(-1, ws, ws, d), ws, H, W)
        torch.roll(o, shifts=(shift, shift), dims=(1, 2)).reshape(T, d).backward(dout.double())
        from srad_amd import ops
        bank[name] = dict(qkv=ops.pad_heads(qkv.detach().float().to(dev), heads), dout=dout.to(dev), table=table.detach().float().to(dev),
                          dqkv=qkv.grad, dtable=table.grad, dtable0=torch.randn((2 * ws - 1) ** 2, heads, generator=g) * 0.1)
    B, H, W, Cc = CONV["B"], CONV["H"], CONV["W"], CONV["C"]
    x = torch.randn(B, Cc, H, W, generator=g).double()
    w = torch.randn(Cc, Cc, 3, 3, generator=g).double().requires_grad_(True)
    b = torch.zeros(Cc).double().requires_grad_(True)
    y = F.conv2d(x, w, b, padding=1)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.double())
    bank["conv"] = dict(x=x.float().permute(0, 2, 3, 1).reshape(-1, Cc).contiguous().to(dev),
                        dy=dy.permute(0, 2, 3, 1).reshape(-1, Cc).contiguous().to(dev), dw=w.grad.reshape(Cc, Cc, 9), db=b.grad,
                        dw0=torch.randn(Cc, Cc, 9, generator=g), db0=torch.randn(Cc, generator=g))
    return bank


ALPHA = 0.5      # of every Linear / conv weight gradient


def build(bank, script):
    """script: op names - 'linA' (immediate), 'defer:linA', 'lnA', 'att8', 'conv', 'launch', 'flush'; a trailing ' makes a second
    instance with outputs of its own.  Returns (steps for ops.wgrad_queue_script, {instance: {output name: tensor}})."""
    from srad_amd import ops
    dev = torch.device("cuda:0")
    steps, outs = [], {}
    for op in script:
        if op == "launch":
            steps.append(ops.wq_launch_deferred())
            continue
        if op == "flush":
            steps.append(ops.wq_flush())
            continue
        assert op not in outs, op
        kind = op.rstrip("'")
        e = bank[kind[6:] if kind.startswith("defer:") else kind]
        if kind.startswith("defer:"):
            o = dict(dw=e["dw0"].to(dev), db=e["db0"].to(dev))
            steps.append(ops.wq_wgrad_deferred(e["dy"], e["x"], o["dw"], o["db"], alpha=ALPHA))
        elif kind in LINEAR:
            o = dict(dw=e["dw0"].to(dev).unsqueeze(2).contiguous(), db=e["db0"].to(dev))
            steps.append(ops.wq_wgrad(e["dy"], e["x"], o["dw"], o["db"], alpha=ALPHA))
        elif kind == "conv":
            o = dict(dw=e["dw0"].to(dev), db=e["db0"].to(dev))
            steps.append(ops.wq_wgrad(e["dy"], e["x"], o["dw"], o["db"], ntaps=9, alpha=ALPHA, **{k: CONV[k] for k in "BHW"}))
        elif kind in LAYERNORM:
            o = dict(out=e["out0"].to(dev), dg=e["dg0"].to(dev), db=e["db0"].to(dev))
            steps.append(ops.wq_layernorm_bwd(e["dxn"], e["x"], e["gamma"], o["out"], o["dg"], o["db"], dres=e["dres"], accumulate=True))
        else:
            a = ATTN[kind]
            o = dict(dqkv=torch.full((e["dout"].shape[0], 3 * a["d"]), 7.0, device=dev), dtable=e["dtable0"].to(dev))
            steps.append(ops.wq_window_attention_bwd(e["qkv"], e["dout"], o["dqkv"], e["table"], o["dtable"],
                                                     **{k: a[k] for k in ("B", "H", "W", "ws", "shift", "heads")}))
        outs[op] = o
    return steps, outs


def run(bank, script, prec, budget=None):
    from srad_amd import ops
    steps, outs = build(bank, script)
    why = ops.wgrad_queue_script(steps, precision=prec, budget_floats=budget)
    torch.cuda.synchronize()
    return why, outs


def check_accuracy(bank, outs, prec):
    """The bars of tests/test_gpu_bwd_ops.py: weight gradients 1e-4 (fp32) / 3e-2 (bf16) - the deferred launch in bf16 mode 6e-3 -,
    LayerNorm 1e-4, attention 2e-4 (fp32 kernels: fp32 mode, and the general kernel of window 4 in both modes) / 2e-2."""
    for op, o in outs.items():
        kind = op.rstrip("'")
        if kind.startswith("defer:") or kind in LINEAR or kind == "conv":
            e = bank[kind[6:] if kind.startswith("defer:") else kind]
            tol = (6e-3 if kind.startswith("defer:") else 3e-2) if prec == "bf16" else 1e-4
            dw = o["dw"].double().cpu().reshape(e["dw"].shape) - e["dw0"].double().reshape(e["dw"].shape)
            ew, eb = _rel(dw, ALPHA * e["dw"]), _rel(o["db"].double().cpu() - e["db0"].double(), ALPHA * e["db"])
            print(f"{op} {prec}: dw {ew:.2e} db {eb:.2e} (bar {tol:.0e})")
            assert ew < tol and eb < tol, (op, ew, eb)
        elif kind in LAYERNORM:
            e = bank[kind]
            eo, eg, eb = _rel(o["out"], e["out"]), _rel(o["dg"].double().cpu() - e["dg0"].double(), e["dg"]), \
                _rel(o["db"].double().cpu() - e["db0"].double(), e["db"])
            print(f"{op}: out {eo:.2e} dgamma {eg:.2e} dbeta {eb:.2e} (bar 1e-04)")
            assert eo < 1e-4 and eg < 1e-4 and eb < 1e-4, (op, eo, eg, eb)
        else:
            e = bank[kind]
            tol = 2e-4 if prec == "fp32" or ATTN[kind]["ws"] != 8 else 2e-2
            eq, et = _rel(o["dqkv"], e["dqkv"]), _rel(o["dtable"].double().cpu() - e["dtable0"].double(), e["dtable"])
            print(f"{op} {prec}: dqkv {eq:.2e} dtable {et:.2e} (bar {tol:.0e})")
            assert eq < tol and et < tol, (op, eq, et)


def check_pressured(bank, script, prec, budget, reasons):
    """Runs the script with `budget` floats and with the whole workspace: the reasons, bit identity, accuracy of both."""
    why_full, full = run(bank, script, prec)
    why, outs = run(bank, script, prec, budget)
    print(f"{prec} budget {budget}: reduce launches {why} (whole workspace: {why_full})")
    assert why == reasons, (why, reasons)
    for op, o in outs.items():
        for k, t in o.items():
            assert torch.equal(t, full[op][k]), f"{op}.{k} differs from the run with the whole workspace"
    check_accuracy(bank, full, prec)
    check_accuracy(bank, outs, prec)
    return why_full


# ---- batch full ------------------------------------------------------------------------------------------------------------
TWELVE = ["conv", "linB", "lnA", "att8", "linC", "lnB", "att4", "linB'", "lnA'"]       # 1 + 1 + 2 + 1 + 1 + 2 + 1 + 1 + 2 items in bf16 mode


@pytest.mark.parametrize("tail,reasons", [([], [EXPLICIT]),                        # exactly 12 items: no early flush
                                          (["linC'"], [BATCH, EXPLICIT]),           # the 13th item, a split-K layer, forces one
                                          (["att8'", "linC'"], [BATCH, EXPLICIT]),  # ... as does a LayerNorm that finds 12 items and needs two entries
                                          ])
def test_batch_full(bank, tail, reasons):
    """All item kinds in one reduce launch - 64 x 64 split-K tiles, the square tiles of the nine-tap kernel (wc > 0), column sums -
    in bf16 mode, where the 16-channel convolution takes that kernel.  A flush the batch forces comes before the 13th item."""
    script = TWELVE[:-1] + tail + TWELVE[-1:] if len(tail) == 2 else TWELVE + tail
    if len(tail) == 2:      # 10 items, the table rows (11), linC' (12), then lnA' needs two entries at 12: the flush comes before its rows
        assert sum(items_of(op, "bf16") for op in script[:-1]) == 12
    else:
        assert sum(items_of(op, "bf16") for op in TWELVE) == 12
    why, outs = run(bank, script, "bf16")
    assert why == reasons, why
    check_accuracy(bank, outs, "bf16")
    # the same outputs as one op per queue launch: flush positions do not matter
    why1, single = run(bank, [x for op in script for x in (op, "flush")], "bf16")
    assert why1 == [EXPLICIT] * len(script), why1
    for op, o in outs.items():
        for k, t in o.items():
            assert torch.equal(t, single[op][k]), f"{op}.{k} differs from the one-op-per-flush run"


# ---- workspace full, one case per reservation site ----------------------------------------------------------------------------
@pytest.mark.parametrize("site,prec,script", [
    ("plan_wgrad", "fp32", ["lnB", "linB", "linC"]),
    ("plan_wgrad", "bf16", ["lnB", "linB", "linC"]),
    ("wgrad_conv9", "bf16", ["lnA", "linC", "conv"]),
    ("reserve_colsum (LayerNorm)", "fp32", ["linC", "att4", "lnB"]),
    ("reserve_colsum (attention)", "fp32", ["linB", "lnB", "att8"]),
    ("reserve_colsum (attention)", "bf16", ["linB", "lnB", "att8"]),
])
def test_workspace_full(bank, site, prec, script):
    """The budget holds everything but the last four floats of the last reservation, with earlier items queued: the queue flushes
    at that reservation, and only there."""
    needs = [need_of(op, prec) for op in script]
    assert all(n > 0 for n in needs), needs
    why_full = check_pressured(bank, script, prec, sum(needs) - 4, [WS, EXPLICIT])
    assert why_full == [EXPLICIT]
    # one float more than the needs computed here and nothing overflows: the budget above is the code's own boundary
    why, _ = run(bank, script, prec, sum(needs))
    assert why == [EXPLICIT], why


# ---- deferred layers pending -------------------------------------------------------------------------------------------------
DEFERRED3 = ["defer:linA", "defer:linB", "defer:linC"]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_flush_with_deferred_layers_pending(bank, prec):
    """The engine's block order with earlier work queued: a written split-K layer, three deferred Linear layers (items queued,
    partials not written before the shared launch), then a LayerNorm backward whose rows overflow the budget, the attention
    backward, a fourth deferred layer, the shared launch, the flush.  The flush the LayerNorm forces may reduce only the written
    layer; the three pending regions stay live, so the rows, the table rows and the fourth layer go into what the written layer
    held.  (In bf16 mode linA is not split: a pending layer without a region, and the launch takes the bf16 kernel.)
    Before the fix that flush reduced the three pending items from partials nobody had written and handed their regions out
    again: wrong dW / db of those layers, no error."""
    script = ["linC"] + DEFERRED3 + ["lnB", "att8", "defer:linB'"]
    needs = {op: need_of(op, prec) for op in script}
    held = needs["linC"] + sum(needs[op] for op in DEFERRED3)
    assert needs["lnB"] + needs["att8"] + needs["defer:linB'"] <= needs["linC"]          # what the flush frees holds the rest
    check_pressured(bank, script, prec, held + needs["lnB"] - 4, [WS, EXPLICIT])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_deferred_layer_overflows_with_layers_pending(bank, prec):
    """A block's own order, nothing queued before it: the fourth deferred layer is the reservation that does not fit.  The flush
    reduces the LayerNorm and table rows, which lie above the three pending regions, and the layer goes there."""
    script = DEFERRED3 + ["lnB", "att8", "defer:linB'"]
    needs = [need_of(op, prec) for op in script]
    check_pressured(bank, script, prec, sum(needs) - 4, [WS, EXPLICIT])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_no_room_next_to_pending_layers_is_an_error(bank, prec):
    """Three pending layers and LayerNorm rows that do not fit beside them, nothing written that a flush could free: an error
    that names the caller, and no output changes (before the fix: rows handed out on top of the pending regions, no error)."""
    script = DEFERRED3 + ["lnB"]
    budget = sum(need_of(op, prec) for op in script) - 4
    steps, outs = build(bank, script)
    before = {op: {k: t.clone() for k, t in o.items()} for op, o in outs.items()}
    from srad_amd import ops
    with pytest.raises(RuntimeError, match=r"ln_bwd: split-K workspace too small next to the deferred layers"):
        ops.wgrad_queue_script(steps, precision=prec, budget_floats=budget)
    torch.cuda.synchronize()
    for op, o in outs.items():
        for k, t in o.items():
            assert torch.equal(t, before[op][k]), f"{op}.{k} changed"


# ---- one reservation larger than the budget --------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,who", [("linC", "wgrad"), ("defer:linC", "wgrad"), ("lnB", "ln_bwd"), ("att4", "window_attn_bwd")])
def test_single_reservation_larger_than_the_budget(bank, op, who):
    steps, outs = build(bank, ["lnA", op])            # lnA's rows are queued, never reduced
    before = {k: {n: t.clone() for n, t in o.items()} for k, o in outs.items()}
    from srad_amd import ops
    with pytest.raises(RuntimeError, match=who + r": split-K workspace too small \(\d+ floats needed, \d+ given\)"):
        ops.wgrad_queue_script(steps, precision="fp32", budget_floats=need_of(op, "fp32") - 4)
    torch.cuda.synchronize()
    for k, o in outs.items():
        for n, t in o.items():
            if k == "lnA" and n == "out":
                continue                                 # its data gradient is written by the LayerNorm kernel itself, before the failing step
            assert torch.equal(t, before[k][n]), f"{k}.{n} changed"
