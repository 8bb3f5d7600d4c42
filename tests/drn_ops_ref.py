"""The case table, inputs and fp64 references shared by tests/test_gpu_drn_ops.py (GPU) and tests/test_drn_ops_host.py (CPU).
Everything here is plain torch on the CPU; the kernel's fp32 / bf16 inputs are taken as exact and widened to fp64."""
import math

import torch

U32 = 2.0 ** -24            # unit round-off of fp32
BAR32 = 1e-5                # fp32 element-wise kernels, of the reference tensor's max (test_gpu_ops.test_layernorm)

# (B, hw, C) -> the launch the RCAB tail and its backward get: slices per image, NI (items a thread holds in registers over
# the gate chain; 0 = the loop).  Worked out by hand from ca_slices (1 below 64 pixels, 8 below 1024, 64 below 128 * 128, then
# 128) and items = ceil(hw / slices) * C / 4: <= 1280 -> 5, <= 2560 -> 10, else 0.
CA_CASES = {
    (2, 63, 40): (1, 5),         # 1 slice, Cr = 2: 63 * 10 = 630 items
    (2, 65, 80): (8, 5),         # 8 slices of 9 pixels, the last one holds 2
    (1, 1000, 80): (8, 10),      # 125 * 20 = 2500
    (1, 1023, 160): (8, 0),      # 128 * 40 = 5120; wide gate (C > 96)
    (2, 1025, 80): (64, 5),      # 64 slices of 17 pixels: 61, 62 and 63 start past the image's end (items < 0)
    (1, 4096, 160): (64, 10),    # 64 * 40 = 2560; wide gate
    (1, 12288, 80): (64, 0),     # 192 * 20 = 3840
    (2, 16384, 80): (128, 10),   # 128 * 20 = 2560
    (1, 16385, 80): (128, 0),    # 129 * 20 = 2580, uneven
    (1, 1024, 512): (64, 10),    # Cr = 32: two row classes in the partial-row sum (256 / 128), 16 * 128 = 2048
    (1, 256, 96): (8, 5),        # the last small gate (C <= 96 and Cr <= 8) ...
    (1, 256, 112): (8, 5),       # ... and the first wide ones: C > 96 with Cr = 7,
    (1, 256, 128): (8, 5),       # and Cr = 8
}
NCHUNK_CASES = [(2, 16384, 80), (1, 1024, 512)]       # also with nchunk = 1, 143, 144, 145, 256: the 12 x nparts trip boundaries
NCHUNKS = [1, 143, 144, 145, 256]
STORAGE_CASES = [(1, 1000, 80), (1, 12288, 80), (2, 16384, 80), (2, 1025, 80)]      # NI = 10, the loop, 10 on 128 slices, and 5
STORAGES = [(False, False, False), (True, True, True), (True, True, False), (True, False, True), (True, False, False)]   # r, x, y as bf16


def ca_weights(C, seed):
    """conv_du weights scaled 2 / sqrt(fan_in), small biases."""
    g = torch.Generator().manual_seed(seed)
    Cr = C // 16
    w1 = torch.randn(Cr, C, generator=g) * (2 / math.sqrt(C))
    b1 = torch.randn(Cr, generator=g) * 0.1
    w2 = torch.randn(C, Cr, generator=g) * (2 / math.sqrt(Cr))
    b2 = torch.randn(C, generator=g) * 0.1
    return w1, b1, w2, b2


def ca_gate64(pool, hw, w1, b1, w2, b2):
    """CALayer (src/drn.py:123-139) on pooled SUMS [B, C], fp64: (gate [B, C], hidden pre-activations [B, Cr])."""
    mean = pool.double() / hw
    pre = mean @ w1.double().t() + b1.double()
    return torch.sigmoid(torch.relu(pre) @ w2.double().t() + b2.double()), pre


def ca_tail64(part, hw, w1, b1, w2, b2, r, x):
    """The RCAB tail in fp64: part [B, nchunk, C], r and x [B*hw, C] -> (y [B*hw, C], gate [B, C], pool [B, C], pre)."""
    B, _, C = part.shape
    pool = part.double().sum(1)
    gate, pre = ca_gate64(pool, hw, w1, b1, w2, b2)
    y = r.double().reshape(B, hw, C) * gate[:, None, :] + x.double().reshape(B, hw, C)
    return y.reshape(B * hw, C), gate, pool, pre


def ca_tail32(part, hw, w1, b1, w2, b2, r, x):
    """The same in plain fp32 (torch's own order of operations): how far fp32 itself is from ca_tail64."""
    B, _, C = part.shape
    mean = part.sum(1) / hw
    gate = torch.sigmoid(torch.relu(mean @ w1.t() + b1) @ w2.t() + b2)
    return (r.reshape(B, hw, C) * gate[:, None, :] + x.reshape(B, hw, C)).reshape(B * hw, C), gate


def ca_inputs(B, hw, C, nchunk=32, seed=0, from_r=False):
    """Inputs of one RCAB tail: r (per-channel offset: the means are not about 0), x, the conv_du weights and the partial rows
    - random rows whose sum is about hw * (offset + noise), or with from_r the true per-chunk sums of r in fp64, rounded.
    The seed moves on until every hidden pre-activation is at least 1e-3 away from 0 (the ReLU mask is then stable under fp32
    rounding); the caller asserts that margin."""
    for s in range(seed, seed + 50):
        g = torch.Generator().manual_seed(1000 * s + 7 * hw + C + B)
        off = torch.rand(C, generator=g) * 2 - 1
        r = torch.randn(B * hw, C, generator=g) * 0.5 + off
        x = torch.randn(B * hw, C, generator=g)
        if from_r:
            per = -(-hw // nchunk)
            rp = torch.zeros(B, nchunk * per, C, dtype=torch.float64)
            rp[:, :hw] = r.double().reshape(B, hw, C)
            part = rp.reshape(B, nchunk, per, C).sum(2).float()
        else:
            part = (off + 0.3 * torch.randn(B, nchunk, C, generator=g)) * (hw / nchunk)
        w1, b1, w2, b2 = ca_weights(C, 1000 * s + C)
        pre = ca_gate64(part.double().sum(1), hw, w1, b1, w2, b2)[1]
        if float(pre.abs().min()) > 2e-3:
            break
    return dict(part=part, w1=w1, b1=b1, w2=w2, b2=b2, r=r, x=x)


def ca_backward64(r, x, g, B, hw, w1, b1, w2, b2):
    """Autograd in fp64 of sum(g * (r * gate(mean r) + x)): (dr [B*hw, C], dpool [B, C] = d/d(pooled sums), dw1, db1, dw2, db2
    summed over the batch, gate, pool, pre)."""
    C = r.shape[1]
    rd = r.double().reshape(B, hw, C).clone().requires_grad_(True)
    ws = [t.double().clone().requires_grad_(True) for t in (w1, b1, w2, b2)]
    pool = rd.sum(1)
    pool.retain_grad()
    pre = (pool / hw) @ ws[0].t() + ws[1]
    gate = torch.sigmoid(torch.relu(pre) @ ws[2].t() + ws[3])
    y = rd * gate[:, None, :] + x.double().reshape(B, hw, C)
    (y * g.double().reshape(B, hw, C)).sum().backward()
    return dict(dr=rd.grad.reshape(B * hw, C), dpool=pool.grad, dw1=ws[0].grad, db1=ws[1].grad, dw2=ws[2].grad, db2=ws[3].grad,
                gate=gate.detach(), pool=pool.detach(), pre=pre.detach())


def gate_backward64(dgate, pool, hw, w1, b1, w2, b2):
    """Autograd in fp64 of sum(dgate * gate(pool / hw)) - the part of the RCAB backward ca_bwd_kernel computes."""
    pl = pool.double().clone().requires_grad_(True)
    ws = [t.double().clone().requires_grad_(True) for t in (w1, b1, w2, b2)]
    pre = (pl / hw) @ ws[0].t() + ws[1]
    gate = torch.sigmoid(torch.relu(pre) @ ws[2].t() + ws[3])
    (gate * dgate.double()).sum().backward()
    return dict(dpool=pl.grad, dw1=ws[0].grad, db1=ws[1].grad, dw2=ws[2].grad, db2=ws[3].grad, gate=gate.detach(), pre=pre.detach())


def bicubic_kernel64(x, scale):
    """bicubic_submean_kernel's formula (A = -0.75, half-pixel centres, border clamp) in fp64: x [B, C, H, W] -> [B, C, Hs, Ws]."""
    A = -0.75
    c1 = lambda t: ((A + 2) * t - (A + 3)) * t * t + 1
    c2 = lambda t: ((A * t - 5 * A) * t + 8 * A) * t - 4 * A

    def axis(n):
        o = torch.arange(n * scale, dtype=torch.float64)
        src = (o + 0.5) / scale - 0.5
        f = torch.floor(src)
        t = src - f
        idx = torch.stack([(f.long() - 1 + k).clamp(0, n - 1) for k in range(4)])
        return idx, torch.stack([c2(t + 1), c1(t), c1(1 - t), c2(2 - t)])
    x = x.double()
    iy, wy = axis(x.shape[2])
    ix, wx = axis(x.shape[3])
    rows = sum(x[:, :, iy[k], :] * wy[k][None, None, :, None] for k in range(4))
    return sum(rows[:, :, :, ix[k]] * wx[k] for k in range(4))
