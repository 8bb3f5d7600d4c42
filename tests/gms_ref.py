"""The gradient-magnitude similarity maps and loss restated on the CPU (DESIGN.md "Gradient-magnitude maps and loss"), for
the tests of ``metrics.gms_maps``, the GMS / MSGMS loss kinds and their kernels: ``gms_maps`` in numpy (exact integers up to
M, then float64 operations in the definition's order and one rounding to float32), ``literal``, the same definition once more
as a per-pixel loop over Python ints and floats (IEEE doubles, math.sqrt), ``upsample``, the bilinear step alone, and
``gms_loss``, the loss in float64 torch with a square root whose derivative is 0 at 0, so autograd gives the reference
gradient.  Also the inputs the loss tests use and the conditioning check they assert."""
import math

import numpy as np
import torch
import torch.nn.functional as F

C_GMS = 0.0026                     # GMSD's 170 / 255^2


def ck2(level, channels):
    K = 3.0 * channels * 255.0 * float(4 ** level)
    return C_GMS * K * K


def _prewitt_sq(s):
    """M = Gx^2 + Gy^2 of int64 planes [n, h, w]: numpy 'reflect' padding by one pixel, tap-pair differences."""
    p = np.pad(s, ((0, 0), (1, 1), (1, 1)), mode="reflect")
    h, w = s.shape[1:]
    t = lambda dy, dx: p[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    gx = (t(-1, 1) - t(-1, -1)) + (t(0, 1) - t(0, -1)) + (t(1, 1) - t(1, -1))
    gy = (t(1, -1) - t(-1, -1)) + (t(1, 0) - t(-1, 0)) + (t(1, 1) - t(-1, 1))
    return gx * gx + gy * gy


def level_planes(sr_u8, hr_u8, levels):
    """[d_0, ..., d_(L-1)]: float64 [n, h_l, w_l] each."""
    sr_u8, hr_u8 = np.asarray(sr_u8), np.asarray(hr_u8)
    channels = sr_u8.shape[3]
    sa, sb = sr_u8.astype(np.int64).sum(3), hr_u8.astype(np.int64).sum(3)
    out = []
    for l in range(levels):
        if l:
            sa = sa[:, 0::2, 0::2] + sa[:, 0::2, 1::2] + sa[:, 1::2, 0::2] + sa[:, 1::2, 1::2]
            sb = sb[:, 0::2, 0::2] + sb[:, 0::2, 1::2] + sb[:, 1::2, 0::2] + sb[:, 1::2, 1::2]
        Ma, Mb = _prewitt_sq(sa), _prewitt_sq(sb)
        r = np.sqrt(Ma.astype(np.float64)) - np.sqrt(Mb.astype(np.float64))
        out.append((r * r) / ((Ma + Mb).astype(np.float64) + ck2(l, channels)))
    return out


def upsample(d, f):
    """Bilinear upsampling (align_corners=False) of float64 planes [n, h, w] by the integer factor f, the definition's order."""
    n, h, w = d.shape

    def axis(size, cells):
        o = (np.arange(size, dtype=np.float64) + 0.5) / f - 0.5
        i0 = np.floor(o)
        t = o - i0
        i0 = i0.astype(np.int64)
        return np.clip(i0, 0, cells - 1), np.clip(i0 + 1, 0, cells - 1), t

    i0, i1, ty = axis(h * f, h)
    j0, j1, tx = axis(w * f, w)
    ty, tx = ty[None, :, None], tx[None, None, :]
    g = lambda i, j: d[:, i[:, None], j[None, :]]
    return (g(i0, j0) * (1.0 - tx) + g(i0, j1) * tx) * (1.0 - ty) + (g(i1, j0) * (1.0 - tx) + g(i1, j1) * tx) * ty


def gms_maps(sr_u8, hr_u8, levels=1):
    """float32 [n, H, W]: the definition of ``srad_gms_maps``."""
    planes = level_planes(sr_u8, hr_u8, levels)
    acc = planes[0]
    for l in range(1, levels):
        acc = acc + upsample(planes[l], 1 << l)
    return (acc * (1.0 / levels)).astype(np.float32)


def literal(sr_u8, hr_u8, levels=1):
    """The same definition as a double loop over Python ints and floats; float32 [n, H, W]."""
    sr_u8, hr_u8 = np.asarray(sr_u8), np.asarray(hr_u8)
    n, H, W, channels = sr_u8.shape
    out = np.zeros((n, H, W), np.float32)
    refl = lambda i, size: 1 if i < 0 else (size - 2 if i >= size else i)
    for i in range(n):
        planes = []
        sa = [[sum(int(v) for v in sr_u8[i, y, x]) for x in range(W)] for y in range(H)]
        sb = [[sum(int(v) for v in hr_u8[i, y, x]) for x in range(W)] for y in range(H)]
        for l in range(levels):
            if l:
                sa = [[sa[2 * y][2 * x] + sa[2 * y][2 * x + 1] + sa[2 * y + 1][2 * x] + sa[2 * y + 1][2 * x + 1]
                       for x in range(len(sa[0]) // 2)] for y in range(len(sa) // 2)]
                sb = [[sb[2 * y][2 * x] + sb[2 * y][2 * x + 1] + sb[2 * y + 1][2 * x] + sb[2 * y + 1][2 * x + 1]
                       for x in range(len(sb[0]) // 2)] for y in range(len(sb) // 2)]
            h, w = len(sa), len(sa[0])

            def M(s, y, x):
                p = lambda yy, xx: s[refl(yy, h)][refl(xx, w)]
                gx = (p(y - 1, x + 1) - p(y - 1, x - 1)) + (p(y, x + 1) - p(y, x - 1)) + (p(y + 1, x + 1) - p(y + 1, x - 1))
                gy = (p(y + 1, x - 1) - p(y - 1, x - 1)) + (p(y + 1, x) - p(y - 1, x)) + (p(y + 1, x + 1) - p(y - 1, x + 1))
                return gx * gx + gy * gy

            d = [[0.0] * w for _ in range(h)]
            for y in range(h):
                for x in range(w):
                    Ma, Mb = M(sa, y, x), M(sb, y, x)
                    r = math.sqrt(float(Ma)) - math.sqrt(float(Mb))
                    d[y][x] = (r * r) / (float(Ma + Mb) + ck2(l, channels))
            planes.append(d)
        for y in range(H):
            for x in range(W):
                acc = planes[0][y][x]
                for l in range(1, levels):
                    f, d = 1 << l, planes[l]
                    h, w = len(d), len(d[0])
                    oy, ox = (y + 0.5) / f - 0.5, (x + 0.5) / f - 0.5
                    fy, fx = math.floor(oy), math.floor(ox)
                    ty, tx = oy - fy, ox - fx
                    i0, i1 = min(max(fy, 0), h - 1), min(max(fy + 1, 0), h - 1)
                    j0, j1 = min(max(fx, 0), w - 1), min(max(fx + 1, 0), w - 1)
                    acc = acc + ((d[i0][j0] * (1.0 - tx) + d[i0][j1] * tx) * (1.0 - ty) + (d[i1][j0] * (1.0 - tx) + d[i1][j1] * tx) * ty)
                out[i, y, x] = np.float32(acc * (1.0 / levels))
    return out


# ---- the loss ------------------------------------------------------------------------------------------------------
class _SafeSqrt(torch.autograd.Function):
    """sqrt with the zero subgradient at 0."""

    @staticmethod
    def forward(ctx, m):
        g = m.sqrt()
        ctx.save_for_backward(g)
        return g

    @staticmethod
    def backward(ctx, grad):
        g, = ctx.saved_tensors
        return torch.where(g > 0, grad / (2.0 * g.clamp_min(1e-300)), torch.zeros_like(grad))


def _grad_sq(x):
    """(gx^2 + gy^2, gx, gy) of [B, 1, h, w] planes: reflect padding, tap-pair differences, then the division by 3."""
    p = F.pad(x, (1, 1, 1, 1), mode="reflect")
    h, w = x.shape[2:]
    t = lambda dy, dx: p[:, :, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    gx = ((t(-1, 1) - t(-1, -1)) + (t(0, 1) - t(0, -1)) + (t(1, 1) - t(1, -1))) / 3.0
    gy = ((t(1, -1) - t(-1, -1)) + (t(1, 0) - t(-1, 0)) + (t(1, 1) - t(-1, 1))) / 3.0
    return gx * gx + gy * gy


def loss_levels(sr, hr, levels, rgb_range=255.0):
    """Per level (Ma, Mb, d) of float64 [B, C, H, W] tensors."""
    xa = (sr.double() / rgb_range).clamp(0.0, 1.0).mean(1, keepdim=True)
    xb = (hr.double() / rgb_range).clamp(0.0, 1.0).mean(1, keepdim=True)
    out = []
    for l in range(levels):
        if l:
            xa, xb = F.avg_pool2d(xa, 2), F.avg_pool2d(xb, 2)
        Ma, Mb = _grad_sq(xa), _grad_sq(xb)
        r = _SafeSqrt.apply(Ma) - _SafeSqrt.apply(Mb)
        out.append((Ma, Mb, (r * r) / (Ma + Mb + C_GMS)))
    return out


def gms_loss(sr, hr, levels, rgb_range=255.0):
    """The GMS (levels 1) / MSGMS (levels 4) loss in float64: (1 / L) sum_l mean(d_l)."""
    return sum(d.mean() for _, _, d in loss_levels(sr, hr, levels, rgb_range)) / levels


def well_conditioned(sr, levels, rgb_range=255.0, floor=1e-3):
    """(every pixel of every level of sr has g == 0 exactly or g >= floor, the smallest non-zero g)."""
    smallest = float("inf")
    for Ma, _, _ in loss_levels(sr, sr, levels, rgb_range):
        g = Ma.sqrt()
        nz = g[g > 0]
        if nz.numel():
            smallest = min(smallest, float(nz.min()))
    return smallest >= floor, smallest


LOSS_SHAPES = [(2, 1, 16, 24), (1, 3, 40, 16), (3, 1, 64, 48), (2, 3, 128, 128)]


def loss_inputs(shape, seed=1):
    """(sr, hr) float32 [B, C, H, W] in [0, 255] units: two slanted ramps mod 256 (the same base in every channel), uniform
    noise in +-1.5, and in sr a block of 300 and a block of -20 (the clamp, and the exact-zero convention inside them)."""
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    sr = np.broadcast_to(((6 * x + 7 * y) % 256).astype(np.float64), shape) + rng.uniform(-1.5, 1.5, shape)
    hr = np.broadcast_to(((7 * x + 5 * y) % 256).astype(np.float64), shape) + rng.uniform(-1.5, 1.5, shape)
    sr[:, :, 4:10, 5:11] = 300.0
    sr[:, :, H - 7:H - 2, 2:8] = -20.0
    return torch.from_numpy(sr.astype(np.float32)), torch.from_numpy(hr.astype(np.float32))
