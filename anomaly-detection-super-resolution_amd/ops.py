"""Single-operator bindings (C ABI ``srad_op_*``).  Activations are NHWC / token-major fp32
tensors on the GPU; weights are given in PyTorch layout and packed by the library."""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
from typing import Optional

import torch

from . import _lib as L


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("srad_amd ops run on the GPU only (HIP); there is no CPU fallback")


# include/srad.h SRAD_PATH_*: the reference paths a test can force instead of the one shape and precision pick
PATHS = {"unfused_blocks": 0, "qkv_via_gemm": 1, "attn_f32_in": 2, "upconv_one_gemm": 3}
# ... and its launch-plan overrides (ids from SRAD_PATH_PLAN_FIRST, then from SRAD_PATH_PLAN2_FIRST): the launches a default path is compared against
PLAN_PATHS = {"block_two_launches": 16, "tail_chain": 17, "ends_chain": 32, "fc2_chain": 48}


@contextlib.contextmanager
def path_override(**paths: bool):
    """Force reference paths inside the block, e.g. ``with ops.path_override(unfused_blocks=True):``, and restore the previous
    settings on exit.  unfused_blocks is read by the DRCT engine when it is created (forward) and at every backward;
    block_two_launches (a Swin block as qkv_attn + mlp_block where the one-launch kernel would run) whenever a forward
    records its launches, i.e. before the first forward of a shape; tail_chain (the Upsample convolutions, conv_last and the
    layout change as their own launches where the folded output end would run) and ends_chain (the final LayerNorm,
    conv_after_body and conv_before_upsample as their own launches where the body-end launch would run) and fc2_chain (a
    Swin block's fc2 and adjust conv as the chain's two GEMMs where the folded second half would run) at every forward; a
    model whose choice changes drops its recorded graph."""
    lib = L.lib()
    ids = {name: PATHS[name] if name in PATHS else PLAN_PATHS[name] for name in paths}
    before = {name: lib.srad_get_path_override(i) for name, i in ids.items()}
    try:
        for name, on in paths.items():
            L.check(lib.srad_set_path_override(ids[name], 1 if on else 0), "set_path_override")
        yield
    finally:
        for name, was in before.items():
            L.check(lib.srad_set_path_override(ids[name], was), "set_path_override")


def _gemm_geometry(x, weight, B, H, W, stride, ln):
    """The (x, w, ldx, Cin, N, ntaps, B, H, W, M) a gemm call hands to the library: channels padded to a multiple of 4."""
    assert x.dim() == 2 and (x.stride(1) == 1 or x.shape[1] == 1) and x.dtype == torch.float32
    ldx = x.stride(0) if x.shape[0] > 1 else x.shape[1]
    ntaps = 9 if weight.dim() == 4 and weight.shape[-1] == 3 else 1
    N, Cin = weight.shape[0], weight.shape[1]
    assert x.shape[1] >= Cin
    w = weight.detach().reshape(N, Cin, ntaps).float()
    if Cin % 4 or ldx % 4 or x.data_ptr() % 16:
        # the kernels address activations as float4: pad the channels (zeros) like the engines do
        cpad = (Cin + 3) // 4 * 4
        x = torch.nn.functional.pad(x[:, :Cin], (0, cpad - Cin)).contiguous()
        w = torch.nn.functional.pad(w, (0, 0, 0, cpad - Cin))
        if ln is not None:
            raise ValueError("LayerNorm fusion needs a channel count that is a multiple of 4")
        Cin, ldx = cpad, cpad
    w = w.contiguous()
    if ntaps == 1 and stride == 1:
        B, H, W = 1, 1, x.shape[0]
    pad, k = (1, 3) if ntaps == 9 else (0, 1)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return x, w, ldx, Cin, N, ntaps, B, H, W, B * Ho * Wo


def gemm(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, B: int = 1, H: int = 0,
         W: int = 0, stride: int = 1, ln: Optional[tuple] = None, act: int = L.ACT_NONE, slope: float = 0.0,
         alpha: float = 1.0, residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
         out_offset: int = 0, pixel_shuffle: bool = False, precision: str = "fp32", plan_only: bool = False):
    """x: [rows, Cin] (row stride = x.stride(0)); weight: [N, Cin] or [N, Cin, 3, 3].
    For a 3x3 / strided conv pass the image geometry (B, H, W) of the NHWC input rows.
    plan_only: launch nothing and return the GemmPlan of this very call (gemm_plan)."""
    _need_cuda(x, weight)
    x, w, ldx, Cin, N, ntaps, B, H, W, M = _gemm_geometry(x, weight, B, H, W, stride, ln)
    if out is None:
        if pixel_shuffle:
            out = torch.empty(M * 4, N // 4, dtype=torch.float32, device=x.device)
        else:
            out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    prec = L.PRECISIONS[precision]
    nbytes = L.lib().srad_op_gemm_scratch_bytes(prec, N, Cin, ntaps)
    scratch = torch.empty(nbytes + 256, dtype=torch.uint8, device=x.device)
    off = (-scratch.data_ptr()) % 256
    g, b_ = (ln if ln is not None else (None, None))
    args = (prec, L.dptr(x), ldx, B, H, W, Cin, L.dptr(w), N, ntaps, stride,
            L.dptr(bias), L.dptr(g), L.dptr(b_), act, slope, alpha, L.dptr(residual),
            0 if residual is None else residual.stride(0), L.dptr(out), out.stride(0),
            out_offset, 2 if pixel_shuffle else 0, C.c_void_p(scratch.data_ptr() + off),
            C.c_size_t(nbytes), L.current_stream_ptr())
    if plan_only:
        plan = L.GemmPlan()
        L.check(L.lib().srad_op_gemm_plan(*args, C.byref(plan)), "op_gemm_plan")
        return _plan_tuple(plan)
    L.check(L.lib().srad_op_gemm(*args), "op_gemm")
    return out


GemmPlan = collections.namedtuple("GemmPlan", "family BM BN CPS LN CONV SPECIAL grid launches")


def _plan_tuple(p: "L.GemmPlan") -> GemmPlan:
    return GemmPlan(L.GEMM_FAMILIES[p.family], p.BM, p.BN, p.CPS, bool(p.LN), bool(p.CONV), bool(p.SPECIAL), (p.grid_x, p.grid_y),
                    p.launches)


def gemm_plan(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, **kw) -> GemmPlan:
    """The kernel family, tile, K-stage depth, template variant and grid that gemm() with the same arguments runs
    (srad_op_gemm_plan): decided on the host, nothing is launched."""
    return gemm(x, weight, bias, plan_only=True, **kw)


def gemm_plan_shape(precision: str, M: int, N: int, Cin: int, *, ntaps: int = 1, stride: int = 1, B: int = 1, H: int = 0, W: int = 0,
                    ln: bool = False, bias: bool = True, act: int = L.ACT_NONE, residual: bool = False,
                    pixel_shuffle: bool = False) -> GemmPlan:
    """gemm_plan from a shape alone, with aligned stand-in pointers that are never dereferenced: needs no GPU.  A row-identity
    problem is M rows; a conv (ntaps = 9 or stride 2) is (B, H, W) input pixels and M is ignored."""
    fake = C.c_void_p(1 << 20)
    if ntaps == 1 and stride == 1:
        B, H, W = 1, 1, M
    prec = L.PRECISIONS[precision]
    plan = L.GemmPlan()
    L.check(L.lib().srad_op_gemm_plan(prec, fake, Cin, B, H, W, Cin, fake, N, ntaps, stride, fake if bias else None,
                                      fake if ln else None, fake if ln else None, act, 0.0, 1.0, fake if residual else None,
                                      N if residual else 0, fake, N // 4 if pixel_shuffle else N, 0, 2 if pixel_shuffle else 0, fake,
                                      C.c_size_t(L.lib().srad_op_gemm_scratch_bytes(prec, N, Cin, ntaps)), None, C.byref(plan)),
            "op_gemm_plan")
    return _plan_tuple(plan)


def window_attention(qkv: torch.Tensor, table: torch.Tensor, B: int, H: int, W: int, ws: int, shift: int,
                     heads: int, precision: str = "fp32", pad_value: float = 0.0) -> torch.Tensor:
    """qkv: [B*H*W, 3d] raster-ordered tokens in the reference's column order (q | k | v, heads
    contiguous) -> [B*H*W, d].  The kernel reads a head-padded layout (every head slice padded to a
    multiple of 4 floats; the engine's QKV GEMM writes it directly), so this wrapper re-lays it out."""
    _need_cuda(qkv, table)
    assert qkv.shape[0] == B * H * W
    d = qkv.shape[1] // 3
    hd = d // heads
    hdp = (hd + 3) // 4 * 4
    padded = torch.nn.functional.pad(qkv.reshape(-1, 3 * heads, hd).float(), (0, hdp - hd), value=pad_value)
    padded = padded.reshape(-1, 3 * heads * hdp).contiguous()   # pad columns are never read as data (any value, NaN too)
    out = torch.empty(qkv.shape[0], d, dtype=torch.float32, device=qkv.device)
    L.check(L.lib().srad_op_window_attn(L.PRECISIONS[precision], L.dptr(padded), L.dptr(out),
                                        L.dptr(table.contiguous()), B, H, W, ws, shift, d, heads, hdp,
                                        L.current_stream_ptr()), "op_window_attn")
    return out


def layernorm(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    _need_cuda(x, g, b)
    assert x.dim() == 2 and x.stride(1) == 1
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    L.check(L.lib().srad_op_layernorm(L.dptr(x), x.stride(0), L.dptr(y), y.stride(0), x.shape[0], x.shape[1],
                                      L.dptr(g), L.dptr(b), L.current_stream_ptr()), "op_layernorm")
    return y


def tail_fold_build(up_weights, up_biases, last_w: torch.Tensor, last_b: torch.Tensor) -> dict:
    """The folded DRCT output end built on the device (C ABI ``srad_op_tail_fold_build``) from the Upsample convolutions
    (one for x2, two for x4: ``[4F, F, 3, 3]`` / ``[4F]``) and conv_last (``[C, F, 3, 3]`` / ``[C]``).  Returns the region and
    views into it: ``wf`` fp32 [9, N, 25, F], ``pack`` bf16 [9, NT, 25, F // 32, 64, 8], ``bias`` fp32 [9, 16 NT]."""
    _need_cuda(last_w, last_b, *up_weights, *up_biases)
    scale, Cc, F = 2 ** len(up_weights), last_w.shape[0], last_w.shape[1]
    offs = [C.c_size_t() for _ in range(4)]
    L.check(L.lib().srad_op_tail_fold_layout(F, Cc, scale, *[C.byref(o) for o in offs]), "op_tail_fold_layout")
    wf_off, pack_off, bias_off, nbytes = [o.value for o in offs]
    keep, ptr, _ = L.ws_buffer(nbytes, last_w.device)
    srcs = [t.detach().float().contiguous() for t in (up_weights[0], up_biases[0])]
    srcs += [t.detach().float().contiguous() for t in (up_weights[1], up_biases[1])] if scale == 4 else [None, None]
    srcs += [last_w.detach().float().contiguous(), last_b.detach().float().contiguous()]
    L.check(L.lib().srad_op_tail_fold_build(F, Cc, scale, *[L.dptr(t) for t in srcs], ptr, C.c_size_t(nbytes), L.current_stream_ptr()),
            "op_tail_fold_build")
    base = ptr.value - keep.data_ptr()
    N, NT = scale * scale * Cc, (scale * scale * Cc + 15) // 16

    def view(off, count, dtype, shape):
        return keep[base + off: base + off + count * dtype.itemsize].view(dtype).view(shape)
    return dict(region=keep, ptr=ptr, scale=scale, C=Cc, F=F,
                wf=view(wf_off, 9 * N * 25 * F, torch.float32, (9, N, 25, F)),
                pack=view(pack_off, 9 * NT * 25 * F * 16, torch.bfloat16, (9, NT, 25, F // 32, 64, 8)),
                bias=view(bias_off, 9 * NT * 16, torch.float32, (9, NT * 16)))


def tail_fold(c2: torch.Tensor, up_weights, up_biases, last_w: torch.Tensor, last_b: torch.Tensor, B: int, H: int, W: int,
              img_range: float = 1.0, mean=(0.0, 0.0, 0.0), fold: Optional[dict] = None) -> torch.Tensor:
    """DRCT's output end as one launch: c2 [B*H*W, 64] (conv_before_upsample's output, NHWC rows) -> y [B, C, sH, sW] =
    conv_last(PixelShuffle(up(...))) / img_range + mean (C ABI ``srad_op_tail_fold``).  Builds the fold unless one is given."""
    _need_cuda(c2)
    assert c2.dim() == 2 and c2.shape == (B * H * W, 64) and c2.is_contiguous() and c2.dtype == torch.float32
    if fold is None:
        fold = tail_fold_build(up_weights, up_biases, last_w, last_b)
    s, Cc = fold["scale"], fold["C"]
    mean = list(mean) + [0.0] * (3 - len(mean))
    y = torch.empty(B, Cc, s * H, s * W, dtype=torch.float32, device=c2.device)
    L.check(L.lib().srad_op_tail_fold(L.dptr(c2), B, H, W, Cc, s, fold["ptr"], img_range, mean[0], mean[1], mean[2], L.dptr(y),
                                      L.current_stream_ptr()), "op_tail_fold")
    return y


def drct_ends_supported(precision: str, E: int, F: int, C_: int, B: int, H: int, W: int, cus: Optional[int] = None) -> bool:
    """Does a DRCT inference forward of this shape run its body end as one launch (C ABI
    ``srad_drct_ends_supported``): bf16, E % 4 == 0, E <= 192, F = 64, gray or RGB, and one round of 16-pixel tiles on the
    device's CUs (``cus``: on that many instead; host code, needs no GPU)."""
    prec = L.PRECISIONS[precision]
    if cus is None:
        return bool(L.lib().srad_drct_ends_supported(prec, E, F, C_, B, H, W))
    return bool(L.lib().srad_drct_ends_supported_cus(prec, E, F, C_, B, H, W, cus))


def drct_body_end(x: torch.Tensor, ln_g: torch.Tensor, ln_b: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, feat0: torch.Tensor,
                  w2: torch.Tensor, b2: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    """DRCT's body end as one launch (C ABI ``srad_op_drct_body_end``): x [B*H*W, >= E] (row stride = x.stride(0)) ->
    c2 [B*H*W, 64] = LeakyReLU_0.01(conv_before_upsample(conv_after_body(LayerNorm(x[:, :E])) + feat0))."""
    _need_cuda(x, ln_g, ln_b, w1, b1, feat0, w2, b2)
    E, F = w1.shape[0], w2.shape[0]
    assert x.dim() == 2 and x.shape[0] == B * H * W and x.stride(1) == 1 and x.dtype == torch.float32
    assert feat0.shape == (B * H * W, E) and feat0.is_contiguous()
    c2 = torch.empty(B * H * W, F, dtype=torch.float32, device=x.device)
    keep, ptr, nbytes = L.ws_buffer(L.lib().srad_op_drct_ends_scratch_bytes(E, F), x.device)
    vec = [t.detach().float().contiguous() for t in (ln_g, ln_b, w1, b1)]
    w2c, b2c = w2.detach().float().contiguous(), b2.detach().float().contiguous()
    L.check(L.lib().srad_op_drct_body_end(L.dptr(x), x.stride(0), B, H, W, E, F, *[L.dptr(t) for t in vec], L.dptr(feat0), L.dptr(w2c),
                                          L.dptr(b2c), L.dptr(c2), ptr, nbytes, L.current_stream_ptr()), "op_drct_body_end")
    return c2


# ----------------------------------------------------------------------------------- backward operators
_WGRAD_WS = {}


def wgrad_workspace(device) -> C.c_void_p:
    """Zeroed-once split-K workspace of the weight-gradient kernel, one per device."""
    key = str(device)
    if key not in _WGRAD_WS:
        n = L.lib().srad_op_wgrad_workspace_bytes()
        _WGRAD_WS[key] = torch.zeros(n + 256, dtype=torch.uint8, device=device)
    t = _WGRAD_WS[key]
    return C.c_void_p(t.data_ptr() + (-t.data_ptr()) % 256)


def wq_wgrad(dy, x, dw, db, *, ntaps: int = 1, B: int = 1, H: int = 0, W: int = 0, stride: int = 1, alpha: float = 1.0):
    """Script step: an immediate weight gradient (Linear, or 3x3 with the image geometry) accumulated into dw [N, Cin, ntaps] / db."""
    if ntaps == 1 and stride == 1:
        B, H, W = 1, 1, x.shape[0]
    return (L.WQ_WGRAD, [dy.stride(0), x.stride(0), B, H, W, dw.shape[0], dw.shape[1], ntaps, stride], alpha, [dy, x, dw, db, None])


def wq_wgrad_deferred(dy, x, dw, db, *, row_scale=None, rps: int = 0, alpha: float = 1.0):
    """Script step: a Linear layer's weight gradient queued for the shared launch (dw [N, Cin])."""
    return (L.WQ_WGRAD_DEFERRED, [dy.stride(0), int(dy.dtype == torch.bfloat16), x.stride(0), int(x.dtype == torch.bfloat16), dy.shape[0],
                                  dw.shape[0], dw.shape[1], rps], alpha, [dy, x, dw, db, row_scale])


def wq_launch_deferred():
    return (L.WQ_LAUNCH_DEFERRED, [], 0.0, [])


def wq_flush():
    return (L.WQ_FLUSH, [], 0.0, [])


def wq_layernorm_bwd(dxn, x, gamma, out, dgamma, dbeta, *, dres=None, accumulate: bool = False):
    """Script step: LayerNorm backward over contiguous [rows, C] tensors (x may be a column block of wider rows)."""
    rows, Cc = dxn.shape
    return (L.WQ_LN_BWD, [x.stride(0), int(accumulate), rows, Cc], 0.0, [dxn, x, gamma, dres, out, dgamma, dbeta])


def wq_window_attention_bwd(qkv_padded, dout, dqkv, table, dtable, *, B: int, H: int, W: int, ws: int, shift: int, heads: int):
    """Script step: the fp32-operand attention backward; qkv_padded as ``pad_heads`` lays it out."""
    d = dout.shape[1]
    return (L.WQ_ATTN_BWD, [B, H, W, ws, shift, d, heads, qkv_padded.shape[1] // (3 * heads)], 0.0, [qkv_padded, dout, dqkv, table, dtable])


def pad_heads(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    """[T, 3d] q | k | v in the reference's column order -> the head-padded layout the attention kernels read."""
    hd = qkv.shape[1] // (3 * heads)
    hdp = (hd + 3) // 4 * 4
    return torch.nn.functional.pad(qkv.reshape(-1, 3 * heads, hd).float(), (0, hdp - hd)).reshape(-1, 3 * heads * hdp).contiguous()


def wgrad_queue_script(steps, *, precision: str = "fp32", budget_floats: Optional[int] = None, device=None):
    """Runs the steps (``wq_*`` above) through ONE split-K queue limited to ``budget_floats`` of the workspace (default: all of
    it), then the deferred launch and a flush (C ABI ``srad_op_wgrad_queue_script``).  Returns the reasons of the reduce
    launches it made, in order (``L.WQ_FLUSH_*``)."""
    device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    nbytes = L.lib().srad_op_wgrad_workspace_bytes()
    if budget_floats is None:
        budget_floats = nbytes // 4
    arr = (L.WqStep * len(steps))()
    keep = []
    for st, (kind, ints, alpha, ptrs) in zip(arr, steps):
        _need_cuda(*ptrs)
        st.kind, st.alpha = kind, alpha
        for j, v in enumerate(ints):
            st.i[j] = int(v)
        for j, t in enumerate(ptrs):
            st.p[j] = None if t is None else t.data_ptr()
        keep.append(ptrs)
    n = C.c_int(0)
    why = (C.c_int * 64)()
    L.check(L.lib().srad_op_wgrad_queue_script(L.PRECISIONS[precision], arr, len(steps), C.c_size_t(budget_floats), wgrad_workspace(device),
                                               C.c_size_t(nbytes), C.byref(n), why, 64, L.current_stream_ptr()), "op_wgrad_queue_script")
    return [int(why[i]) for i in range(min(n.value, 64))] + [-1] * max(0, n.value - 64)


WgradPlan = collections.namedtuple("WgradPlan", "families full grids precision conv launches reduce_tiles NT cpw nchunks layers")
WgradLayerPlan = collections.namedtuple("WgradLayerPlan", "launch ksplit rows_per tn tc XH YH blk0 nblk")


def _wgrad_plan_tuple(p: "L.WgradPlan") -> WgradPlan:
    """families / full / grids: one entry per launch; layers: one WgradLayerPlan per layer, in the order given."""
    layers = tuple(WgradLayerPlan(p.launch[i], p.ksplit[i], p.rows_per[i], p.tn[i], p.tc[i], bool(p.XH[i]), bool(p.YH[i]), p.blk0[i], p.nblk[i])
                   for i in range(p.count))
    n = p.launches
    return WgradPlan(tuple(L.WGRAD_FAMILIES[p.family[j]] for j in range(n)), tuple(bool(p.FULL[j]) for j in range(n)),
                     tuple(p.grid[j] for j in range(n)), ("fp32", "bf16")[p.precision], bool(p.CONV), n, p.reduce_tiles, p.NT, p.cpw,
                     p.nchunks, layers)


def _wgrad_geometry(rows: int, ntaps: int, stride: int, B: int, H: int, W: int):
    """A Linear layer is `rows` rows, or B samples of H * W rows when the caller gives them (row_scale is per sample)."""
    if ntaps == 1 and stride == 1 and H == 0:
        return 1, 1, rows
    return B, H, W


def wgrad(dy: torch.Tensor, x: torch.Tensor, N: int, Cin: int, *, ntaps: int = 1, B: int = 1, H: int = 0, W: int = 0,
          stride: int = 1, row_scale: Optional[torch.Tensor] = None, alpha: float = 1.0, bias: bool = True,
          precision: str = "fp32", n_real: Optional[int] = None, cin_real: Optional[int] = None, grp_real: int = 0,
          grp_pad: int = 0, ycol0: int = 0, dw: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None,
          plan_only: bool = False):
    """Weight / bias gradient of Linear (ntaps 1) or a 3x3 conv: dy [B*Ho*Wo, >= ycol0 + N], x [B*H*W, >= Cin] NHWC rows.
    Returns (dW [n_real, cin_real, ntaps], db [n_real] or None), freshly zeroed and accumulated into by the kernel - or the
    caller's ``dw`` / ``db`` (contiguous fp32 of that many elements, e.g. views into larger buffers), accumulated into.
    N, Cin: the stored channel counts (multiples of 4); n_real / cin_real: the extents of dW; grp_pad > 0: x holds groups of
    grp_pad channels with grp_real real ones each (C ABI ``srad_op_wgrad_ex``).  plan_only: launch nothing, return the WgradPlan."""
    _need_cuda(dy, x)
    assert dy.stride(1) == 1 and x.stride(1) == 1 and N % 4 == 0 and Cin % 4 == 0
    B, H, W = _wgrad_geometry(x.shape[0], ntaps, stride, B, H, W)
    n_real = N if n_real is None else n_real
    cin_real = Cin if cin_real is None else cin_real
    if plan_only:
        plan = L.WgradPlan()
        L.check(L.lib().srad_op_wgrad_plan(L.PRECISIONS[precision], L.dptr(dy), dy.stride(0), ycol0, int(dy.dtype == torch.bfloat16), L.dptr(x),
                                           x.stride(0), int(x.dtype == torch.bfloat16), B, H, W, N, Cin, n_real, cin_real, grp_real, grp_pad,
                                           ntaps, stride, L.dptr(row_scale), C.byref(plan)), "op_wgrad_plan")
        return _wgrad_plan_tuple(plan)
    if dw is None:
        dw = torch.zeros(n_real, cin_real, ntaps, dtype=torch.float32, device=x.device)
    if db is None and bias:
        db = torch.zeros(n_real, dtype=torch.float32, device=x.device)
    assert dw.is_contiguous() and dw.dtype == torch.float32 and dw.numel() == n_real * cin_real * ntaps
    assert db is None or (db.is_contiguous() and db.dtype == torch.float32 and db.numel() == n_real)
    L.check(L.lib().srad_op_wgrad_ex(L.PRECISIONS[precision], L.dptr(dy), dy.stride(0), ycol0, L.dptr(x), x.stride(0), B, H, W, N,
                                     Cin, n_real, cin_real, grp_real, grp_pad, ntaps, stride, L.dptr(row_scale), alpha, L.dptr(dw),
                                     L.dptr(db), wgrad_workspace(x.device), L.current_stream_ptr()), "op_wgrad")
    return dw, db


def wgrad_plan(dy: torch.Tensor, x: torch.Tensor, N: int, Cin: int, **kw) -> WgradPlan:
    """The kernel family, variant, row splits, tiles and grid that wgrad() with the same arguments runs (C ABI
    ``srad_op_wgrad_plan``): decided on the host by the launch's own functions, nothing is launched.  bf16 ``dy`` / ``x`` plan
    the bf16-storage kernels (wgrad_conv9_bf16)."""
    return wgrad(dy, x, N, Cin, plan_only=True, **kw)


def wgrad_plan_shape(precision: str, N: int, Cin: int, *, M: int = 0, ntaps: int = 1, stride: int = 1, B: int = 1, H: int = 0, W: int = 0,
                     ldy: Optional[int] = None, ldx: Optional[int] = None, ycol0: int = 0, n_real: Optional[int] = None,
                     cin_real: Optional[int] = None, grp_real: int = 0, grp_pad: int = 0, row_scale: bool = False, dy_bf16: bool = False,
                     x_bf16: bool = False) -> WgradPlan:
    """wgrad_plan from a shape alone, with aligned stand-in pointers that are never dereferenced: needs no GPU.  A Linear layer
    is M rows (or B samples of H * W rows); a conv is (B, H, W) input pixels."""
    fake = C.c_void_p(1 << 20)
    B, H, W = _wgrad_geometry(M, ntaps, stride, B, H, W)
    plan = L.WgradPlan()
    L.check(L.lib().srad_op_wgrad_plan(L.PRECISIONS[precision], fake, ycol0 + N if ldy is None else ldy, ycol0, int(dy_bf16), fake,
                                       Cin if ldx is None else ldx, int(x_bf16), B, H, W, N, Cin, N if n_real is None else n_real,
                                       Cin if cin_real is None else cin_real, grp_real, grp_pad, ntaps, stride,
                                       fake if row_scale else None, C.byref(plan)), "op_wgrad_plan")
    return _wgrad_plan_tuple(plan)


WGRAD_STORAGES = {"f32": (False, False), "xh": (True, False), "xh+yh": (True, True)}      # (X stored as bf16, dY stored as bf16)


def wgrad_deferred_plan(layers, precision: str = "bf16") -> WgradPlan:
    """The plan of 1 to 6 Linear layers queued for the shared launch one after the other and then sent (C ABI
    ``srad_op_wgrad_deferred_plan``).  A layer is a ``wq_wgrad_deferred`` step, or a shape ``(M, N, Cin, storage, rps)`` with
    storage one of WGRAD_STORAGES and rps the rows per row_scale entry (0: no row_scale) - that form needs no GPU."""
    fake = 1 << 20
    arr = (L.WqStep * len(layers))()
    for st, layer in zip(arr, layers):
        if len(layer) == 5:
            M, N, Cin, storage, rps = layer
            xh, yh = WGRAD_STORAGES[storage]
            ints, ptrs = [N, int(yh), Cin, int(xh), M, N, Cin, rps], [fake, fake, fake, fake, fake if rps else None]
        else:
            kind, ints, _, tensors = layer
            assert kind == L.WQ_WGRAD_DEFERRED
            ptrs = [None if t is None else t.data_ptr() for t in tensors]
        st.kind, st.alpha = L.WQ_WGRAD_DEFERRED, 1.0
        for j, v in enumerate(ints):
            st.i[j] = int(v)
        for j, v in enumerate(ptrs):
            st.p[j] = v
    plan = L.WgradPlan()
    L.check(L.lib().srad_op_wgrad_deferred_plan(L.PRECISIONS[precision], arr, len(layers), C.byref(plan)), "op_wgrad_deferred_plan")
    return _wgrad_plan_tuple(plan)


def conv80_bf16(x_h: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, B: int, H: int, W: int, act: int = 0,
                slope: float = 0.0, residual: Optional[torch.Tensor] = None, rmode: int = 0, out_bf16: bool = True,
                pool: bool = False):
    """The 80 -> 80 channel 3x3 convolution on a bf16 activation array, as DRN's bf16 chains run it (C ABI ``srad_op_conv80_h``):
    ``x_h`` [B*H*W, 80] bf16 NHWC rows, ``weight`` [80, 80, 3, 3]; ``residual`` bf16 or fp32 [B*H*W, 80] (rmode 0: added; 2: the
    output is multiplied by (residual > 0 ? 1 : slope)); output bf16 or fp32.  ``pool=True`` also returns the per-tile column
    sums [B*H*W/128, 80]."""
    _need_cuda(x_h, weight)
    assert x_h.dtype == torch.bfloat16 and x_h.is_contiguous() and x_h.shape == (B * H * W, 80)
    w = weight.detach().reshape(80, 80, 9).float().contiguous()
    y = torch.empty(B * H * W, 80, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x_h.device)
    part = torch.empty(B * H * W // 128, 80, dtype=torch.float32, device=x_h.device) if pool else None
    prec = L.PRECISIONS["bf16"]
    nbytes = L.lib().srad_op_gemm_scratch_bytes(prec, 80, 80, 9)
    scratch = torch.empty(nbytes + 256, dtype=torch.uint8, device=x_h.device)
    sp = C.c_void_p(scratch.data_ptr() + (-scratch.data_ptr()) % 256)
    r_h = residual if residual is not None and residual.dtype == torch.bfloat16 else None
    r_f = residual if residual is not None and residual.dtype == torch.float32 else None
    L.check(L.lib().srad_op_conv80_h(L.dptr(x_h), L.dptr(w), L.dptr(bias), act, slope, L.dptr(r_h), L.dptr(r_f), rmode, B, H, W,
                                     L.dptr(y) if out_bf16 else None, None if out_bf16 else L.dptr(y), L.dptr(part), sp, nbytes,
                                     L.current_stream_ptr()), "op_conv80_h")
    return (y, part) if pool else y


def wgrad_conv9_bf16(dy_h: torch.Tensor, x: torch.Tensor, *, B: int, H: int, W: int):
    """Weight / bias gradient of that convolution from a bf16 dY and a bf16 or fp32 X (C ABI ``srad_op_wgrad_conv9_h``):
    returns (dW [80, 80, 9], db [80])."""
    _need_cuda(dy_h, x)
    assert dy_h.dtype == torch.bfloat16 and dy_h.is_contiguous() and x.is_contiguous() and dy_h.shape == x.shape == (B * H * W, 80)
    dw = torch.zeros(80, 80, 9, dtype=torch.float32, device=x.device)
    db = torch.zeros(80, dtype=torch.float32, device=x.device)
    L.check(L.lib().srad_op_wgrad_conv9_h(L.dptr(dy_h), L.dptr(x), int(x.dtype == torch.bfloat16), B, H, W, L.dptr(dw), L.dptr(db),
                                          wgrad_workspace(x.device), L.current_stream_ptr()), "op_wgrad_conv9_h")
    return dw, db


def dgrad(dy: torch.Tensor, weight: torch.Tensor, *, B: int = 1, H: int = 0, W: int = 0, r: Optional[torch.Tensor] = None,
          rmode: int = 0, slope: float = 0.0, alpha: float = 1.0, row_scale: Optional[torch.Tensor] = None,
          precision: str = "fp32") -> torch.Tensor:
    """Data gradient dx = dy . W of Linear / 3x3 stride-1 conv (weight [N, Cin] or [N, Cin, 3, 3])."""
    _need_cuda(dy, weight)
    ntaps = 9 if weight.dim() == 4 and weight.shape[-1] == 3 else 1
    N, Cin = weight.shape[0], weight.shape[1]
    w = weight.detach().reshape(N, Cin, ntaps).float().contiguous()
    if ntaps == 1:
        B, H, W = 1, 1, dy.shape[0]
    dx = torch.empty(dy.shape[0], Cin, dtype=torch.float32, device=dy.device)
    prec = L.PRECISIONS[precision]
    nbytes = L.lib().srad_op_gemm_scratch_bytes(prec, Cin, N, ntaps)
    scratch = torch.empty(nbytes + 256, dtype=torch.uint8, device=dy.device)
    off = (-scratch.data_ptr()) % 256
    L.check(L.lib().srad_op_dgrad(prec, L.dptr(dy), dy.stride(0), B, H, W, N, L.dptr(w), Cin, ntaps, L.dptr(r),
                                  0 if r is None else r.stride(0), rmode, slope, alpha, L.dptr(row_scale), L.dptr(dx),
                                  dx.stride(0), C.c_void_p(scratch.data_ptr() + off), C.c_size_t(nbytes),
                                  L.current_stream_ptr()), "op_dgrad")
    return dx


def layernorm_bwd(dxn: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, dres: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None):
    """Returns (dx (+ dres, + out if given), dgamma, dbeta)."""
    _need_cuda(dxn, x, gamma)
    rows, Cc = dxn.shape
    acc = out is not None
    if out is None:
        out = torch.empty(rows, Cc, dtype=torch.float32, device=x.device)
    dg = torch.zeros(Cc, dtype=torch.float32, device=x.device)
    db = torch.zeros(Cc, dtype=torch.float32, device=x.device)
    L.check(L.lib().srad_op_layernorm_bwd(L.dptr(dxn.contiguous()), L.dptr(x), x.stride(0), L.dptr(gamma),
                                          L.dptr(None if dres is None else dres.contiguous()), L.dptr(out), 1 if acc else 0,
                                          L.dptr(dg), L.dptr(db), rows, Cc, wgrad_workspace(x.device),
                                          L.current_stream_ptr()), "op_layernorm_bwd")
    return out, dg, db


def window_attention_bwd(qkv: torch.Tensor, dout: torch.Tensor, table: torch.Tensor, B: int, H: int, W: int, ws: int,
                         shift: int, heads: int, precision: str = "fp32"):
    """Backward of window_attention: qkv [T, 3d] (reference column order), dout [T, d] -> (dqkv [T, 3d], dtable)."""
    _need_cuda(qkv, dout, table)
    d = qkv.shape[1] // 3
    hd = d // heads
    hdp = (hd + 3) // 4 * 4
    padded = torch.nn.functional.pad(qkv.reshape(-1, 3 * heads, hd).float(), (0, hdp - hd)).reshape(-1, 3 * heads * hdp).contiguous()
    dqkv = torch.empty(qkv.shape[0], 3 * d, dtype=torch.float32, device=qkv.device)
    dtable = torch.zeros_like(table, dtype=torch.float32).contiguous()
    L.check(L.lib().srad_op_window_attn_bwd(L.PRECISIONS[precision], L.dptr(padded), L.dptr(dout.contiguous()), L.dptr(dqkv), L.dptr(table.contiguous()),
                                            L.dptr(dtable), B, H, W, ws, shift, d, heads, hdp, wgrad_workspace(qkv.device),
                                            L.current_stream_ptr()),
            "op_window_attn_bwd")
    return dqkv, dtable


def wgrad_linear_deferred(dy: torch.Tensor, x: torch.Tensor, row_scale: Optional[torch.Tensor] = None, rps: int = 0,
                          alpha: float = 1.0, bias: bool = True, precision: str = "bf16"):
    """dW [N, Cin] (and db [N]) of a Linear layer from dy [M, N] and x [M, Cin], issued the way the training step does
    (deferred launch + reduce).  fp32 or bf16 operand tensors (bf16 dy: already scaled, needs a bf16 x)."""
    _need_cuda(dy, x)
    M, N = dy.shape
    Cin = x.shape[1]
    dw = torch.zeros(N, Cin, dtype=torch.float32, device=dy.device)
    db = torch.zeros(N, dtype=torch.float32, device=dy.device) if bias else None
    dy, x = dy.contiguous(), x.contiguous()
    L.check(L.lib().srad_op_wgrad_deferred(L.PRECISIONS[precision], L.dptr(dy), N, int(dy.dtype == torch.bfloat16), L.dptr(x), Cin,
                                           int(x.dtype == torch.bfloat16), M, N, Cin, L.dptr(row_scale), rps, alpha, L.dptr(dw), L.dptr(db),
                                           wgrad_workspace(dy.device), L.current_stream_ptr()), "op_wgrad_deferred")
    return dw, db


def window_attention_bwd_bf16io(qkv: torch.Tensor, dout: torch.Tensor, table: torch.Tensor, B: int, H: int, W: int, ws: int,
                                shift: int, heads: int, pad_fill: float = float("nan")):
    """The training step's form of ``window_attention_bwd`` (head dim <= 128): the operands cross the boundary as bf16 in
    per-head slots of ``hp = ceil8(head dim)`` columns - q already scaled, as the fused forward saves it - and dq | dk | dv
    come back as bf16.  ``pad_fill`` goes into dO's padding columns, which the kernel must ignore."""
    _need_cuda(qkv, dout, table)
    d = qkv.shape[1] // 3
    hd = d // heads
    hp = (hd + 7) // 8 * 8
    T = qkv.shape[0]
    q3 = qkv.reshape(T, 3, heads, hd).float().clone()
    q3[:, 0] *= hd ** -0.5
    qkv_h = torch.zeros(T, 3, heads, hp, dtype=torch.bfloat16, device=qkv.device)
    qkv_h[..., :hd] = q3.to(torch.bfloat16)
    dout_h = torch.full((T, heads, hp), pad_fill, dtype=torch.bfloat16, device=qkv.device)
    dout_h[..., :hd] = dout.reshape(T, heads, hd).to(torch.bfloat16)
    dqkv_h = torch.empty(T, 3 * d, dtype=torch.bfloat16, device=qkv.device)
    dtable = torch.zeros_like(table, dtype=torch.float32).contiguous()
    L.check(L.lib().srad_op_window_attn_bwd_h(L.dptr(qkv_h), L.dptr(dout_h), L.dptr(dqkv_h), L.dptr(table.contiguous()), L.dptr(dtable),
                                              B, H, W, ws, shift, d, heads, hp, wgrad_workspace(qkv.device), L.current_stream_ptr()),
            "op_window_attn_bwd_h")
    return dqkv_h.float(), dtable


def mlp_bwd(dx2: Optional[torch.Tensor], hpre: torch.Tensor, x1: torch.Tensor, gamma: torch.Tensor, w_fc1: torch.Tensor,
            w_fc2: torch.Tensor, rs2: Optional[torch.Tensor] = None, rps: int = 0, adjust=None, proj=None):
    """Fused backward of a Swin block's MLP branch (bf16 MFMA, C ABI ``srad_op_mlp_bwd``; src/drct.py:510, 184-190).

    ``dx2`` [M, d] is the gradient of ``x2 = x1 + rs2 * fc2(gelu(fc1(LN(x1))))``, or None when ``adjust`` =
    ``(dA [M, KA], y_act [M, KA] or None, slope, alpha, w_adj [KA, d])`` is given: then dx2 = alpha * (dA * lrelu'(y_act)) @ w_adj
    is computed first.  ``proj`` = ``(w_proj [d, d], rs1 or None)`` adds dO = (dx1 @ w_proj) * rs1.
    Returns a dict: dh [M, m], dx1 [M, d], dgamma, dbeta, and dx2 / dA (adjust) / dO (proj)."""
    _need_cuda(hpre, x1, gamma, w_fc1, w_fc2)
    M, d = x1.shape
    m = hpre.shape[1]
    dev = x1.device
    f = lambda t: None if t is None else t.detach().float().contiguous()
    out = {"dh": torch.empty(M, m, dtype=torch.float32, device=dev), "dx1": torch.empty(M, d, dtype=torch.float32, device=dev),
           "dgamma": torch.zeros(d, dtype=torch.float32, device=dev), "dbeta": torch.zeros(d, dtype=torch.float32, device=dev)}
    KA, dA, y_act, slope, alpha, w_adj, dA_out = 0, None, None, 0.0, 1.0, None, None
    if adjust is not None:
        dA, y_act, slope, alpha, w_adj = adjust
        dA, y_act, w_adj = f(dA), f(y_act), f(w_adj)
        KA = dA.shape[1]
        dx2 = torch.empty(M, d, dtype=torch.float32, device=dev)
        dA_out = torch.empty(M, KA, dtype=torch.float32, device=dev)
        out["dA"] = dA_out
    else:
        dx2 = f(dx2).clone()
    out["dx2"] = dx2
    w_proj, rs1, dO = None, None, None
    if proj is not None:
        w_proj, rs1 = f(proj[0]), f(proj[1])
        dO = out["dO"] = torch.empty(M, d, dtype=torch.float32, device=dev)
    keep = [f(hpre), f(x1), f(gamma), f(w_fc1), f(w_fc2), f(rs2)]
    nbytes = L.lib().srad_op_mlp_bwd_scratch_bytes(d, m, KA)
    sbuf, sp, sb = L.ws_buffer(nbytes, dev)
    L.check(L.lib().srad_op_mlp_bwd(M, d, m, L.dptr(dx2), L.dptr(keep[0]), L.dptr(keep[1]), L.dptr(keep[2]), L.dptr(keep[3]),
                                    L.dptr(keep[4]), L.dptr(keep[5]), int(rps), L.dptr(out["dh"]), L.dptr(out["dx1"]),
                                    L.dptr(out["dgamma"]), L.dptr(out["dbeta"]), KA, L.dptr(dA), KA, L.dptr(y_act), KA,
                                    float(slope), float(alpha), L.dptr(w_adj), L.dptr(dA_out), L.dptr(w_proj), L.dptr(rs1),
                                    L.dptr(dO), sp, sb, wgrad_workspace(dev), L.current_stream_ptr()), "op_mlp_bwd")
    return out


def lin_ln_bwd(dy: torch.Tensor, w: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, dres: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None):
    """Data gradient of ``Linear(w [K, d])`` applied to ``LayerNorm(x)`` plus the LayerNorm backward, one launch
    (bf16 MFMA, ``srad_op_lin_ln_bwd``): returns (dres + LN'(dy @ w) (+ out if given), dgamma, dbeta)."""
    _need_cuda(dy, w, x, gamma)
    M, K = dy.shape
    d = w.shape[1]
    dev = x.device
    acc = out is not None
    if out is None:
        out = torch.empty(M, d, dtype=torch.float32, device=dev)
    dg = torch.zeros(d, dtype=torch.float32, device=dev)
    db = torch.zeros(d, dtype=torch.float32, device=dev)
    keep = [dy.detach().float().contiguous(), w.detach().float().contiguous(), gamma.detach().float().contiguous(),
            None if dres is None else dres.detach().float().contiguous()]
    nbytes = L.lib().srad_op_lin_ln_bwd_scratch_bytes(K, d)
    sbuf, sp, sb = L.ws_buffer(nbytes, dev)
    L.check(L.lib().srad_op_lin_ln_bwd(M, K, d, L.dptr(keep[0]), L.dptr(keep[1]), L.dptr(x), x.stride(0), L.dptr(keep[2]),
                                       L.dptr(keep[3]), L.dptr(out), out.stride(0), 1 if acc else 0, L.dptr(dg), L.dptr(db),
                                       sp, sb, wgrad_workspace(dev), L.current_stream_ptr()), "op_lin_ln_bwd")
    return out, dg, db


# ----------------------------------------------------------------------------------- C5: the 64 x 64-window attention's two kernels
def ln_qkv(x: torch.Tensor, ln_g: torch.Tensor, ln_b: torch.Tensor, w_qkv: torch.Tensor, b_qkv: torch.Tensor, heads: int,
           ws: int = 64, shift: int = 0) -> torch.Tensor:
    """norm1 + attn.qkv in one launch (``srad_op_ln_qkv``; src/drct.py:477, 278) -> the bf16 operands of the 64 x 64-window
    attention, [M, 3, heads, hdp]: q times head_dim^-0.5 log2 e, padding 0, column head_dim of the v slices 1."""
    _need_cuda(x, ln_g, ln_b, w_qkv, b_qkv)
    d = w_qkv.shape[1]
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32 and w_qkv.shape[0] == 3 * d
    qs = L.lib().srad_op_window_attn_qscale(ws, shift, d, heads)
    if qs == 0.0:
        raise ValueError(f"window {ws} / shift {shift} / head dim {d // heads}: not the bf16-operand attention path")
    hdp = (d // heads + 3) // 4 * 4
    f = lambda t: t.detach().float().contiguous()
    keep = [f(ln_g), f(ln_b), f(w_qkv), f(b_qkv)]
    out = torch.empty(x.shape[0], 3, heads, hdp, dtype=torch.bfloat16, device=x.device)
    sbuf, sp, sb = L.ws_buffer(L.lib().srad_op_ln_qkv_scratch_bytes(d, heads), x.device)
    L.check(L.lib().srad_op_ln_qkv(L.dptr(x), x.stride(0), x.shape[0], d, heads, L.dptr(keep[0]), L.dptr(keep[1]), L.dptr(keep[2]),
                                   L.dptr(keep[3]), L.dptr(out), hdp, float(qs), sp, sb, L.current_stream_ptr()), "op_ln_qkv")
    return out


def window_attention_bf16_in(qkv_h: torch.Tensor, table: torch.Tensor, B: int, H: int, W: int, ws: int, shift: int, d: int) -> torch.Tensor:
    """WindowAttention on ``ln_qkv``'s operands (``srad_op_window_attn_bf16_in``; src/drct.py:281-299, 482-504) -> [B*H*W, d] fp32."""
    _need_cuda(qkv_h, table)
    T, three, heads, hdp = qkv_h.shape
    assert three == 3 and T == B * H * W and qkv_h.dtype == torch.bfloat16 and qkv_h.is_contiguous()
    tb = table.detach().float().contiguous()
    out = torch.empty(T, d, dtype=torch.float32, device=qkv_h.device)
    L.check(L.lib().srad_op_window_attn_bf16_in(L.dptr(qkv_h), L.dptr(out), L.dptr(tb), B, H, W, ws, shift, d, heads, hdp,
                                                L.current_stream_ptr()), "op_window_attn_bf16_in")
    return out


# ----------------------------------------------------------------------------------- fused Swin-block halves (bf16, window 8)
def qkv_attn(x: torch.Tensor, ln_g: torch.Tensor, ln_b: torch.Tensor, w_qkv: torch.Tensor, b_qkv: torch.Tensor,
             table: torch.Tensor, B: int, H: int, W: int, shift: int, heads: int, out_bf16: bool = False,
             precision: str = "bf16") -> torch.Tensor:
    """First half of a Swin block in ONE launch (``srad_op_qkv_attn``; src/drct.py:477-504 up to attn.proj, 271-299):
    x [B*H*W, >=d] block input rows (columns [0, d) are read), w_qkv [3d, d], table [225, heads] -> attention output
    [B*H*W, d] in token order (window partition, cyclic shift and their inverses are index arithmetic inside); fp32, or
    with ``out_bf16`` the bf16 tensor the engines hand to ``mlp_block``.  precision "bf16" or "bf16x3" (split-bf16: fp32 out)."""
    _need_cuda(x, ln_g, ln_b, w_qkv, b_qkv, table)
    d = w_qkv.shape[1]
    assert x.dim() == 2 and x.shape[0] == B * H * W and x.stride(1) == 1 and x.dtype == torch.float32 and w_qkv.shape[0] == 3 * d
    f = lambda t: t.detach().float().contiguous()
    keep = [f(ln_g), f(ln_b), f(w_qkv), f(b_qkv), f(table)]
    out = torch.empty(x.shape[0], d, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x.device)
    sbuf, sp, sb = L.ws_buffer(L.lib().srad_op_swin_scratch_bytes(d, heads, 4, 4), x.device)
    L.check(L.lib().srad_op_qkv_attn(L.PRECISIONS[precision], L.dptr(x), x.stride(0), B, H, W, shift, d, heads, L.dptr(keep[0]), L.dptr(keep[1]),
                                     L.dptr(keep[2]), L.dptr(keep[3]), L.dptr(keep[4]), L.dptr(out), int(out_bf16), sp, sb,
                                     L.current_stream_ptr()), "op_qkv_attn")
    return out


def qkv_attn_grid(B: int, H: int, W: int, d: int, heads: int, no_qsplit: bool = False, precision: str = "bf16") -> tuple:
    """The grid (x, y) ``qkv_attn`` and the engines launch for this shape on the current device (``srad_qkv_attn_grid``):
    (windows, heads), or (windows, 2 heads) for the query split when that leaves fewer workgroups than CUs."""
    g = (C.c_int * 2)()
    L.check(L.lib().srad_qkv_attn_grid(L.PRECISIONS[precision], B, H, W, d, heads, int(no_qsplit), g), "qkv_attn_grid")
    return g[0], g[1]


def qkv_attn_train(x: torch.Tensor, ln_g, ln_b, w_qkv, b_qkv, table, B: int, H: int, W: int, shift: int, heads: int,
                   hdp: int, hp_h: int, no_qsplit: bool = False, fill: float = 0.0) -> dict:
    """``qkv_attn`` (bf16 out) with every save the training forward can ask for (``srad_op_qkv_attn_train``): LN1(x) as
    fp32 and bf16 [T, d], q | k | v as fp32 [T, 3, heads, hdp] (q unscaled) and as bf16 [T, 3, heads, hp_h] (as the
    attention used them).  The save buffers start as ``fill``; ``no_qsplit`` forces the plain (windows, heads) grid."""
    _need_cuda(x, ln_g, ln_b, w_qkv, b_qkv, table)
    d = w_qkv.shape[1]
    T = B * H * W
    assert x.dim() == 2 and x.shape[0] == T and x.stride(1) == 1 and x.dtype == torch.float32 and w_qkv.shape[0] == 3 * d
    f = lambda t: t.detach().float().contiguous()
    keep = [f(ln_g), f(ln_b), f(w_qkv), f(b_qkv), f(table)]
    dev = x.device
    r = {"out_h": torch.full((T, d), fill, dtype=torch.bfloat16, device=dev),
         "xn": torch.full((T, d), fill, dtype=torch.float32, device=dev),
         "xn_h": torch.full((T, d), fill, dtype=torch.bfloat16, device=dev),
         "qkv": torch.full((T, 3, heads, hdp), fill, dtype=torch.float32, device=dev),
         "qkv_h": torch.full((T, 3, heads, hp_h), fill, dtype=torch.bfloat16, device=dev)}
    sbuf, sp, sb = L.ws_buffer(L.lib().srad_op_swin_scratch_bytes(d, heads, 4, 4), dev)
    L.check(L.lib().srad_op_qkv_attn_train(L.dptr(x), x.stride(0), B, H, W, shift, d, heads, *[L.dptr(k) for k in keep],
                                           L.dptr(r["out_h"]), L.dptr(r["xn"]), L.dptr(r["xn_h"]), L.dptr(r["qkv"]), hdp,
                                           L.dptr(r["qkv_h"]), hp_h, int(no_qsplit), sp, sb, L.current_stream_ptr()), "op_qkv_attn_train")
    return r


def mlp_block(attn: torch.Tensor, shortcut: torch.Tensor, w_proj, b_proj, ln_g, ln_b, w_fc1, b_fc1, w_fc2, b_fc2, w_adj, b_adj, *,
              act: int = L.ACT_LRELU, slope: float = 0.2, alpha: float = 1.0, residual: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None, out_offset: int = 0, fm: int = 0, precision: str = "bf16") -> torch.Tensor:
    """Second half of a Swin block + the RDG's 1x1 adjust conv in ONE launch (``srad_op_mlp_block``; src/drct.py:300,
    509-510, 184-190, 389-396).  attn [M, d] (crosses the boundary as bf16 - the operand the MFMA takes; an fp32 tensor is
    rounded here; with precision "bf16x3" it crosses as fp32), shortcut [M, >=d]; returns / fills out[:, out_offset:out_offset+no]."""
    _need_cuda(attn, shortcut, w_proj, w_fc1, w_fc2, w_adj)
    M, d = attn.shape
    m, no = w_fc1.shape[0], w_adj.shape[0]
    f = lambda t: t.detach().float().contiguous()
    keep = [f(w_proj), f(b_proj), f(ln_g), f(ln_b), f(w_fc1), f(b_fc1), f(w_fc2), f(b_fc2), f(w_adj.reshape(no, d)), f(b_adj)]
    attn = attn.detach().to(torch.float32 if L.PRECISIONS[precision] == L.PREC_BF16X3 else torch.bfloat16).contiguous()
    if out is None:
        out = torch.empty(M, no, dtype=torch.float32, device=attn.device)
    sbuf, sp, sb = L.ws_buffer(L.lib().srad_op_swin_scratch_bytes(d, 1, m, no), attn.device)
    L.check(L.lib().srad_op_mlp_block(L.PRECISIONS[precision], M, d, m, no, int(fm), L.dptr(attn), L.dptr(shortcut), shortcut.stride(0), *[L.dptr(k) for k in keep],
                                      int(act), float(slope), float(alpha), L.dptr(residual), 0 if residual is None else residual.stride(0),
                                      L.dptr(out), out.stride(0), int(out_offset), sp, sb, L.current_stream_ptr()), "op_mlp_block")
    return out


def swin_block_supported(B: int, H: int, W: int, d: int, heads: int, hidden: int, no: int, ws: int = 8, precision: str = "bf16") -> bool:
    """Does the one-launch Swin block kernel take this shape on the current device (``srad_swin_block_supported``)?"""
    return bool(L.lib().srad_swin_block_supported(L.PRECISIONS[precision], ws, B, H, W, d, heads, hidden, no))


def swin_block(x: torch.Tensor, ln1_g, ln1_b, w_qkv, b_qkv, table, w_proj, b_proj, ln2_g, ln2_b, w_fc1, b_fc1, w_fc2, b_fc2, w_adj, b_adj,
               B: int, H: int, W: int, shift: int, heads: int, *, act: int = L.ACT_LRELU, slope: float = 0.2, alpha: float = 1.0,
               residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, out_offset: int = 0,
               precision: str = "bf16") -> torch.Tensor:
    """A whole Swin block + the RDG's 1x1 adjust conv in ONE launch (``srad_op_swin_block``): ``qkv_attn`` followed by
    ``mlp_block`` with x [B*H*W, >=d] as the shortcut.  bf16, 8 x 8 windows, B * H/8 * W/8 * 4 <= the device's CUs; anything
    else raises.  Returns / fills out[:, out_offset:out_offset+no]; ``out`` may be x itself with out_offset >= d."""
    _need_cuda(x, w_qkv, w_proj, w_fc1, w_fc2, w_adj)
    d = w_qkv.shape[1]
    m, no = w_fc1.shape[0], w_adj.shape[0]
    assert x.dim() == 2 and x.shape[0] == B * H * W and x.stride(1) == 1 and x.dtype == torch.float32 and w_qkv.shape[0] == 3 * d
    f = lambda t: t.detach().float().contiguous()
    keep = [f(ln1_g), f(ln1_b), f(w_qkv), f(b_qkv), f(table), f(w_proj), f(b_proj), f(ln2_g), f(ln2_b), f(w_fc1), f(b_fc1), f(w_fc2), f(b_fc2),
            f(w_adj.reshape(no, d)), f(b_adj)]
    if out is None:
        out = torch.empty(x.shape[0], no, dtype=torch.float32, device=x.device)
    sbuf, sp, sb = L.ws_buffer(L.lib().srad_op_swin_scratch_bytes(d, heads, m, no), x.device)
    L.check(L.lib().srad_op_swin_block(L.PRECISIONS[precision], L.dptr(x), x.stride(0), B, H, W, shift, d, heads, m, no, *[L.dptr(k) for k in keep],
                                       int(act), float(slope), float(alpha), L.dptr(residual), 0 if residual is None else residual.stride(0),
                                       L.dptr(out), out.stride(0), int(out_offset), sp, sb, L.current_stream_ptr()), "op_swin_block")
    return out


def mlp_fold_compose(w_fc2: torch.Tensor, b_fc2: torch.Tensor, w_adj: torch.Tensor, b_adj: torch.Tensor) -> dict:
    """The folded second-half weight of a Swin block built on the device (``srad_op_mlp_fold_compose``): ``wf`` fp32
    [no, 32 (ceil(d / 32) + ceil(m / 32))] = [A | A W2] with both parts zero-padded to whole 32-wide chunks, ``bias`` fp32 [no] =
    A b2 + b_a, ``pack`` (the bf16 fragment pack, raw bytes), ``kc32`` (the column where the A W2 part starts)."""
    _need_cuda(w_fc2, b_fc2, w_adj, b_adj)
    d, m = w_fc2.shape
    no = w_adj.shape[0]
    f = lambda t: t.detach().float().contiguous()
    keep = [f(w_fc2), f(b_fc2), f(w_adj.reshape(no, d)), f(b_adj)]
    lib = L.lib()
    sbuf, sp, sb = L.ws_buffer(lib.srad_op_mlp_fold_scratch_bytes(d, m, no), w_fc2.device)
    offs = [C.c_size_t() for _ in range(3)]
    kf = C.c_int()
    L.check(lib.srad_op_mlp_fold_compose(d, m, no, *[L.dptr(t) for t in keep], sp, sb, *[C.byref(o) for o in offs], C.byref(kf),
                                         L.current_stream_ptr()), "op_mlp_fold_compose")
    base = sp.value - sbuf.data_ptr()

    def view(off, nbytes, dtype):
        return sbuf[base + off:base + off + nbytes].view(dtype)
    wf = view(offs[0].value, no * kf.value * 4, torch.float32).reshape(no, kf.value)
    pack_bytes = (no + 127) // 128 * 128 * kf.value * 2
    return {"wf": wf, "bias": view(offs[2].value, no * 4, torch.float32), "pack": view(offs[1].value, pack_bytes, torch.uint8),
            "kc32": 32 * ((d + 31) // 32), "buf": sbuf}


def swin_block_fold_supported(B: int, H: int, W: int, d: int, heads: int, hidden: int, no: int, ws: int = 8, precision: str = "bf16") -> bool:
    """Does the one-launch Swin block kernel have a folded form for this shape (``srad_swin_block_fold_supported``)?"""
    return bool(L.lib().srad_swin_block_fold_supported(L.PRECISIONS[precision], ws, B, H, W, d, heads, hidden, no))


def swin_block_folded(x: torch.Tensor, ln1_g, ln1_b, w_qkv, b_qkv, table, w_proj, b_proj, ln2_g, ln2_b, w_fc1, b_fc1, w_fc2, b_fc2, w_adj, b_adj,
                      B: int, H: int, W: int, shift: int, heads: int, *, act: int = L.ACT_LRELU, slope: float = 0.2, alpha: float = 1.0,
                      residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, out_offset: int = 0,
                      precision: str = "bf16") -> torch.Tensor:
    """``swin_block`` with fc2 folded into the adjust conv (``srad_op_swin_block_folded``; inference): the same arguments and
    the same result up to rounding - adjust(x1 + fc2(h) + b2) as one GEMM [A | A W2] [x1 | h] + (A b2 + b_a)."""
    _need_cuda(x, w_qkv, w_proj, w_fc1, w_fc2, w_adj)
    d = w_qkv.shape[1]
    m, no = w_fc1.shape[0], w_adj.shape[0]
    assert x.dim() == 2 and x.shape[0] == B * H * W and x.stride(1) == 1 and x.dtype == torch.float32 and w_qkv.shape[0] == 3 * d
    f = lambda t: t.detach().float().contiguous()
    keep = [f(ln1_g), f(ln1_b), f(w_qkv), f(b_qkv), f(table), f(w_proj), f(b_proj), f(ln2_g), f(ln2_b), f(w_fc1), f(b_fc1), f(w_fc2), f(b_fc2),
            f(w_adj.reshape(no, d)), f(b_adj)]
    if out is None:
        out = torch.empty(x.shape[0], no, dtype=torch.float32, device=x.device)
    lib = L.lib()
    sbuf, sp, sb = L.ws_buffer(lib.srad_op_swin_scratch_bytes(d, heads, m, no) + lib.srad_op_mlp_fold_scratch_bytes(d, m, no), x.device)
    L.check(lib.srad_op_swin_block_folded(L.PRECISIONS[precision], L.dptr(x), x.stride(0), B, H, W, shift, d, heads, m, no, *[L.dptr(k) for k in keep],
                                          int(act), float(slope), float(alpha), L.dptr(residual), 0 if residual is None else residual.stride(0),
                                          L.dptr(out), out.stride(0), int(out_offset), sp, sb, L.current_stream_ptr()), "op_swin_block_folded")
    return out


def mlp_block_fold_supported(T: int, d: int, hidden: int, no: int, precision: str = "bf16") -> bool:
    """Does a ``mlp_block`` launch of T rows have a folded form at the tile height it picks (``srad_mlp_block_fold_supported``)?"""
    return bool(L.lib().srad_mlp_block_fold_supported(L.PRECISIONS[precision], T, d, hidden, no))


def mlp_block_folded(attn: torch.Tensor, shortcut: torch.Tensor, w_proj, b_proj, ln_g, ln_b, w_fc1, b_fc1, w_fc2, b_fc2, w_adj, b_adj, *,
                     act: int = L.ACT_LRELU, slope: float = 0.2, alpha: float = 1.0, residual: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None, out_offset: int = 0, fm: int = 0, precision: str = "bf16") -> torch.Tensor:
    """``mlp_block`` with fc2 folded into the adjust conv (``srad_op_mlp_block_folded``; bf16 inference): the same arguments and
    the same result up to rounding - adjust(x1 + fc2(h) + b2) as one GEMM [A | A W2] [x1 | h] + (A b2 + b_a)."""
    _need_cuda(attn, shortcut, w_proj, w_fc1, w_fc2, w_adj)
    M, d = attn.shape
    m, no = w_fc1.shape[0], w_adj.shape[0]
    f = lambda t: t.detach().float().contiguous()
    keep = [f(w_proj), f(b_proj), f(ln_g), f(ln_b), f(w_fc1), f(b_fc1), f(w_fc2), f(b_fc2), f(w_adj.reshape(no, d)), f(b_adj)]
    attn = attn.detach().to(torch.bfloat16).contiguous()
    if out is None:
        out = torch.empty(M, no, dtype=torch.float32, device=attn.device)
    lib = L.lib()
    sbuf, sp, sb = L.ws_buffer(lib.srad_op_swin_scratch_bytes(d, 1, m, no) + lib.srad_op_mlp_fold_scratch_bytes(d, m, no), attn.device)
    L.check(lib.srad_op_mlp_block_folded(L.PRECISIONS[precision], M, d, m, no, int(fm), L.dptr(attn), L.dptr(shortcut), shortcut.stride(0),
                                         *[L.dptr(k) for k in keep], int(act), float(slope), float(alpha), L.dptr(residual),
                                         0 if residual is None else residual.stride(0), L.dptr(out), out.stride(0), int(out_offset), sp, sb,
                                         L.current_stream_ptr()), "op_mlp_block_folded")
    return out


# ----------------------------------------------------------------------------------- self-ensemble x8
def _ensemble_arg(t: torch.Tensor, what: str) -> torch.Tensor:
    _need_cuda(t)
    if t.dim() != 4 or t.dtype != torch.float32:
        raise ValueError(f"{what}: expected a 4-d fp32 tensor, got {tuple(t.shape)} {t.dtype}")
    return t.detach().contiguous()


def ensemble_batches(x: torch.Tensor) -> list:
    """The forward batches of the self-ensemble of x [B,C,H,W] (DESIGN.md "Self-ensemble"), filled by one launch
    (``srad_ensemble_inputs``): for square input one stacked [8B,C,H,W] tensor, otherwise members 0..3 as [4B,C,H,W] and
    members 4..7 as [4B,C,W,H].  Image b of member t is at index t*B + b of the stack (t - 4 in the second tensor)."""
    x = _ensemble_arg(x, "ensemble_inputs")
    B, Cc, H, W = x.shape
    if H == W:
        batches = [torch.empty(8 * B, Cc, H, W, dtype=torch.float32, device=x.device)]
        a, b = batches[0][:4 * B], batches[0][4 * B:]
    else:
        batches = [torch.empty(4 * B, Cc, H, W, dtype=torch.float32, device=x.device),
                   torch.empty(4 * B, Cc, W, H, dtype=torch.float32, device=x.device)]
        a, b = batches
    L.check(L.lib().srad_ensemble_inputs(L.dptr(x), B, Cc, H, W, L.dptr(a), L.dptr(b), L.current_stream_ptr()), "ensemble_inputs")
    return batches


def ensemble_inputs(x: torch.Tensor) -> tuple:
    """(a, b): members 0..3 of x [B,C,H,W] as [4B,C,H,W] and members 4..7 as [4B,C,W,H]; for square input both are views of
    one [8B,C,H,W] allocation (``ensemble_batches``)."""
    batches = ensemble_batches(x)
    if len(batches) == 1:
        n = batches[0].shape[0] // 2
        return batches[0][:n], batches[0][n:]
    return batches[0], batches[1]


def ensemble_mean(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a [4B,C,H,W] and b [4B,C,W,H], the network's outputs for members 0..3 and 4..7 -> [B,C,H,W]: every member's
    transform undone, then ``(((z0 + z1) + z2) + ... + z7) * 0.125`` in fp32 (``srad_ensemble_mean``)."""
    a, b = _ensemble_arg(a, "ensemble_mean"), _ensemble_arg(b, "ensemble_mean")
    n, Cc, H, W = a.shape
    if n % 4 or tuple(b.shape) != (n, Cc, W, H):
        raise ValueError(f"ensemble_mean: {tuple(a.shape)} and {tuple(b.shape)} are not the two halves of an x8 ensemble")
    out = torch.empty(n // 4, Cc, H, W, dtype=torch.float32, device=a.device)
    L.check(L.lib().srad_ensemble_mean(L.dptr(a), L.dptr(b), n // 4, Cc, H, W, L.dptr(out), L.current_stream_ptr()), "ensemble_mean")
    return out


# ----------------------------------------------------------------------------------- tiled inference
TilePlan = collections.namedtuple("TilePlan", "h w tile overlap granule scale ph pw ty tx stride ny nx oy ox")
TilePlan.__doc__ = """The cover of an LR image [h, w] with tiles (include/srad.h ``srad_tile_geom`` + the origins): padded extents
ph x pw, tile extents ty x tx, ny x nx tiles at the origins oy / ox, numbered row-major."""


def tile_plan(h: int, w: int, tile: int, overlap: int = 0, granule: int = 1, scale: int = 1) -> TilePlan:
    """The tile cover both kernels use (``srad_tile_plan``; host only, needs no GPU).  ValueError for what the library refuses:
    tile < 1, overlap outside [0, tile), tile % granule != 0, overlap * scale > 4094."""
    g = L.TileGeom()
    if L.lib().srad_tile_plan(int(h), int(w), int(tile), int(overlap), int(granule), int(scale), C.byref(g)):
        raise ValueError(L.lib().srad_last_error().decode())
    oy, ox = (C.c_int32 * g.ny)(), (C.c_int32 * g.nx)()
    L.check(L.lib().srad_tile_origins(C.byref(g), oy, ox), "tile_origins")
    return TilePlan(*[getattr(g, n) for n, _ in L.TileGeom._fields_], tuple(oy), tuple(ox))


def _tile_arg(t: torch.Tensor, what: str) -> torch.Tensor:
    _need_cuda(t)
    if t.dim() != 4 or t.dtype != torch.float32:
        raise ValueError(f"{what}: expected a 4-d fp32 tensor, got {tuple(t.shape)} {t.dtype}")
    return t.detach()


def tile_gather(x: torch.Tensor, tile: int, overlap: int = 0, granule: int = 1) -> torch.Tensor:
    """x [B,C,h,w] -> its tiles [B*ny*nx, C, ty, tx] under ``tile_plan(h, w, tile, overlap, granule)``, the symmetric padding
    included (``srad_tile_gather``): a pure copy."""
    x = _tile_arg(x, "tile_gather")
    B, Cc, h, w = x.shape
    plan = tile_plan(h, w, tile, overlap, granule)            # its refusals come before any GPU work
    x = x.contiguous()
    tiles = torch.empty(B * plan.ny * plan.nx, Cc, plan.ty, plan.tx, dtype=torch.float32, device=x.device)
    L.check(L.lib().srad_tile_gather(L.dptr(x), B, Cc, h, w, int(tile), int(overlap), int(granule), L.dptr(tiles), L.current_stream_ptr()),
            "tile_gather")
    return tiles


def tile_blend(y: torch.Tensor, h: int, w: int, tile: int, overlap: int = 0, granule: int = 1, scale: int = 1, mode: str = "mean",
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y [B*ny*nx, C, ty*scale, tx*scale], the network's outputs for the tiles of an [B,C,h,w] batch -> [B,C,h*scale,w*scale]
    (``srad_tile_blend``): every pixel the mean ('mean') or the feathered mean ('feather') of the tiles that cover it, summed
    in tile order in fp32."""
    if mode not in L.TILE_BLENDS:
        raise ValueError(f"tile_blend: mode {mode!r}: one of {sorted(L.TILE_BLENDS)}")
    plan = tile_plan(h, w, tile, overlap, granule, scale)
    y = _tile_arg(y, "tile_blend").contiguous()
    n, Cc = y.shape[:2]
    per = plan.ny * plan.nx
    if n % per or tuple(y.shape[2:]) != (plan.ty * scale, plan.tx * scale):
        raise ValueError(f"tile_blend: {tuple(y.shape)} is not a batch of {plan.ny} x {plan.nx} tiles of "
                         f"{plan.ty * scale} x {plan.tx * scale} per image")
    B = n // per
    if out is None:
        out = torch.empty(B, Cc, h * scale, w * scale, dtype=torch.float32, device=y.device)
    elif tuple(out.shape) != (B, Cc, h * scale, w * scale) or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"tile_blend: out must be a contiguous fp32 GPU tensor of shape {(B, Cc, h * scale, w * scale)}")
    L.check(L.lib().srad_tile_blend(L.dptr(y), B, Cc, int(h), int(w), int(tile), int(overlap), int(granule), int(scale),
                                    L.TILE_BLENDS[mode], L.dptr(out), L.current_stream_ptr()), "tile_blend")
    return out


# ----------------------------------------------------------------------------------- 8-bit resize, equal to PIL.Image.resize
def resample_coeffs(in_size: int, out_size: int, filter: str = "lanczos"):
    """(ksize, bounds int32 [out, 2], coeffs int32 [out, ksize]) of one axis as numpy arrays (``srad_resample_coeffs``; host
    only, needs no GPU): Pillow's own fixed-point taps.  ValueError for an unknown filter, RuntimeError for refused sizes."""
    import numpy as np
    if filter not in L.RESAMPLE_FILTERS:
        raise ValueError(f"resample filter {filter!r}: one of {sorted(L.RESAMPLE_FILTERS)}")
    f, k = L.RESAMPLE_FILTERS[filter], C.c_int()
    L.check(L.lib().srad_resample_ksize(int(in_size), int(out_size), f, C.byref(k)), "resample_ksize")
    bounds = np.empty((int(out_size), 2), dtype=np.int32)
    coeffs = np.empty((int(out_size), k.value), dtype=np.int32)
    L.check(L.lib().srad_resample_coeffs(int(in_size), int(out_size), f, bounds.ctypes.data, coeffs.ctypes.data), "resample_coeffs")
    return k.value, bounds, coeffs


_RESAMPLE_TABLES: dict = {}


def resample_table(in_size: int, out_size: int, filter: str, device) -> tuple:
    """The ``_lib.ResampleTable`` of one axis on ``device`` and what keeps its arrays alive, cached per (in, out, filter,
    device): the tables are built and uploaded once."""
    key = (int(in_size), int(out_size), filter, str(device))
    hit = _RESAMPLE_TABLES.get(key)
    if hit is None:
        ksize, bounds, coeffs = resample_coeffs(in_size, out_size, filter)
        dev_bounds, dev_coeffs = torch.from_numpy(bounds).to(device), torch.from_numpy(coeffs).to(device)
        table = L.ResampleTable(int(in_size), int(out_size), ksize, bounds.ctypes.data, dev_bounds.data_ptr(), dev_coeffs.data_ptr())
        hit = _RESAMPLE_TABLES[key] = (table, (bounds, dev_bounds, dev_coeffs))
    return hit


def resize_u8(x: torch.Tensor, size, filter: str = "lanczos", *, out: Optional[torch.Tensor] = None,
              tmp: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x uint8 [n,H,W,C] (C = 1..4) on the GPU -> uint8 [n,h,w,C] with ``size = (h, w)``: every byte equals
    ``PIL.Image.resize((w, h), LANCZOS | BICUBIC)`` of the image (``srad_resize_u8``).  ``out`` / ``tmp`` ([n,H,w,C]): buffers to
    use instead of fresh ones."""
    _need_cuda(x)
    if x.dim() != 4 or x.dtype != torch.uint8:
        raise ValueError(f"resize_u8: expected a uint8 [n,H,W,C] tensor, got {tuple(x.shape)} {x.dtype}")
    x = x.contiguous()
    n, H, W, Cc = x.shape
    h, w = int(size[0]), int(size[1])
    if h < 1 or w < 1 or n < 1:
        raise ValueError(f"resize_u8: {n} images to {h}x{w}: every size must be >= 1")
    for t, shape, what in ((out, (n, h, w, Cc), "out"), (tmp, (n, H, w, Cc), "tmp")):
        if t is not None and not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"resize_u8: {what} must be a contiguous uint8 GPU tensor of shape {shape}")
    if out is None:
        out = torch.empty(n, h, w, Cc, dtype=torch.uint8, device=x.device)
    xt =resample_table(W, w, filter, x.device)[0] if W != w else None
    yt = resample_table(H, h, filter, x.device)[0] if H != h else None
    if tmp is None and xt is not None and yt is not None:
        tmp = torch.empty(n, H, w, Cc, dtype=torch.uint8, device=x.device)
    L.check(L.lib().srad_resize_u8(L.dptr(x), n, H, W, Cc, L.dptr(out), h, w, xt, yt, L.dptr(tmp), L.current_stream_ptr()), "resize_u8")
    return out


# ----------------------------------------------------------------------------------- float32 resize, equal to PIL's mode-F resize
def resample_coeffs_f64(in_size: int, out_size: int, filter: str = "bilinear"):
    """(ksize, bounds int32 [out, 2], coeffs float64 [out, ksize]) of one axis as numpy arrays (``srad_resample_coeffs_f64``;
    host only, needs no GPU): the taps Pillow resamples mode-F images with, divided by their sum and left in double.
    ValueError for an unknown filter, RuntimeError for refused sizes."""
    import numpy as np
    if filter not in L.RESAMPLE_FILTERS_F:
        raise ValueError(f"resample filter {filter!r}: one of {sorted(L.RESAMPLE_FILTERS_F)}")
    f, k = L.RESAMPLE_FILTERS_F[filter], C.c_int()
    L.check(L.lib().srad_resample_ksize_f64(int(in_size), int(out_size), f, C.byref(k)), "resample_ksize_f64")
    bounds = np.empty((int(out_size), 2), dtype=np.int32)
    coeffs = np.empty((int(out_size), k.value), dtype=np.float64)
    L.check(L.lib().srad_resample_coeffs_f64(int(in_size), int(out_size), f, bounds.ctypes.data, coeffs.ctypes.data), "resample_coeffs_f64")
    return k.value, bounds, coeffs


_RESAMPLE_TABLES_F: dict = {}


def resample_table_f(in_size: int, out_size: int, filter: str, device) -> tuple:
    """``resample_table`` for the float32 resize: the ``_lib.ResampleTableF`` of one axis on ``device`` and what keeps its arrays
    alive, cached per (in, out, filter, device)."""
    key = (int(in_size), int(out_size), filter, str(device))
    hit = _RESAMPLE_TABLES_F.get(key)
    if hit is None:
        ksize, bounds, coeffs = resample_coeffs_f64(in_size, out_size, filter)
        dev_bounds, dev_coeffs = torch.from_numpy(bounds).to(device), torch.from_numpy(coeffs).to(device)
        table = L.ResampleTableF(int(in_size), int(out_size), ksize, bounds.ctypes.data, dev_bounds.data_ptr(), dev_coeffs.data_ptr())
        hit = _RESAMPLE_TABLES_F[key] = (table, (bounds, dev_bounds, dev_coeffs))
    return hit


def resize_f32(x: torch.Tensor, size, filter: str = "bilinear", *, out: Optional[torch.Tensor] = None,
               tmp: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x float32 [n,H,W], contiguous, on the GPU -> float32 [n,h,w] with ``size = (h, w)``: every value equals, bit for bit,
    ``Image.fromarray(a, mode='F').resize((w, h), BILINEAR | BICUBIC | LANCZOS)`` of the map (``srad_resize_f32``).  ``out`` /
    ``tmp`` ([n,H,w]): buffers to use instead of fresh ones."""
    _need_cuda(x)
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"resize_f32: expected a contiguous float32 [n,H,W] tensor, got {tuple(x.shape)} {x.dtype}"
                         f"{'' if x.is_contiguous() else ', not contiguous'}")
    if filter not in L.RESAMPLE_FILTERS_F:
        raise ValueError(f"resample filter {filter!r}: one of {sorted(L.RESAMPLE_FILTERS_F)}")
    n, H, W = x.shape
    h, w = int(size[0]), int(size[1])
    if h < 1 or w < 1 or n < 1 or H < 1 or W < 1:
        raise ValueError(f"resize_f32: {n} maps of {H}x{W} to {h}x{w}: every size must be >= 1")
    for t, shape, what in ((out, (n, h, w), "out"), (tmp, (n, H, w), "tmp")):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"resize_f32: {what} must be a contiguous float32 GPU tensor of shape {shape}")
    if out is None:
        out = torch.empty(n, h, w, dtype=torch.float32, device=x.device)
    xt = resample_table_f(W, w, filter, x.device)[0] if W != w else None
    yt = resample_table_f(H, h, filter, x.device)[0] if H != h else None
    if tmp is None and xt is not None and yt is not None:
        tmp = torch.empty(n, H, w, dtype=torch.float32, device=x.device)
    L.check(L.lib().srad_resize_f32(L.dptr(x), n, H, W, L.dptr(out), h, w, xt, yt, L.dptr(tmp), L.current_stream_ptr()), "resize_f32")
    return out


# ----------------------------------------------------------------------------------- overlay: heat map and mask outline on the image
def overlay_rgb(src: torch.Tensor, maps: torch.Tensor, masks: torch.Tensor, lut: torch.Tensor, scale: float, contour_radius: int = 1,
                contour_rgb=(255, 255, 255), *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src uint8 [n,H,W,Cs] (Cs 1 or 3; gray is replicated), maps float32 [n,H,W], masks uint8 [n,H,W], lut uint8 [256,4]
    (r, g, b, alpha per level), all contiguous on the GPU -> uint8 [n,H,W,3] (``srad_overlay_rgb``): level = ``maps * scale``
    truncated into 0..255 (NaN: 0), ``out_c = (src_c * (255 - a) + lut_c * a + 127) // 255``, and a mask pixel with a 0 or the
    image's border within Chebyshev distance ``contour_radius`` (0..4; 0 draws none) takes ``contour_rgb``."""
    _need_cuda(src, maps, masks, lut, out)
    if src.dim() != 4 or src.dtype != torch.uint8 or src.shape[3] not in (1, 3) or not src.is_contiguous():
        raise ValueError(f"overlay_rgb: expected a contiguous uint8 [n,H,W,1|3] source, got {tuple(src.shape)} {src.dtype}")
    n, H, W, Cs = src.shape
    for t, dtype, shape, what in ((maps, torch.float32, (n, H, W), "maps"), (masks, torch.uint8, (n, H, W), "masks"),
                                  (lut, torch.uint8, (256, 4), "lut"), (out, torch.uint8, (n, H, W, 3), "out")):
        if t is not None and not (t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"overlay_rgb: {what} must be a contiguous {dtype} GPU tensor of shape {shape}, got {tuple(t.shape)} {t.dtype}")
    r = int(contour_radius)
    colour = [int(v) for v in contour_rgb]
    if r != contour_radius or len(colour) != 3:
        raise ValueError(f"overlay_rgb: contour radius {contour_radius!r} / colour {contour_rgb!r}: an integer and three integers")
    if out is None:
        out = torch.empty(n, H, W, 3, dtype=torch.uint8, device=src.device)
    L.check(L.lib().srad_overlay_rgb(L.dptr(src), n, H, W, Cs, L.dptr(maps), L.dptr(masks), L.dptr(lut), float(scale), r, *colour,
                                     L.dptr(out), L.current_stream_ptr()), "overlay_rgb")
    return out


# ----------------------------------------------------------------------------------- DRN's own kernels, one by one
# (C ABI ``srad_op_drn_*``, csrc/kernels_drn.hip).  Every call goes through the launcher the engines use, so grid, slices per image,
# NI and storage instance are the engines' own.  ``out=`` tensors let a test place an output inside a guarded allocation.
def _out(out: Optional[torch.Tensor], shape, dtype, device) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    assert tuple(out.shape) == tuple(shape) and out.dtype == dtype and out.is_contiguous() and out.is_cuda, (out.shape, shape, out.dtype)
    return out


def _rows(t: torch.Tensor, what: str) -> torch.Tensor:
    assert t.dim() == 2 and t.is_contiguous() and t.dtype in (torch.float32, torch.bfloat16), what
    return t


def drn_ca_plan(hw: int, C_: int) -> tuple:
    """(slices per image, NI) the streaming channel-attention kernels get for an image of ``hw`` pixels and ``C_`` channels
    (``srad_drn_ca_plan``; host only)."""
    sl, ni = C.c_int(), C.c_int()
    L.check(L.lib().srad_drn_ca_plan(hw, C_, C.byref(sl), C.byref(ni)), "drn_ca_plan")
    return sl.value, ni.value


def drn_bicubic(x: torch.Tensor, scale: int, mw: torch.Tensor, mb: torch.Tensor, *, raw: bool = False,
                out: Optional[torch.Tensor] = None, raw_out: Optional[torch.Tensor] = None):
    """x [B, C, H, W] (C = 1 | 3) -> bicubic x ``scale`` + sub_mean as NHWC[4] rows [B*Hs*Ws, 4]; with ``raw`` also the
    upsampled image before sub_mean, same layout."""
    _need_cuda(x, mw, mb)
    assert x.dim() == 4 and x.is_contiguous() and x.dtype == torch.float32
    B, Cc, H, W = x.shape
    T = B * H * scale * W * scale
    y = _out(out, (T, 4), torch.float32, x.device)
    r = _out(raw_out, (T, 4), torch.float32, x.device) if raw or raw_out is not None else None
    L.check(L.lib().srad_op_drn_bicubic(L.dptr(x), B, Cc, H, W, scale, L.dptr(mw.contiguous()), L.dptr(mb.contiguous()), L.dptr(y),
                                        L.dptr(r), L.current_stream_ptr()), "op_drn_bicubic")
    return (y, r) if r is not None else y


def drn_affine_to_nchw(x: torch.Tensor, B: int, Cc: int, mw: torch.Tensor, mb: torch.Tensor, *,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """add_mean + NHWC -> NCHW: x [B*HW, ld] rows (columns [0, Cc)) -> [B, Cc, HW]."""
    _need_cuda(x, mw, mb)
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32 and x.shape[0] % B == 0
    HW = x.shape[0] // B
    y = _out(out, (B, Cc, HW), torch.float32, x.device)
    L.check(L.lib().srad_op_drn_affine_to_nchw(L.dptr(x), x.stride(0), B, Cc, HW, L.dptr(mw.contiguous()), L.dptr(mb.contiguous()),
                                               L.dptr(y), L.current_stream_ptr()), "op_drn_affine_to_nchw")
    return y


def drn_pool_dot(r: torch.Tensor, B: int, *, g: Optional[torch.Tensor] = None, nchunk: int = 32,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """part [B, nchunk, C]: per-chunk column sums of r [B*hw, C] (fp32 or bf16), times g (fp32) when given."""
    _need_cuda(r, g)
    _rows(r, "r")
    hw, Cc = r.shape[0] // B, r.shape[1]
    assert r.shape[0] == B * hw and (g is None or (g.shape == r.shape and g.dtype == torch.float32 and g.is_contiguous()))
    part = _out(out, (B, nchunk, Cc), torch.float32, r.device)
    L.check(L.lib().srad_op_drn_pool_dot(L.dptr(g), L.dptr(r), int(r.dtype == torch.bfloat16), B, hw, Cc, nchunk, L.dptr(part),
                                         L.current_stream_ptr()), "op_drn_pool_dot")
    return part


def drn_ca_scale_add(part: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, r: torch.Tensor,
                     x: torch.Tensor, *, y_bf16: bool = False, keep: bool = True, out: Optional[torch.Tensor] = None,
                     gate_out: Optional[torch.Tensor] = None, pool_out: Optional[torch.Tensor] = None):
    """The RCAB tail: y = r * gate + x with gate = sigmoid(w2 relu(w1 mean + b1) + b2), mean = part.sum(1) / hw.  part
    [B, nchunk, C] fp32; r [B*hw, C] and x [B*hw, >= C] (row stride x.stride(0)) fp32 or bf16 - the storage combination picks
    the kernel instance; ``keep``: also return the gate and the pooled sums [B, C] (training keeps them).
    Returns y, or (y, gate, pool)."""
    _need_cuda(part, w1, b1, w2, b2, r, x)
    _rows(r, "r")
    B, nchunk, Cc = part.shape
    hw = r.shape[0] // B
    assert part.is_contiguous() and part.dtype == torch.float32 and r.shape == (B * hw, Cc)
    assert x.dim() == 2 and x.stride(1) == 1 and x.shape[0] == B * hw and x.shape[1] >= Cc and x.dtype in (torch.float32, torch.bfloat16)
    y = _out(out, (B * hw, Cc), torch.bfloat16 if y_bf16 else torch.float32, r.device)
    gate = _out(gate_out, (B, Cc), torch.float32, r.device) if keep else None
    pool = _out(pool_out, (B, Cc), torch.float32, r.device) if keep else None
    L.check(L.lib().srad_op_drn_ca_scale_add(L.dptr(part), nchunk, B, hw, Cc, L.dptr(w1.contiguous()), L.dptr(b1.contiguous()),
                                             L.dptr(w2.contiguous()), L.dptr(b2.contiguous()), L.dptr(r), int(r.dtype == torch.bfloat16),
                                             L.dptr(x), int(x.dtype == torch.bfloat16), x.stride(0), L.dptr(y), int(y_bf16),
                                             L.dptr(gate), L.dptr(pool), L.current_stream_ptr()), "op_drn_ca_scale_add")
    return (y, gate, pool) if keep else y


def drn_ca_apply_bwd(g: torch.Tensor, gate: torch.Tensor, part: torch.Tensor, pool: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor,
                     w2: torch.Tensor, *, dr_bf16: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d/dr of r * gate(mean r) + x under the upstream gradient g [B*hw, C]: part = drn_pool_dot(r, B, g=g), gate and pool as
    drn_ca_scale_add kept them.  Returns dr [B*hw, C] fp32 or bf16."""
    _need_cuda(g, gate, part, pool, w1, b1, w2)
    B, nchunk, Cc = part.shape
    hw = g.shape[0] // B
    assert g.shape == (B * hw, Cc) and g.is_contiguous() and g.dtype == torch.float32 and part.is_contiguous()
    assert gate.shape == pool.shape == (B, Cc) and gate.is_contiguous() and pool.is_contiguous()
    dr = _out(out, (B * hw, Cc), torch.bfloat16 if dr_bf16 else torch.float32, g.device)
    L.check(L.lib().srad_op_drn_ca_apply_bwd(L.dptr(g), L.dptr(gate), L.dptr(part), nchunk, L.dptr(pool), B, hw, Cc,
                                             L.dptr(w1.contiguous()), L.dptr(b1.contiguous()), L.dptr(w2.contiguous()), L.dptr(dr),
                                             int(dr_bf16), L.current_stream_ptr()), "op_drn_ca_apply_bwd")
    return dr


def drn_ca_bwd(part: torch.Tensor, pool: torch.Tensor, gate: torch.Tensor, hw: int, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor,
               dw1: torch.Tensor, db1: torch.Tensor, dw2: torch.Tensor, db2: torch.Tensor, *,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The channel attention's weight / bias gradients summed over the batch, ACCUMULATED into dw1 [Cr, C], db1 [Cr],
    dw2 [C, Cr], db2 [C]; returns dpool [B, C] (the gradient of the pooled sums)."""
    _need_cuda(part, pool, gate, w1, b1, w2, dw1, db1, dw2, db2)
    B, nchunk, Cc = part.shape
    for t in (part, pool, gate, dw1, db1, dw2, db2):
        assert t.is_contiguous() and t.dtype == torch.float32
    assert dw1.shape == (Cc // 16, Cc) and dw2.shape == (Cc, Cc // 16) and db1.shape == (Cc // 16,) and db2.shape == (Cc,)
    dpool = _out(out, (B, Cc), torch.float32, part.device)
    L.check(L.lib().srad_op_drn_ca_bwd(L.dptr(part), nchunk, L.dptr(pool), L.dptr(gate), B, hw, Cc, L.dptr(w1.contiguous()),
                                       L.dptr(b1.contiguous()), L.dptr(w2.contiguous()), L.dptr(dw1), L.dptr(db1), L.dptr(dw2),
                                       L.dptr(db2), L.dptr(dpool), L.current_stream_ptr()), "op_drn_ca_bwd")
    return dpool


def drn_affine_bwd(dy: torch.Tensor, t: torch.Tensor, w: torch.Tensor, dw: torch.Tensor, db: torch.Tensor, *, want_dt: bool = True,
                   out: Optional[torch.Tensor] = None):
    """MeanShift backward.  dy [B, C, HW] (NCHW) or [T, 4] rows; t [T, ld] rows (columns [0, C)), w [C, C]; dw [C, C] and db [C]
    are ACCUMULATED into; returns dt [T, 4] (= w^T dy, column C.. zero) or None."""
    _need_cuda(dy, t, w, dw, db)
    Cc = w.shape[0]
    assert dy.is_contiguous() and dy.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and dw.is_contiguous() and db.is_contiguous()
    nchw = dy.dim() == 3
    if nchw:
        B, HW = dy.shape[0], dy.shape[2]
        assert dy.shape[1] == Cc
    else:
        B, HW = 1, dy.shape[0]
        assert dy.shape[1] == 4
    assert t.shape[0] == B * HW
    dt = _out(out, (B * HW, 4), torch.float32, dy.device) if want_dt else None
    L.check(L.lib().srad_op_drn_affine_bwd(L.dptr(dy) if nchw else None, None if nchw else L.dptr(dy), L.dptr(t), t.stride(0), L.dptr(dt),
                                           B, Cc, HW, L.dptr(w.contiguous()), L.dptr(dw), L.dptr(db), L.current_stream_ptr()),
            "op_drn_affine_bwd")
    return dt


def drn_zero_upsample(dy: torch.Tensor, B: int, Ho: int, Wo: int, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dy [B*Ho*Wo, C] -> [B*2Ho*2Wo, C]: dy at the even pixels, zero elsewhere (the stride-2 convolution's backward)."""
    _need_cuda(dy)
    assert dy.dim() == 2 and dy.is_contiguous() and dy.dtype == torch.float32 and dy.shape[0] == B * Ho * Wo
    z = _out(out, (4 * B * Ho * Wo, dy.shape[1]), torch.float32, dy.device)
    L.check(L.lib().srad_op_drn_zero_upsample(L.dptr(dy), L.dptr(z), B, Ho, Wo, dy.shape[1], L.current_stream_ptr()), "op_drn_zero_upsample")
    return z


def drn_add_cols(src: torch.Tensor, dst: torch.Tensor, Cc: int) -> torch.Tensor:
    """dst[:, :Cc] += src[:, :Cc] in place (row strides may exceed Cc); returns dst."""
    _need_cuda(src, dst)
    assert src.dim() == dst.dim() == 2 and src.stride(1) == dst.stride(1) == 1 and src.shape[0] == dst.shape[0]
    assert src.dtype == dst.dtype == torch.float32 and src.shape[1] >= Cc and dst.shape[1] >= Cc
    L.check(L.lib().srad_op_drn_add_cols(L.dptr(src), src.stride(0), L.dptr(dst), dst.stride(0), src.shape[0], Cc, L.current_stream_ptr()),
            "op_drn_add_cols")
    return dst


def conv_pool_rows(B: int, H: int, W: int, Cc: int, precision: str = "fp32") -> int:
    """Partial rows per image the conv epilogue writes for an RCAB's second conv of this shape, 0 when it is not eligible (the
    query form of ``srad_op_conv_pool``; host only)."""
    rows = C.c_int(-1)
    L.check(L.lib().srad_op_conv_pool(L.PRECISIONS[precision], None, None, None, B, H, W, Cc, None, None, C.byref(rows), None, 0, None),
            "op_conv_pool")
    return rows.value


def conv_pool(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, *, B: int, H: int, W: int, precision: str = "fp32",
              out: Optional[torch.Tensor] = None, part_out: Optional[torch.Tensor] = None):
    """One C -> C 3x3 convolution with bias as DRN's forward runs an RCAB's second conv: x [B*H*W, C] fp32 rows, weight
    [C, C, 3, 3].  Returns (y [B*H*W, C], part, rows): rows partial rows per image from the conv's epilogue in part[:, :rows]
    (part is [B, 256, C] unless ``part_out`` is given, which must be [B, conv_pool_rows(...), C]); rows = 0: not eligible."""
    _need_cuda(x, weight, bias)
    Cc = weight.shape[0]
    assert x.shape == (B * H * W, Cc) and x.is_contiguous() and x.dtype == torch.float32 and weight.shape[1] == Cc
    w = weight.detach().reshape(Cc, Cc, 9).float().contiguous()
    y = _out(out, (B * H * W, Cc), torch.float32, x.device)
    want = conv_pool_rows(B, H, W, Cc, precision)
    part = _out(part_out, (B, want if part_out is not None else 256, Cc), torch.float32, x.device)
    prec = L.PRECISIONS[precision]
    keep, sp, nb = L.ws_buffer(L.lib().srad_op_gemm_scratch_bytes(prec, Cc, Cc, 9), x.device)
    rows = C.c_int(-1)
    L.check(L.lib().srad_op_conv_pool(prec, L.dptr(x), L.dptr(w), L.dptr(bias.contiguous()), B, H, W, Cc, L.dptr(y), L.dptr(part),
                                      C.byref(rows), sp, nb, L.current_stream_ptr()), "op_conv_pool")
    assert rows.value == want, (rows.value, want)
    return y, part, rows.value
