"""Reconstruction-error scorer on the GPU - host side of the C ABI's scorer entry points
(include/srad.h), mirroring reference src/metrics.py, the u8 conversions of src/evaluate.py:214-215
and src/trainer.py:45-47, and ``sklearn.metrics.roc_auc_score`` as src/evaluate.py uses it.
No CPU fallback: tensors must live on the GPU."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._lib import ws_buffer as _ws_buffer      # the name tests/test_gpu_pro.py calls for its direct C-ABI checks


def _call_with_ws(query: str, qargs: tuple, fn: str, args: tuple, device, sized: bool = True) -> None:
    """``srad_<fn>(*args, workspace[, workspace bytes], stream)`` with a fresh workspace of the size ``srad_<query>(*qargs)``
    reports (``sized=False``: the entry point takes no byte count)."""
    lib = L.lib()
    nbytes = C.c_size_t()
    L.check(getattr(lib, "srad_" + query)(*qargs, C.byref(nbytes)), query)
    keep, wp, wb = _ws_buffer(nbytes.value, device)
    L.check(getattr(lib, "srad_" + fn)(*args, wp, *((wb,) if sized else ()), L.current_stream_ptr()), fn)


def _need_cuda(*ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("srad_amd.metrics runs on the GPU only (HIP scorer); there is no CPU fallback")


def to_u8_hwc(x: torch.Tensor, rgb_range: float = 255.0) -> torch.Tensor:
    """``x.mul(255/range).clamp(0,255).byte().permute(0,2,3,1)`` - TRUNCATION, as the evaluator
    converts images (src/evaluate.py:214-215).  x: [B,C,H,W] fp32 -> [B,H,W,C] uint8."""
    _need_cuda(x)
    x = x.detach().float().contiguous()
    B, Cc, H, W = x.shape
    out = torch.empty(B, H, W, Cc, dtype=torch.uint8, device=x.device)
    L.check(L.lib().srad_to_u8_hwc(L.dptr(x), B, Cc, H, W, float(rgb_range), L.dptr(out), L.current_stream_ptr()), "to_u8_hwc")
    return out


def quantize(x: torch.Tensor, rgb_range: float = 255.0) -> torch.Tensor:
    """``quantize`` of the trainer (src/trainer.py:45-47): mul, clamp, ROUND (half to even), div."""
    _need_cuda(x)
    x = x.detach().float().contiguous()
    y = torch.empty_like(x)
    L.check(L.lib().srad_quantize(L.dptr(x), L.dptr(y), C.c_int64(x.numel()), float(rgb_range), L.current_stream_ptr()), "quantize")
    return y


def _u8_stacks(sr_u8: torch.Tensor, hr_u8: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The [n,H,W,C] uint8 GPU image stacks (SR, HR) of the scorer's entry points, checked and contiguous."""
    _need_cuda(sr_u8, hr_u8)
    assert sr_u8.dtype == torch.uint8 and hr_u8.dtype == torch.uint8 and sr_u8.shape == hr_u8.shape and sr_u8.dim() == 4
    return sr_u8.contiguous(), hr_u8.contiguous()


def score_pairs(sr_u8: torch.Tensor, hr_u8: torch.Tensor, window_sizes: Sequence[int]
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per-pair scores of [n,H,W,C] uint8 image stacks (SR, HR):
    ssim[n, len(window_sizes)] = ssim_numpy(hr/255, sr/255, ws) (src/metrics.py:26-67), mse[n], psnr[n]
    (float64 tensors on the GPU)."""
    sr_u8, hr_u8 = _u8_stacks(sr_u8, hr_u8)
    n, H, W, Cc = sr_u8.shape
    ws = (C.c_int32 * max(1, len(window_sizes)))(*[int(w) for w in window_sizes])
    dev = sr_u8.device
    ssim = torch.empty(n, len(window_sizes), dtype=torch.float64, device=dev)
    mse = torch.empty(n, dtype=torch.float64, device=dev)
    psnr = torch.empty(n, dtype=torch.float64, device=dev)
    _call_with_ws("score_workspace_bytes", (n, H, W), "score_pairs",
                  (L.dptr(sr_u8), L.dptr(hr_u8), n, H, W, Cc, ws, len(window_sizes), L.dptr(ssim), L.dptr(mse), L.dptr(psnr)), dev)
    return ssim, mse, psnr


SCORE_KERNELS = ("lds", "rows", "any")     # srad_score_plan's kernel numbers 0, 1, 2


def score_plan(n_img: int, H: int, W: int) -> Tuple[int, int]:
    """The path ``score_pairs`` takes for ``n_img`` H x W pairs (``srad_score_plan``; needs no GPU): (kernel, chunk) with
    kernel 0 = the LDS sweep (power-of-two widths 64..1024), 1 = the corner kernel (other multiples of 64), 2 = any width
    (names in ``SCORE_KERNELS``), and chunk = images per summed-area table chunk."""
    k, c = C.c_int(), C.c_int()
    L.check(L.lib().srad_score_plan(int(n_img), int(H), int(W), C.byref(k), C.byref(c)), "score_plan")
    return k.value, c.value


def val_metrics(sr: torch.Tensor, hr: torch.Tensor, rgb_range: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """psnr_torch / ssim_torch of Trainer.test (src/metrics.py:70-108) per image, with the
    reference's quirks kept verbatim: 4-px shave, zero padding, C1/C2 scaled by 255^2.  RuntimeError for
    W > 8 with H <= 8, where the shave leaves no row (the reference's PSNR is NaN there and its SSIM raises)."""
    _need_cuda(sr, hr)
    sr, hr = sr.detach().float().contiguous(), hr.detach().float().contiguous()
    if sr.shape[-2] > hr.shape[-2] or sr.shape[-1] > hr.shape[-1]:
        sr = sr[..., :hr.shape[-2], :hr.shape[-1]].contiguous()
    assert sr.shape == hr.shape
    B, Cc, H, W = sr.shape
    psnr = torch.empty(B, dtype=torch.float64, device=sr.device)
    ssim = torch.empty(B, dtype=torch.float64, device=sr.device)
    L.check(L.lib().srad_val_metrics(L.dptr(sr), L.dptr(hr), B, Cc, H, W, float(rgb_range), L.dptr(psnr), L.dptr(ssim),
                                     None, C.c_size_t(0), L.current_stream_ptr()), "val_metrics")
    return psnr, ssim


def roc_auc(y_true: Sequence[int], scores: Sequence[float]) -> float:
    """Binary ROC-AUC, equal to ``sklearn.metrics.roc_auc_score`` (ties count one half)."""
    y = np.ascontiguousarray(np.asarray(y_true), dtype=np.int32)
    s = np.ascontiguousarray(np.asarray(scores), dtype=np.float64)
    if y.shape != s.shape or y.ndim != 1:
        raise ValueError("y_true and scores must be 1-D and of equal length")
    out = C.c_double()
    rc = L.lib().srad_roc_auc(y.ctypes.data_as(C.POINTER(C.c_int32)), s.ctypes.data_as(C.POINTER(C.c_double)), len(y), C.byref(out))
    if rc:
        raise ValueError(L.lib().srad_last_error().decode())
    return out.value


def average_precision(y_true: Sequence[int], scores: Sequence[float]) -> Tuple[float, float]:
    """(average precision, F1-max) of binary labels: ``sklearn.metrics.average_precision_score``, and the best
    ``2 tp / (2 tp + fp + fn)`` over the thresholds "predict iff score >= s" at every distinct score s (compared exactly, in
    integers).  Host only, like ``roc_auc``.  ValueError for a NaN score, no positive label and a shape mismatch."""
    y = np.ascontiguousarray(np.asarray(y_true), dtype=np.int32)
    s = np.ascontiguousarray(np.asarray(scores), dtype=np.float64)
    if y.shape != s.shape or y.ndim != 1:
        raise ValueError("y_true and scores must be 1-D and of equal length")
    ap, f1 = C.c_double(), C.c_double()
    rc = L.lib().srad_average_precision(y.ctypes.data_as(C.POINTER(C.c_int32)), s.ctypes.data_as(C.POINTER(C.c_double)), len(y),
                                        C.byref(ap), C.byref(f1))
    if rc:
        raise ValueError(L.lib().srad_last_error().decode())
    return ap.value, f1.value


MAP_REDUCTIONS = ("mean", "max")           # srad_*_maps_multi's reduce numbers 0, 1
def _maps(query: str, fn: str, sr_u8: torch.Tensor, hr_u8: torch.Tensor, ws, reduce: Optional[str] = None) -> torch.Tensor:
    """float32 [n,H,W] maps of the stacks from ``srad_<fn>`` (workspace size from ``srad_<query>``): ``ws`` is one window size,
    or with ``reduce`` the checked list of ``_map_sizes``."""
    sr_u8, hr_u8 = _u8_stacks(sr_u8, hr_u8)
    n, H, W, Cc = sr_u8.shape
    sizes = (int(ws),) if reduce is None else ((C.c_int32 * len(ws))(*ws), len(ws), MAP_REDUCTIONS.index(reduce))
    out = torch.empty(n, H, W, dtype=torch.float32, device=sr_u8.device)
    _call_with_ws(query, (n, H, W), fn, (L.dptr(sr_u8), L.dptr(hr_u8), n, H, W, Cc, *sizes, L.dptr(out)), sr_u8.device)
    return out


def _map_sizes(fn: str, window_sizes: Sequence[int], reduce: str) -> List[int]:
    """The window sizes of a multi-scale map call as ints; ValueError (led by ``fn``) for an unknown ``reduce`` or an empty list."""
    if reduce not in MAP_REDUCTIONS:
        raise ValueError(f"{fn}: reduce = {reduce!r}, must be one of {MAP_REDUCTIONS}")
    sizes = [int(w) for w in window_sizes]
    if not sizes:
        raise ValueError(f"{fn}: the window-size list is empty")
    return sizes


def anomaly_maps(sr_u8: torch.Tensor, hr_u8: torch.Tensor, ws: int) -> torch.Tensor:
    """Per-pixel anomaly maps ``1 - ssim_map`` of [n,H,W,C] uint8 image stacks (SR, HR) at window size ``ws``: the map
    ``ssim_numpy(hr/255, sr/255, ws)`` averages (src/metrics.py:26-67).  Returns float32 [n,H,W] on the GPU."""
    return _maps("anomaly_map_workspace_bytes", "anomaly_maps", sr_u8, hr_u8, ws)


def anomaly_maps_multi(sr_u8: torch.Tensor, hr_u8: torch.Tensor, window_sizes: Sequence[int], reduce: str = "mean") -> torch.Tensor:
    """Multi-scale anomaly maps: ``anomaly_maps`` at every size of ``window_sizes`` reduced per pixel (``reduce`` = 'mean' or
    'max') in one kernel pass over tables built once.  The fp32 accumulation is in list order (DESIGN.md "Multi-scale maps"), so
    the result is bit for bit ``acc = acc + anomaly_maps(.., ws_k)`` then ``acc * float32(1 / K)`` (``torch.maximum`` for 'max');
    a size listed twice counts twice.  Returns float32 [n,H,W] on the GPU.  ValueError for an empty list or an unknown
    ``reduce``; RuntimeError for a size ``anomaly_maps`` refuses."""
    sizes = _map_sizes("anomaly_maps_multi", window_sizes, reduce)
    return _maps("anomaly_map_workspace_bytes", "anomaly_maps_multi", sr_u8, hr_u8, sizes, reduce)


MAP_SOURCES = ("ssim", "mse")              # what the evaluator's pixel-level maps are made of (--map-source)


def error_maps(sr_u8: torch.Tensor, hr_u8: torch.Tensor, ws: int = 1) -> torch.Tensor:
    """Squared-error maps of [n,H,W,C] uint8 image stacks (SR, HR), the per-pixel form of the MSE score (src/evaluate.py:251-265):
    with the integer ``e = sum_c (sr - hr)^2`` and ``S`` its sum over the reflect-padded ``ws`` x ``ws`` window of
    ``anomaly_maps``, the map is ``float32(float64(S) * (1.0 / (C * ws * ws * 65025)))`` bit for bit (DESIGN.md "Squared-error
    maps"); ``ws = 1`` is the raw per-pixel squared error, whose mean is the image's MSE.  Returns float32 [n,H,W] on the GPU,
    values in [0, 1].  RuntimeError for a window ``anomaly_maps`` refuses."""
    return _maps("error_map_workspace_bytes", "error_maps", sr_u8, hr_u8, ws)


def error_maps_multi(sr_u8: torch.Tensor, hr_u8: torch.Tensor, window_sizes: Sequence[int], reduce: str = "mean") -> torch.Tensor:
    """Multi-scale squared-error maps: ``error_maps`` at every size of ``window_sizes`` reduced per pixel exactly as
    ``anomaly_maps_multi`` reduces its maps, so the result is bit for bit ``acc = acc + error_maps(.., ws_k)`` in list order then
    ``acc * float32(1 / K)`` (``torch.maximum`` for 'max'); a size listed twice counts twice.  Returns float32 [n,H,W] on the
    GPU.  ValueError for an empty list or an unknown ``reduce``; RuntimeError for a size ``error_maps`` refuses."""
    sizes = _map_sizes("error_maps_multi", window_sizes, reduce)
    return _maps("error_map_workspace_bytes", "error_maps_multi", sr_u8, hr_u8, sizes, reduce)


GMS_MAP_SOURCES = {"gms": 1, "msgms": 4}    # the window-free map sources and their pyramid levels (DESIGN.md "Gradient-magnitude maps and loss")


def check_gms_levels(levels: int, H: int, W: int) -> int:
    """``levels`` as an int once H x W images can carry that many pyramid levels: 1..4, H and W multiples of ``2^(levels-1)``
    and at least twice that.  ValueError otherwise.  Needs no GPU."""
    levels = int(levels)
    if not 1 <= levels <= 4:
        raise ValueError(f"gms_maps: levels = {levels}, must be 1..4")
    f = 1 << (levels - 1)
    if H % f or W % f or H < 2 * f or W < 2 * f:
        raise ValueError(f"gms_maps: {levels} levels need H and W to be multiples of {f} and at least {2 * f} (got {H}x{W})")
    return levels


def gms_maps(sr_u8: torch.Tensor, hr_u8: torch.Tensor, levels: int = 1) -> torch.Tensor:
    """Gradient-magnitude similarity maps of [n,H,W,C] uint8 image stacks (SR, HR): per pyramid level the Prewitt gradient
    magnitudes of the channel sums (reflect padding) compared as ``(ga - gb)^2 / (ga^2 + gb^2 + c)``, the coarser levels
    upsampled bilinearly, the mean over ``levels`` (1 = GMS, 4 = MSGMS) rounded to float32 once - ``srad_gms_maps`` in
    include/srad.h states every operation.  Exactly 0 where the images agree, in [0, 1), symmetric in (SR, HR).  Returns float32
    [n,H,W] on the GPU.  ValueError for levels the image size cannot carry; the stacks may be views that start at any byte."""
    _need_cuda(sr_u8, hr_u8)
    assert sr_u8.dtype == torch.uint8 and hr_u8.dtype == torch.uint8 and sr_u8.shape == hr_u8.shape and sr_u8.dim() == 4
    n, H, W, Cc = sr_u8.shape
    levels = check_gms_levels(levels, H, W)
    if Cc not in (1, 3):
        raise ValueError(f"gms_maps: channels must be 1 or 3 (got {Cc})")
    sr_u8, hr_u8 = sr_u8.contiguous(), hr_u8.contiguous()
    out = torch.empty(n, H, W, dtype=torch.float32, device=sr_u8.device)
    _call_with_ws("gms_map_workspace_bytes", (n, H, W, levels), "gms_maps", (L.dptr(sr_u8), L.dptr(hr_u8), n, H, W, Cc, levels, L.dptr(out)),
                  sr_u8.device)
    return out


def check_map_scales(window_sizes: Sequence[int], H: int, W: int) -> List[int]:
    """The sizes of ``window_sizes`` as a list, once every one passes the window check of the map kernels for H x W images
    (a window may reflect over an image edge once).  ValueError otherwise.  Needs no GPU, so callers can check their arguments
    before any work."""
    sizes = [int(w) for w in window_sizes]
    for ws in sizes:
        if not (ws >= 1 and ws // 2 < min(H, W)):
            raise ValueError(f"map scales: window {ws} needs more than one reflection of a {H}x{W} image "
                             f"(sizes from 1 to {2 * min(H, W) - 1} fit)")
    return sizes


def pixel_roc_auc(scores: torch.Tensor, labels: torch.Tensor) -> float:
    """Exact pixel-level ROC-AUC (``sklearn.metrics.roc_auc_score`` of the flattened arrays, ties count one half) of GPU
    tensors: float32 scores, labels nonzero = positive (any integer or bool dtype).  Raises ValueError like ``roc_auc``
    when one class is absent, and when a score is NaN."""
    _need_cuda(scores, labels)
    s = scores.detach().reshape(-1).float().contiguous()
    y = labels.detach().reshape(-1)
    y = (y != 0).to(torch.uint8).contiguous() if y.dtype != torch.uint8 else y.contiguous()
    if s.numel() != y.numel():
        raise ValueError("scores and labels must have the same number of elements")
    if s.numel() == 0:
        raise ValueError("pixel_roc_auc of no elements")
    counts = torch.empty(4, dtype=torch.int64, device=s.device)          # u64 on the device; the values stay below 2^62
    auc = torch.empty((), dtype=torch.float64, device=s.device)
    _call_with_ws("pixel_auc_workspace_bytes", (C.c_int64(s.numel()),), "pixel_roc_auc",
                  (L.dptr(s), L.dptr(y), C.c_int64(s.numel()), L.dptr(counts), L.dptr(auc)), s.device)
    n_pos, n_neg, n_nan, _ = counts.tolist()
    if n_nan:
        raise ValueError(f"pixel_roc_auc: {n_nan} of {s.numel()} scores are NaN")
    if n_pos == 0 or n_neg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    return float(auc.item())


PIXEL_PR_COUNTS = ("n_pos", "n_neg", "n_nan", "n_points", "tp", "fp", "score_bits")     # srad_pixel_pr's counts_out


def _pixel_pr(scores: torch.Tensor, labels: torch.Tensor, curve: bool):
    """``srad_pixel_pr`` on the flattened tensors after the checks of ``pixel_pr``: (counts under ``PIXEL_PR_COUNTS``, ap, the
    three curve tensors cut to n_points or None)."""
    _need_cuda(scores, labels)
    s = scores.detach().reshape(-1).float().contiguous()
    y = labels.detach().reshape(-1)
    y = (y != 0).to(torch.uint8).contiguous() if y.dtype != torch.uint8 else y.contiguous()
    if s.numel() != y.numel():
        raise ValueError("scores and labels must have the same number of elements")
    if s.numel() == 0:
        raise ValueError("pixel_pr of no elements")
    n, dev = s.numel(), s.device
    counts = torch.empty(len(PIXEL_PR_COUNTS), dtype=torch.int64, device=dev)       # u64 on the device; the values stay below 2^32
    ap = torch.empty((), dtype=torch.float64, device=dev)
    cap = n if curve else 0                                                          # at most one point per score
    pts = [torch.empty(cap, dtype=t, device=dev) for t in (torch.float64, torch.float64, torch.float32)] if curve else [None] * 3
    _call_with_ws("pixel_pr_workspace_bytes", (C.c_int64(n),), "pixel_pr",
                  (L.dptr(s), L.dptr(y), C.c_int64(n), L.dptr(counts), L.dptr(ap), *(L.dptr(p) for p in pts), C.c_int64(cap)), dev)
    c = dict(zip(PIXEL_PR_COUNTS, counts.tolist()))
    if c["n_nan"]:
        raise ValueError(f"pixel_pr: {c['n_nan']} of {n} scores are NaN")
    if c["n_pos"] == 0:
        raise ValueError("No positive class found in y_true. Average precision is not defined in that case.")
    return c, float(ap.item()), ([p[:c["n_points"]] for p in pts] if curve else None)


def pixel_pr(scores: torch.Tensor, labels: torch.Tensor) -> dict:
    """Exact pixel-level precision-recall of GPU tensors (float32 scores; labels nonzero = positive, any integer or bool dtype, as
    ``pixel_roc_auc``), DESIGN.md "Precision-recall".  Every distinct score s is a threshold "predict iff score >= s".  Returns
    ``ap`` (``sklearn.metrics.average_precision_score`` of the flattened arrays) and the point of the highest F1, compared
    exactly in integers, the higher threshold keeping a tie: ``f1max``, ``precision`` and ``recall`` (Python floats from the
    integer counts ``tp``, ``fp``, ``fn``), ``score`` = its s*, ``threshold`` = the largest float32 below s*, for the
    ``map > threshold`` convention of ``operating_point`` and ``evaluate --threshold`` (for s* = -inf there is none and -inf is
    returned, which leaves the -inf scores out), and ``n_pos``, ``n_neg``.  With no negative label AP = 1.  ValueError for a NaN
    score, no positive label, a size mismatch and an empty input."""
    c, ap, _ = _pixel_pr(scores, labels, curve=False)
    tp, fp = c["tp"], c["fp"]
    fn = c["n_pos"] - tp
    star = np.array([c["score_bits"]], dtype=np.uint32).view(np.float32)[0]
    return dict(ap=ap, f1max=2 * tp / (2 * tp + fp + fn), precision=tp / (tp + fp), recall=tp / c["n_pos"], score=float(star),
                threshold=float(np.nextafter(star, np.float32(-np.inf))), tp=tp, fp=fp, fn=fn, n_pos=c["n_pos"], n_neg=c["n_neg"])


def pr_curve(scores: torch.Tensor, labels: torch.Tensor) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The precision-recall curve behind ``pixel_pr``: (precision float64, recall float64, thresholds float32), one point per
    distinct score from the HIGHEST down, point k being "predict iff score >= thresholds[k]" (a zero threshold is +0.0).
    These are the points of ``sklearn.metrics.precision_recall_curve`` in reverse order and without the (precision 1, recall 0)
    end point that sklearn appends.  ValueError as ``pixel_pr``."""
    _, _, pts = _pixel_pr(scores, labels, curve=True)
    return tuple(p.cpu().numpy() for p in pts)


def _mask_stack(masks: torch.Tensor) -> torch.Tensor:
    """[n,H,W] (or [H,W]) GPU masks of any integer or bool dtype -> contiguous u8 [n,H,W], nonzero = defect."""
    _need_cuda(masks)
    m = masks.detach()
    if m.dim() == 2:
        m = m[None]
    if m.dim() != 3 or m.numel() == 0:
        raise ValueError(f"masks must be a non-empty [n, H, W] tensor, got shape {tuple(masks.shape)}")
    return (m != 0).to(torch.uint8).contiguous() if m.dtype != torch.uint8 else m.contiguous()


def mask_regions(masks: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """Regions of ground-truth masks [n,H,W] (nonzero = defect): the 8-connected components of each image's mask
    (``scipy.ndimage.label(m_i, structure=np.ones((3, 3)))`` per image).  Returns (int32 [n,H,W] on the GPU: the pixel count of
    each pixel's region, 0 for ok pixels; the number of regions over all images)."""
    m = _mask_stack(masks)
    n, H, W = m.shape
    size = torch.empty(n, H, W, dtype=torch.int32, device=m.device)     # u32 on the device; sizes stay below 2^31
    counts = torch.empty(3, dtype=torch.int64, device=m.device)
    _call_with_ws("mask_regions_workspace_bytes", (n, H, W), "mask_regions", (L.dptr(m), n, H, W, L.dptr(size), L.dptr(counts)),
                  m.device)
    return size, int(counts[0].item())


def _pixel_pro(scores: torch.Tensor, masks: torch.Tensor, fpr_limit: float, curve: bool):
    lim = float(fpr_limit)
    if not 0.0 < lim <= 1.0:
        raise ValueError(f"fpr_limit = {fpr_limit}, must be in (0, 1]")
    _need_cuda(scores, masks)
    m = _mask_stack(masks)
    s = scores.detach().float()
    if s.dim() == 2:
        s = s[None]
    if tuple(s.shape) != tuple(m.shape):
        raise ValueError(f"scores {tuple(scores.shape)} and masks {tuple(masks.shape)} must have the same shape")
    s = s.contiguous()
    n, H, W = m.shape
    dev = s.device
    counts = torch.empty(5, dtype=torch.int64, device=dev)              # u64 on the device; the values stay below 2^62
    out = torch.empty((), dtype=torch.float64, device=dev)
    cap = n * H * W + 2 if curve else 0                                  # at most one point per distinct score, plus the two ends
    fpr = torch.empty(cap, dtype=torch.float64, device=dev) if curve else None
    pro = torch.empty(cap, dtype=torch.float64, device=dev) if curve else None
    _call_with_ws("pixel_pro_workspace_bytes", (n, H, W), "pixel_pro",
                  (L.dptr(s), L.dptr(m), n, H, W, C.c_double(lim), L.dptr(counts), L.dptr(out), L.dptr(fpr), L.dptr(pro),
                   C.c_int64(cap)), dev)
    n_reg, n_ok, _, n_nan, n_pts = counts.tolist()
    if n_nan:
        raise ValueError(f"aupro: {n_nan} of {s.numel()} scores are NaN")
    if n_reg == 0:
        raise ValueError("aupro: the masks have no defect region; PRO is not defined")
    if n_ok == 0:
        raise ValueError("aupro: the masks have no ok pixel; the false-positive rate is not defined")
    if curve:
        return fpr[:n_pts].cpu().numpy(), pro[:n_pts].cpu().numpy()
    return float(out.item())


def pro_curve(scores: torch.Tensor, masks: torch.Tensor) -> Tuple[np.ndarray, np.ndarray]:
    """The per-region overlap curve of float32 anomaly maps against ground-truth masks, both [n,H,W] GPU tensors (masks of any
    integer or bool dtype, nonzero = defect): float64 arrays (fpr, pro) with one point per distinct score from the highest down,
    led by (0, 0) and closed by (1, 1) (DESIGN.md "AU-PRO").  Raises ValueError for NaN scores, masks without a defect region
    or without an ok pixel, and a shape mismatch."""
    return _pixel_pro(scores, masks, 1.0, curve=True)


def aupro(scores: torch.Tensor, masks: torch.Tensor, fpr_limit: float = 0.3) -> float:
    """AU-PRO (Bergmann et al., IJCV 2021): the area under ``pro_curve`` for fpr in [0, fpr_limit], divided by fpr_limit.
    ValueError as ``pro_curve``, and for a limit outside (0, 1]."""
    return _pixel_pro(scores, masks, fpr_limit, curve=False)


def rank_for_rate(n: int, rate: float) -> int:
    """The ascending rank (0-based) whose value is the threshold of ``n`` calibration values at false-positive rate ``rate``
    (DESIGN.md "Operating point"): ``m = floor(rate * n)`` in Python doubles, clipped to [0, n - 1], and ``k = n - 1 - m``, so at
    most ``m`` values lie strictly above the value of rank ``k`` whatever the ties.  Host only.  ValueError for n < 1 and for a
    rate outside (0, 1) (NaN included)."""
    n, rate = int(n), float(rate)
    if n < 1:
        raise ValueError(f"rank_for_rate: n = {n}, must be >= 1")
    if not 0.0 < rate < 1.0:
        raise ValueError(f"rank_for_rate: rate = {rate}, must be in (0, 1)")
    m = min(max(int(np.floor(rate * n)), 0), n - 1)
    return n - 1 - m


def select_kth(values: torch.Tensor, k: int) -> Tuple[float, int, int]:
    """The value of ascending rank ``k`` (0-based) of a float32 GPU tensor of any shape, exactly (``np.sort(v.ravel())[k]``; a
    zero comes back as +0.0), by a radix select that neither sorts nor copies the values: (value, values below it, values equal
    to it).  ValueError for an empty tensor, 2^31 values or more, a rank outside [0, n), and a NaN among the values."""
    _need_cuda(values)
    v = values.detach().reshape(-1)
    if v.dtype != torch.float32:
        raise ValueError(f"select_kth takes float32 values, got {v.dtype}")
    v = v.contiguous()
    n, k = v.numel(), int(k)
    if not 1 <= n < 2 ** 31:
        raise ValueError(f"select_kth of {n} values: 1 to 2^31 - 1 are supported")
    if not 0 <= k < n:
        raise ValueError(f"select_kth: rank k = {k}, must be in [0, {n})")
    value = torch.empty((), dtype=torch.float32, device=v.device)
    counts = torch.empty(3, dtype=torch.int64, device=v.device)          # u64 on the device; the values stay below 2^31
    _call_with_ws("select_kth_workspace_bytes", (C.c_int64(n),), "select_kth",
                  (L.dptr(v), C.c_int64(n), C.c_int64(k), L.dptr(value), L.dptr(counts)), v.device)
    n_nan, n_below, n_equal = counts.tolist()
    if n_nan:
        raise ValueError(f"select_kth: {n_nan} of {n} values are NaN")
    return float(value.item()), n_below, n_equal


def map_threshold(values: torch.Tensor, rate: float) -> Tuple[float, float]:
    """The threshold that calibration ``values`` (float32 on the GPU: all pixels of defect-free maps, or their per-image maxima)
    give at false-positive rate ``rate``: the value of rank ``rank_for_rate(n, rate)``, always one of the values, nothing
    interpolated.  Returns (threshold, achieved rate = the share of the values strictly above it, <= rate).  ValueError as
    ``rank_for_rate`` and ``select_kth``."""
    _need_cuda(values)
    n = values.numel()
    if n < 1:
        raise ValueError("map_threshold of no values")
    t, n_below, n_equal = select_kth(values, rank_for_rate(n, rate))
    return t, (n - n_below - n_equal) / n


OPERATING_POINT_COUNTS = ("tp", "fp", "fn", "tn", "n_nan", "n_regions", "pro_hi", "pro_lo")   # srad_operating_point's counts_out


def operating_point(maps: torch.Tensor, threshold: float, masks: Optional[torch.Tensor] = None, min_area: int = 1
                    ) -> Tuple[torch.Tensor, torch.Tensor, dict]:
    """The prediction of float32 anomaly maps [n,H,W] on the GPU at ``threshold`` and its counts (DESIGN.md "Operating point"):
    a pixel is predicted iff ``map > threshold`` (the comparison of the float32 map values with the Python float, exactly); with ``min_area`` > 1 the 8-connected components (per image, as
    ``mask_regions``) of fewer than ``min_area`` predicted pixels are removed.  ``masks``: ground truth of the same shape (any
    integer or bool dtype, nonzero = defect), or None = every pixel ok.  Returns (pred: uint8 [n,H,W] in {0, 1}; img_pred:
    int32 [n], the surviving predicted pixels of each image; counts: Python ints under ``OPERATING_POINT_COUNTS``, with
    ``pro_hi * 2^64 + pro_lo`` = the sum over predicted defect pixels of ``floor(2^64 / |region|)``).  ValueError for a NaN
    threshold, ``min_area`` < 1, a shape mismatch and a NaN in the maps."""
    t, area = float(threshold), int(min_area)
    if t != t:
        raise ValueError("operating_point: the threshold is NaN")
    if area < 1 or area != min_area:
        raise ValueError(f"operating_point: min_area = {min_area}, must be an integer >= 1")
    with np.errstate(over="ignore"):
        tf = np.float32(t)
    if float(tf) > t:                                         # the largest float32 <= t: for float32 maps, map > tf iff map > t
        tf = np.nextafter(tf, np.float32(-np.inf))
    _need_cuda(maps)
    s = maps.detach()
    if s.dim() == 2:
        s = s[None]
    if s.dim() != 3 or s.numel() == 0 or s.dtype != torch.float32:
        raise ValueError(f"operating_point takes a non-empty float32 [n, H, W] tensor, got {s.dtype} {tuple(maps.shape)}")
    s = s.contiguous()
    m = None
    if masks is not None:
        m = _mask_stack(masks)
        if tuple(m.shape) != tuple(s.shape):
            raise ValueError(f"maps {tuple(maps.shape)} and masks {tuple(masks.shape)} must have the same shape")
    n, H, W = s.shape
    dev = s.device
    pred = torch.empty(n, H, W, dtype=torch.uint8, device=dev)
    img_pred = torch.empty(n, dtype=torch.int32, device=dev)            # u32 on the device; at most H x W < 2^31
    counts = torch.empty(8, dtype=torch.int64, device=dev)              # u64 on the device
    _call_with_ws("operating_point_workspace_bytes", (n, H, W), "operating_point",
                  (L.dptr(s), L.dptr(m), n, H, W, C.c_float(float(tf)), min(area, 2 ** 31 - 1), L.dptr(pred), L.dptr(img_pred),
                   L.dptr(counts)), dev)
    out = {k: int(v) & (2 ** 64 - 1) for k, v in zip(OPERATING_POINT_COUNTS, counts.tolist())}      # pro_lo uses all 64 bits
    if out["n_nan"]:
        raise ValueError(f"operating_point: {out['n_nan']} of {s.numel()} map values are NaN")
    return pred, img_pred, out


def _ratio(a: int, b: int) -> float:
    return a / b if b else 0.0


def operating_point_stats(counts: Optional[dict], img_pred, y_true: Sequence[int]) -> dict:
    """The report of an operating point (host only).  Image level, from ``img_pred`` (surviving predicted pixels per image; an
    image is flagged iff it has one) and the labels ``y_true`` (nonzero = defective): ``image_tp/fp/fn/tn``, ``image_tpr``,
    ``image_fpr``.  Pixel level, when ``counts`` (of ``operating_point`` with masks) is given: ``pixel_tp/fp/fn/tn``,
    ``precision``, ``recall``, ``f1``, ``iou``, ``fpr`` and ``pro_at_threshold`` = (1/R) sum over predicted defect pixels of
    1/|region|.  A ratio with a zero denominator is 0.0.  ValueError when the lengths differ."""
    flagged = [int(v) > 0 for v in (img_pred.tolist() if hasattr(img_pred, "tolist") else img_pred)]
    y = [int(v) != 0 for v in y_true]
    if len(flagged) != len(y):
        raise ValueError(f"operating_point_stats: {len(flagged)} images, {len(y)} labels")
    tp = sum(f and d for f, d in zip(flagged, y))
    fp = sum(f and not d for f, d in zip(flagged, y))
    fn = sum(d and not f for f, d in zip(flagged, y))
    tn = len(y) - tp - fp - fn
    out = dict(image_tp=tp, image_fp=fp, image_fn=fn, image_tn=tn, image_tpr=_ratio(tp, tp + fn), image_fpr=_ratio(fp, fp + tn))
    if counts is not None:
        tp, fp, fn, tn = (int(counts[k]) for k in ("tp", "fp", "fn", "tn"))
        num = (int(counts["pro_hi"]) << 64) + int(counts["pro_lo"])
        out.update(pixel_tp=tp, pixel_fp=fp, pixel_fn=fn, pixel_tn=tn, precision=_ratio(tp, tp + fp), recall=_ratio(tp, tp + fn),
                   f1=_ratio(2 * tp, 2 * tp + fp + fn), iou=_ratio(tp, tp + fp + fn), fpr=_ratio(fp, fp + tn),
                   pro_at_threshold=_ratio(num, int(counts["n_regions"]) << 64))
    return out


REGION_FIELDS = ("image", "area", "box", "sum_y", "sum_x", "overlap")      # of every region table; with scores also REGION_PEAK
REGION_PEAK = ("peak", "peak_y", "peak_x")
_REGION_CAP = 4096                                                          # records of region_table's first call


def _region_call(m, s, o, cap: int):
    """One ``srad_region_table``: (records as int32 [cap, 14], R, NaN scores inside regions)."""
    n, H, W = m.shape
    rec = torch.empty(cap, 14, dtype=torch.int32, device=m.device)       # srad_region_record: 56 bytes
    counts = torch.empty(3, dtype=torch.int64, device=m.device)          # u64 on the device; the values stay below 2^31
    _call_with_ws("region_table_workspace_bytes", (n, H, W), "region_table",
                  (L.dptr(m), L.dptr(s), L.dptr(o), n, H, W, L.dptr(rec) if cap else None, C.c_int64(cap), L.dptr(counts)), m.device)
    n_reg, n_nan, _ = counts.tolist()
    return rec, n_reg, n_nan


def region_table(masks: torch.Tensor, scores: Optional[torch.Tensor] = None, other: Optional[torch.Tensor] = None,
                 cap: Optional[int] = None) -> dict:
    """The table of regions of GPU masks [n,H,W] (any integer or bool dtype, nonzero = member): one row per 8-connected
    component of each image's mask (the components of ``mask_regions``), ordered by image and, within an image, by the region's
    first pixel in raster order - the order of ``scipy.ndimage.label(m_i, np.ones((3, 3)))`` (DESIGN.md "Defect regions").
    Returns GPU tensors of length R under ``REGION_FIELDS``: ``image`` int32, ``area`` int32, ``box`` int32 [R, 4] = (y0, x0, y1,
    x1), inclusive, ``sum_y`` / ``sum_x`` int64 (centroid = sum / area), ``overlap`` int32 = member pixels where ``other`` (a
    second mask of the same shape) is nonzero, 0 without it; with ``scores`` (float32, same shape) also ``peak`` float32, the
    region's largest score, and ``peak_y`` / ``peak_x`` int32, of equal maxima (-0.0 == +0.0) the first in raster order; and
    ``n_regions`` = R, a Python int.  ``cap``: the records of the first call (default 4096); when R exceeds it the call is
    repeated once at R.  R = 0 gives empty tensors.  ValueError for a shape mismatch, scores that are not float32, an empty
    tensor, a negative ``cap`` and a NaN score inside a region (a NaN outside every region is not looked at)."""
    m = _mask_stack(masks)
    s = o = None
    if scores is not None:
        _need_cuda(scores)
        s = scores.detach()
        if s.dim() == 2:
            s = s[None]
        if s.dtype != torch.float32:
            raise ValueError(f"region_table takes float32 scores, got {s.dtype}")
        if tuple(s.shape) != tuple(m.shape):
            raise ValueError(f"scores {tuple(scores.shape)} and masks {tuple(masks.shape)} must have the same shape")
        s = s.contiguous()
    if other is not None:
        o = _mask_stack(other)
        if tuple(o.shape) != tuple(m.shape):
            raise ValueError(f"other {tuple(other.shape)} and masks {tuple(masks.shape)} must have the same shape")
    first = _REGION_CAP if cap is None else int(cap)
    if first < 0:
        raise ValueError(f"region_table: cap = {cap}, must be >= 0")
    rec, n_reg, n_nan = _region_call(m, s, o, first)
    if n_nan:
        raise ValueError(f"region_table: {n_nan} scores inside the regions are NaN")
    if n_reg > first:
        rec, n_reg, _ = _region_call(m, s, o, n_reg)
    rec = rec[:n_reg]
    out = dict(image=rec[:, 0].contiguous(), area=rec[:, 1].contiguous(), box=rec[:, 2:6].contiguous(),
               sum_y=rec[:, 6:8].contiguous().view(torch.int64).reshape(-1),       # u64 on the device; below 2^62
               sum_x=rec[:, 8:10].contiguous().view(torch.int64).reshape(-1), overlap=rec[:, 10].contiguous())
    if s is not None:
        out.update(peak=rec[:, 11].contiguous().view(torch.float32), peak_y=rec[:, 12].contiguous(), peak_x=rec[:, 13].contiguous())
    out["n_regions"] = n_reg
    return out


def _column(table: dict, key: str) -> np.ndarray:
    v = table[key]
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v)


def region_stats(pred_table: dict, gt_table: dict, n_images: int, y_true: Sequence[int], min_overlap: float = 0.0) -> dict:
    """Detection counts at the level of regions (host only), from two tables of ``region_table``: ``pred_table`` of the predicted
    masks with ``other`` = the ground truth, ``gt_table`` of the ground-truth masks with ``other`` = the prediction.
    ``region_pred``; ``region_hit`` = predicted regions that touch the ground truth (``overlap`` >= 1); ``region_precision`` =
    hit / pred; ``region_false_alarms`` = pred - hit; ``false_alarms_per_image`` (over ``n_images``); ``false_alarms_on_good`` =
    the false alarms in images with ``y_true`` 0; ``region_gt``; ``region_found`` = ground-truth regions with ``overlap`` >=
    max(1, ceil(min_overlap * area)); ``region_recall`` = found / gt.  A ratio with a zero denominator is 0.0.  ValueError for
    ``min_overlap`` outside [0, 1] and for ``y_true`` of another length than ``n_images``."""
    f = float(min_overlap)
    if not 0.0 <= f <= 1.0:
        raise ValueError(f"region_stats: min_overlap = {min_overlap}, must be in [0, 1]")
    n_images = int(n_images)
    good = np.asarray([int(v) == 0 for v in y_true], dtype=bool)
    if len(good) != n_images:
        raise ValueError(f"region_stats: {n_images} images, {len(good)} labels")
    p_img, p_ov = _column(pred_table, "image").astype(np.int64), _column(pred_table, "overlap").astype(np.int64)
    g_area, g_ov = _column(gt_table, "area").astype(np.int64), _column(gt_table, "overlap").astype(np.int64)
    miss = p_ov < 1
    pred, hit = int(p_ov.size), int(p_ov.size - miss.sum())
    need = np.maximum(1, np.ceil(f * g_area.astype(np.float64)).astype(np.int64))
    gt, found = int(g_area.size), int((g_ov >= need).sum())
    return dict(region_pred=pred, region_hit=hit, region_precision=_ratio(hit, pred), region_false_alarms=pred - hit,
                false_alarms_per_image=_ratio(pred - hit, n_images),
                false_alarms_on_good=int(good[p_img[miss]].sum()) if pred else 0, region_gt=gt, region_found=found,
                region_recall=_ratio(found, gt))


def gaussian_weights(sigma: float, truncate: float = 4.0) -> np.ndarray:
    """The half ``[r:]`` of ``scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, r)`` with ``r = int(truncate * sigma + 0.5)``:
    float64 [r + 1], the centre weight first.  Computed here, with numpy's exp, so that the device filter uses scipy's weights
    to the last bit."""
    sigma = float(sigma)
    r = int(float(truncate) * sigma + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[r:])


def smooth_radius(sigma: float, H: int, W: int, truncate: float = 4.0) -> int:
    """The radius ``smooth_maps`` filters [.., H, W] maps with at this sigma: ``int(truncate * sigma + 0.5)``, 0 for
    sigma <= 1e-15.  ValueError for a negative (or NaN) sigma and for a radius above 128 or above min(H, W) (scipy would reflect
    more than once).  Needs no GPU, so callers can check their arguments before any work."""
    sigma = float(sigma)
    if not sigma >= 0.0:
        raise ValueError(f"smooth_maps: sigma = {sigma}, must be >= 0")
    if sigma <= 1e-15:
        return 0
    r = int(float(truncate) * sigma + 0.5)
    if r > min(H, W, 128):
        raise ValueError(f"smooth_maps: sigma = {sigma:g} (truncate {float(truncate):g}) gives radius {r}; the filter takes radii "
                         f"up to min(128, H, W) = {min(H, W, 128)} for the {H}x{W} maps (one reflection at the edges)")
    return r


def smooth_maps(maps: torch.Tensor, sigma: float, truncate: float = 4.0, with_max: bool = False):
    """Gaussian smoothing of float32 anomaly maps [n,H,W] on the GPU:
    ``scipy.ndimage.gaussian_filter(maps, (0, sigma, sigma), mode='reflect', truncate=truncate)`` bit for bit (DESIGN.md
    "Map smoothing").  ``sigma == 0`` returns the maps unchanged, as scipy does.  With ``with_max`` returns (smoothed, per-image
    maximum float32 [n], NaN for an image with a NaN pixel).  ValueError for a negative sigma and for a radius
    ``int(truncate * sigma + 0.5)`` above 128 or above min(H, W) (scipy would reflect more than once)."""
    _need_cuda(maps)
    sigma = float(sigma)
    m = maps.detach()
    if m.dim() != 3 or m.numel() == 0 or m.dtype != torch.float32:
        raise ValueError(f"smooth_maps takes a non-empty float32 [n, H, W] tensor, got {m.dtype} {tuple(m.shape)}")
    m = m.contiguous()
    n, H, W = m.shape
    r = smooth_radius(sigma, H, W, truncate)
    if sigma <= 1e-15 and not with_max:
        return m                                              # scipy skips an axis with sigma <= 1e-15
    w = gaussian_weights(sigma, truncate) if r > 0 else np.ones(1)              # radius 0: the kernel copies
    out = torch.empty_like(m)
    img_max = torch.empty(n, dtype=torch.float32, device=m.device) if with_max else None
    _call_with_ws("smooth_maps_workspace_bytes", (n, H, W, r), "smooth_maps",
                  (L.dptr(m), n, H, W, w.ctypes.data_as(C.POINTER(C.c_double)), r, L.dptr(out), L.dptr(img_max)), m.device)
    return (out, img_max) if with_max else out


def _map_stack(who: str, maps: torch.Tensor) -> torch.Tensor:
    """``maps`` as the float32 [n, H, W] tensor on the GPU the baseline kernels take; a contiguous one is passed as it is."""
    _need_cuda(maps)
    m = maps.detach()
    if m.dim() != 3 or m.numel() == 0 or m.dtype != torch.float32:
        raise ValueError(f"{who} takes a non-empty float32 [n, H, W] tensor, got {m.dtype} {tuple(m.shape)}")
    return m.contiguous()


def _map_plane(who: str, name: str, p: torch.Tensor, like: torch.Tensor, dtype) -> torch.Tensor:
    """A [H, W] plane of the baseline, checked against the maps ``like``: same device, ``dtype``, the maps' H x W, contiguous."""
    _need_cuda(p)
    if p.dtype != dtype or tuple(p.shape) != tuple(like.shape[1:]) or p.device != like.device or not p.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous {dtype} {tuple(like.shape[1:])} tensor on {like.device}, "
                         f"got {p.dtype} {tuple(p.shape)} on {p.device}")
    return p


def map_stats_accumulate(maps: torch.Tensor, s1: Optional[torch.Tensor] = None, s2: Optional[torch.Tensor] = None
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The per-pixel sums of float32 maps [n,H,W] on the GPU, in float64 [H,W]: ``s1 += sum_i m_i`` and ``s2 += sum_i m_i * m_i``,
    added sequentially in image order with one rounding per add (DESIGN.md "Baseline"), so a stack split over consecutive
    calls gives the bits of one call.  Without ``s1`` and ``s2`` the sums start at +0.0; with them they are updated in place and
    returned.  A NaN pixel makes that pixel's sums NaN."""
    m = _map_stack("map_stats_accumulate", maps)
    if (s1 is None) != (s2 is None):
        raise ValueError("map_stats_accumulate: give both s1 and s2, or neither")
    n, H, W = m.shape
    if s1 is None:
        s1 = torch.zeros(H, W, dtype=torch.float64, device=m.device)
        s2 = torch.zeros(H, W, dtype=torch.float64, device=m.device)
    else:
        s1 = _map_plane("map_stats_accumulate", "s1", s1, m, torch.float64)
        s2 = _map_plane("map_stats_accumulate", "s2", s2, m, torch.float64)
    L.check(L.lib().srad_map_stats_accumulate(L.dptr(m), n, H, W, L.dptr(s1), L.dptr(s2), L.current_stream_ptr()), "map_stats_accumulate")
    return s1, s2


def _normalize_out(who: str, m: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
    if out is None:
        return torch.empty_like(m)
    _need_cuda(out)
    if out.dtype != torch.float32 or out.shape != m.shape or out.device != m.device or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous float32 {tuple(m.shape)} tensor on {m.device}, "
                         f"got {out.dtype} {tuple(out.shape)} on {out.device}")
    return out


def normalize_maps(maps: torch.Tensor, mu: torch.Tensor, inv_sd: torch.Tensor, with_max: bool = False,
                   out: Optional[torch.Tensor] = None):
    """Per-pixel z-scores of float32 maps [n,H,W] on the GPU against the float32 planes ``mu`` and ``inv_sd`` [H,W]:
    ``z = fl32(fl32(m - mu) * inv_sd)``, signed, NaN propagating (DESIGN.md "Baseline").  ``out``: where to write them, which
    may be ``maps`` itself (in place).  With ``with_max`` returns (z, per-image maximum float32 [n], NaN for an image with a
    NaN pixel)."""
    m = _map_stack("normalize_maps", maps)
    mu = _map_plane("normalize_maps", "mu", mu, m, torch.float32)
    inv_sd = _map_plane("normalize_maps", "inv_sd", inv_sd, m, torch.float32)
    out = _normalize_out("normalize_maps", m, out)
    n, H, W = m.shape
    img_max = torch.empty(n, dtype=torch.float32, device=m.device) if with_max else None
    _call_with_ws("map_normalize_workspace_bytes", (n,), "map_normalize",
                  (L.dptr(m), n, H, W, L.dptr(mu), L.dptr(inv_sd), L.dptr(out), L.dptr(img_max)), m.device)
    return (out, img_max) if with_max else out


def normalize_maps_loo(maps: torch.Tensor, s1: torch.Tensor, s2: torch.Tensor, n: int, floor: float, with_max: bool = False):
    """Leave-one-out z-scores of float32 maps [k,H,W] that are part of the float64 sums ``s1``, ``s2`` [H,W] over ``n`` >= 3
    maps (``map_stats_accumulate``): each map against the mean and spread of the other ``n - 1``, in float64 with the fitted
    ``floor`` > 0 under the spread, rounded to float32 once (DESIGN.md "Baseline").  With ``with_max`` returns (z, per-image
    maximum)."""
    m = _map_stack("normalize_maps_loo", maps)
    s1 = _map_plane("normalize_maps_loo", "s1", s1, m, torch.float64)
    s2 = _map_plane("normalize_maps_loo", "s2", s2, m, torch.float64)
    if int(n) != n or int(n) < 3:
        raise ValueError(f"normalize_maps_loo: n = {n}, leave-one-out needs sums over at least 3 maps")
    floor = float(floor)
    if not (floor > 0.0 and np.isfinite(floor)):
        raise ValueError(f"normalize_maps_loo: floor = {floor}, must be finite and > 0")
    out = torch.empty_like(m)
    k, H, W = m.shape
    img_max = torch.empty(k, dtype=torch.float32, device=m.device) if with_max else None
    _call_with_ws("map_normalize_workspace_bytes", (k,), "map_normalize_loo",
                  (L.dptr(m), k, H, W, L.dptr(s1), L.dptr(s2), int(n), C.c_double(floor), L.dptr(out), L.dptr(img_max)), m.device)
    return (out, img_max) if with_max else out


def l1_loss(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """nn.L1Loss(reduction='mean') (src/loss.py:84) -> 0-d float64 tensor on the GPU."""
    _need_cuda(a, b)
    a, b = a.detach().float().contiguous(), b.detach().float().contiguous()
    assert a.shape == b.shape
    out = torch.empty((), dtype=torch.float64, device=a.device)
    _call_with_ws("l1_workspace_bytes", (), "l1_loss", (L.dptr(a), L.dptr(b), C.c_int64(a.numel()), L.dptr(out)), a.device,
                  sized=False)
    return out


# ------------------------------------------------------------------ reference-named conveniences
def sweep_window_sizes(min_dim: int) -> List[int]:
    """Window sizes the evaluator sweeps (src/evaluate.py:231-233)."""
    max_w = max(3, min_dim - 3)
    return [w for w in range(3, max_w + 1, 10) if w % 2 == 1] or [3]


def _as_u8_stack(img) -> torch.Tensor:
    a = np.asarray(img)
    if a.dtype != np.uint8:
        q = np.rint(a.astype(np.float64) * 255.0)
        if not np.allclose(q / 255.0, a, atol=1e-6):
            raise ValueError("ssim_numpy/psnr_numpy here take uint8 images or floats that are exact multiples of 1/255 "
                             "(what src/evaluate.py passes); use score_pairs for anything else")
        a = q.astype(np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    return torch.from_numpy(np.ascontiguousarray(a))[None].cuda()


def ssim_numpy(img_ref, img, win_size: int = 11) -> float:
    """Drop-in for ``src.metrics.ssim_numpy(hr/255, sr/255, ws)`` as the evaluator calls it."""
    s, _, _ = score_pairs(_as_u8_stack(img), _as_u8_stack(img_ref), [win_size])
    return float(s[0, 0].item())


def psnr_numpy(img_ref, img) -> float:
    """Drop-in for ``src.metrics.psnr_numpy(hr/255, sr/255)``."""
    _, _, p = score_pairs(_as_u8_stack(img), _as_u8_stack(img_ref), [])
    return float(p[0].item())


def psnr_torch(sr: torch.Tensor, hr: torch.Tensor, rgb_range: float) -> float:
    """src/metrics.py:70-79 (batch of one image, as Trainer.test calls it)."""
    p, _ = val_metrics(sr, hr, rgb_range)
    return float(p.mean().item()) if p.numel() > 1 else float(p[0].item())


def ssim_torch(sr: torch.Tensor, hr: torch.Tensor, rgb_range: float, win_size: int = 11) -> float:
    """src/metrics.py:82-108."""
    if win_size != 11:
        raise ValueError("the validation SSIM kernel is built for the 11x11 window the trainer uses")
    _, s = val_metrics(sr, hr, rgb_range)
    return float(s.mean().item()) if s.numel() > 1 else float(s[0].item())


def best_window(y_true: Sequence[int], ssim_cols: np.ndarray, sizes: Sequence[int]) -> Tuple[int, List[float]]:
    """The window sweep of the evaluator (src/evaluate.py:236-249): column j of ``ssim_cols`` holds the images' SSIM at window
    size ``sizes[j]`` (further columns are not looked at).  Returns (the index of the size with the highest image-level AUC of
    ``1 - SSIM``, the AUC of every size).  Strict '>': the first maximum wins (evaluate.py:246)."""
    best_j, best_auc, sweep = 0, -1.0, []
    for j in range(len(sizes)):
        sweep.append(roc_auc(y_true, 1.0 - ssim_cols[:, j]))
        if sweep[j] > best_auc:
            best_auc, best_j = sweep[j], j
    return best_j, sweep


def evaluate_pairs(y_true: Sequence[int], sr_u8: torch.Tensor, hr_u8: torch.Tensor) -> dict:
    """Window sweep + final scores + the three AUCs of ``evaluate_on_test`` (src/evaluate.py:226-267)
    for image stacks already on the GPU.  One scorer launch sequence covers every window size."""
    n, H, W, _ = hr_u8.shape
    sizes = sweep_window_sizes(min(H, W))
    ssim, mse, psnr = score_pairs(sr_u8, hr_u8, sizes)
    ssim_h, mse_h, psnr_h = ssim.cpu().numpy(), mse.cpu().numpy(), psnr.cpu().numpy()
    best_j, sweep = best_window(y_true, ssim_h, sizes)
    best_ws = sizes[best_j]
    s_ssim = (1.0 - ssim_h[:, best_j]).tolist()
    return dict(window_sizes=sizes, sweep_auc=sweep, best_ws=best_ws,
                scores_ssim=s_ssim, scores_mse=mse_h.tolist(), scores_psnr=psnr_h.tolist(),
                auc_ssim=roc_auc(y_true, s_ssim), auc_mse=roc_auc(y_true, mse_h),
                auc_psnr=roc_auc(y_true, -psnr_h))
