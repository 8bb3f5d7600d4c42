"""Predict on raw images: "defective or not, and where" for new, unlabelled, unprepared images.

    python -m srad_amd.predict --run-dir <run> --calibrate <dir of defect-free images> --threshold-fpr 0.01 [--map-ws 11 ...]
    python -m srad_amd.predict --run-dir <run> --input <files or directories> [--threshold T] [--save-masks ...]
    python -m srad_amd.predict --run-dir <run> --input <files or directories> --source-frame --save-overlays

``Detector`` chains what the evaluator already has - SR forward, anomaly maps (``evaluate.MapSpec``), operating point
(``metrics.operating_point``) - behind one step the evaluator leaves to ``prepare_mvtec_data``: turning a raw image into the
(LR, HR) pair the model was trained on.  That is two ``PIL.Image.resize(..., LANCZOS)`` calls, source -> hr x hr -> hr // scale,
and here both run on the GPU (``ops.resize_u8``, equal to PIL byte for byte; DESIGN.md "Resize on the device"), so the pair is
exactly what ``prepare_mvtec_data._write_pyramid`` followed by ``evaluate.iter_split`` gives and the maps and thresholds mean
what they mean in the evaluator.  Calibration writes ``<run-dir>/operating_point.json``; prediction reads it back.  One GPU;
image decoding stays on the host.

Every decision is taken in the model's frame (hr x hr).  ``--source-frame`` / ``--save-overlays`` add renderings of those
decisions at each source image's own size: the map and the filtered mask resized bilinearly on the GPU (``ops.resize_f32``,
equal to Pillow's mode-F resize bit for bit) and the heat map with the mask's outline drawn on the source
(``ops.overlay_rgb``; DESIGN.md "Maps and masks at source size").  ``--save-regions`` lists the defects: ``regions.csv`` has one row
per 8-connected component of the filtered masks (``metrics.region_table``; DESIGN.md "Defect regions")."""
from __future__ import annotations

import argparse
import csv
import json
import os
from dataclasses import asdict
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import baseline as B
from . import metrics as M
from . import ops
from .data import rgb2y, set_channel
from .evaluate import MapSpec, _with_window, infer_from_run_dir, resolve_checkpoint, save_anomaly_maps, save_masks, save_sr_image, super_resolve_dev
from .options import (ALL_MAP_SOURCES, GMS_MAP_SOURCES, _finite_or_inf_float, _map_scales, _nonnegative_float, _open_unit_float,
                      _positive_int, add_baseline_args, add_tile_args, build_opt, check_baseline_args, check_tile_args, tile_suffix)

OPERATING_POINT_FILE = 'operating_point.json'
OPERATING_POINT_VERSION = 1
IMAGE_SUFFIXES = ('.png', '.jpg', '.jpeg', '.bmp', '.tif', '.tiff')
MAP_WS_DEFAULT = 11                                           # skimage's default SSIM window: no labelled sweep picks one here


def luma_table() -> np.ndarray:
    """float32 [256]: what the loader makes of a gray value v once ``prepare_mvtec_data`` has written it as RGB (v, v, v) -
    ``data.rgb2y`` (float64) cast to float32 by ``np2Tensor``.  The float32 value does not depend on the shape of the array
    ``rgb2y`` is given (its float64 one does, in the last bits), so one table serves every image."""
    v = np.arange(256, dtype=np.uint8)
    return rgb2y(np.stack([v, v, v], axis=1)[:, None, :])[:, 0].astype(np.float32)


def as_source(image) -> np.ndarray:
    """A raw image as the uint8 array the resize starts from: [H,W] for gray (mode L, one channel, or r = g = b everywhere),
    [H,W,3] otherwise.  ``image``: a uint8 array [H,W], [H,W,1] or [H,W,3], or a path, read as ``prepare_mvtec_data.resize_image``
    reads it (anything but L and RGB goes through ``convert('RGB')``)."""
    if isinstance(image, (str, os.PathLike)):
        from PIL import Image
        with Image.open(image) as im:
            a = np.asarray(im if im.mode in ('L', 'RGB') else im.convert('RGB'))
    else:
        a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)) or a.size == 0:
        raise ValueError(f"predict takes uint8 images [H,W], [H,W,1] or [H,W,3], got {a.dtype} {a.shape}")
    if a.ndim == 3 and (a.shape[2] == 1 or (np.array_equal(a[..., 0], a[..., 1]) and np.array_equal(a[..., 0], a[..., 2]))):
        a = a[..., 0]
    return np.ascontiguousarray(a)


OVERLAY_ALPHA_DEFAULT = 0.6                                   # --overlay-alpha: the opacity of the hottest level
OVERLAY_CONTOUR_DEFAULT = 1                                   # --overlay-contour: the outline's Chebyshev radius, 0 draws none
OVERLAY_CONTOUR_RGB = (255, 255, 255)


def heat_lut(alpha_max: int) -> np.ndarray:
    """uint8 [256, 4]: (r, g, b, alpha) of every map level for ``ops.overlay_rgb``, from integer formulas alone.  Alpha is
    ``(alpha_max * level + 127) // 255``: 0 at level 0, never decreasing, ``alpha_max`` (0..255) at level 255.  The colours are
    a piecewise-linear ramp over four segments of 64 levels, ``t = 4 * (level % 64)``: blue (0, t, 255) -> cyan (0, 255, 255 - t)
    -> green (t, 255, 0) -> yellow (255, 255 - t, 0), ending near red.  With ``overlay_scale`` the threshold sits at level 127,
    the cyan -> green / green -> yellow boundary: what is below the threshold is blue to green and faint, what is above it
    yellow to red."""
    if not float(alpha_max).is_integer() or not 0 <= alpha_max <= 255:         # NaN and infinities are no integers
        raise ValueError(f"heat_lut: alpha_max = {alpha_max!r}, must be an integer in 0..255")
    level = np.arange(256, dtype=np.int64)
    seg, t = level // 64, 4 * (level % 64)
    zero, full = np.zeros_like(t), np.full_like(t, 255)
    r = np.choose(seg, [zero, zero, t, full])
    g = np.choose(seg, [t, full, full, 255 - t])
    b = np.choose(seg, [full, 255 - t, zero, zero])
    a = (int(alpha_max) * level + 127) // 255
    return np.stack([r, g, b, a], axis=1).astype(np.uint8)


def overlay_scale(threshold) -> np.float32:
    """The factor that takes a map value to its level: ``float32(127.5 / threshold)``, so the threshold sits at the middle of
    the ramp.  A threshold that is not finite or is <= 0 gives 255.0 (the maps lie in [0, 1]: the whole ramp)."""
    t = float(threshold)
    if not np.isfinite(t) or t <= 0.0:
        return np.float32(255.0)
    return np.float32(min(127.5 / t, float(np.finfo(np.float32).max)))      # finite for every threshold > 0


def check_spec(spec: MapSpec) -> MapSpec:
    """A predict-time spec names its window: ``ws`` >= 1 or scales.  'ssim' with ``ws`` 0 means the labelled sweep's best_ws in
    the evaluator, and there are no labels here."""
    if spec.needs_best_ws:
        raise ValueError("predict: an SSIM map spec needs its window size (--map-ws >= 1) or --map-scales; "
                         "window 0 is the labelled sweep's best_ws, and prediction has no labels")
    return spec


class Detector:
    """A model, a map spec and (once calibrated or given) a threshold.  ``hr_size``: the side the model's HR images have
    (default ``opt.patch_size``), or ``(H, W)`` for a rectangular frame - every source is resized to it, the LR images are
    ``(H // scale, W // scale)``, and a model that tiles (``Model.tile``) takes any such frame; scale, ``n_colors`` and
    ``rgb_range`` come from ``opt``.  ``overlay_alpha`` (0..255, the
    ``alpha_max`` of ``heat_lut``) and ``overlay_contour`` (0..4) shape the overlays ``predict(..., overlays=True)`` draws."""

    def __init__(self, opt, model, spec: MapSpec, threshold: Optional[float] = None, min_area: int = 1, self_ensemble: bool = False,
                 hr_size: Optional[int] = None, overlay_alpha: int = int(OVERLAY_ALPHA_DEFAULT * 255 + 0.5),
                 overlay_contour: int = OVERLAY_CONTOUR_DEFAULT, baseline: Optional[B.MapBaseline] = None):
        self.opt, self.model, self.self_ensemble = opt, model, bool(self_ensemble)
        self.baseline, self._fitted_on = None, None
        self._lut_host = heat_lut(overlay_alpha)
        if not float(overlay_contour).is_integer() or not 0 <= overlay_contour <= 4:
            raise ValueError(f"predict: overlay_contour = {overlay_contour!r}, must be an integer in 0..4")
        self.overlay_contour, self._lut = int(overlay_contour), None
        if isinstance(hr_size, (tuple, list)):                # a rectangular frame (H, W)
            if len(hr_size) != 2:
                raise ValueError(f"predict: hr_size = {hr_size!r}, must be a side or (H, W)")
            self.frame = (int(hr_size[0]), int(hr_size[1]))
        else:
            self.frame = (int(hr_size or opt.patch_size),) * 2
        self.hr_size = self.frame[0] if self.frame[0] == self.frame[1] else self.frame
        self.scale = int(opt.scale[-1] if isinstance(opt.scale, (list, tuple)) else opt.scale)
        self.n_colors, self.rgb_range = int(opt.n_colors), float(opt.rgb_range)
        if min(self.frame) // self.scale < 1:
            raise ValueError(f"predict: HR size {self.hr_size} is below the scale {self.scale}")
        self.lr_frame = (self.frame[0] // self.scale, self.frame[1] // self.scale)
        self.spec = _with_window(check_spec(spec).resolve(self.lr_frame[0] * self.scale, self.lr_frame[1] * self.scale), None, 1)      # mse: window 0 means 1
        if int(min_area) < 1 or int(min_area) != min_area:
            raise ValueError(f"predict: min_area = {min_area}, must be an integer >= 1")
        self.threshold, self.min_area = (None if threshold is None else float(threshold)), int(min_area)
        self.device = model.device
        self._luma = None
        model.eval()                                          # H1 of the evaluator: deterministic scoring
        if baseline is not None:
            self.set_baseline(baseline)

    @property
    def map_shape(self) -> Tuple[int, int]:
        """(H, W) of the maps: the HR frame cropped to LR * scale."""
        return self.lr_frame[0] * self.scale, self.lr_frame[1] * self.scale

    def set_baseline(self, baseline: Optional[B.MapBaseline]) -> None:
        """Maps are in sigmas of ``baseline`` from here on (None: the raw maps again).  ValueError for one of another frame."""
        if baseline is not None and baseline.shape != self.map_shape:
            raise ValueError(f"predict: the baseline is {baseline.shape}, the maps of this frame are {self.map_shape}")
        self.baseline, self._fitted_on = baseline, None

    # ---------------------------------------------------------------------------------------------------------- the pair
    def _pyramid(self, stack: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """uint8 [n,H,W,C] sources of one shape, on the GPU -> (LR uint8 [n,h,w,C], HR uint8 [n,hr,hr,C]): two LANCZOS resizes."""
        hr = ops.resize_u8(stack, self.frame, 'lanczos')
        return ops.resize_u8(hr, self.lr_frame, 'lanczos'), hr

    def prepare(self, images: Sequence) -> Tuple[torch.Tensor, torch.Tensor]:
        """Raw images (``as_source``), of any and mixed sizes -> (lr float32 [n,C,h,w] with values in [0, 255], hr uint8
        [n,H,W,C]) on the GPU, equal to ``iter_split`` of the tree ``prepare_mvtec_data`` writes from them: source to RGB,
        LANCZOS to hr x hr, that to hr // scale, ``set_channel``, HR cropped to LR * scale and truncated to u8.  One resize
        launch pair per source shape.  Gray sources resize one channel; with ``n_colors`` 1 their luma is the 256-entry float32
        table of ``luma_table`` (LR) and its truncation (HR); true colour with ``n_colors`` 1 takes ``data.set_channel`` on the
        host; ``n_colors`` 3 replicates gray."""
        return self._prepare(images, False)[:2]

    def _prepare(self, images: Sequence, keep_sources: bool):
        """``prepare``, and with ``keep_sources`` the groups it worked in: [(indices into ``images``, their sources as one
        uint8 [n,H,W,C] tensor on the GPU)], one entry per source shape - the upload the resize needed, kept."""
        sources = [as_source(im) for im in images]
        if not sources:
            raise ValueError("predict: no images")
        C_ = self.n_colors
        (lr_h, lr_w), crop_h, crop_w = self.lr_frame, self.lr_frame[0] * self.scale, self.lr_frame[1] * self.scale
        lr_out = torch.empty(len(sources), C_, lr_h, lr_w, dtype=torch.float32, device=self.device)
        hr_out = torch.empty(len(sources), crop_h, crop_w, C_, dtype=torch.uint8, device=self.device)
        groups: dict = {}
        for i, a in enumerate(sources):
            groups.setdefault(a.shape, []).append(i)
        kept = []
        for shape, idx in groups.items():
            stack = np.stack([sources[i] for i in idx])
            gray = len(shape) == 2
            stack = torch.from_numpy(stack[..., None] if gray else stack).to(self.device)
            if keep_sources:
                kept.append((idx, stack))
            lr, hr = self._pyramid(stack)
            if gray and C_ == 1:
                if self._luma is None:
                    table = luma_table()
                    self._luma = (torch.from_numpy(table).to(self.device), torch.from_numpy(table.astype(np.uint8)).to(self.device))
                lr_f, hr_u = self._luma[0][lr.long()], self._luma[1][hr.long()]
            elif gray:
                lr_f, hr_u = lr.expand(-1, -1, -1, C_).float(), hr.expand(-1, -1, -1, C_)
            elif C_ == 1:                                     # true colour to luma: the loader's own float64 arithmetic, on the host
                lr_h, hr_h = lr.cpu().numpy(), hr.cpu().numpy()
                ys = [set_channel([l], h, n_channels=1) for l, h in zip(lr_h, hr_h)]
                lr_f = torch.from_numpy(np.stack([y[0][0] for y in ys])).float().to(self.device)
                hr_u = torch.from_numpy(np.stack([y[1] for y in ys])).float().clamp(0, 255).to(torch.uint8).to(self.device)
            else:
                lr_f, hr_u = lr.float(), hr
            where = torch.tensor(idx, device=self.device)
            lr_out[where] = lr_f.permute(0, 3, 1, 2)
            hr_out[where] = hr_u[:, :crop_h, :crop_w]         # the loader crops after set_channel
        return lr_out, hr_out, kept

    # ---------------------------------------------------------------------------------------------------------- the maps
    def _maps(self, images: Sequence, with_max: bool, keep_sources: bool = False, raw: bool = False):
        """``raw``: the spec's maps even with a baseline (what a baseline is fitted on and leaves one out of)."""
        lr, hr, kept = self._prepare(images, keep_sources)
        sr = super_resolve_dev(self.model, lr, hr.shape[1:3], self.rgb_range, self_ensemble=self.self_ensemble)
        if self.baseline is None or raw:
            maps, img_max = self.spec.make(sr, hr, with_max and not raw)
        else:                                                 # the maximum is taken after the normalisation
            maps, _ = self.spec.make(sr, hr, False)
            maps, img_max = self.baseline.apply(maps, with_max=True, out=maps)
        return sr, hr, maps, img_max, kept

    @staticmethod
    def _image_keys(images: Sequence) -> list:
        return [os.fspath(im) if isinstance(im, (str, os.PathLike)) else id(im) for im in images]

    def fit_baseline(self, images: Sequence, floor_rel: float = B.FLOOR_REL_DEFAULT) -> B.MapBaseline:
        """Fits a per-pixel baseline (``baseline.MapBaseline``; DESIGN.md "Baseline") on the maps of the defect-free
        ``images`` - at least 3 - and makes it this detector's: ``predict`` then gives maps in sigmas of it, and a ``calibrate``
        on these same images takes their leave-one-out maps.  The fitted maps are kept until that calibration."""
        floor_rel = B.check_floor_rel(floor_rel)
        B.check_count(len(images))
        _, _, maps, _, _ = self._maps(images, False, raw=True)
        self.baseline = B.MapBaseline.fit(maps, floor_rel)
        self._fitted_on = (self._image_keys(images), maps)
        return self.baseline

    def calibrate(self, images: Sequence, fpr: float, level: str = 'pixel') -> Tuple[float, float]:
        """The threshold that the maps of the defect-free ``images`` give at false-positive rate ``fpr`` - on all their pixels
        (``level`` 'pixel') or on each map's maximum ('image') - as the evaluator's ``--threshold-fpr`` calibrates it
        (``metrics.map_threshold``).  Sets and returns it, with the rate achieved.  With a baseline the ``images`` must be
        the ones it was fitted on (``fit_baseline``), and the threshold comes from their leave-one-out maps."""
        if level not in ('pixel', 'image'):
            raise ValueError(f"predict: level = {level!r}, must be 'pixel' or 'image'")
        M.rank_for_rate(1, fpr)                               # the rate's own check, before any work
        if self.baseline is None:
            _, _, maps, img_max, _ = self._maps(images, level == 'image')
        else:
            if self._fitted_on is None or self._fitted_on[0] != self._image_keys(images):
                raise ValueError("predict: with a baseline the threshold is calibrated on the images the baseline was fitted on "
                                 "(fit_baseline on them first): in-sample z-scores of other maps are not leave-one-out")
            maps, img_max = self.baseline.apply_loo(self._fitted_on[1], with_max=True)
            self._fitted_on = None
        self.threshold, achieved = M.map_threshold(img_max if level == 'image' else maps, fpr)
        return self.threshold, achieved

    def predict(self, images: Sequence, source_frame: bool = False, overlays: bool = False, regions: bool = False) -> dict:
        """Per image (lists, in input order): ``ssim``, ``mse``, ``psnr`` of SR against HR (``metrics.score_pairs``; the SSIM at
        the spec's window, the mean over its scales where it has scales), ``map_max``, ``defect_pixels`` (pixels above the
        threshold that survive the area filter) and ``defective`` (any such pixel); ``maps`` float32 [n,H,W] and ``masks``
        uint8 {0, 1} [n,H,W] stay on the GPU, as do ``sr`` and ``hr`` (uint8 [n,H,W,C]).  ValueError without a threshold.

        All of that is in the model's frame and does not depend on the two flags.  ``source_frame`` adds renderings of it at
        each image's own size, as lists in input order (the sizes differ), on the GPU: ``maps_src[i]`` float32 [H_i,W_i],
        ``ops.resize_f32`` of ``maps[i]`` (bilinear, equal to Pillow's mode-F resize), and ``masks_src[i]`` uint8 {0, 1},
        the same resize of the float mask at >= 0.5 - a component the area filter removed stays removed.  ``overlays`` implies
        ``source_frame`` and adds ``overlays[i]`` uint8 [H_i,W_i,3]: ``ops.overlay_rgb`` of the raw source (``as_source``; true
        colour stays colour) under ``maps_src[i]`` through ``heat_lut`` at ``overlay_scale(threshold)``, ``masks_src[i]``
        outlined.

        ``regions`` adds the list of defects: ``regions``, ``metrics.region_table`` of ``masks`` against ``maps`` (one row per
        8-connected component that survived the area filter, so every area is >= ``min_area``; tensors on the GPU), and
        ``region_count``, the rows of each image; with the source frame also ``src_box``, int [R, 4] on the host, each region's
        box in its source image (``source_box``)."""
        if self.threshold is None:
            raise ValueError("predict: no threshold (calibrate on defect-free images first, or give one)")
        source_frame = bool(source_frame or overlays)
        sr, hr, maps, img_max, kept = self._maps(images, True, source_frame)
        sizes = list(self.spec.scales) or [self.spec.ws or MAP_WS_DEFAULT]      # the GMS maps have no window: the SSIM score's default
        ssim, mse, psnr = M.score_pairs(sr, hr, sizes)
        masks, img_pred, _ = M.operating_point(maps, self.threshold, None, self.min_area)
        pixels = [int(v) for v in img_pred.tolist()]
        res = dict(ssim=ssim.mean(1).tolist() if len(sizes) > 1 else ssim[:, 0].tolist(), mse=mse.tolist(), psnr=psnr.tolist(),
                   map_max=[float(v) for v in img_max.tolist()], defective=[v > 0 for v in pixels], defect_pixels=pixels,
                   threshold=self.threshold, maps=maps, masks=masks, sr=sr, hr=hr)
        if source_frame:
            res.update(self._source_frame(kept, maps, masks, bool(overlays)))
        if regions:
            table = M.region_table(masks, maps)
            res.update(regions=table, region_count=np.bincount(table['image'].cpu().numpy(), minlength=len(pixels)).tolist())
            if source_frame:
                sizes_src = [tuple(m.shape) for m in res['maps_src']]
                res['src_box'] = np.array([source_box(b, tuple(maps.shape[1:]), sizes_src[i])
                                           for i, b in zip(table['image'].tolist(), table['box'].tolist())], dtype=np.int64).reshape(-1, 4)
        return res

    def _source_frame(self, kept, maps: torch.Tensor, masks: torch.Tensor, overlays: bool) -> dict:
        """The model-frame ``maps`` and ``masks`` at the size of their sources, one resize (and one overlay) call per source
        shape: ``kept`` is ``_prepare``'s [(indices, sources uint8 [n,H,W,C] on the GPU)]."""
        n = maps.shape[0]
        out = dict(maps_src=[None] * n, masks_src=[None] * n)
        if overlays:
            out['overlays'] = [None] * n
            if self._lut is None:
                self._lut = torch.from_numpy(self._lut_host).to(self.device)
            scale = overlay_scale(self.threshold)
        for idx, src in kept:
            size = tuple(src.shape[1:3])
            where = torch.tensor(idx, device=self.device)
            m = ops.resize_f32(maps[where], size, 'bilinear')
            k = (ops.resize_f32(masks[where].float(), size, 'bilinear') >= 0.5).to(torch.uint8)
            o = ops.overlay_rgb(src, m, k, self._lut, scale, self.overlay_contour, OVERLAY_CONTOUR_RGB) if overlays else None
            for j, i in enumerate(idx):
                out['maps_src'][i], out['masks_src'][i] = m[j], k[j]
                if overlays:
                    out['overlays'][i] = o[j]
        return out


# -------------------------------------------------------------------------------------------------------------------- files
def list_images(paths: Sequence[str]) -> List[Path]:
    """The image files of ``paths``: a file is taken as it is, a directory gives its image files (by suffix), sorted by name."""
    out: List[Path] = []
    for p in paths:
        p = Path(p)
        if p.is_dir():
            out.extend(sorted(f for f in p.iterdir() if f.is_file() and f.suffix.lower() in IMAGE_SUFFIXES))
        elif p.is_file():
            out.append(p)
        else:
            raise FileNotFoundError(f"no such image file or directory: {p}")
    return out


def unique_names(files: Sequence[Path]) -> List[str]:
    """A name per file for the outputs: the stem, with ``_2``, ``_3``, .. where a stem comes again."""
    seen: dict = {}
    names = []
    for f in files:
        k = seen[f.stem] = seen.get(f.stem, 0) + 1
        names.append(f.stem if k == 1 else f"{f.stem}_{k}")
    return names


def source_box(box, model_hw, source_hw) -> Tuple[int, int, int, int]:
    """A model-frame box (y0, x0, y1, x1), inclusive, in a source image of ``source_hw`` = (H, W), when the model's frame is
    ``model_hw``: the source pixels that the box's pixels cover when pixel c of M spans [c * S / M, (c + 1) * S / M) - per axis
    ``src0 = (c0 * S) // M`` and ``src1 = ceil((c1 + 1) * S / M) - 1``, in integers, clipped to the image.  ``src1 >= src0``
    always; M == S is the identity."""
    out = []
    for (c0, c1), m, s in zip(((box[0], box[2]), (box[1], box[3])), model_hw, source_hw):
        c0, c1, m, s = int(c0), int(c1), int(m), int(s)
        if m < 1 or s < 1 or not 0 <= c0 <= c1 < m:
            raise ValueError(f"source_box: box {tuple(box)} in a {tuple(model_hw)} frame, source {tuple(source_hw)}")
        lo, hi = (c0 * s) // m, -((-(c1 + 1) * s) // m) - 1
        out.append((min(max(lo, 0), s - 1), min(max(hi, 0), s - 1)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


REGION_COLUMNS = ('area', 'y0', 'x0', 'y1', 'x1', 'centroid_y', 'centroid_x', 'peak', 'peak_y', 'peak_x')


def write_regions_csv(path, table: dict, names: Sequence[str], kinds: Sequence[str], src_box=None) -> int:
    """``regions.csv``: one row per region of ``table`` (``metrics.region_table`` with scores; tensors or arrays) - name, kind
    (the image's split or predicted kind), region (its index within the image), ``REGION_COLUMNS``, ``gt_overlap`` where the
    table has ``gt_overlap`` (a table made against ground-truth masks), ``src_y0 .. src_x1`` where ``src_box`` is given.  The
    centroid is ``sum / area`` in doubles; floats are written with ``repr``.  Returns the number of rows."""
    col = {k: np.asarray(v.cpu() if hasattr(v, 'cpu') else v) for k, v in table.items() if k != 'n_regions'}
    header = ['name', 'kind', 'region'] + list(REGION_COLUMNS) + (['gt_overlap'] if 'gt_overlap' in col else [])
    header += ['src_y0', 'src_x0', 'src_y1', 'src_x1'] if src_box is not None else []
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    with open(path, 'w', newline='') as fh:
        w = csv.writer(fh)
        w.writerow(header)
        seen: dict = {}
        for r in range(len(col['image'])):
            i, area = int(col['image'][r]), int(col['area'][r])
            k = seen[i] = seen.get(i, -1) + 1
            row = [names[i], kinds[i], k, area] + [int(v) for v in col['box'][r]]
            row += [repr(int(col['sum_y'][r]) / area), repr(int(col['sum_x'][r]) / area), repr(float(col['peak'][r])),
                    int(col['peak_y'][r]), int(col['peak_x'][r])]
            row += [int(col['gt_overlap'][r])] if 'gt_overlap' in col else []
            row += [int(v) for v in src_box[r]] if src_box is not None else []
            w.writerow(row)
    return len(col['image'])


def write_operating_point(path, threshold: float, fpr: float, level: str, achieved: float, n_images: int, min_area: int, spec: MapSpec,
                          self_ensemble: bool, checkpoint: str, tile=None, frame=None, baseline=None) -> dict:
    """``operating_point.json``: everything a threshold depends on next to it.  Python's JSON writes a float's shortest
    round-trip form, so the threshold reads back bit for bit.  ``tile`` (tile, overlap, blend) and ``frame`` (H, W) are written
    only when they are set: a file without them says whole images in the square frame of the run's resolution.  So is
    ``baseline`` (``baseline_entry``: the file of the per-pixel baseline beside this one and its hash): a file without it says
    the threshold is in the maps' own units."""
    doc = dict(version=OPERATING_POINT_VERSION, threshold=float(threshold), threshold_source='fpr', threshold_fpr=float(fpr),
               threshold_level=level, calib_rate=float(achieved), calib_images=int(n_images), min_region_area=int(min_area),
               map_spec=dict(asdict(spec), scales=list(spec.scales)), self_ensemble=bool(self_ensemble),
               checkpoint=os.path.basename(checkpoint))
    if tile:
        doc['tile'] = [int(tile[0]), int(tile[1]), str(tile[2])]
    if frame:
        doc['frame'] = [int(frame[0]), int(frame[1])]
    if baseline:
        doc['baseline'] = _baseline_entry(baseline)
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Path(path).write_text(json.dumps(doc, indent=2) + "\n")
    return doc


def _baseline_entry(e: dict) -> dict:
    """The ``baseline`` entry of ``operating_point.json`` with its five keys and their types (KeyError for a missing one)."""
    return dict(file=str(e['file']), n_images=int(e['n_images']), floor_rel=float(e['floor_rel']), floor=float(e['floor']),
                sha256=str(e['sha256']))


def baseline_entry(baseline: B.MapBaseline, path, sha256: str) -> dict:
    """What ``write_operating_point(baseline=...)`` takes for ``baseline`` saved at ``path`` (``MapBaseline.save`` returns the hash)."""
    return dict(file=os.path.basename(path), n_images=baseline.n, floor_rel=baseline.floor_rel, floor=baseline.floor, sha256=sha256)


def baseline_from_args(args, stored: Optional[dict], folder) -> Optional[dict]:
    """Which saved baseline a prediction runs with: None, or dict(path, sha256 or None).  With ``stored`` (the operating point
    a threshold was calibrated at): what it holds, its file beside it in ``folder`` - and ``--baseline`` or a
    ``--baseline-floor`` that says otherwise is a ValueError, as the threshold is in sigmas of that baseline or in none.  With
    a given ``--threshold`` and ``--baseline``: ``folder``'s ``map_baseline.npz``, which must be there."""
    want, floor = bool(getattr(args, 'baseline', False)), getattr(args, 'baseline_floor', None)
    if stored is None:
        if not want or getattr(args, 'calibrate', ''):
            return None
        path = Path(folder) / B.BASELINE_FILE
        if not path.is_file():
            raise ValueError(f"--baseline: no {path} (--calibrate DIR --threshold-fpr RATE --baseline writes it)")
        return dict(path=path, sha256=None, floor_rel=floor)
    kept = stored.get('baseline')
    if want and kept is None:
        raise ValueError("--baseline contradicts the calibrated operating point (calibrated without a baseline): "
                         "calibrate again with it, or give --threshold")
    if kept is not None and floor is not None and floor != kept['floor_rel']:
        raise ValueError(f"--baseline-floor {floor:g} contradicts the calibrated operating point (floor_rel = {kept['floor_rel']:g}): "
                         f"calibrate again with it, or give --threshold")
    return None if kept is None else dict(path=Path(folder) / kept['file'], sha256=kept['sha256'], floor_rel=None)


def load_baseline(which: dict, det: 'Detector') -> B.MapBaseline:
    """The saved baseline ``baseline_from_args`` named, for ``det``: the file's hash (where the operating point recorded one),
    its frame and its map spec are checked against the detector's.  ValueError for a mismatch or an unreadable file."""
    path = which['path']
    if not Path(path).is_file():
        raise ValueError(f"{path}: the baseline of the calibrated operating point is missing")
    if which.get('sha256') is not None and B.file_sha256(path) != which['sha256']:
        raise ValueError(f"{path}: the file's sha256 is not the one the operating point was calibrated with")
    b = B.load(path, device=det.device, shape=det.map_shape, spec=det.spec)
    if which.get('floor_rel') is not None and which['floor_rel'] != b.floor_rel:
        raise ValueError(f"--baseline-floor {which['floor_rel']:g} contradicts {path} (floor_rel = {b.floor_rel:g})")
    return b


def read_operating_point(path) -> dict:
    """The document ``write_operating_point`` wrote, its ``map_spec`` as a ``MapSpec``.  ValueError for another version or a
    missing entry."""
    doc = json.loads(Path(path).read_text())
    if doc.get('version') != OPERATING_POINT_VERSION:
        raise ValueError(f"{path}: version {doc.get('version')!r}, this build reads version {OPERATING_POINT_VERSION}")
    try:
        m = doc['map_spec']
        doc['map_spec'] = MapSpec(source=m['source'], ws=int(m['ws']), scales=list(m['scales']) or (), reduce=m['reduce'], sigma=float(m['sigma']))
        doc['threshold'], doc['min_region_area'], doc['self_ensemble'] = float(doc['threshold']), int(doc['min_region_area']), bool(doc['self_ensemble'])
        tile, frame = doc.get('tile'), doc.get('frame')       # absent in files written before tiling, and whenever it is off
        doc['tile'] = (int(tile[0]), int(tile[1]), str(tile[2])) if tile else None
        doc['frame'] = (int(frame[0]), int(frame[1])) if frame else None
        doc['baseline'] = _baseline_entry(doc['baseline']) if doc.get('baseline') else None      # absent whenever it is off
    except KeyError as e:
        raise ValueError(f"{path}: entry {e} is missing")
    return doc


def tile_from_args(args, stored: Optional[dict] = None):
    """((tile, overlap, blend) or None, (H, W) or None) of the command line.  With ``stored`` (the operating point a threshold
    was calibrated at): what it holds, and a ``--tile*`` or ``--frame`` flag that says otherwise is a ValueError - the
    threshold belongs to the SR images it was calibrated on."""
    tile = (int(args.tile), int(args.tile_overlap), str(args.tile_blend)) if getattr(args, 'tile', 0) else None
    frame = tuple(int(v) for v in args.frame) if getattr(args, 'frame', None) else None
    if stored is None:
        return tile, frame
    kept_tile, kept_frame = stored.get('tile'), stored.get('frame')
    if tile is not None and tile != kept_tile:
        was = "without tiling" if kept_tile is None else f"with --tile {kept_tile[0]} --tile-overlap {kept_tile[1]} --tile-blend {kept_tile[2]}"
        raise ValueError(f"--tile {tile[0]} --tile-overlap {tile[1]} --tile-blend {tile[2]} contradicts the calibrated operating point "
                         f"(calibrated {was}): calibrate again with it, or give --threshold")
    if frame is not None and frame != kept_frame:
        was = "in the square frame of the resolution" if kept_frame is None else f"with --frame {kept_frame[0]} {kept_frame[1]}"
        raise ValueError(f"--frame {frame[0]} {frame[1]} contradicts the calibrated operating point (calibrated {was}): "
                         f"calibrate again with it, or give --threshold")
    return kept_tile, kept_frame


MAP_FLAGS = (('map_source', '--map-source', 'source'), ('map_ws', '--map-ws', 'ws'), ('map_scales', '--map-scales', 'scales'),
             ('map_reduce', '--map-reduce', 'reduce'), ('map_sigma', '--map-sigma', 'sigma'))


def spec_from_args(args, stored: Optional[MapSpec] = None, side: int = 0) -> MapSpec:
    """The map spec of the command line.  Without ``stored``: the flags, ``--map-ws`` defaulting to 11 where neither it nor
    scales are given.  With ``stored`` (the spec a threshold was calibrated on): that spec, and a ``--map-*`` flag that says
    otherwise is a ValueError - a threshold belongs to the maps it was calibrated on (``side``: the HR side, which says what
    ``--map-scales sweep`` stands for)."""
    if stored is not None:
        for attr, flag, field in MAP_FLAGS:
            given, kept = getattr(args, attr), getattr(stored, field)
            if field == 'scales' and given == 'sweep' and side:
                given = M.sweep_window_sizes(side)
            if field == 'ws' and given == 0 and (args.map_source or stored.source) == 'mse' and not stored.scales:
                given = 1                                     # the squared-error maps' window 0 is stored as what it means, 1
            if given is not None and (list(given) != list(kept) if field == 'scales' else given != kept):
                raise ValueError(f"{flag} {given} contradicts the calibrated operating point ({field} = {kept}): "
                                 f"calibrate again with it, or give --threshold")
        return stored
    scales = args.map_scales or ()
    if scales and args.map_ws:
        raise ValueError("--map-scales and --map-ws exclude each other (the scales replace the single window size)")
    ws = args.map_ws if args.map_ws is not None else (0 if scales or args.map_source in GMS_MAP_SOURCES else MAP_WS_DEFAULT)
    return MapSpec(source=args.map_source or 'ssim', ws=ws, scales=scales, reduce=args.map_reduce or 'mean', sigma=args.map_sigma or 0.0)


def _unit_float(text: str) -> float:
    v = float(text)
    if not 0.0 <= v <= 1.0:                                   # NaN too
        raise argparse.ArgumentTypeError(f"{text} is not an opacity in [0, 1]")
    return v


def save_source_frame(res: dict, names: Sequence[str], kinds: Sequence[str], output_dir: str, sigmas: bool = False) -> None:
    """What ``Detector.predict(..., source_frame=True)`` added, as PNGs at source size under ``output_dir``:
    ``source_maps/{good,bad}/<name>.png`` (8-bit gray, the conversion of ``save_anomaly_maps``, its ``sigmas`` included),
    ``source_masks/`` (0 / 255) and, where there are overlays, ``overlays/`` (RGB)."""
    from PIL import Image
    k = 1.0 / B.SAVED_MAP_SIGMAS if sigmas else 1.0
    folders = [('source_maps', [M.to_u8_hwc((m * k if sigmas else m)[None, None], rgb_range=1.0)[0, :, :, 0] for m in res['maps_src']]),
               ('source_masks', [k * 255 for k in res['masks_src']])]
    if 'overlays' in res:
        folders.append(('overlays', res['overlays']))
    for folder, images in folders:
        for image, name, kind in zip(images, names, kinds):
            d = Path(output_dir) / folder / kind
            d.mkdir(parents=True, exist_ok=True)
            Image.fromarray(image.cpu().numpy()).save(str(d / f"{name}.png"))


def parse_predict_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description='Predict on raw images: calibrate a threshold on defect-free images, then flag and '
                                            'localise defects in new ones')
    p.add_argument('--model-type', type=str, default='drct', choices=['drct', 'drn-l'])
    p.add_argument('--classe', type=str, default='grid')
    p.add_argument('--scale', type=int, default=4)
    p.add_argument('--resolution', type=int, default=128)
    p.add_argument('--run-dir', type=str, default='')
    p.add_argument('--checkpoint', type=str, default='')
    p.add_argument('--ema', action='store_true', default=False, help="the averaged weights of a run trained with --ema (as evaluate.py)")
    p.add_argument('--dtype', type=str, default='bf16x3', choices=['fp32', 'bf16', 'bf16x3'])
    p.add_argument('--input', type=str, nargs='+', default=[], metavar='PATH', help="image files, or directories of images, to predict on")
    p.add_argument('--calibrate', type=str, default='', metavar='DIR',
                   help="calibrate the threshold on the defect-free images of DIR at --threshold-fpr and write "
                        f"<run-dir>/{OPERATING_POINT_FILE} (or <output-dir>/ without a run directory)")
    p.add_argument('--threshold-fpr', type=_open_unit_float, default=None, metavar='RATE', help="false-positive rate of --calibrate, in (0, 1)")
    p.add_argument('--threshold-level', type=str, default='pixel', choices=['pixel', 'image'],
                   help="what --calibrate calibrates on: every pixel of the maps, or each map's maximum")
    p.add_argument('--min-region-area', type=_positive_int, default=None, metavar='A',
                   help="remove predicted 8-connected components of fewer than A pixels (default: the calibrated file's, else 1)")
    p.add_argument('--threshold', type=_finite_or_inf_float, default=None, metavar='VALUE',
                   help=f"predict with this threshold instead of the one in {OPERATING_POINT_FILE}")
    p.add_argument('--map-source', type=str, default=None, choices=list(ALL_MAP_SOURCES))
    p.add_argument('--map-ws', type=int, default=None, help=f"window size of the anomaly maps (default {MAP_WS_DEFAULT}; there is no labelled sweep here)")
    p.add_argument('--map-scales', type=_map_scales, default=None, metavar='LIST|sweep')
    p.add_argument('--map-reduce', type=str, default=None, choices=['mean', 'max'])
    p.add_argument('--map-sigma', type=_nonnegative_float, default=None)
    p.add_argument('--self-ensemble', action='store_true', default=False)
    p.add_argument('--save-anomaly-maps', action='store_true', default=False)
    p.add_argument('--save-masks', action='store_true', default=False)
    p.add_argument('--save-images', action='store_true', default=False, help="write the SR images too")
    p.add_argument('--source-frame', action='store_true', default=False,
                   help="write every map and mask at its source image's own size too: source_maps/ and source_masks/ "
                        "(bilinear on the GPU; the decisions stay in the model's frame)")
    p.add_argument('--save-overlays', action='store_true', default=False,
                   help="write overlays/: the heat map and the mask's outline on every source image (implies --source-frame)")
    p.add_argument('--overlay-alpha', type=_unit_float, default=None, metavar='A',
                   help=f"opacity of the hottest level of the overlay, in [0, 1] (default {OVERLAY_ALPHA_DEFAULT})")
    p.add_argument('--overlay-contour', type=int, default=None, choices=range(5), metavar='R',
                   help=f"radius of the mask outline in pixels, 0..4, 0 draws none (default {OVERLAY_CONTOUR_DEFAULT})")
    p.add_argument('--save-regions', action='store_true', default=False,
                   help="write regions.csv: one row per predicted defect region (area, box, centroid, peak; with --source-frame "
                        "its box in the source image too)")
    p.add_argument('--output-dir', type=str, default='')
    add_tile_args(p)
    p.add_argument('--frame', type=_positive_int, nargs=2, default=None, metavar=('H', 'W'),
                   help="the model's frame: every source is resized to H x W (default: the square of --resolution); with --tile any "
                        "rectangle at least the scale on a side, without it what the network takes whole")
    add_baseline_args(p, '--baseline', "of --calibrate DIR; written as map_baseline.npz beside the operating point, which then "
                      "says so, and read back from there when predicting")
    args = p.parse_args(argv)
    check_tile_args(p, args)
    check_baseline_args(p, args, 'baseline', '--baseline')
    if args.map_source in GMS_MAP_SOURCES and (args.map_ws or args.map_scales):
        p.error(f"--map-source {args.map_source}: the GMS maps have no window (no --map-ws, no --map-scales); smooth with --map-sigma")
    if args.save_regions and not args.input:
        p.error("--save-regions lists the regions of --input images: give --input too")
    if (args.overlay_alpha is not None or args.overlay_contour is not None) and not args.save_overlays:
        p.error("--overlay-alpha and --overlay-contour shape what --save-overlays writes: give it too")
    args.source_frame = args.source_frame or args.save_overlays
    args.overlay_alpha = OVERLAY_ALPHA_DEFAULT if args.overlay_alpha is None else args.overlay_alpha
    args.overlay_contour = OVERLAY_CONTOUR_DEFAULT if args.overlay_contour is None else args.overlay_contour
    if args.ema and args.checkpoint:
        p.error("--ema and --checkpoint exclude each other (an explicit file is already a choice)")
    if not args.calibrate and not args.input:
        p.error("nothing to do: give --calibrate DIR, --input PATH..., or both")
    if bool(args.calibrate) != (args.threshold_fpr is not None):
        p.error("--calibrate DIR and --threshold-fpr RATE go together")
    if args.calibrate and args.threshold is not None:
        p.error("--calibrate and --threshold exclude each other (a calibrated threshold or a given one)")
    return args


def main(argv=None):
    return _run(parse_predict_args(argv))


def _note(det: Detector) -> str:
    """What the summary lines append with a baseline, '' without."""
    return det.baseline.note() if det.baseline is not None else ""


def _run(args) -> dict:
    model_type, class_name, resolution, scale = args.model_type, args.classe, args.resolution, args.scale
    if args.run_dir:
        inf = infer_from_run_dir(args.run_dir)
        model_type = inf.get('model_type') or model_type
        class_name = inf.get('classe') or class_name
        resolution = inf.get('resolution') or resolution
        scale = inf.get('scale') or scale
    out_dir = args.output_dir or (os.path.join(args.run_dir, 'predictions') if args.run_dir else './workspace/predictions')
    op_file = Path(args.run_dir or out_dir) / OPERATING_POINT_FILE
    stored = None
    if not args.calibrate and args.threshold is None:         # before the model is loaded
        if not op_file.is_file():
            raise SystemExit(f"no threshold: give --threshold, or calibrate first (--calibrate DIR --threshold-fpr RATE writes {op_file})")
        stored = read_operating_point(op_file)
        if args.self_ensemble and not stored['self_ensemble']:
            raise SystemExit(f"--self-ensemble contradicts the calibrated operating point ({op_file} was calibrated without it)")
    try:
        tile, frame = tile_from_args(args, stored)
        which_baseline = baseline_from_args(args, stored, op_file.parent)
        side = min(frame) if frame else int(resolution)       # what --map-scales sweep stands for
        spec = check_spec(spec_from_args(args, stored['map_spec'] if stored else None, side // int(scale) * int(scale)))
    except ValueError as e:
        raise SystemExit(str(e))
    self_ensemble = stored['self_ensemble'] if stored else args.self_ensemble
    min_area = args.min_region_area if args.min_region_area is not None else (stored['min_region_area'] if stored else 1)
    calib_files = list_images([args.calibrate]) if args.calibrate else []
    files = list_images(args.input)
    if args.calibrate and not calib_files:
        raise SystemExit(f"--calibrate: no image under {args.calibrate}")
    ckpt = resolve_checkpoint(args)
    if stored and stored.get('checkpoint') != os.path.basename(ckpt):
        print(f"Note: {op_file.name} was calibrated with {stored.get('checkpoint')}, these weights are {os.path.basename(ckpt)}")
    opt = build_opt(model_type, class_name, resolution, scale, 1, args.dtype, pre_train=ckpt)
    opt.test_only = True
    if tile:
        opt.tile, opt.tile_overlap, opt.tile_blend = tile
    from .model import Model
    try:
        model = Model(opt, None, dual_model=(model_type == 'drn-l'))
        det = Detector(opt, model, spec, threshold=stored['threshold'] if stored else args.threshold, min_area=min_area,
                       self_ensemble=self_ensemble, hr_size=frame or int(resolution), overlay_alpha=int(args.overlay_alpha * 255 + 0.5),
                       overlay_contour=args.overlay_contour)
        if which_baseline:
            det.set_baseline(load_baseline(which_baseline, det))
    except ValueError as e:
        raise SystemExit(str(e))
    out: dict = {}
    if args.calibrate:
        wrote = {}
        if args.baseline:                                     # fitted on DIR; the threshold then comes from DIR's leave-one-out maps
            try:
                fitted = det.fit_baseline(calib_files, B.FLOOR_REL_DEFAULT if args.baseline_floor is None else args.baseline_floor)
            except ValueError as e:
                raise SystemExit(f"--baseline: {e}")
            b_file = op_file.parent / B.BASELINE_FILE
            wrote = dict(baseline=baseline_entry(fitted, b_file, fitted.save(b_file, det.spec)))
        t, achieved = det.calibrate(calib_files, args.threshold_fpr, args.threshold_level)
        out['operating_point'] = write_operating_point(op_file, t, args.threshold_fpr, args.threshold_level, achieved, len(calib_files), min_area,
                                                       det.spec, self_ensemble, ckpt, tile=tile, frame=frame, **wrote)
        print(f"Calibrated - {det.spec.text()}{_note(det)}, threshold={t:.9g} (fpr {args.threshold_fpr:g} on {args.threshold_level}s of "
              f"{len(calib_files)} defect-free images, achieved {achieved:.6f}), min_area={min_area}: {op_file}")
    if files:
        names = unique_names(files)
        res = det.predict(files, source_frame=args.source_frame, overlays=args.save_overlays, regions=args.save_regions)
        out.update(res, names=names, files=[str(f) for f in files])
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, 'predictions.csv'), 'w', newline='') as fh:
            w = csv.writer(fh)
            w.writerow(['name', 'file', 'defective', 'defect_pixels', 'map_max', 'ssim', 'mse', 'psnr', 'threshold'])
            for k, name in enumerate(names):
                w.writerow([name, str(files[k]), int(res['defective'][k]), res['defect_pixels'][k], repr(res['map_max'][k]), repr(res['ssim'][k]),
                            repr(res['mse'][k]), repr(res['psnr'][k]), repr(det.threshold)])
        kinds = ['bad' if d else 'good' for d in res['defective']]        # the evaluator's folder names, by prediction
        sigmas = dict(sigmas=True) if det.baseline is not None else {}     # 8-bit maps of z-scores: z / 16 (baseline.SAVED_MAP_SIGMAS)
        if args.save_anomaly_maps:
            save_anomaly_maps(res['maps'], names, kinds, out_dir, **sigmas)
        if args.save_masks:
            save_masks(res['masks'], names, kinds, out_dir)
        if args.source_frame:
            save_source_frame(res, names, kinds, out_dir, **sigmas)
        if args.save_regions:
            write_regions_csv(os.path.join(out_dir, 'regions.csv'), res['regions'], names, kinds, res.get('src_box'))
        if args.save_images:
            sr_host = res['sr'].cpu().numpy()
            for k, name in enumerate(names):
                save_sr_image(sr_host[k], name, kinds[k], det.scale, out_dir)
        print(f"Predicted - {det.spec.text()}{_note(det)}, threshold={det.threshold:.9g}, min_area={min_area}: {sum(res['defective'])} of {len(files)} "
              f"images defective; {os.path.join(out_dir, 'predictions.csv')}" + (" (self-ensemble x8)" if self_ensemble else "")
              + tile_suffix(model))
    return out


if __name__ == "__main__":
    main()
