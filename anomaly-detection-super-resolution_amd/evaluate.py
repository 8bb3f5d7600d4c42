"""Standalone evaluator: SR every test image -> truncating u8 -> SSIM window sweep -> AUCs, the
flow of reference src/evaluate.py:138-267 with the SR forward and the whole scorer on the GPU.
Images of the test split are independent, so with ``--gpus N`` (one process per GPU under
``torch.distributed.run``) rank r scores images r::N and only the per-image score rows are gathered
(SURVEY.md §8(e)); there is no collective on the data path.

    python -m srad_amd.evaluate --run-dir <run> [--checkpoint f.pt | --ema] [--dtype bf16]

Deliberate, documented departures from the reference (SURVEY.md §8 hazards): the model is put in
eval mode (H1: the reference leaves DRCT's DropPath active, so its scores are not reproducible); the
u8 conversion truncates exactly as the reference's evaluator does (H2).
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, replace
from pathlib import Path
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import baseline as B
from . import metrics as M
from .model import Model
from .options import build_opt, parse_eval_args, set_tile_opt, tile_suffix


def infer_from_run_dir(run_dir: str) -> dict:
    """src/evaluate.py:48-122: directory-name pattern first, then config.txt overrides."""
    result = {'model_type': None, 'dataset': None, 'classe': None, 'resolution': None, 'scale': None}
    for seg in Path(run_dir).parts:
        if seg in ('drct', 'drn-l'):
            result['model_type'] = seg
            break
    m = re.match(r"(?P<ds>\w+)_(?P<cls>\w+)_(?P<res>\d+)_X(?P<scale>\d+)", Path(run_dir).name)
    if m:
        result.update(dataset=m.group('ds'), classe=m.group('cls'), resolution=int(m.group('res')), scale=int(m.group('scale')))
    cfg_path = Path(run_dir) / 'config.txt'
    if cfg_path.exists():
        lines = cfg_path.read_text().splitlines()

        def read_val(key):
            for line in lines:
                if line.strip().startswith(f"{key}:"):
                    return line.split(':', 1)[1].strip()
            return None
        for key, dst in (('model_name', 'model_type'), ('dataset', 'dataset'), ('classe', 'classe')):
            v = read_val(key)
            if v:
                result[dst] = v
        res = read_val('patch_size')
        if res and res.isdigit():
            result['resolution'] = int(res)
        scale_val = read_val('upscale') or read_val('scale')
        if scale_val:
            ms = re.findall(r"\d+", scale_val)
            if ms:
                result['scale'] = int(ms[-1])
    return result


def resolve_checkpoint(args) -> str:
    """src/evaluate.py:125-135.  ``--ema``: the averaged weights of the run directory (model_ema_best.pt, then
    model_ema_latest.pt) and nothing else - no fall-back to the raw weights."""
    if getattr(args, 'ema', False):
        names = ('model_ema_best.pt', 'model_ema_latest.pt')
        for name in names:
            cand = os.path.join(args.run_dir, 'model', name)
            if args.run_dir and os.path.isfile(cand):
                return cand
        where = os.path.join(args.run_dir, 'model') if args.run_dir else '<--run-dir>/model'
        raise FileNotFoundError(f"--ema: neither {names[0]} nor {names[1]} under {where} (a run trained with --ema writes them)")
    if args.checkpoint:
        return args.checkpoint
    if args.run_dir:
        for name in ('model_best.pt', 'model_latest.pt'):
            cand = os.path.join(args.run_dir, 'model', name)
            if os.path.isfile(cand):
                return cand
    raise FileNotFoundError('Please provide --checkpoint or a valid --run-dir containing model/*.pt')


def iter_split(data_root: str, classe: str, split: str, scale, n_colors: int, rgb_range: float = 255.0, part: str = 'test'
               ) -> Iterable[Tuple[str, np.ndarray, np.ndarray]]:
    """(name, LR u8 HWC, HR u8 HWC) of ``{root}/{class}/{part}/{split}`` (``part`` = 'test', or 'val' for the held-out
    defect-free images ``main.py`` validates on) read the way the reference's evaluator reads the test split
    (src/evaluate.py:140-150,204-217): the MVTec test loader (``data.MVTec(train=False)``: LR_{s} / LR_bicubic/X{s} / LR
    next to HR, ``set_channel``, HR cropped to LR * scale) and the TRUNCATING u8 conversion of the HR tensor.  The LR image
    is what the loader feeds the model, kept as u8 when it is integral (PNG input), so the forward sees the same values."""
    from .data import MVTec

    class _O:
        pass
    o = _O()
    o.scale = list(scale) if isinstance(scale, (list, tuple)) else [scale]
    o.data_dir = str(Path(data_root) / classe / part / split)
    o.n_colors, o.rgb_range, o.no_augment, o.patch_size, o.batch_size, o.test_every = n_colors, 255, True, 0, 1, 1
    ds = MVTec(o, train=False)
    for i in range(len(ds)):
        lr, hr, name = ds.sample(i)
        hr_u8 = hr.clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy()          # .byte(): truncation
        lr0 = lr[0].permute(1, 2, 0).numpy()
        yield name, (lr0.astype(np.uint8) if np.array_equal(lr0, np.floor(lr0)) and lr0.min() >= 0 and lr0.max() <= 255 else lr0), hr_u8


def save_sr_image(sr_u8_hwc: np.ndarray, name: str, split: str, scale_value: int, output_dir: str) -> None:
    """src/evaluate.py:193-202: ``<output_dir>/<split>/x<scale>/<name>.png`` of the truncated u8 SR image."""
    from PIL import Image
    out_dir = Path(output_dir) / split / f"x{scale_value}"
    out_dir.mkdir(parents=True, exist_ok=True)
    img = Image.fromarray(sr_u8_hwc[:, :, 0]) if sr_u8_hwc.shape[2] == 1 else Image.fromarray(np.ascontiguousarray(sr_u8_hwc))
    img.save(str(out_dir / f"{name}.png"))


def load_masks(data_root: str, classe: str, names: Sequence[Tuple[str, str]], hr_shapes: Sequence[Tuple[int, int]]
               ) -> Tuple[List[Optional[np.ndarray]], List[str]]:
    """Ground-truth masks of the test split for pixel-level metrics: ``names`` = (split, name) per image, ``hr_shapes`` = the
    (H, W) of its HR image as ``iter_split`` returns it.  Good images get all-zero masks; a bad image reads
    ``{root}/{class}/test/bad/GT/<name>.png`` (written by ``prepare_mvtec_data --with-masks``), cropped top-left to the HR size
    like the HR image.  Returns (masks: uint8 {0, 1} [H, W] arrays, None where a bad image has no usable mask; the names of
    those bad images)."""
    from PIL import Image
    masks: List[Optional[np.ndarray]] = []
    missing: List[str] = []
    for (split, name), (h, w) in zip(names, hr_shapes):
        if split == 'good':
            masks.append(np.zeros((h, w), dtype=np.uint8))
            continue
        f = Path(data_root) / classe / 'test' / 'bad' / 'GT' / f"{name}.png"
        m = None
        if f.is_file():
            with Image.open(f) as im:
                a = np.array(im.convert('L'))
            if a.shape[0] >= h and a.shape[1] >= w:
                m = (a[:h, :w] != 0).astype(np.uint8)
        if m is None:
            missing.append(name)
        masks.append(m)
    return masks, missing


def _save_gray(u8: np.ndarray, folder: str, names: Sequence[str], splits: Sequence[str], output_dir: str) -> None:
    """``<output_dir>/<folder>/{good,bad}/<name>.png`` of the 8-bit gray images ``u8`` [n,H,W]."""
    from PIL import Image
    for k, (name, split) in enumerate(zip(names, splits)):
        d = Path(output_dir) / folder / split
        d.mkdir(parents=True, exist_ok=True)
        Image.fromarray(u8[k]).save(str(d / f"{name}.png"))


def save_anomaly_maps(maps: torch.Tensor, names: Sequence[str], splits: Sequence[str], output_dir: str, sigmas: bool = False) -> None:
    """``<output_dir>/anomaly_maps/{good,bad}/<name>.png``: 8-bit gray of ``255 * clip(map, 0, 1)``, truncated (the u8 conversion
    of the evaluator at rgb_range 1).  ``sigmas``: the maps are z-scores of a baseline and ``z / baseline.SAVED_MAP_SIGMAS`` is
    what is converted, so negative values become 0 and 16 sigmas saturate."""
    if sigmas:
        maps = maps * (1.0 / B.SAVED_MAP_SIGMAS)
    _save_gray(M.to_u8_hwc(maps[:, None], rgb_range=1.0).cpu().numpy()[..., 0], 'anomaly_maps', names, splits, output_dir)


def save_masks(pred: torch.Tensor, names: Sequence[str], splits: Sequence[str], output_dir: str) -> None:
    """``<output_dir>/anomaly_masks/{good,bad}/<name>.png``: the predicted masks (uint8 {0, 1} [n,H,W]) as 8-bit gray, 0 / 255."""
    _save_gray((pred * 255).cpu().numpy(), 'anomaly_masks', names, splits, output_dir)

@dataclass
class OperatingPoint:
    """What ``evaluate_on_test(operating_point=...)`` takes (a dict with these keys does too): a given ``threshold``, or the
    rate ``fpr`` in (0, 1) to calibrate one at on the defect-free (LR, HR) u8 pairs ``calib`` - on all pixels of their maps
    (``level`` 'pixel') or on each map's maximum ('image'); ``min_area``: predicted components below it are removed;
    ``save_masks``: write the predicted masks under ``output_dir/anomaly_masks``.  ``region_metrics``: add the region-level
    counts of ``metrics.region_stats`` (DESIGN.md "Defect regions"), a ground-truth region counting as found at
    ``region_min_overlap`` of its pixels; ``save_regions``: then also write ``output_dir/regions.csv``."""
    threshold: Optional[float] = None
    fpr: Optional[float] = None
    level: str = 'pixel'
    min_area: int = 1
    save_masks: bool = False
    calib: Sequence[Tuple[np.ndarray, np.ndarray]] = ()
    region_metrics: bool = False
    region_min_overlap: float = 0.0
    save_regions: bool = False

    def check(self) -> 'OperatingPoint':
        if (self.threshold is None) == (self.fpr is None):
            raise ValueError("operating point: give either a threshold or a false-positive rate to calibrate one at")
        if self.threshold is not None and float(self.threshold) != float(self.threshold):
            raise ValueError("operating point: the threshold is NaN")
        if self.fpr is not None:
            M.rank_for_rate(1, self.fpr)                      # the rate's own check
        if self.level not in ('pixel', 'image'):
            raise ValueError(f"operating point: level = {self.level!r}, must be 'pixel' or 'image'")
        if int(self.min_area) < 1 or int(self.min_area) != self.min_area:
            raise ValueError(f"operating point: min_area = {self.min_area}, must be an integer >= 1")
        if not 0.0 <= float(self.region_min_overlap) <= 1.0:
            raise ValueError(f"operating point: region_min_overlap = {self.region_min_overlap}, must be in [0, 1]")
        if self.save_regions and not self.region_metrics:
            raise ValueError("operating point: save_regions belongs to region_metrics")
        return self


def val_good_dir(data_root: str, classe: str) -> Path:
    """Where the calibration images of ``--threshold-fpr`` live: the defect-free validation split of the prepared tree."""
    return Path(data_root) / classe / 'val' / 'good'


def resolve_map_scales(map_scales, H: int, W: int) -> List[int]:
    """The window sizes of ``--map-scales`` for H x W images: 'sweep' = ``metrics.sweep_window_sizes(min(H, W))``, otherwise the
    list itself; ValueError for a size the map kernels refuse at this image size (``metrics.check_map_scales``)."""
    if isinstance(map_scales, str):
        if map_scales != 'sweep':
            raise ValueError(f"map_scales = {map_scales!r}: a list of window sizes or 'sweep'")
        map_scales = M.sweep_window_sizes(min(H, W))
    return M.check_map_scales(map_scales, H, W)


@dataclass(frozen=True)
class MapSpec:
    """What the pixel-level anomaly maps are made of.  ``source``: 'ssim' = ``1 - SSIM map``, 'mse' = the squared-error maps of
    ``metrics.error_maps`` (DESIGN.md "Squared-error maps"), 'gms' / 'msgms' = the gradient-magnitude similarity maps of
    ``metrics.gms_maps`` at 1 / 4 levels, which have no window (``ws`` 0, no scales; ``levels``).
    One window size ``ws``, or ``scales`` in its place: a list of
    window sizes, or 'sweep' for every size of the image-level sweep, reduced per pixel by ``reduce`` ('mean' or 'max';
    ``metrics.anomaly_maps_multi``).  ``sigma`` > 0: the maps are smoothed once with that Gaussian sigma
    (``metrics.smooth_maps``) before anything is saved or scored.  ``ws`` 0 without scales means the SSIM sweep's best_ws for
    'ssim' - the one value only rank 0 knows (``needs_best_ws``) - and window size 1, the raw squared error, for 'mse'.
    The test images and the calibration images get their maps from one spec (``make``), and the spec words what it adds to
    the result (``entries``) and what the printed lines call the maps (``text``).  An unknown source is a ValueError
    when the spec is made, before anything else; ``resolve`` checks the rest against the image size."""
    source: str = 'ssim'
    ws: int = 0
    scales: object = ()
    reduce: str = 'mean'
    sigma: float = 0.0

    def __post_init__(self):
        if self.source not in M.MAP_SOURCES and self.source not in M.GMS_MAP_SOURCES:
            raise ValueError(f"map_source = {self.source!r}, must be one of {M.MAP_SOURCES + tuple(M.GMS_MAP_SOURCES)}")
        if self.levels and (int(self.ws) or isinstance(self.scales, str) or len(self.scales)):
            raise ValueError("the GMS maps have no window; smooth with map_sigma")

    @property
    def levels(self) -> int:
        """Pyramid levels of a GMS source ('gms' 1, 'msgms' 4); 0 for the windowed sources."""
        return M.GMS_MAP_SOURCES.get(self.source, 0)

    def check_sigma(self, H: int, W: int) -> None:
        """ValueError for a sigma that H x W maps cannot be smoothed with: negative, or a radius above min(128, H, W)."""
        if self.sigma:
            M.smooth_radius(self.sigma, H, W)

    def check_scales(self, H: int, W: int) -> List[int]:
        """The scales as a list of sizes; [] without scales, and ``reduce`` is then not looked at.  ValueError for scales together
        with a non-zero ``ws``, an unknown ``reduce``, and a size that H x W images are too small for."""
        if not (isinstance(self.scales, str) or len(self.scales)):
            return []
        if int(self.ws):
            raise ValueError("map_scales and a non-zero map_ws exclude each other")
        if self.reduce not in M.MAP_REDUCTIONS:
            raise ValueError(f"map_reduce = {self.reduce!r}, must be one of {M.MAP_REDUCTIONS}")
        return resolve_map_scales(self.scales, H, W)

    def resolve(self, H: int, W: int) -> 'MapSpec':
        """The spec for H x W images with its scales a list of sizes, after both checks."""
        self.check_sigma(H, W)
        if self.levels:
            M.check_gms_levels(self.levels, H, W)
        return replace(self, ws=int(self.ws), scales=self.check_scales(H, W), sigma=float(self.sigma))

    @property
    def needs_best_ws(self) -> bool:
        """The single case in which rank 0's sweep result has to reach the other ranks."""
        return self.source == 'ssim' and not self.scales and int(self.ws) <= 0

    def make(self, sr: torch.Tensor, hr: torch.Tensor, with_max: bool):
        """(maps of the (sr, hr) u8 stacks, their per-image maxima or None without ``with_max``)."""
        if self.levels:
            maps = M.gms_maps(sr, hr, self.levels)
        else:
            one, multi = (M.error_maps, M.error_maps_multi) if self.source == 'mse' else (M.anomaly_maps, M.anomaly_maps_multi)
            maps = multi(sr, hr, self.scales, self.reduce) if self.scales else one(sr, hr, self.ws)
        if with_max:
            return M.smooth_maps(maps, self.sigma, with_max=True)
        return (M.smooth_maps(maps, self.sigma) if self.sigma > 0 else maps), None

    def entries(self, found: dict) -> dict:
        """The result entries of these maps around ``found``: ``map_source`` (for 'mse' only), ``map_ws`` or ``map_scales`` and
        ``map_reduce``, then ``found``, then ``map_sigma`` when it is above 0."""
        if self.levels:
            out = dict(map_source=self.source, map_levels=self.levels, **found)
        else:
            out = dict(map_source=self.source) if self.source == 'mse' else {}
            out.update(dict(map_scales=list(self.scales), map_reduce=self.reduce) if self.scales else dict(map_ws=self.ws), **found)
        if self.sigma > 0:
            out["map_sigma"] = self.sigma
        return out

    def text(self, extra: str = '', always_sigma: bool = False) -> str:
        """What a printed line calls these maps, as in ``SSIM map (ws=11, fpr <= 0.3, sigma=4)``: ``extra`` comes before the
        sigma, which is left out at 0 unless ``always_sigma``."""
        what = f"levels={self.levels}" if self.levels else (f"scales={list(self.scales)}, {self.reduce}" if self.scales else f"ws={self.ws}")
        sigma = f", sigma={self.sigma:g}" if self.sigma > 0 or always_sigma else ""
        return f"{'GMS' if self.levels else 'MSE' if self.source == 'mse' else 'SSIM'} map ({what}{extra}{sigma})"


def shard_indices(n: int, rank: int, world: int) -> List[int]:
    """Images rank ``rank`` of ``world`` scores: r, r + world, ... (image-parallel, no data-path collective)."""
    return list(range(rank, n, world))


def gather_score_rows(mine: Sequence[int], rows: np.ndarray, total: int, rank: int, world: int):
    """Assemble the [total, n_ws + 2] score table on rank 0 from every rank's rows (the only
    cross-rank exchange of the evaluator: a few floats per image).  Other ranks get None."""
    if world == 1:
        return rows
    import torch.distributed as dist
    gathered = [None] * world
    dist.all_gather_object(gathered, (list(mine), rows))
    if rank != 0:
        return None
    full = np.zeros((total, rows.shape[1]), dtype=np.float64)
    seen = np.zeros(total, dtype=bool)
    for idx, r in gathered:
        full[idx] = r
        seen[idx] = True
    if not seen.all():
        raise RuntimeError("score rows missing after the gather")
    return full


@torch.no_grad()
def super_resolve_u8(model, lr_u8: Sequence[np.ndarray], hr_u8: Sequence[np.ndarray], rgb_range: float, batch: int = 0,
                     self_ensemble: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """collect_pairs (src/evaluate.py:204-224): forward, crop to the HR size, truncate to u8.
    Returns (sr, hr) uint8 stacks [n,H,W,C] on the GPU.  ``batch`` images per forward; 0 = as many as make ~64 k LR pixels
    (64 images at 128 px / x4, one 1024 px tile): the reference forwards one image at a time, the outputs per image are the same
    and the chip is only filled from a few thousand tokens up (78 pairs at 128 px: 1830 -> 2120 images/s in split-bf16 mode).
    ``self_ensemble``: the forwards go through ``model.forward_x8`` (``Model``; DESIGN.md "Self-ensemble"), whose stacked forward
    holds 8 members per image, so the automatic batch is an eighth; crop and u8 conversion come after the mean."""
    dev = model.device if hasattr(model, 'device') else next(model.parameters()).device
    if batch <= 0 and len(lr_u8):
        batch = _auto_batch(lr_u8[0].shape[0], lr_u8[0].shape[1], self_ensemble)
    forward = model.forward_x8 if self_ensemble else model
    sr_out: List[torch.Tensor] = []
    for i in range(0, len(lr_u8), batch):
        lr = torch.from_numpy(np.stack(lr_u8[i:i + batch])).to(dev).permute(0, 3, 1, 2).float() * (rgb_range / 255.0)   # np2Tensor
        sr_out.append(_forward_u8(forward, lr, hr_u8[i].shape[:2], rgb_range))
    hr = torch.from_numpy(np.stack(hr_u8)).to(dev)
    return torch.cat(sr_out), hr


def _auto_batch(lr_h: int, lr_w: int, self_ensemble: bool) -> int:
    """Images per forward when none is asked for: as many as make ~64 k LR pixels, an eighth of that under the self-ensemble."""
    batch = max(1, min(64, 65536 // max(1, lr_h * lr_w)))
    return max(1, batch // 8) if self_ensemble else batch


def _forward_u8(forward, lr: torch.Tensor, hr_hw, rgb_range: float) -> torch.Tensor:
    """One forward of ``lr`` [b,C,h,w] (already in [0, rgb_range]): the last output, cropped to the HR size, truncated to u8 HWC."""
    sr = forward(lr)
    if isinstance(sr, list):
        sr = sr[-1]
    return M.to_u8_hwc(sr[..., :hr_hw[0], :hr_hw[1]].contiguous(), rgb_range)


@torch.no_grad()
def super_resolve_dev(model, lr: torch.Tensor, hr_hw, rgb_range: float, batch: int = 0, self_ensemble: bool = False) -> torch.Tensor:
    """``super_resolve_u8`` for LR images that are on the GPU already: ``lr`` float32 [n,C,h,w] with values in [0, 255] (what
    ``np.stack(lr_u8)`` holds there, channels first), ``hr_hw`` the HR size to crop to.  The same batching, the same scaling by
    ``rgb_range / 255`` and the same forward and u8 conversion, so the SR stack uint8 [n,H,W,C] has ``super_resolve_u8``'s bits."""
    if batch <= 0 and len(lr):
        batch = _auto_batch(lr.shape[2], lr.shape[3], self_ensemble)
    forward = model.forward_x8 if self_ensemble else model
    return torch.cat([_forward_u8(forward, lr[i:i + batch].float() * (rgb_range / 255.0), hr_hw, rgb_range)
                      for i in range(0, len(lr), batch)])


@dataclass
class Shard:
    """One rank's share of the test split: the (sr, hr) u8 stacks of the images ``mine`` (indices into the whole split) next to
    what every rank knows of the whole split - the labels ``y_true`` and the ``names``, which may be fewer than the images."""
    sr: torch.Tensor
    hr: torch.Tensor
    mine: Sequence[int]
    y_true: Sequence[int]
    names: Sequence[str] = ()
    rank: int = 0
    world: int = 1
    output_dir: str = ''

    def my_names(self) -> List[str]:
        return [self.names[i] if i < len(self.names) else f"{i:05d}" for i in self.mine]

    def my_splits(self) -> List[str]:
        return ['good' if self.y_true[i] == 0 else 'bad' for i in self.mine]


@dataclass(frozen=True)
class Request:
    """What was asked of the pixel stage; ``op`` is a checked ``OperatingPoint`` or None."""
    save_maps: bool = False
    map_image_score: bool = False
    pixel_metrics: bool = False
    aupro: bool = False
    pro_fpr_limit: float = 0.3
    op: Optional[OperatingPoint] = None
    pr: bool = False

    @property
    def scored(self) -> bool:                                 # what needs a mask for every image
        return bool(self.pixel_metrics or self.aupro or self.pr)

    @property
    def single(self) -> bool:                                 # what runs on one rank only
        return self.scored or self.op is not None


def evaluate_on_test(opt, model, good: Sequence[Tuple[np.ndarray, np.ndarray]], bad: Sequence[Tuple[np.ndarray, np.ndarray]],
                     rank: int = 0, world: int = 1, names: Sequence[str] = (), output_dir: str = '', save_images: bool = False,
                     masks: Optional[Sequence[Optional[np.ndarray]]] = None, pixel_metrics: bool = False, save_maps: bool = False,
                     map_ws: int = 0, map_scales=(), map_reduce: str = 'mean', map_source: str = 'ssim', operating_point=None,
                     pr_metrics: bool = False, self_ensemble: bool = False, map_baseline=None, map_sigma: float = 0.0,
                     map_image_score: bool = False, aupro: bool = False, pro_fpr_limit: float = 0.3) -> dict:
    """src/evaluate.py:138-267 for in-memory (LR, HR) u8 pairs.  With world > 1 every rank scores its
    share r::world; rank 0 gathers the score rows and returns the AUCs (others return {}).  ``save_images``: every rank
    writes the SR images it produced under ``output_dir/{good,bad}/x{scale}`` (src/evaluate.py:190-224).

    Pixel level (off by default): the anomaly maps of each rank's own images as ``MapSpec`` describes them (``map_source``,
    ``map_ws``, ``map_scales``, ``map_reduce``, ``map_sigma``), and on them what ``_pixel_stage`` does with ``save_maps``,
    ``map_image_score``, ``pixel_metrics``, ``aupro`` (with ``pro_fpr_limit``), ``operating_point`` (an ``OperatingPoint`` or a
    dict of its fields) and the ``masks`` (good + bad order, as ``load_masks`` returns them).  ValueError for maps that cannot
    be made of these images and for an inconsistent operating point, before any image is super-resolved.

    ``pr_metrics`` (off by default): average precision and F1-max next to every AUC - of the three image scores (``ap_*``,
    ``f1max_*``, on rank 0 from the gathered table), of the map maximum with ``map_image_score``, and of the pixels
    (``_pixel_scores``) where the pixel metrics can run.

    ``self_ensemble`` (off by default): every SR image - test and calibration - is the x8 self-ensemble of the model
    (``Model.forward_x8``); the result then carries ``self_ensemble: True``.

    ``map_baseline`` (off by default; DESIGN.md "Baseline"): ``dict(calib=defect-free (LR, HR) u8 pairs, floor_rel=F)``.  A
    ``baseline.MapBaseline`` is fitted on the maps of the calibration pairs - at least 3, made by the resolved spec - and the
    test maps are put in sigmas of it before anything is saved or scored; per-image maxima are taken after that.  An
    operating point calibrated at a rate is then calibrated on these same pairs (its own ``calib`` may be left empty; one
    super-resolve pass serves both) and on their leave-one-out maps.  One rank only: ValueError with ``world`` > 1, before
    any image is super-resolved.  The result gains ``map_baseline`` and the printed map lines `` [baseline: ...]``."""
    spec = MapSpec(source=map_source, ws=map_ws, scales=map_scales, reduce=map_reduce, sigma=map_sigma)
    op = None
    if operating_point is not None:
        op = (OperatingPoint(**operating_point) if isinstance(operating_point, dict) else operating_point).check()
        if map_baseline is not None and op.fpr is not None:
            op = _calib_of_baseline(op, map_baseline)
        if op.fpr is not None and world == 1 and not len(op.calib):
            raise ValueError("operating point: a false-positive rate needs calibration pairs (defect-free images)")
    want = Request(save_maps=save_maps, map_image_score=map_image_score, pixel_metrics=pixel_metrics, aupro=aupro,
                   pro_fpr_limit=pro_fpr_limit, op=op, pr=pr_metrics)
    if map_baseline is not None:
        floor_rel = _check_baseline_request(map_baseline, world)
    pairs = list(good) + list(bad)
    if pairs:
        spec = spec.resolve(*pairs[0][1].shape[:2])
    model.eval()                                              # H1: deterministic scoring
    y_true = [0] * len(good) + [1] * len(bad)
    if len(set(y_true)) < 2:
        print('Test set lacks both classes; AUC not available')
        return {}
    mine = shard_indices(len(pairs), rank, world)
    x8 = dict(self_ensemble=True) if self_ensemble else {}    # off: the call as it always was
    sr, hr = super_resolve_u8(model, [pairs[i][0] for i in mine], [pairs[i][1] for i in mine], float(opt.rgb_range), **x8)
    shard = Shard(sr=sr, hr=hr, mine=mine, y_true=y_true, names=names, rank=rank, world=world, output_dir=output_dir)
    if save_images and output_dir:
        scale_value = opt.scale[-1] if isinstance(opt.scale, list) else int(opt.scale)
        sr_host = sr.cpu().numpy()
        for k, (name, split) in enumerate(zip(shard.my_names(), shard.my_splits())):
            save_sr_image(sr_host[k], name, split, scale_value, output_dir)
    H, W = hr.shape[1:3]
    sizes = M.sweep_window_sizes(min(H, W))
    ssim, mse, psnr = M.score_pairs(sr, hr, sizes)
    rows = torch.cat([ssim, mse[:, None], psnr[:, None]], dim=1)          # [n_mine, n_ws + 2] float64
    full = gather_score_rows(mine, rows.cpu().numpy(), len(pairs), rank, world)
    if full is None:
        _pixel_stage(shard=shard, spec=spec, want=want, masks=masks, best_ws=None)     # its collectives, on every rank
        return {}
    best_j, sweep = M.best_window(y_true, full, sizes)
    best_ws = sizes[best_j]
    out = dict(best_ws=best_ws, auc_ssim=sweep[best_j], auc_mse=M.roc_auc(y_true, full[:, -2]),
               auc_psnr=M.roc_auc(y_true, -full[:, -1]), n_images=len(pairs), window_sizes=sizes)
    if self_ensemble:
        out["self_ensemble"] = True
    if getattr(model, 'tile', 0):                             # tiled inference is the model's own setting (Model.forward_tiled)
        out["tile"] = [int(model.tile), int(model.tile_overlap), str(model.tile_blend)]
    print(f"Test AUCs - SSIM(best ws={best_ws}): {out['auc_ssim']:.4f}, MSE: {out['auc_mse']:.4f}, PSNR: {out['auc_psnr']:.4f}"
          + (" (self-ensemble x8)" if self_ensemble else "") + tile_suffix(model))
    if want.pr:                                               # the AUCs' score orientation: 1 - SSIM at best_ws, MSE, -PSNR
        cols = (("ssim", 1.0 - full[:, best_j]), ("mse", full[:, -2]), ("psnr", -full[:, -1]))
        pr = {k: M.average_precision(y_true, s) for k, s in cols}
        out.update({f"ap_{k}": v[0] for k, v in pr.items()}, **{f"f1max_{k}": v[1] for k, v in pr.items()})
        print(f"Test APs - SSIM(best ws={best_ws}): {out['ap_ssim']:.4f}, MSE: {out['ap_mse']:.4f}, PSNR: {out['ap_psnr']:.4f}; "
              f"F1-max - SSIM: {out['f1max_ssim']:.4f}, MSE: {out['f1max_mse']:.4f}, PSNR: {out['f1max_psnr']:.4f}")
    calib = None
    if op is not None and op.fpr is not None and world == 1:          # the calibration images go the test images' way
        calib = super_resolve_u8(model, [lr for lr, _ in op.calib], [h for _, h in op.calib], float(opt.rgb_range), **x8)
    if map_baseline is None:
        out.update(_pixel_stage(shard=shard, spec=spec, want=want, masks=masks, best_ws=best_ws, calib=calib))
        return out
    if calib is None:                                         # with a calibrated operating point its pass serves both
        pairs_c = map_baseline['calib']
        calib = super_resolve_u8(model, [lr for lr, _ in pairs_c], [h for _, h in pairs_c], float(opt.rgb_range), **x8)
    out.update(_pixel_stage(shard=shard, spec=spec, want=want, masks=masks, best_ws=best_ws, calib=calib, floor_rel=floor_rel))
    return out


def _check_baseline_request(map_baseline, world: int) -> float:
    """The checks of ``evaluate_on_test(map_baseline=...)`` that need no GPU; returns its floor_rel."""
    if not isinstance(map_baseline, dict) or set(map_baseline) - {'calib', 'floor_rel'} or 'calib' not in map_baseline:
        raise ValueError("map_baseline: a dict(calib=defect-free (LR, HR) pairs, floor_rel=F)")
    if world > 1:
        raise ValueError("map_baseline needs one rank (the baseline is fitted and applied where the maps are, like the operating point)")
    floor_rel = map_baseline.get('floor_rel')
    floor_rel = B.check_floor_rel(B.FLOOR_REL_DEFAULT if floor_rel is None else floor_rel)
    B.check_count(len(map_baseline['calib']))
    return floor_rel


def _calib_of_baseline(op: OperatingPoint, map_baseline) -> OperatingPoint:
    """With a baseline, a rate is calibrated on the baseline's own calibration pairs (leave-one-out): the operating point's
    ``calib`` is filled from them where it is empty, and must be them where it is not."""
    pairs_c = map_baseline.get('calib', ()) if isinstance(map_baseline, dict) else ()
    if len(op.calib):
        same = len(op.calib) == len(pairs_c) and all(a is c or (np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]))
                                                      for a, c in zip(op.calib, pairs_c))
        if not same:
            raise ValueError("operating point: with map_baseline the rate is calibrated on the baseline's calibration pairs "
                             "(leave-one-out); its own calib must be those pairs, or empty")
        return op
    return replace(op, calib=pairs_c)


def _pixel_stage(shard: Shard, spec: MapSpec, want: Request, masks, best_ws, calib=None, floor_rel=None) -> dict:
    """The anomaly maps of this rank's images and what was asked for on them: saved maps and the map-maximum image AUC on any
    number of ranks; the pixel-level AUC, AU-PRO and the operating point (``calib`` = the (sr, hr) u8 stacks of its
    calibration pairs) on a single rank.  ``spec`` is resolved; ``best_ws`` is None off rank 0.  Every branch that leads to a
    collective depends only on ``spec``, ``want`` and ``shard.world``, which all ranks share, so all ranks make the same
    collective calls: at most one broadcast (``_with_window``) and one gather (``_map_max_auc``).

    ``floor_rel`` (a single rank only, with ``calib``): a ``baseline.MapBaseline`` is fitted on the maps of ``calib`` - made by
    the spec after ``_with_window`` - and the test maps and their maxima are the normalised ones from here on."""
    found, maps, bl, cmaps, note = {}, None, None, None, ''
    if want.save_maps or want.map_image_score or (want.single and shard.world == 1):      # what needs the maps here
        spec = _with_window(spec, best_ws, shard.world)
        if floor_rel is None:
            maps, img_max = spec.make(shard.sr, shard.hr, want.map_image_score)
        else:
            cmaps, _ = spec.make(calib[0], calib[1], False)
            bl = B.MapBaseline.fit(cmaps, floor_rel)
            maps, _ = spec.make(shard.sr, shard.hr, False)
            maps, img_max = bl.apply(maps, with_max=True, out=maps)
            found, note = bl.entries(), bl.note()
        if want.save_maps and shard.output_dir:
            save_anomaly_maps(maps, shard.my_names(), shard.my_splits(), shard.output_dir, **(dict(sigmas=True) if bl else {}))
        if want.map_image_score:
            found = dict(found, **_map_max_auc(shard, spec, img_max, want.pr, note))
    runs, labels = _single_rank_gate(shard, want, masks, best_ws, maps)
    if not runs:
        return spec.entries(found) if found else {}
    out = spec.entries(found)
    out.update(_pixel_scores(spec, want, maps, labels, note))
    if want.op is not None:
        out.update(_operating_point(shard, spec, want.op, maps, labels, calib, note, bl, cmaps))
    return out


def _with_window(spec: MapSpec, best_ws, world: int) -> MapSpec:
    """The spec with its one window size filled in (scales have none): the sweep's best_ws, which only rank 0 has and
    broadcasts, where ``spec.needs_best_ws`` - a fact about the SSIM score - and at least 1 otherwise."""
    if spec.needs_best_ws:
        if world > 1:
            import torch.distributed as dist
            box = [best_ws]
            dist.broadcast_object_list(box, src=0)
            best_ws = int(box[0])
        return replace(spec, ws=best_ws)
    return spec if spec.scales or spec.levels else replace(spec, ws=max(spec.ws, 1))      # the GMS maps have no window


def _map_max_auc(shard: Shard, spec: MapSpec, img_max: torch.Tensor, pr: bool = False, note: str = '') -> dict:
    """``auc_map_max``, the ROC-AUC of each image's map maximum: every rank's maxima are gathered to rank 0 like the score
    rows (one more gather, one column); {} on the other ranks.  No masks needed.  ``pr``: also ``ap_map_max`` and
    ``f1max_map_max`` of the same gathered maxima."""
    full = gather_score_rows(shard.mine, img_max.double().cpu().numpy()[:, None], len(shard.y_true), shard.rank, shard.world)
    if full is None:
        return {}
    auc = M.roc_auc(shard.y_true, full[:, 0])
    print(f"Image AUC - max of the {spec.text(always_sigma=True)}{note}: {auc:.4f}")
    if not pr:
        return dict(auc_map_max=auc)
    ap, f1 = M.average_precision(shard.y_true, full[:, 0])
    print(f"Image AP - max of the {spec.text(always_sigma=True)}{note}: {ap:.4f}, F1-max: {f1:.4f}")
    return dict(auc_map_max=auc, ap_map_max=ap, f1max_map_max=f1)


def _single_rank_gate(shard: Shard, want: Request, masks, best_ws, maps):
    """(whether what runs on one rank only runs here, the ground-truth stack of this rank's images or None).  It runs where
    it was asked for and the sweep's result is (rank 0), on a single rank - the maps and masks are not gathered - and, but for
    the operating point, which then reports the image level only, with a mask of the images' size for every image."""
    if not want.single or best_ws is None:
        return False, None
    if shard.world > 1:
        print("Pixel metrics need --gpus 1 (the maps and masks are not gathered across ranks); skipped")
        return False, None
    lacking = [i for i in range(len(shard.y_true)) if masks is None or i >= len(masks) or masks[i] is None]
    if lacking:
        if want.scored:
            print(f"Pixel metrics skipped: {len(lacking)} test image(s) have no ground-truth mask")
        return want.op is not None, None
    H, W = maps.shape[1:]
    for i in shard.mine:
        if tuple(masks[i].shape) != (H, W):
            raise ValueError(f"mask {i} has shape {tuple(masks[i].shape)}, the images are {H}x{W}")
    return True, torch.from_numpy(np.stack([np.asarray(masks[i]) for i in shard.mine])).to(maps.device)


def _pixel_scores(spec: MapSpec, want: Request, maps: torch.Tensor, labels, note: str = '') -> dict:
    """``auc_pixel``, the exact pixel-level ROC-AUC, ``aupro`` with ``pro_fpr_limit``, the normalised area under the
    per-region overlap curve up to that limit, and ``ap_pixel`` with the best-F1 point of ``metrics.pixel_pr`` (``f1max_pixel``,
    its ``f1max_pixel_precision`` and ``f1max_pixel_recall``, and ``f1max_pixel_threshold``, which ``--threshold`` takes: predict
    iff map > it): each where asked for and ``labels`` are there."""
    out = {}
    if want.pixel_metrics and labels is not None:
        out["auc_pixel"] = M.pixel_roc_auc(maps, labels)
        print(f"Pixel AUC - {spec.text()}{note}: {out['auc_pixel']:.4f}")
    if want.aupro and labels is not None:
        limit = float(want.pro_fpr_limit)
        out["aupro"], out["pro_fpr_limit"] = M.aupro(maps, labels, want.pro_fpr_limit), limit
        print(f"AU-PRO - {spec.text(f', fpr <= {limit:g}')}{note}: {out['aupro']:.4f}")
    if want.pr and labels is not None:
        r = M.pixel_pr(maps, labels)
        out.update(ap_pixel=r["ap"], f1max_pixel=r["f1max"], f1max_pixel_threshold=r["threshold"],
                   f1max_pixel_precision=r["precision"], f1max_pixel_recall=r["recall"])
        print(f"Pixel AP - {spec.text()}{note}: {r['ap']:.4f}, F1-max: {r['f1max']:.4f} (precision={r['precision']:.4f} "
              f"recall={r['recall']:.4f} at threshold={r['threshold']:.9g})")
    return out


def _operating_point(shard: Shard, spec: MapSpec, op: OperatingPoint, maps: torch.Tensor, labels, calib, note: str = '',
                     baseline=None, calib_maps=None) -> dict:
    """The maps thresholded (DESIGN.md "Operating point") at the given threshold, or at the one that the maps of the
    calibration stacks - made by the same ``spec`` - give at the asked false-positive rate: ``threshold``,
    ``threshold_source`` ('given' or 'fpr'; then also ``threshold_fpr``, ``threshold_level``, ``calib_images`` and
    ``calib_rate``, the rate achieved on the calibration values), ``min_region_area``, the image-level counts and rates of
    ``metrics.operating_point_stats`` and, with ``labels``, its pixel-level ones; the masks are saved where asked for.  With
    ``op.region_metrics`` also the entries of ``metrics.region_stats`` and ``region_min_overlap``, from the table of the
    predicted regions against ``labels`` and the table of the ground-truth regions against the prediction (without ``labels``
    every image counts as all-ok: no ground-truth region, every predicted region a false alarm).  With a ``baseline`` (fitted
    on ``calib_maps``, the maps of ``calib``; ``maps`` are in its sigmas) a rate is calibrated on the leave-one-out maps."""
    if op.fpr is not None and baseline is not None:
        cmaps, cmax = baseline.apply_loo(calib_maps, with_max=True)
    elif op.fpr is not None:
        cmaps, cmax = spec.make(calib[0], calib[1], op.level == 'image')
    if op.fpr is not None:
        t, achieved = M.map_threshold(cmax if op.level == 'image' else cmaps, op.fpr)
        out = dict(threshold=t, threshold_source='fpr', threshold_fpr=float(op.fpr), threshold_level=op.level,
                   calib_images=int(cmaps.shape[0]), calib_rate=achieved)
        src = f"fpr {float(op.fpr):g} on {op.level}s of {cmaps.shape[0]} defect-free images, achieved {achieved:.6f}"
    else:
        t = float(op.threshold)
        out, src = dict(threshold=t, threshold_source='given'), "given"
    out["min_region_area"] = int(op.min_area)
    pred, img_pred, counts = M.operating_point(maps, t, labels, int(op.min_area))
    st = M.operating_point_stats(counts if labels is not None else None, img_pred, [shard.y_true[i] for i in shard.mine])
    out.update(st)
    line = (f"Operating point - {spec.text()}{note}, threshold={t:.9g} ({src}), min_area={int(op.min_area)}: "
            f"image tp={st['image_tp']} fp={st['image_fp']} fn={st['image_fn']} tn={st['image_tn']} "
            f"tpr={st['image_tpr']:.4f} fpr={st['image_fpr']:.4f}")
    if labels is not None:
        line += (f"; pixel tp={st['pixel_tp']} fp={st['pixel_fp']} fn={st['pixel_fn']} tn={st['pixel_tn']} "
                 f"precision={st['precision']:.4f} recall={st['recall']:.4f} f1={st['f1']:.4f} iou={st['iou']:.4f} "
                 f"fpr={st['fpr']:.6f} pro={st['pro_at_threshold']:.4f}")
    print(line)
    if op.save_masks and shard.output_dir:
        save_masks(pred, shard.my_names(), shard.my_splits(), shard.output_dir)
    if op.region_metrics:
        out.update(_region_metrics(shard, op, maps, pred, labels))
    return out


def _region_metrics(shard: Shard, op: OperatingPoint, maps: torch.Tensor, pred: torch.Tensor, labels) -> dict:
    """``metrics.region_stats`` of the surviving prediction ``pred`` against ``labels`` (None: no defect anywhere), the
    ``Regions - ...`` line, and ``regions.csv`` where asked for."""
    ptab = M.region_table(pred, maps, labels)
    gtab = M.region_table(labels if labels is not None else torch.zeros_like(pred), None, pred)
    y = [shard.y_true[i] for i in shard.mine]
    st = M.region_stats(ptab, gtab, len(y), y, float(op.region_min_overlap))
    out = dict(st, region_min_overlap=float(op.region_min_overlap))
    print(f"Regions - predicted={st['region_pred']} hit={st['region_hit']} precision={st['region_precision']:.4f} "
          f"false_alarms={st['region_false_alarms']} per_image={st['false_alarms_per_image']:.4f} "
          f"on_good={st['false_alarms_on_good']}; ground truth={st['region_gt']} found={st['region_found']} "
          f"recall={st['region_recall']:.4f} (min_overlap={float(op.region_min_overlap):g})")
    if op.save_regions and shard.output_dir:
        from .predict import write_regions_csv
        if labels is not None:
            ptab = dict(ptab, gt_overlap=ptab['overlap'])
        write_regions_csv(os.path.join(shard.output_dir, 'regions.csv'), ptab, shard.my_names(), shard.my_splits())
    return out


def main(argv=None):
    args = parse_eval_args(argv)
    from .launch import spawn
    if spawn(_run, getattr(args, "gpus", 1), (args,)):      # --gpus N without a launcher: N fresh ranks (image-parallel)
        return
    return _run(args)                                        # evaluate_on_test's dict ({} off rank 0)


def _run(args):
    model_type, class_name, resolution, scale = args.model_type, args.classe, args.resolution, args.scale
    if args.run_dir:
        inf = infer_from_run_dir(args.run_dir)
        model_type = inf.get('model_type') or model_type
        class_name = inf.get('classe') or class_name
        resolution = inf.get('resolution') or resolution
        scale = inf.get('scale') or scale
    if args.device == 'cpu':
        raise SystemExit("--device cpu is the reference's own path; this build has no CPU fallback")
    spec = MapSpec(source=args.map_source, ws=args.map_ws, scales=args.map_scales, reduce=args.map_reduce, sigma=args.map_sigma)
    if resolution:                                            # before the model and the data are loaded
        levels = (lambda H, W: M.check_gms_levels(spec.levels, H, W)) if spec.levels else (lambda H, W: None)
        for flag, check in ((f"--map-sigma {args.map_sigma:g}", spec.check_sigma), ("--map-scales", spec.check_scales),
                            (f"--map-source {args.map_source}", levels)):
            try:
                check(int(resolution), int(resolution))
            except ValueError as e:
                raise SystemExit(f"{flag}: {e}")
    want_op = args.threshold is not None or args.threshold_fpr is not None
    want_baseline = bool(getattr(args, 'map_baseline', False))
    if want_baseline and int(os.environ.get('WORLD_SIZE', '1')) > 1:      # before the model is loaded
        raise SystemExit("--map-baseline needs --gpus 1 (the baseline is fitted and applied on one rank, like the operating point)")
    if args.threshold_fpr is not None or want_baseline:       # before the model is loaded
        data_root = args.data_root if args.data_root != 'auto' else f"data/mvtec_{resolution}"
        val_dir = val_good_dir(data_root, class_name)
        n_val = len(list((val_dir / 'HR').glob('*.png')))
        if not n_val and args.threshold_fpr is not None:
            raise SystemExit(f"--threshold-fpr calibrates on defect-free images, and there is none under {val_dir} "
                             f"(HR/*.png with LR_<scale> beside it, as prepare_mvtec_data writes the validation split)")
        if want_baseline and n_val < B.MIN_IMAGES:
            raise SystemExit(f"--map-baseline fits on defect-free images, and there are {n_val} under {val_dir}, fewer than {B.MIN_IMAGES} "
                             f"(HR/*.png with LR_<scale> beside it, as prepare_mvtec_data writes the validation split)")
    ckpt = resolve_checkpoint(args)
    world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
        dist.init_process_group('nccl')
    opt = build_opt(model_type, class_name, resolution, scale, args.batch_size, args.dtype, pre_train=ckpt,
                    data_root=args.data_root)
    opt.test_only = True
    set_tile_opt(opt, args)
    try:
        model = Model(opt, None, dual_model=(model_type == 'drn-l'))
    except ValueError as e:                                   # a tile setting the network cannot take (not a multiple of its window)
        if not getattr(args, 'tile', 0):
            raise
        raise SystemExit(f"--tile {args.tile} --tile-overlap {args.tile_overlap}: {e}")
    g = list(iter_split(opt.data_root, class_name, 'good', opt.scale, opt.n_colors))
    b = list(iter_split(opt.data_root, class_name, 'bad', opt.scale, opt.n_colors))
    out_dir = args.output_dir or (os.path.join(args.run_dir, 'eval_results') if args.run_dir else './workspace/eval_results')
    masks = None
    if (args.pixel_metrics or args.aupro or args.pr_metrics or want_op) and world == 1:
        masks, missing = load_masks(opt.data_root, class_name, [('good', n) for n, _, _ in g] + [('bad', n) for n, _, _ in b],
                                    [hr.shape[:2] for _, _, hr in g + b])
        if missing:
            print(f"No ground-truth mask for {len(missing)} bad image(s) under test/bad/GT (prepare_mvtec_data --with-masks), "
                  f"e.g. {missing[0]}")
    op = None
    calib = []
    if (args.threshold_fpr is not None or want_baseline) and world == 1:      # more ranks skip the operating point: nothing to read
        calib = [(lr, hr) for _, lr, hr in iter_split(opt.data_root, class_name, 'good', opt.scale, opt.n_colors, part='val')]
    baseline = dict(map_baseline=dict(calib=calib, floor_rel=getattr(args, 'baseline_floor', None))) if want_baseline else {}
    if want_op:
        op = OperatingPoint(threshold=args.threshold, fpr=args.threshold_fpr, level=args.threshold_level,
                            min_area=args.min_region_area, save_masks=args.save_masks, calib=calib,
                            region_metrics=args.region_metrics, region_min_overlap=args.region_min_overlap,
                            save_regions=args.save_regions)
    out = evaluate_on_test(opt, model, [(lr, hr) for _, lr, hr in g], [(lr, hr) for _, lr, hr in b], rank, world,
                           names=[n for n, _, _ in g] + [n for n, _, _ in b], output_dir=out_dir, save_images=args.save_images,
                           masks=masks, pixel_metrics=args.pixel_metrics, save_maps=args.save_anomaly_maps, map_ws=args.map_ws,
                           aupro=args.aupro, pro_fpr_limit=args.pro_fpr_limit, map_sigma=args.map_sigma,
                           map_image_score=args.map_image_score, map_scales=args.map_scales, map_reduce=args.map_reduce,
                           map_source=args.map_source, operating_point=op, pr_metrics=args.pr_metrics,
                           self_ensemble=args.self_ensemble, **baseline)
    if getattr(args, 'ema', False) and out:                   # rank 0's result says which weights it is of
        out['ema'] = True
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return out


if __name__ == "__main__":
    main()
