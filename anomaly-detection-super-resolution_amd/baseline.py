"""The per-pixel baseline of anomaly maps (DESIGN.md "Baseline"): the mean and spread of the map value at every pixel over
defect-free images, and the maps in sigmas of it.  A reconstruction-error map carries structure that sits in the same place
in every image of a fixed set-up - edges, fine lattice, frame borders - and one threshold for the whole frame has to clear
it; in sigmas a faint defect in a quiet area stands out.

``MapBaseline`` keeps the float64 sums on the GPU (``metrics.map_stats_accumulate``), derives the planes on the host in numpy
float64 from one copy of the sums per fit (``host_planes``), and applies them with ``metrics.normalize_maps`` - or, for the
maps the sums were made of, ``metrics.normalize_maps_loo``: in-sample z-scores are bounded by (N - 1) / sqrt(N), so a threshold
calibrated on them would fire on fresh good images."""
from __future__ import annotations

import hashlib
import json
import zipfile
from dataclasses import asdict
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import metrics as M

BASELINE_VERSION = 1
BASELINE_FILE = 'map_baseline.npz'
FLOOR_REL_DEFAULT = 0.1                                       # a user setting: the least spread, as a share of the pooled one
MIN_IMAGES = 3                                                # leave-one-out divides by N - 2
SAVED_MAP_SIGMAS = 16.0                                       # saved 8-bit maps of z-scores: z / 16, so 16 sigmas saturate


def check_floor_rel(floor_rel) -> float:
    f = float(floor_rel)
    if not (np.isfinite(f) and f > 0.0):
        raise ValueError(f"map baseline: floor_rel = {floor_rel}, must be finite and > 0")
    return f


def check_count(n: int) -> int:
    if int(n) < MIN_IMAGES:
        raise ValueError(f"map baseline: {int(n)} calibration map(s), at least {MIN_IMAGES} are needed")
    return int(n)


def host_planes(s1: np.ndarray, s2: np.ndarray, n: int, floor_rel: float) -> dict:
    """The planes of ``n`` maps' float64 sums, in numpy float64: mean = S1 / N, var = max(S2 - S1 * S1 / N, 0) / (N - 1),
    pooled = sqrt(mean of var), floor = floor_rel * pooled, sd = max(sqrt(var), floor); ``mu32`` = float32(mean), ``inv32`` =
    float32(1 / sd).  ValueError for fewer than 3 maps, a bad ``floor_rel`` and a pooled spread that is 0 or not finite."""
    n, floor_rel = check_count(n), check_floor_rel(floor_rel)
    s1, s2 = np.asarray(s1, dtype=np.float64), np.asarray(s2, dtype=np.float64)
    with np.errstate(all='ignore'):
        mean = s1 / n
        var = np.maximum(s2 - s1 * s1 / n, 0) / (n - 1)
        pooled = float(np.sqrt(var.mean()))
        if not np.isfinite(pooled) or pooled == 0.0:
            raise ValueError(f"map baseline: the calibration maps do not vary (pooled spread {pooled}); a baseline needs "
                             f"defect-free maps that differ from image to image and hold no NaN")
        floor = floor_rel * pooled
        sd = np.maximum(np.sqrt(var), floor)
        return dict(mu32=np.float32(mean), inv32=np.float32(1.0 / sd), floor=float(floor), pooled=pooled)


def spec_text(spec) -> str:
    """A ``MapSpec`` (or None) as the JSON text the saved baseline carries, its scales a list as in ``operating_point.json``."""
    return json.dumps(None if spec is None else dict(asdict(spec), scales=list(spec.scales)), sort_keys=True)


def file_sha256(path) -> str:
    return hashlib.sha256(Path(path).read_bytes()).hexdigest()


class MapBaseline:
    """Sums of ``n`` calibration maps and, once there are at least 3, their planes.  ``fit`` = ``update`` on a new baseline;
    ``update`` may be called again with more maps (the sums of chunks equal the sums of the whole stack bit for bit)."""

    def __init__(self, floor_rel: float = FLOOR_REL_DEFAULT):
        self.floor_rel = check_floor_rel(floor_rel)
        self.n, self.s1, self.s2, self._planes = 0, None, None, None

    @classmethod
    def fit(cls, maps: torch.Tensor, floor_rel: float = FLOOR_REL_DEFAULT) -> 'MapBaseline':
        b = cls(floor_rel)
        check_count(maps.shape[0] if maps.dim() == 3 else 0)
        b.update(maps)
        b.planes()                                            # a fit that cannot be applied fails here
        return b

    def update(self, maps: torch.Tensor) -> 'MapBaseline':
        if self.s1 is not None and tuple(maps.shape[1:]) != tuple(self.s1.shape):
            raise ValueError(f"map baseline: maps of {tuple(maps.shape[1:])}, the baseline is {tuple(self.s1.shape)}")
        self.s1, self.s2 = M.map_stats_accumulate(maps, self.s1, self.s2)
        self.n += int(maps.shape[0])
        self._planes = None
        return self

    @property
    def shape(self):
        return None if self.s1 is None else tuple(self.s1.shape)

    def planes(self) -> dict:
        """``host_planes`` of the sums (copied back once per fit) with ``mu`` and ``inv_sd`` on the sums' device."""
        if self._planes is None:
            p = host_planes(self.s1.cpu().numpy(), self.s2.cpu().numpy(), self.n, self.floor_rel)
            p['mu'] = torch.from_numpy(p['mu32']).to(self.s1.device)
            p['inv_sd'] = torch.from_numpy(p['inv32']).to(self.s1.device)
            self._planes = p
        return self._planes

    @property
    def floor(self) -> float:
        return self.planes()['floor']

    def _check_maps(self, maps: torch.Tensor) -> None:
        if maps.dim() != 3 or tuple(maps.shape[1:]) != self.shape:
            raise ValueError(f"map baseline: maps of {tuple(maps.shape)}, the baseline is {self.shape}")

    def apply(self, maps: torch.Tensor, with_max: bool = False, out: Optional[torch.Tensor] = None):
        """The maps in sigmas of the baseline (``metrics.normalize_maps``)."""
        p = self.planes()
        self._check_maps(maps)
        return M.normalize_maps(maps, p['mu'], p['inv_sd'], with_max=with_max, out=out)

    def apply_loo(self, maps: torch.Tensor, with_max: bool = False):
        """For maps that are part of the sums: each against the other ``n - 1`` (``metrics.normalize_maps_loo``)."""
        p = self.planes()
        self._check_maps(maps)
        return M.normalize_maps_loo(maps, self.s1, self.s2, self.n, p['floor'], with_max=with_max)

    def entries(self) -> dict:
        p = self.planes()
        return dict(map_baseline=dict(n_images=self.n, floor_rel=self.floor_rel, floor=p['floor'], pooled_sd=p['pooled']))

    def note(self) -> str:
        """What the printed map lines append."""
        return f" [baseline: {self.n} good images, floor {self.floor_rel:g}]"

    def save(self, path, spec=None) -> str:
        """``path`` (.npz): version, n, floor_rel, floor, the sums, and the map spec as JSON text.  Returns the file's sha256."""
        p = self.planes()
        Path(path).parent.mkdir(parents=True, exist_ok=True)
        with open(path, 'wb') as fh:
            np.savez(fh, version=np.int64(BASELINE_VERSION), n=np.int64(self.n), floor_rel=np.float64(self.floor_rel),
                     floor=np.float64(p['floor']), s1=self.s1.cpu().numpy(), s2=self.s2.cpu().numpy(), map_spec=np.array(spec_text(spec)))
        return file_sha256(path)


def load(path, device=None, shape=None, spec=None) -> MapBaseline:
    """The baseline ``MapBaseline.save`` wrote, its sums on ``device``: the planes are derived again and equal the fitted ones
    bit for bit.  ValueError for another version, for sums that are not [H, W] float64 planes of one shape or (``shape``
    given) not the maps' shape, for a map spec other than ``spec`` (given), and for a stored floor that the sums do not give."""
    try:
        with np.load(path, allow_pickle=False) as z:
            doc = {k: z[k] for k in ('version', 'n', 'floor_rel', 'floor', 's1', 's2', 'map_spec')}
    except KeyError as e:
        raise ValueError(f"{path}: entry {e} is missing")
    except (OSError, ValueError, EOFError, zipfile.BadZipFile) as e:
        raise ValueError(f"{path}: not a readable baseline file ({e})")
    if int(doc['version']) != BASELINE_VERSION:
        raise ValueError(f"{path}: version {int(doc['version'])}, this build reads version {BASELINE_VERSION}")
    s1, s2 = doc['s1'], doc['s2']
    if s1.dtype != np.float64 or s2.dtype != np.float64 or s1.ndim != 2 or s1.shape != s2.shape:
        raise ValueError(f"{path}: the sums are {s1.dtype} {s1.shape} and {s2.dtype} {s2.shape}, not two float64 [H, W] planes")
    if shape is not None and tuple(s1.shape) != tuple(shape):
        raise ValueError(f"{path}: the baseline is {tuple(s1.shape)}, the maps are {tuple(shape)}")
    if spec is not None and str(doc['map_spec']) != spec_text(spec):
        raise ValueError(f"{path}: the baseline was fitted on other maps ({str(doc['map_spec'])}, asked for {spec_text(spec)})")
    b = MapBaseline(float(doc['floor_rel']))
    b.n = check_count(int(doc['n']))
    b.s1 = torch.from_numpy(np.ascontiguousarray(s1))
    b.s2 = torch.from_numpy(np.ascontiguousarray(s2))
    if device is not None:
        b.s1, b.s2 = b.s1.to(device), b.s2.to(device)
    if b.planes()['floor'] != float(doc['floor']):
        raise ValueError(f"{path}: the stored floor {float(doc['floor'])!r} is not what the stored sums give ({b.planes()['floor']!r})")
    b.map_spec_text = str(doc['map_spec'])
    return b
