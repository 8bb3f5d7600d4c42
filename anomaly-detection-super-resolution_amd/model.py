"""Model registry + wrapper: drop-in for reference src/model.py (``make_model`` 46-52, ``Model``
54-170, dual ``DownBlock`` 8-44) whose networks run on the HIP engine."""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from .nets import DRCT, DRN, DownBlock  # noqa: F401  (DownBlock re-exported like the reference module)


def make_model(opt):
    """src/model.py:46-52 - unknown names print and return None, as the reference does."""
    if opt.model_name == 'drct':
        return DRCT(opt)
    elif opt.model_name == 'drn-l':
        return DRN(opt)
    else:
        print(f"No model with this name: {opt.model_name}")


class _NullLog:
    log_file = None

    def write_log(self, msg, refresh=False):
        print(msg)


class Model(nn.Module):
    """Same attributes and methods as the reference wrapper: ``forward(x, idx_scale=0)``, ``device``,
    ``model``, ``dual_models``, ``get_model()``, ``state_dict()``, ``save(path, is_best)``,
    ``load(pre_train, pre_train_dual, cpu)``, ``count_parameters(model)``."""

    def __init__(self, opt, ckp=None, dual_model=False):
        super().__init__()
        print('Making model...')
        ckp = ckp or _NullLog()
        self.opt = opt
        self.scale = opt.scale
        self.idx_scale = 0
        self.self_ensemble = getattr(opt, 'self_ensemble', False)
        # tiled inference (DESIGN.md "Tiled inference"): off at tile 0; tile_batch = tiles per network call, 0 = by the tile's size
        self.tile = int(getattr(opt, 'tile', 0) or 0)
        self.tile_overlap = int(getattr(opt, 'tile_overlap', 0) or 0)
        self.tile_blend = getattr(opt, 'tile_blend', 'mean') or 'mean'
        self.tile_batch = 0
        self.cpu = getattr(opt, 'cpu', False)
        if self.cpu:
            raise RuntimeError("--device cpu: this build runs the SR path on the HIP engine only; the CPU path is "
                               "the reference itself (or oracle/ for tests).  There is no CPU fallback.")
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the HIP engine cannot run (there is no CPU fallback)")
        self.device = torch.device('cuda', torch.cuda.current_device())
        ckp.write_log(f"Using device: {self.device}")
        self.n_GPUs = getattr(opt, 'n_GPUs', 1)
        self.dual_model = dual_model
        self.model = make_model(opt).to(self.device)
        if self.dual_model:
            self.dual_models = []
            for _ in self.opt.scale:
                self.dual_models.append(DownBlock(opt, 2).to(self.device))
        if self.tile:                                         # refused before anything runs: a ValueError names the setting
            from . import ops
            if self.tile_blend not in ('mean', 'feather'):
                raise ValueError(f"tile_blend {self.tile_blend!r}: one of 'mean', 'feather'")
            scales = opt.scale if isinstance(opt.scale, (list, tuple)) else [opt.scale]
            ops.tile_plan(1, 1, self.tile, self.tile_overlap, self.model.granule, max(int(s) for s in scales))
        elif self.tile_overlap or self.tile_blend != 'mean':
            raise ValueError("tile_overlap / tile_blend are settings of tiled inference: set tile > 0")
        self.load(getattr(opt, 'pre_train', '.'), getattr(opt, 'pre_train_dual', '.'), cpu=False)
        if not getattr(opt, 'test_only', False) and getattr(ckp, 'log_file', None) is not None:
            print(self.model, file=ckp.log_file)
            if self.dual_model:
                print(self.dual_models, file=ckp.log_file)
        num_parameter = self.count_parameters(self.model)
        ckp.write_log(f"The number of parameters is {num_parameter / 1000 ** 2:.2f}M")

    def forward(self, x, idx_scale=0):
        self.idx_scale = idx_scale
        if self.self_ensemble and not self.training:
            return self.forward_x8(x)
        if self.tile > 0 and not self.training:
            return self.forward_tiled(x)
        return self.model(x)

    def forward_tiled(self, x):
        """The network over overlapping tiles of ``x`` [B,C,h,w] (DESIGN.md "Tiled inference"; ``--tile`` / ``--tile_overlap`` of
        the public DRCT and SwinIR test scripts): the cover of ``ops.tile_plan`` for (h, w), ``tile``, ``tile_overlap`` and the
        network's granule, the tiles cut by one launch, the network on ``tile_batch`` tiles at a time (the last chunk may be
        smaller), one blend launch per output.  A list of outputs (DRN-L) is blended output by output, each at its own scale
        ``out.shape[2] // tile height``.  Any h, w >= 1.  Inference only: the result carries no graph."""
        from . import ops
        from .evaluate import _auto_batch
        g = self.model.granule
        h, w = x.shape[-2:]
        tiles = ops.tile_gather(x, self.tile, self.tile_overlap, g)
        ty, tx = tiles.shape[-2:]
        step = self.tile_batch if self.tile_batch > 0 else _auto_batch(ty, tx, False)
        ys = [self.model(tiles[i:i + step]) for i in range(0, tiles.shape[0], step)]
        many = isinstance(ys[0], (list, tuple))
        outs = []
        for per_out in zip(*(y if many else [y] for y in ys)):
            y = per_out[0] if len(per_out) == 1 else torch.cat(per_out)
            outs.append(ops.tile_blend(y, h, w, self.tile, self.tile_overlap, g, y.shape[2] // ty, self.tile_blend))
        return outs if many else outs[0]

    def forward_x8(self, x):
        """Self-ensemble x8 (DESIGN.md "Self-ensemble"; ``forward_x8`` of the EDSR / DRN code the reference descends from):
        the network's outputs for the 8 flips and transposes of ``x``, each transform undone, averaged in member order.
        Square input is one forward of the stacked [8B,C,H,W] batch; other input two forwards, members 0..3 as [4B,C,H,W] and
        4..7 as [4B,C,W,H].  A list of outputs (DRN-L) is ensembled output by output.  Inference only: the result carries no
        graph."""
        from . import ops
        net = self.forward_tiled if self.tile > 0 and not self.training else self.model      # each member tiled with its own plan
        ys = [net(b) for b in ops.ensemble_batches(x)]
        many = isinstance(ys[0], (list, tuple))
        outs = []
        for per_batch in zip(*(y if many else [y] for y in ys)):
            if len(per_batch) == 1:                           # square: both halves live in the one stacked output
                n = per_batch[0].shape[0] // 2
                per_batch = (per_batch[0][:n], per_batch[0][n:])
            outs.append(ops.ensemble_mean(*per_batch))
        return outs if many else outs[0]

    def get_model(self):
        return self.model

    def get_dual_model(self, idx):
        return self.dual_models[idx]

    def state_dict(self, **kwargs):
        return self.get_model().state_dict(**kwargs)

    def count_parameters(self, model):
        return sum(p.numel() for p in model.parameters() if p.requires_grad)

    def save(self, path, is_best=False):
        """model/model_latest.pt (+ model_best.pt) = raw state_dict; dual models as a LIST of
        state_dicts in dual_model_{latest,best}.pt (src/model.py:123-147).  A network that keeps a weight average also
        gets model/model_ema_latest.pt (+ model_ema_best.pt) = ``ema_state_dict()``, loadable like any checkpoint."""
        target = self.get_model()
        os.makedirs(os.path.join(path, 'model'), exist_ok=True)
        torch.save(target.state_dict(), os.path.join(path, 'model', 'model_latest.pt'))
        if is_best:
            torch.save(target.state_dict(), os.path.join(path, 'model', 'model_best.pt'))
        if getattr(target, 'flat_ema', None) is not None:      # a run with a weight average (--ema): the averaged network too
            ema = target.ema_state_dict()
            torch.save(ema, os.path.join(path, 'model', 'model_ema_latest.pt'))
            if is_best:
                torch.save(ema, os.path.join(path, 'model', 'model_ema_best.pt'))
        if self.dual_model:
            dual_models = [self.get_dual_model(i).state_dict() for i in range(len(self.dual_models))]
            torch.save(dual_models, os.path.join(path, 'model', 'dual_model_latest.pt'))
            if is_best:
                torch.save(dual_models, os.path.join(path, 'model', 'dual_model_best.pt'))

    def load(self, pre_train='.', pre_train_dual='.', cpu=False):
        """``torch.load(weights_only=True)`` + ``load_state_dict(strict=False)`` (src/model.py:149-170)."""
        if pre_train != '.':
            print('Loading model from {}'.format(pre_train))
            self.get_model().load_state_dict(torch.load(pre_train, weights_only=True, map_location=self.device),
                                             strict=False)
        if self.dual_model and pre_train_dual != '.':
            print('Loading dual model from {}'.format(pre_train_dual))
            dual_models = torch.load(pre_train_dual, weights_only=True, map_location=self.device)
            for i in range(len(self.dual_models)):
                self.get_dual_model(i).load_state_dict(dual_models[i], strict=False)
