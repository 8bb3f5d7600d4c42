"""Option objects and argument parsing with the reference's names, defaults and quirks
(src/main.py:35-294; src/evaluate.py:20-45).  The choices are a superset: --scale 2 and
--resolution 512/1024 are accepted for the BASELINE configs, plus --dtype and --gpus."""
from __future__ import annotations

import argparse
import os
import sys
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import yaml


@dataclass
class DRN:
    model_name: str = 'drn-l'
    n_threads: int = -2
    cpu: bool = False
    n_GPUs: int = 1
    seed: int = 1
    data_dir: str = './workspace/gkd/DC2/unlabeled/HR_512_grayscale/'
    data_train: str = ''
    data_test: str = ''
    data_range: str = '1-224/225-280'
    scale: object = 4
    patch_size: int = 512
    rgb_range: int = 255
    n_colors: int = 1
    no_augment: bool = False
    pre_train: str = '.'
    pre_train_dual: str = '.'
    n_blocks: int = 40
    n_feats: int = 20
    negval: float = 0.2
    test_every: int = 10
    epochs: int = 10
    batch_size: int = 4
    self_ensemble: bool = False
    test_only: bool = False
    lr: float = 1e-4
    eta_min: float = 1e-7
    beta1: float = 0.9
    beta2: float = 0.999
    epsilon: float = 1e-8
    weight_decay: float = 1e-8
    loss: str = '1*L1'
    skip_threshold: float = 1.5
    dual_weight: float = 0.1
    save: str = './workspace/experiment/drn-l/gkd_dc2_unlabeld_X4_10_grayscale/'
    print_every: int = 10
    save_results: bool = True
    dual: bool = True
    patience: int = 10
    min_delta: float = 0.0
    dataset: str = ''
    classe: str = ''
    slurm: bool = False
    ssim_window_size: int = 11
    best_auc: float = 1.0
    precision: str = 'fp32'
    use_graph: bool = True


@dataclass
class DRCT:
    model_name: str = 'drct'
    n_threads: int = 1
    cpu: bool = False
    n_GPUs: int = 1
    seed: int = 1
    data_dir: str = './workspace/gkd/DC2/unlabeled/HR_512_grayscale/'
    data_train: str = ''
    data_test: str = ''
    data_range: str = '1-260/261-299'
    scale: object = 4
    patch_size: int = 512
    rgb_range: int = 255
    n_colors: int = 1
    no_augment: bool = False
    pre_train: str = '.'
    pre_train_dual: str = '.'
    negval: float = 0.2
    test_every: int = 30
    epochs: int = 10
    batch_size: int = 2
    self_ensemble: bool = False
    test_only: bool = False
    lr: float = 1e-4
    eta_min: float = 1e-7
    beta1: float = 0.9
    beta2: float = 0.999
    epsilon: float = 1e-8
    loss: str = '1*L1'
    skip_threshold: float = 1e6
    dual_weight: float = 0.1
    save: str = './workspace/experiment/drct/gkd_dc2_unlabeled_X4_10_test_grayscale/'
    print_every: int = 10
    save_results: bool = True
    dual: bool = False
    upscale: int = 4
    img_size: int = 128
    window_size: int = 16
    compress_ratio: int = 3
    squeeze_factor: int = 30
    conv_scale: float = 0.01
    overlap_ratio: float = 0.5
    img_range: float = 1.0
    depths: tuple = (6,) * 12
    embed_dim: int = 180
    num_heads: tuple = (6,) * 12
    mlp_ratio: int = 2
    upsampler: str = 'pixelshuffle'
    resi_connection: str = '1conv'
    ema_decay: float = 0.999
    weight_decay: float = 0.0
    betas: tuple = (0.9, 0.99)
    patience: int = 10
    min_delta: float = 0.0
    dataset: str = ''
    classe: str = ''
    slurm: bool = False
    ssim_window_size: int = 11
    best_auc: float = 1.0
    precision: str = 'fp32'
    use_graph: bool = True


def setup_opt_drn(opt: DRN, best_auc, ssim_window_size, dataset, classe, slurm, scale, no_augment, n_colors, epochs,
                  batch_size, patch_size, data_dir, save, data_range, test_every, print_every, patience, min_delta,
                  n_threads, pre_trained, pre_trained_dual, loss) -> DRN:
    """src/main.py:144-205 (same positional signature)."""
    opt.scale = [pow(2, s + 1) for s in range(int(np.log2(scale)))]
    if scale == 2:
        opt.n_blocks, opt.n_feats = 44, 40
    elif scale == 4:
        opt.n_blocks, opt.n_feats = 40, 20
    elif scale == 8:
        opt.n_blocks, opt.n_feats = 36, 10
    else:
        print(f"No setup for this scale: {scale}")
    opt.no_augment, opt.n_colors, opt.epochs, opt.batch_size = no_augment, n_colors, epochs, batch_size
    opt.patch_size, opt.data_dir, opt.save = patch_size, data_dir, save
    opt.test_every, opt.print_every, opt.patience, opt.min_delta = test_every, print_every, patience, min_delta
    opt.n_threads, opt.pre_train, opt.pre_train_dual, opt.loss = n_threads, pre_trained, pre_trained_dual, loss
    opt.dataset, opt.classe, opt.slurm = dataset, classe, slurm
    opt.ssim_window_size, opt.best_auc = ssim_window_size, best_auc
    return opt


def setup_opt_drct(opt: DRCT, best_auc, ssim_window_size, dataset, classe, slurm, scale, no_augment, n_colors, epochs,
                   batch_size, patch_size, img_size, data_dir, save, data_range, test_every, print_every, patience,
                   min_delta, n_threads, pre_trained, loss) -> DRCT:
    """src/main.py:243-294: note ``window_size = img_size // 4``."""
    opt.upscale = scale
    opt.scale = [scale]
    opt.no_augment, opt.n_colors, opt.epochs, opt.batch_size = no_augment, n_colors, epochs, batch_size
    opt.patch_size, opt.data_dir, opt.data_range, opt.save = patch_size, data_dir, data_range, save
    opt.test_every, opt.print_every, opt.img_size = test_every, print_every, img_size
    opt.patience, opt.min_delta, opt.n_threads, opt.pre_train = patience, min_delta, n_threads, pre_trained
    opt.window_size = img_size // 4
    opt.loss, opt.dataset, opt.classe, opt.slurm = loss, dataset, classe, slurm
    opt.ssim_window_size, opt.best_auc = ssim_window_size, best_auc
    return opt


def _with_config(parser: argparse.ArgumentParser, pre_args) -> None:
    if pre_args.config is not None and os.path.isfile(pre_args.config):
        with open(pre_args.config, 'r') as f:
            cfg = yaml.safe_load(f) or {}
        parser.set_defaults(**{k.replace('-', '_'): v for k, v in cfg.items()})


def parse_train_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    """src/main.py:207-241 (+ --dtype, --gpus; wider --scale / --resolution choices)."""
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument('--config', type=str, default=None)
    pre_args, _ = pre.parse_known_args(argv)
    p = argparse.ArgumentParser(description='Training/Evaluation entrypoint', parents=[pre])
    p.add_argument('--model-type', type=str, default='drct', choices=['drct', 'drn-l'])
    p.add_argument('--dataset', type=str, default='mvtec', choices=['mvtec'])
    p.add_argument('--classe', type=str, default='grid', choices=['grid', 'carpet'])
    p.add_argument('--scale', type=int, default=4, choices=[2, 4, 8])
    p.add_argument('--resolution', type=int, default=128, choices=[32, 64, 128, 256, 512, 1024])
    p.add_argument('--epochs', type=int, default=2)
    p.add_argument('--batch-size', type=int, default=4)
    p.add_argument('--lr', type=float, default=2e-4)      # parsed but never applied, like the reference (H5)
    p.add_argument('--no-augment', action='store_true')
    p.add_argument('--device', type=str, default='auto', choices=['auto', 'cuda', 'mps', 'cpu'])
    p.add_argument('--data-root', type=str, default='auto')
    p.add_argument('--save-dir', type=str, default='./workspace/experiment')
    p.add_argument('--pretrain', action='store_true')
    p.add_argument('--test-only', action='store_true')
    p.add_argument('--workers', type=int, default=0 if sys.platform == 'darwin' else 4)
    p.add_argument('--dtype', type=str, default='fp32', choices=['fp32', 'bf16'], help="training precision (the evaluation at the end of "
                   "a run uses the evaluator's split-bf16 mode when this is fp32)")
    p.add_argument('--gpus', type=int, default=1)
    p.add_argument('--self-ensemble', action='store_true', default=False,
                   help="use self-ensemble method for test: the validation of a run (Trainer.test) and --test-only average the "
                        "model's outputs for the 8 flips and transposes of each input")
    p.add_argument('--ema', action='store_true', default=False,
                   help="keep an exponential moving average of the weights in the fused Adam step (BasicSR's model_ema): the "
                        "validation runs on it and model/model_ema_{latest,best}.pt are written beside the raw weights")
    p.add_argument('--ema-decay', type=_ema_decay, default=None, metavar='D',
                   help="decay of --ema, in [0, 1); default: the option set's ema_decay (0.999)")
    p.add_argument('--grad-clip', type=_grad_clip, default=None, metavar='MAX_NORM',
                   help="clip the gradients' global L2 norm to MAX_NORM (> 0) before every Adam step, on the device "
                        "(torch.nn.utils.clip_grad_norm_; BasicSR's use_grad_clip); a guarded step also skips non-finite gradients")
    p.add_argument('--skip-nonfinite', action='store_true', default=False,
                   help="drop every optimizer step whose gradients hold an inf or a NaN (what the reference's GradScaler.step did): "
                        "weights, moments and the weight average keep their bits and the bias correction counts applied steps")
    p.add_argument('--loss', type=_loss_spec, default='1*L1', metavar='SPEC',
                   help="the training loss as w*TYPE(+w*TYPE)*, e.g. 0.8*L1+0.2*MSGMS; types " + ', '.join(LOSS_TYPES) +
                        "; the default 1*L1 runs the graphed step, any other string the eager one")
    add_tile_args(p)                                          # test time only, like --self-ensemble
    _with_config(p, pre_args)
    args = p.parse_args(argv)
    check_tile_args(p, args)
    try:                                                      # a value from a config file gets the command line's check
        args.loss = _loss_spec(str(args.loss))
    except argparse.ArgumentTypeError as e:
        p.error(f"argument --loss: {e}")
    if args.ema_decay is not None:                            # a value from a config file gets the command line's check
        try:
            args.ema_decay = _ema_decay(str(args.ema_decay))
        except (argparse.ArgumentTypeError, ValueError) as e:
            p.error(f"argument --ema-decay: {e}")
    if args.grad_clip is not None:                            # the same for --grad-clip
        try:
            args.grad_clip = _grad_clip(str(args.grad_clip))
        except (argparse.ArgumentTypeError, ValueError) as e:
            p.error(f"argument --grad-clip: {e}")
    return args


def _nonnegative_int(text: str) -> int:
    try:
        v = int(text)
    except ValueError:
        v = -1
    if v < 0:
        raise argparse.ArgumentTypeError(f"{text!r} is not an integer >= 0")
    return v


TILE_BLENDS = ('mean', 'feather')


def add_tile_args(p: argparse.ArgumentParser) -> None:
    """--tile / --tile-overlap / --tile-blend (DESIGN.md "Tiled inference"), the same three in every parser; all off by default."""
    p.add_argument('--tile', type=_nonnegative_int, default=0, metavar='T',
                   help="tiled inference (--tile of the public DRCT / SwinIR test scripts): cover every LR image with overlapping "
                        "T x T tiles, super-resolve the tiles and blend the overlaps; any image size, bounded memory; 0 = whole "
                        "images (for DRCT, T must be a multiple of the window size)")
    p.add_argument('--tile-overlap', type=_nonnegative_int, default=None, metavar='O',
                   help="LR pixels neighbouring tiles share, in [0, T); default 0 (with --tile)")
    p.add_argument('--tile-blend', type=str, default=None, choices=list(TILE_BLENDS),
                   help="how overlaps are combined: the plain mean of the covering tiles (the public scripts' rule, the default) "
                        "or a feathered mean whose weights fall off towards each tile's edge (with --tile)")


def check_tile_args(p: argparse.ArgumentParser, args: argparse.Namespace) -> None:
    """The checks of the three flags, for values from a config file too; fills the defaults of the two that belong to --tile."""
    try:
        args.tile = _nonnegative_int(str(args.tile))
        if args.tile_overlap is not None:
            args.tile_overlap = _nonnegative_int(str(args.tile_overlap))
    except argparse.ArgumentTypeError as e:
        p.error(f"argument --tile / --tile-overlap: {e}")
    if args.tile_blend is not None and args.tile_blend not in TILE_BLENDS:
        p.error(f"argument --tile-blend: invalid choice: {args.tile_blend!r} (choose from 'mean', 'feather')")
    if not args.tile and (args.tile_overlap is not None or args.tile_blend is not None):
        p.error("--tile-overlap and --tile-blend belong to --tile: give it too")
    args.tile_overlap = 0 if args.tile_overlap is None else args.tile_overlap
    args.tile_blend = 'mean' if args.tile_blend is None else args.tile_blend
    if args.tile and args.tile_overlap >= args.tile:
        p.error(f"argument --tile-overlap: {args.tile_overlap} is not below the tile size {args.tile}")


def set_tile_opt(opt, args) -> None:
    """Carries the parsed tile setting to the option object the Model reads - only when it is on, so a run without the flags
    builds (and writes, config.txt) the option object it always did."""
    if getattr(args, 'tile', 0):
        opt.tile, opt.tile_overlap, opt.tile_blend = int(args.tile), int(args.tile_overlap), str(args.tile_blend)


def tile_suffix(model) -> str:
    """' (tiles T/O blend)' for a model that tiles, '' otherwise: what the summary lines append."""
    t = int(getattr(model, 'tile', 0) or 0)
    return f" (tiles {t}/{int(model.tile_overlap)} {model.tile_blend})" if t else ""


def _positive_finite_float(text: str) -> float:
    v = float(text)
    if not 0.0 < v < float('inf'):                            # zero, negatives, infinities and NaN
        raise argparse.ArgumentTypeError(f"{text} is not a finite number > 0")
    return v


def add_baseline_args(p: argparse.ArgumentParser, flag: str, where: str) -> None:
    """``flag`` (--map-baseline in the evaluator, --baseline in predict) and --baseline-floor (DESIGN.md "Baseline"); off by default."""
    p.add_argument(flag, action='store_true', default=False,
                   help=f"per-pixel baseline: fit the mean and spread of the anomaly maps on the defect-free images {where} and "
                        "score, threshold and save the maps in sigmas of it (needs at least 3 such images)")
    p.add_argument('--baseline-floor', type=_positive_finite_float, default=None, metavar='F',
                   help=f"the least per-pixel spread of the baseline, as a share of the pooled spread; finite and > 0, default 0.1 (with {flag})")


def check_baseline_args(p: argparse.ArgumentParser, args: argparse.Namespace, attr: str, flag: str) -> None:
    """The checks of the two flags, for values from a config file too; --baseline-floor stays None where it was not given."""
    if not isinstance(getattr(args, attr), bool):
        p.error(f"argument {flag}: {getattr(args, attr)!r} is not a boolean")
    if args.baseline_floor is not None:
        try:
            args.baseline_floor = _positive_finite_float(str(args.baseline_floor))
        except (argparse.ArgumentTypeError, ValueError) as e:
            p.error(f"argument --baseline-floor: {e}")
        if not getattr(args, attr):
            p.error(f"--baseline-floor belongs to {flag}: give it too")


LOSS_TYPES = ('L1', 'MSE', 'PSNR', 'SSIM', 'GMS', 'MSGMS')     # loss.KINDS, kept here so that parsing needs no torch


def _loss_spec(text: str) -> str:
    """--loss: ``w*TYPE(+w*TYPE)*`` with finite weights and types of ``LOSS_TYPES`` (the string itself)."""
    for term in text.split('+'):
        parts = term.split('*')
        try:
            weight = float(parts[0]) if len(parts) == 2 else float('nan')
        except ValueError:
            weight = float('nan')
        if len(parts) != 2 or weight != weight or weight in (float('inf'), float('-inf')) or parts[1] not in LOSS_TYPES:
            raise argparse.ArgumentTypeError(f"{text!r} is not w*TYPE(+w*TYPE)* with finite weights and types of {LOSS_TYPES}")
    return text


def _grad_clip(text: str) -> float:
    v = float(text)
    if not v > 0.0:                                           # zero, negatives and NaN
        raise argparse.ArgumentTypeError(f"{text} is not a norm > 0")
    return v


def _ema_decay(text: str) -> float:
    v = float(text)
    if not 0.0 <= v < 1.0:                                    # NaN too
        raise argparse.ArgumentTypeError(f"{text} is not a decay in [0, 1)")
    return v


def _nonnegative_float(text: str) -> float:
    v = float(text)
    if not v >= 0.0:                                          # NaN too
        raise argparse.ArgumentTypeError(f"{text} is not a number >= 0")
    return v


def _open_unit_float(text: str) -> float:
    v = float(text)
    if not 0.0 < v < 1.0:                                     # NaN too
        raise argparse.ArgumentTypeError(f"{text} is not a rate in (0, 1)")
    return v


def _closed_unit_float(text: str) -> float:
    v = float(text)
    if not 0.0 <= v <= 1.0:                                   # NaN too
        raise argparse.ArgumentTypeError(f"{text} is not a share in [0, 1]")
    return v


def _finite_or_inf_float(text: str) -> float:
    v = float(text)
    if v != v:
        raise argparse.ArgumentTypeError("a threshold cannot be NaN")
    return v


def _positive_int(text: str) -> int:
    try:
        v = int(text)
    except ValueError:
        v = 0
    if v < 1:
        raise argparse.ArgumentTypeError(f"{text!r} is not an integer >= 1")
    return v


GMS_MAP_SOURCES = ('gms', 'msgms')                            # metrics.GMS_MAP_SOURCES, kept here so that parsing needs no torch
ALL_MAP_SOURCES = ('ssim', 'mse') + GMS_MAP_SOURCES


def _map_scales(text: str):
    """--map-scales: 'sweep', or a comma-separated list of positive integers (the list; '' = none)."""
    text = text.strip()
    if text == 'sweep':
        return 'sweep'
    sizes = []
    for part in (text.split(',') if text else []):
        try:
            v = int(part.strip())
        except ValueError:
            v = 0
        if v < 1:
            raise argparse.ArgumentTypeError(f"{part.strip()!r} is not a positive integer (a list like 11,21,31, or 'sweep')")
        sizes.append(v)
    return sizes


def parse_eval_args(argv=None) -> argparse.Namespace:
    """src/evaluate.py:20-45 (+ --dtype, --gpus)."""
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument('--config', type=str, default=None)
    pre_args, _ = pre.parse_known_args(argv)
    p = argparse.ArgumentParser(description='Evaluation entrypoint', parents=[pre])
    p.add_argument('--model-type', type=str, default='drct', choices=['drct', 'drn-l'])
    p.add_argument('--dataset', type=str, default='mvtec', choices=['mvtec'])
    p.add_argument('--classe', type=str, default='grid')
    p.add_argument('--scale', type=int, default=4)
    p.add_argument('--resolution', type=int, default=128)
    p.add_argument('--device', type=str, default='auto', choices=['auto', 'cuda', 'mps', 'cpu'])
    p.add_argument('--data-root', type=str, default='auto')
    p.add_argument('--run-dir', type=str, default='')
    p.add_argument('--checkpoint', type=str, default='')
    p.add_argument('--batch-size', type=int, default=1)
    p.add_argument('--output-dir', type=str, default='')
    p.add_argument('--save-images', action='store_true', default=True)
    p.add_argument('--workers', type=int, default=0 if sys.platform == 'darwin' else 4)
    p.add_argument('--dtype', type=str, default='bf16x3', choices=['fp32', 'bf16', 'bf16x3'],
                   help="bf16x3 = split-bf16 (fp32-grade outputs on the bf16 matrix pipe; the default: AUC parity), fp32 = exact-fp32 MFMA, "
                        "bf16 = fastest, outside the +-0.002 AUC bar")
    p.add_argument('--gpus', type=int, default=1)
    p.add_argument('--pixel-metrics', action='store_true', default=False,
                   help="pixel-level ROC-AUC of the anomaly maps against the test/bad/GT masks (needs --gpus 1)")
    p.add_argument('--save-anomaly-maps', action='store_true', default=False,
                   help="write the per-pixel anomaly maps (1 - SSIM map) as <output-dir>/anomaly_maps/{good,bad}/<name>.png")
    p.add_argument('--map-ws', type=int, default=0, help="window size of the anomaly maps; 0 = the image-level sweep's best_ws")
    p.add_argument('--aupro', action='store_true', default=False,
                   help="AU-PRO of the anomaly maps against the test/bad/GT masks: the per-region overlap curve's normalised area "
                        "up to --pro-fpr-limit (needs --gpus 1)")
    p.add_argument('--pro-fpr-limit', type=float, default=0.3, help="false-positive-rate limit of --aupro, in (0, 1]")
    p.add_argument('--pr-metrics', action='store_true', default=False,
                   help="average precision and F1-max next to the AUCs: of the image scores, of the map maximum with "
                        "--map-image-score, and of the anomaly maps against the test/bad/GT masks (the pixel level needs --gpus 1); "
                        "the F1-max threshold it prints can be passed to --threshold")
    p.add_argument('--map-sigma', type=_nonnegative_float, default=0.0,
                   help="Gaussian sigma (px) the anomaly maps are smoothed with before they are saved or scored "
                        "(scipy.ndimage.gaussian_filter, truncate 4); 4 is the MVTec convention, 0 = the raw maps")
    p.add_argument('--map-image-score', action='store_true', default=False,
                   help="image-level ROC-AUC of each image's anomaly-map maximum (smoothed with --map-sigma); no masks needed")
    p.add_argument('--map-scales', type=_map_scales, default=[], metavar='LIST|sweep',
                   help="multi-scale anomaly maps: a comma-separated list of SSIM window sizes (e.g. 11,21,31) or 'sweep' for every "
                        "size of the image-level sweep, combined per pixel with --map-reduce; replaces --map-ws")
    p.add_argument('--map-reduce', type=str, default='mean', choices=['mean', 'max'],
                   help="how --map-scales combines the maps of its window sizes")
    p.add_argument('--map-source', type=str, default='ssim', choices=list(ALL_MAP_SOURCES),
                   help="what the pixel-level maps are made of: 1 - SSIM map, (mse) the squared error averaged over the window "
                        "(--map-ws 0 then means window size 1, the raw per-pixel squared error), or the gradient-magnitude "
                        "similarity at one level (gms) or four (msgms), which has no window: smooth with --map-sigma")
    p.add_argument('--threshold', type=_finite_or_inf_float, default=None, metavar='VALUE',
                   help="operating point: a pixel is predicted defective iff its anomaly-map value is > VALUE; reports the "
                        "image-level (and, with test/bad/GT masks, pixel-level) counts at it (needs --gpus 1)")
    p.add_argument('--threshold-fpr', type=_open_unit_float, default=None, metavar='RATE',
                   help="operating point at the threshold that the defect-free images of <class>/val/good give at this "
                        "false-positive rate, in (0, 1); excludes --threshold")
    p.add_argument('--threshold-level', type=str, default='pixel', choices=['pixel', 'image'],
                   help="what --threshold-fpr calibrates on: every pixel of the val/good maps, or each map's maximum")
    p.add_argument('--min-region-area', type=_positive_int, default=1, metavar='A',
                   help="remove predicted 8-connected components of fewer than A pixels (1 = keep all)")
    p.add_argument('--save-masks', action='store_true', default=False,
                   help="write the predicted masks (0 / 255) as <output-dir>/anomaly_masks/{good,bad}/<name>.png")
    p.add_argument('--self-ensemble', action='store_true', default=False,
                   help="use self-ensemble method for test: every SR image is the mean of the model's outputs for the 8 flips "
                        "and transposes of its input, each transform undone (8 forwards per image)")
    p.add_argument('--ema', action='store_true', default=False,
                   help="evaluate the averaged weights of a run trained with --ema: --run-dir's model/model_ema_best.pt, else "
                        "model_ema_latest.pt (no fall-back to the raw weights; excludes --checkpoint)")
    p.add_argument('--region-metrics', action='store_true', default=False,
                   help="detection counts at the level of defect regions at the operating point: predicted regions that touch the "
                        "ground truth, false alarms (per image, on good images), ground-truth regions found; needs --threshold or "
                        "--threshold-fpr, the test/bad/GT masks and --gpus 1")
    p.add_argument('--region-min-overlap', type=_closed_unit_float, default=None, metavar='F',
                   help="a ground-truth region counts as found when at least this share of its pixels is predicted (and at least "
                        "one pixel), in [0, 1]; default 0 (with --region-metrics)")
    p.add_argument('--save-regions', action='store_true', default=False,
                   help="write <output-dir>/regions.csv: one row per predicted region (with --region-metrics)")
    add_tile_args(p)
    add_baseline_args(p, '--map-baseline', "of <class>/val/good (the images of --threshold-fpr)")
    _with_config(p, pre_args)
    args = p.parse_args(argv)
    check_tile_args(p, args)
    check_baseline_args(p, args, 'map_baseline', '--map-baseline')
    if args.map_baseline and int(args.gpus) > 1:
        p.error("--map-baseline needs --gpus 1 (the baseline is fitted and applied on one rank, like the operating point)")
    if args.map_baseline and not (args.pixel_metrics or args.aupro or args.pr_metrics or args.save_anomaly_maps or args.map_image_score
                                  or args.threshold is not None or args.threshold_fpr is not None):
        p.error("--map-baseline normalises the anomaly maps: give a flag that makes them too (--pixel-metrics, --aupro, "
                "--pr-metrics, --map-image-score, --save-anomaly-maps, --threshold or --threshold-fpr)")
    if args.ema and args.checkpoint:
        p.error("--ema and --checkpoint exclude each other (an explicit file is already a choice)")
    if args.region_metrics and args.threshold is None and args.threshold_fpr is None:
        p.error("--region-metrics counts the regions of an operating point against the ground-truth masks: give --threshold or "
                "--threshold-fpr (and prepare the data with masks, test/bad/GT)")
    if (args.region_min_overlap is not None or args.save_regions) and not args.region_metrics:
        p.error("--region-min-overlap and --save-regions belong to --region-metrics: give it too")
    args.region_min_overlap = 0.0 if args.region_min_overlap is None else args.region_min_overlap
    if args.threshold is not None and args.threshold_fpr is not None:
        p.error("--threshold and --threshold-fpr exclude each other (a given threshold or a calibrated one)")
    if isinstance(args.map_scales, (list, tuple)):            # a list from a config file gets the command line's check
        try:
            args.map_scales = _map_scales(','.join(str(v) for v in args.map_scales))
        except argparse.ArgumentTypeError as e:
            p.error(f"argument --map-scales: {e}")
    if args.map_source not in ALL_MAP_SOURCES:                # a value from a config file gets the command line's check
        p.error(f"argument --map-source: invalid choice: {args.map_source!r} (choose from {', '.join(repr(m) for m in ALL_MAP_SOURCES)})")
    if args.map_source in GMS_MAP_SOURCES and (args.map_ws or args.map_scales):
        p.error(f"--map-source {args.map_source}: the GMS maps have no window (no --map-ws, no --map-scales); smooth with --map-sigma")
    if args.map_scales and args.map_ws:
        p.error("--map-scales and --map-ws exclude each other (the scales replace the single window size)")
    return args


def build_opt(model_type: str, class_name: str, resolution: int, scale: int, batch_size: int = 1, dtype: str = 'fp32',
              pre_train: str = '.', pre_train_dual: str = '.', data_root: str = 'auto', save: str = './workspace/eval',
              epochs: int = 1, no_augment: bool = True, loss: str = '1*L1'):
    """The option object main.py / evaluate.py build before calling Model (src/main.py:398-471,
    src/evaluate.py:293-334)."""
    n_colors = 3 if class_name == 'carpet' else 1
    img_size = resolution // scale
    if data_root == 'auto':
        data_root = f"data/mvtec_{resolution}"
    data_dir = f"{data_root}/{class_name}/train/good"
    if model_type == 'drn-l':
        opt = setup_opt_drn(DRN(), 0.0, 11, 'mvtec', class_name, False, scale, no_augment, n_colors, epochs, batch_size,
                            resolution, data_dir, save, '', 1, 1, 1, 0.0, 4, pre_train, pre_train_dual, loss)
    else:
        opt = setup_opt_drct(DRCT(), 0.0, 11, 'mvtec', class_name, False, scale, no_augment, n_colors, epochs, batch_size,
                             resolution, img_size, data_dir, save, '', 1, 1, 1, 0.0, 4, pre_train, loss)
    opt.model_name = model_type
    opt.data_root = data_root
    opt.precision = dtype
    return opt
