"""ctypes loader for libsrad.so (the HIP engine).  There is NO CPU fallback: if the library is
missing or a call fails, the product path raises."""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# SRAD_LIB_PATH: a differently built libsrad (an A/B build of tools/), else the in-tree library
LIB_PATH = os.environ.get("SRAD_LIB_PATH") or os.path.join(_HERE, "libsrad.so")

PREC_F32 = 0
PREC_BF16 = 1
PREC_BF16X3 = 2      # split-bf16: operands as hi + lo bf16 terms, three bf16 MFMAs per product, fp32-grade outputs (inference)
PRECISIONS = {"fp32": PREC_F32, "f32": PREC_F32, "float32": PREC_F32, "bf16": PREC_BF16, "bfloat16": PREC_BF16,
              "bf16x3": PREC_BF16X3, "split-bf16": PREC_BF16X3}

ACT_NONE, ACT_GELU, ACT_LRELU, ACT_RELU = 0, 1, 2, 3


class DrctConfig(C.Structure):
    _fields_ = [("in_chans", C.c_int32), ("img_size", C.c_int32), ("window_size", C.c_int32),
                ("upscale", C.c_int32), ("embed_dim", C.c_int32), ("n_rdg", C.c_int32),
                ("num_heads", C.c_int32), ("gc", C.c_int32), ("num_feat", C.c_int32),
                ("mlp_ratio", C.c_float), ("img_range", C.c_float), ("precision", C.c_int32),
                ("use_graph", C.c_int32)]


class DrnConfig(C.Structure):
    _fields_ = [("n_colors", C.c_int32), ("scale", C.c_int32), ("n_blocks", C.c_int32),
                ("n_feats", C.c_int32), ("negval", C.c_float), ("rgb_range", C.c_float),
                ("precision", C.c_int32), ("use_graph", C.c_int32)]


class WqStep(C.Structure):
    """One step of srad_op_wgrad_queue_script (include/srad.h srad_wq_step)."""
    _fields_ = [("kind", C.c_int32), ("i", C.c_int32 * 9), ("alpha", C.c_float), ("p", C.c_void_p * 7)]


class GemmPlan(C.Structure):
    """What srad_op_gemm runs for a set of arguments (include/srad.h srad_gemm_plan)."""
    _fields_ = [(n, C.c_int32) for n in ("family", "BM", "BN", "CPS", "LN", "CONV", "SPECIAL", "grid_x", "grid_y", "launches")]


GEMM_FAMILIES = ("tiled", "conv80", "conv80x4", "thin", "tail")      # SRAD_GEMM_*

WGRAD_PLAN_LAYERS = 6                                                # SRAD_WGRAD_PLAN_LAYERS


class WgradPlan(C.Structure):
    """What a weight-gradient call runs (include/srad.h srad_wgrad_plan): per launch, per layer."""
    _fields_ = ([(n, C.c_int32) for n in ("count", "launches", "reduce_tiles", "precision")] +
                [(n, C.c_int32 * 2) for n in ("family", "FULL", "grid")] +
                [(n, C.c_int32) for n in ("CONV", "NT", "cpw", "nchunks")] +
                [(n, C.c_int32 * WGRAD_PLAN_LAYERS) for n in ("launch", "ksplit", "rows_per", "tn", "tc", "XH", "YH", "blk0", "nblk")])


WGRAD_FAMILIES = ("tile64", "w80", "conv9", "multi", "multi_hh")     # SRAD_WGRAD_FAM_*


class ResampleTable(C.Structure):
    """One axis of srad_resize_u8 (include/srad.h srad_resample_table): the bounds on the host and the device copies."""
    _fields_ = [("in_size", C.c_int32), ("out_size", C.c_int32), ("ksize", C.c_int32), ("bounds", C.c_void_p),
                ("dev_bounds", C.c_void_p), ("dev_coeffs", C.c_void_p)]


class ResampleTableF(C.Structure):
    """One axis of srad_resize_f32 (include/srad.h srad_resample_table_f): as ResampleTable, the device taps are double."""
    _fields_ = ResampleTable._fields_


class TileGeom(C.Structure):
    """The cover of an LR image with tiles (include/srad.h srad_tile_geom)."""
    _fields_ = [(n, C.c_int32) for n in ("h", "w", "tile", "overlap", "granule", "scale", "ph", "pw", "ty", "tx", "stride", "ny", "nx")]


TILE_BLENDS = {"mean": 0, "feather": 1}                              # SRAD_TILE_BLEND_*

RESAMPLE_FILTERS = {"lanczos": 0, "bicubic": 1}
RESAMPLE_FILTERS_F = dict(RESAMPLE_FILTERS, bilinear=2)      # the float32 resize takes BILINEAR too

WQ_WGRAD, WQ_WGRAD_DEFERRED, WQ_LAUNCH_DEFERRED, WQ_LN_BWD, WQ_ATTN_BWD, WQ_FLUSH = 1, 2, 3, 4, 5, 6
WQ_FLUSH_EXPLICIT, WQ_FLUSH_BATCH, WQ_FLUSH_WS = 0, 1, 2

_lock = threading.Lock()
_lib = None

_P = C.c_void_p
_SIG = {
    "srad_last_error": (C.c_char_p, []),
    "srad_version": (C.c_int, []),
    # DRCT
    "srad_drct_create": (C.c_int, [C.POINTER(DrctConfig), C.POINTER(_P)]),
    "srad_drct_destroy": (None, [_P]),
    "srad_drct_arena_bytes": (C.c_int, [_P, C.POINTER(C.c_size_t)]),
    "srad_drct_bind_arena": (C.c_int, [_P, _P, C.c_size_t]),
    "srad_drct_num_params": (C.c_int, [_P]),
    "srad_drct_param_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64)]),
    "srad_drct_set_param": (C.c_int, [_P, C.c_char_p, _P, C.c_int64, _P]),
    "srad_drct_workspace_bytes": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "srad_drct_forward": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "srad_drct_graph_captures": (C.c_int, [_P]),
    "srad_drct_flops": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    # DRCT training
    "srad_drct_train_param_floats": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "srad_drct_train_param_offset": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64)]),
    "srad_drct_train_arena_bytes": (C.c_int, [_P, C.POINTER(C.c_size_t)]),
    "srad_drct_train_bind": (C.c_int, [_P, _P, C.c_size_t]),
    "srad_drct_train_set_wgrad_budget": (C.c_int, [_P, C.c_size_t]),
    "srad_drct_train_wgrad_stats": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "srad_drct_sync_params": (C.c_int, [_P, _P, _P]),
    "srad_drct_train_workspace_bytes": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "srad_drct_forward_train": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "srad_drct_num_buckets": (C.c_int, [_P]),
    "srad_drct_bucket_range": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "srad_drct_backward": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_size_t, _P, _P, _P]),
    "srad_l1_grad": (C.c_int, [_P, _P, _P, C.c_int64, C.c_float, _P]),
    "srad_adam_step": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                 C.c_int, C.c_float, _P]),
    "srad_adam_step_dev": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P]),
    "srad_adam_ema_step": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                     C.c_int, C.c_float, C.c_float, _P]),
    "srad_adam_ema_step_dev": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                         _P, _P]),
    "srad_grad_guard_workspace": (C.c_int, [C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "srad_grad_guard_partials": (C.c_int, [_P, C.c_int64, _P, C.c_size_t, C.c_int, _P]),
    "srad_grad_guard_finalize": (C.c_int, [_P, C.c_size_t, C.c_int, _P, C.c_float, C.c_float, C.c_double, _P]),
    "srad_adam_guarded_step": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P]),
    "srad_adam_ema_guarded_step": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                             _P, _P]),
    "srad_set4": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    # DRN
    "srad_drn_create": (C.c_int, [C.POINTER(DrnConfig), C.POINTER(_P)]),
    "srad_drn_destroy": (None, [_P]),
    "srad_drn_arena_bytes": (C.c_int, [_P, C.POINTER(C.c_size_t)]),
    "srad_drn_bind_arena": (C.c_int, [_P, _P, C.c_size_t]),
    "srad_drn_num_params": (C.c_int, [_P]),
    "srad_drn_param_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64)]),
    "srad_drn_set_param": (C.c_int, [_P, C.c_char_p, _P, C.c_int64, _P]),
    "srad_drn_workspace_bytes": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "srad_drn_forward": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(_P), C.c_int, _P, C.c_size_t, _P]),
    "srad_drn_flops": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "srad_drn_train_param_floats": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "srad_drn_train_param_offset": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64)]),
    "srad_drn_train_arena_bytes": (C.c_int, [_P, C.POINTER(C.c_size_t)]),
    "srad_drn_train_bind": (C.c_int, [_P, _P, C.c_size_t]),
    "srad_drn_sync_params": (C.c_int, [_P, _P, _P]),
    "srad_drn_train_workspace_bytes": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "srad_drn_forward_train": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(_P), C.c_int, _P, C.c_size_t, _P]),
    "srad_drn_num_buckets": (C.c_int, [_P]),
    "srad_drn_bucket_range": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "srad_drn_backward": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P, _P, _P]),
    "srad_dual_backward_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "srad_dual_backward": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_float, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P,
                                     C.c_size_t, C.c_int, _P]),
    "srad_dual_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "srad_dual_forward": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_float, _P, C.c_int, C.c_int, C.c_int, _P, _P,
                                    C.c_size_t, C.c_int, _P]),
    # self-ensemble x8
    "srad_ensemble_inputs": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "srad_ensemble_mean": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    # tiled inference
    "srad_tile_plan": (C.c_int, [C.c_int] * 6 + [C.POINTER(TileGeom)]),
    "srad_tile_origins": (C.c_int, [C.POINTER(TileGeom), _P, _P]),
    "srad_tile_gather": (C.c_int, [_P] + [C.c_int] * 7 + [_P, _P]),
    "srad_tile_blend": (C.c_int, [_P] + [C.c_int] * 9 + [_P, _P]),
    # 8-bit resize (PIL-exact)
    "srad_resample_ksize": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "srad_resample_coeffs": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P]),
    "srad_resize_u8": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.POINTER(ResampleTable),
                                 C.POINTER(ResampleTable), _P, _P]),
    # float32 resize (PIL mode F exact) and the overlay
    "srad_resample_ksize_f64": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "srad_resample_coeffs_f64": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P]),
    "srad_resize_f32": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.POINTER(ResampleTableF),
                                  C.POINTER(ResampleTableF), _P, _P]),
    "srad_overlay_rgb": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int,
                                   _P, _P]),
    # scorer
    "srad_to_u8_hwc": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P]),
    "srad_quantize": (C.c_int, [_P, _P, C.c_int64, C.c_float, _P]),
    "srad_score_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "srad_score_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "srad_score_pairs": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int,
                                   _P, _P, _P, _P, C.c_size_t, _P]),
    "srad_val_metrics": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P, _P, C.c_size_t, _P]),
    "srad_roc_auc": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double)]),
    "srad_average_precision": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double),
                                         C.POINTER(C.c_double)]),
    "srad_anomaly_map_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "srad_anomaly_maps": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "srad_anomaly_maps_multi": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, _P, _P,
                                          C.c_size_t, _P]),
    "srad_error_map_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "srad_error_maps": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "srad_error_maps_multi": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, _P, _P,
                                        C.c_size_t, _P]),
    "srad_gms_map_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "srad_gms_maps": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "srad_pixel_auc_workspace_bytes": (C.c_int, [C.c_int64, C.POINTER(C.c_size_t)]),
    "srad_pixel_roc_auc": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P, C.c_size_t, _P]),
    "srad_pixel_pr_workspace_bytes": (C.c_int, [C.c_int64, C.POINTER(C.c_size_t)]),
    "srad_pixel_pr": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P, _P, _P, C.c_int64, _P, C.c_size_t, _P]),
    "srad_mask_regions_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "srad_mask_regions": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "srad_pixel_pro_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "srad_pixel_pro": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_double, _P, _P, _P, _P, C.c_int64, _P, C.c_size_t, _P]),
    "srad_select_kth_workspace_bytes": (C.c_int, [C.c_int64, C.POINTER(C.c_size_t)]),
    "srad_select_kth": (C.c_int, [_P, C.c_int64, C.c_int64, _P, _P, _P, C.c_size_t, _P]),
    "srad_operating_point_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "srad_operating_point": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P, _P, _P, _P, C.c_size_t, _P]),
    "srad_region_table_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "srad_region_table": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P, _P, C.c_size_t, _P]),
    "srad_smooth_maps_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "srad_smooth_maps": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "srad_map_stats_accumulate": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "srad_map_normalize_workspace_bytes": (C.c_int, [C.c_int, C.POINTER(C.c_size_t)]),
    "srad_map_normalize": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "srad_map_normalize_loo": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_double, _P, _P, _P, C.c_size_t, _P]),
    "srad_l1_workspace_bytes": (C.c_int, [C.POINTER(C.c_size_t)]),
    "srad_l1_loss": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P]),
    "srad_loss_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "srad_loss_forward": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P,
                                    _P, C.c_size_t, _P]),
    "srad_loss_backward": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P,
                                     _P, C.c_float, _P, C.c_int, _P, C.c_size_t, _P]),
    # reference paths for tests
    "srad_set_path_override": (C.c_int, [C.c_int, C.c_int]),
    "srad_get_path_override": (C.c_int, [C.c_int]),
    # event profiler
    "srad_prof_enable": (C.c_int, [C.c_int]),
    "srad_prof_num_classes": (C.c_int, []),
    "srad_prof_class_name": (C.c_char_p, [C.c_int]),
    "srad_prof_collect": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    C.POINTER(C.c_double)]),
    # the folded DRCT output end
    "srad_op_tail_fold_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                           C.POINTER(C.c_size_t)]),
    "srad_op_tail_fold_build": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "srad_op_tail_fold": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P]),
    # the DRCT body end as one launch
    "srad_drct_ends_supported": (C.c_int, [C.c_int] * 7),
    "srad_drct_ends_supported_cus": (C.c_int, [C.c_int] * 8),
    "srad_op_drct_ends_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "srad_op_drct_body_end": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_size_t,
                                        _P]),
    # single operators
    "srad_op_gemm": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                               _P, _P, _P, C.c_int, C.c_float, C.c_float, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                               _P, C.c_size_t, _P]),
    "srad_op_gemm_plan": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                    _P, _P, _P, C.c_int, C.c_float, C.c_float, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                    _P, C.c_size_t, _P, C.POINTER(GemmPlan)]),
    "srad_bench_gemm": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                  _P, _P, _P, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, C.c_size_t,
                                  C.c_int, C.POINTER(C.c_float), _P]),
    "srad_bench_window_attn": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), _P]),
    "srad_bench_mlp_block": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_size_t, C.c_int, C.c_int,
                                       C.POINTER(C.c_float), _P]),
    "srad_bench_qkv_attn": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t,
                                      C.c_int, C.POINTER(C.c_float), _P]),
    "srad_op_swin_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "srad_op_qkv_attn": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_int, _P,
                                   C.c_size_t, _P]),
    "srad_op_qkv_attn_train": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P,
                                         _P, _P, _P, C.c_int, _P, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "srad_qkv_attn_grid": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "srad_op_mlp_block": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P,
                                    _P, _P, C.c_int, C.c_float, C.c_float, _P, C.c_int, _P, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "srad_swin_block_supported": (C.c_int, [C.c_int] * 9),
    "srad_op_swin_block": (C.c_int, [C.c_int, _P, C.c_int] + [C.c_int] * 8 + [_P] * 15 + [C.c_int, C.c_float, C.c_float, _P, C.c_int, _P, C.c_int,
                                     C.c_int, _P, C.c_size_t, _P]),
    "srad_op_mlp_fold_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "srad_op_mlp_fold_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "srad_op_mlp_fold_compose": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                           C.POINTER(C.c_size_t), C.POINTER(C.c_int), _P]),
    "srad_swin_block_fold_supported": (C.c_int, [C.c_int] * 9),
    "srad_op_swin_block_folded": (C.c_int, [C.c_int, _P, C.c_int] + [C.c_int] * 8 + [_P] * 15 + [C.c_int, C.c_float, C.c_float, _P, C.c_int, _P, C.c_int,
                                            C.c_int, _P, C.c_size_t, _P]),
    "srad_mlp_block_fold_supported": (C.c_int, [C.c_int] * 5),
    "srad_mlp_block_stage_counts": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "srad_op_mlp_block_folded": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P,
                                           _P, _P, C.c_int, C.c_float, C.c_float, _P, C.c_int, _P, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "srad_bench_swin_block": (C.c_int, [_P] + [C.c_int] * 8 + [_P, _P, _P, C.c_size_t, C.c_int, C.POINTER(C.c_float), _P]),
    "srad_op_gemm_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "srad_op_window_attn": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, _P]),
    "srad_op_layernorm": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "srad_op_window_attn_qscale": (C.c_float, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "srad_op_ln_qkv_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "srad_op_ln_qkv": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_int, C.c_float, _P, C.c_size_t, _P]),
    "srad_op_window_attn_bf16_in": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    # backward operators
    "srad_op_wgrad": (C.c_int, [C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_int, _P, C.c_float, _P, _P, _P, _P]),
    "srad_op_wgrad_ex": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, _P, C.c_int] + [C.c_int] * 11 + [_P, C.c_float, _P, _P, _P, _P]),
    "srad_op_wgrad_plan": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int] + [C.c_int] * 11 +
                           [_P, C.POINTER(WgradPlan)]),
    "srad_op_wgrad_deferred_plan": (C.c_int, [C.c_int, C.POINTER(WqStep), C.c_int, C.POINTER(WgradPlan)]),
    "srad_op_wgrad_workspace_bytes": (C.c_size_t, []),
    "srad_op_wgrad_queue_script": (C.c_int, [C.c_int, C.POINTER(WqStep), C.c_int, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_int),
                                             C.POINTER(C.c_int), C.c_int, _P]),
    "srad_op_dgrad": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P,
                                C.c_int, C.c_int, C.c_float, C.c_float, _P, _P, C.c_int, _P, C.c_size_t, _P]),
    "srad_op_mlp_bwd_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "srad_op_mlp_bwd": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P,
                                  C.c_int, _P, C.c_int, _P, C.c_int, C.c_float, C.c_float, _P, _P, _P, _P, _P,
                                  _P, C.c_size_t, _P, _P]),
    "srad_op_lin_ln_bwd_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "srad_op_lin_ln_bwd": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, _P,
                                     _P, C.c_size_t, _P, _P]),
    "srad_op_layernorm_bwd": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, C.c_int, _P, _P, C.c_int, C.c_int, _P, _P]),
    "srad_op_window_attn_bwd": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, _P, _P]),
    "srad_op_conv80_h": (C.c_int, [_P, _P, _P, C.c_int, C.c_float, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_size_t, _P]),
    "srad_op_wgrad_conv9_h": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "srad_op_wgrad_deferred": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int,
                                         C.c_float, _P, _P, _P, _P]),
    "srad_bench_wgrad_block": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, _P]),
    "srad_op_window_attn_bwd_h": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, _P, _P]),
    # DRN's own kernels, one by one (csrc/kernels_drn.hip)
    "srad_drn_ca_plan": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "srad_op_drn_bicubic": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "srad_op_drn_affine_to_nchw": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "srad_op_drn_pool_dot": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "srad_op_drn_ca_scale_add": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_int, _P, C.c_int, C.c_int,
                                           _P, C.c_int, _P, _P, _P]),
    "srad_op_drn_ca_apply_bwd": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, _P]),
    "srad_op_drn_ca_bwd": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "srad_op_drn_affine_bwd": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "srad_op_drn_zero_upsample": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "srad_op_drn_add_cols": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int64, C.c_int, _P]),
    "srad_op_conv_pool": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.POINTER(C.c_int), _P,
                                    C.c_size_t, _P]),
}

BUCKET_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int)


def exported_symbols():
    """Names every entry point include/srad.h declares (checked by the CPU test-suite)."""
    return sorted(_SIG)


def lib() -> C.CDLL:
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"libsrad.so not found at {LIB_PATH}: build it with "
                    "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
                    "There is no CPU fallback for the product path.")
            # PyTorch ships its own libamdhip64 (torch/lib) and libsrad.so names /opt/rocm's by SONAME: whichever is loaded
            # first serves both.  Load torch's first - with two HIP runtimes in one process the engine's launches fail
            # with "no ROCm-capable device is detected" (seen when build() dlopen'ed libsrad before torch was imported).
            import torch  # noqa: F401
            l = C.CDLL(LIB_PATH)
            missing = [n for n in _SIG if not hasattr(l, n)]
            if missing:
                raise RuntimeError(f"{LIB_PATH} does not export {missing}; rebuild it")
            for name, (res, args) in _SIG.items():
                fn = getattr(l, name)
                fn.restype = res
                fn.argtypes = args
            _lib = l
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().srad_last_error()
        raise RuntimeError(f"libsrad {what} failed ({rc}): {msg.decode() if msg else '?'}")


def current_stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dptr(t) -> C.c_void_p:
    """Device pointer of a torch tensor (None -> NULL)."""
    return C.c_void_p(0 if t is None else t.data_ptr())


def ws_buffer(nbytes: int, device):
    """A device workspace of ``nbytes`` that starts on a 256-byte boundary: (the tensor to keep alive while the call runs,
    the aligned pointer, nbytes as size_t)."""
    import torch
    t = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    off = (-t.data_ptr()) % 256
    return t, C.c_void_p(t.data_ptr() + off), C.c_size_t(nbytes)


def prof_enable(on: bool) -> None:
    check(lib().srad_prof_enable(1 if on else 0), "prof_enable")


def prof_collect() -> dict:
    """{class name: dict(launches, ms, flops, bytes)} of everything launched since the last call
    while profiling was enabled (HIP events on the launch stream)."""
    n = lib().srad_prof_num_classes()
    la, ms, fl, by = (C.c_int64 * n)(), (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)()
    check(lib().srad_prof_collect(la, ms, fl, by), "prof_collect")
    out = {}
    for i in range(n):
        if la[i]:
            out[lib().srad_prof_class_name(i).decode()] = dict(launches=int(la[i]), ms=float(ms[i]),
                                                               flops=float(fl[i]), bytes=float(by[i]))
    return out
