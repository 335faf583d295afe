"""MI355X-native scan-matching / particle-filter engine — Python binding of the C ABI.

The product is the shared library ``lib/libslam_hip.so`` (hand-written HIP kernels for gfx950 behind
the plain-C interface of ``include/slam_hip.h``).  This module is only a ctypes view of that ABI so
that tests, ``bench.py`` and Python hosts can call it; the C host program under ``host/`` links the
same library directly.  There is NO CPU fallback: importing works without a GPU (so the build check
can load the library and verify its symbols), but creating an ``Engine`` raises when no gfx950 device
is present, and a missing library raises at import of the symbols.

Reference mapping (paths relative to the reference repository):
  Engine.edt_host / grid_upload  <- euclidean_distance_transform{,2}  Subsystem_1/main_accelerated.c:215-283
  Engine.fastmatch               <- FastMatch / FastMatch2            Subsystem_1/main.c:381-809
  Engine.score_poses*            <- the per-pose body of FastMatch    Subsystem_1/main.c:459-518
  motion / EKF / weights / resample: no reference counterpart
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
import os as _os

# SLAM_HIP_LIB: another build of the same library (kernel-tuning measurements); the product is lib/libslam_hip.so
LIB_PATH = Path(_os.environ["SLAM_HIP_LIB"]) if _os.environ.get("SLAM_HIP_LIB") else PKG_DIR / "lib" / "libslam_hip.so"
HEADER_PATH = PKG_DIR.parent / "include" / "slam_hip.h"

SLAM_OK = 0
SLAM_MAX_BEAMS = 4096
SLAM_MAX_OBS = 8192
EKF_OBS_CHUNK = 32


class SlamError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        super().__init__(f"{where}: {status_string(status)} ({status})" + (f": {detail}" if detail else ""))


class GridMeta(C.Structure):
    """``slam_grid_meta`` — rows, cols, ld, pixel, min_x, min_y (reference: MyGrid, main.c:200-213)."""

    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("ld", C.c_int32), ("pixel", C.c_float),
                ("min_x", C.c_float), ("min_y", C.c_float)]


class PfMode(C.Structure):
    """``slam_pf_mode`` — one cluster of the particle cloud: pose, mass, centre cell, member cells, weight."""

    _fields_ = [("pose", C.c_float * 3), ("mass", C.c_float), ("cell", C.c_int32 * 3), ("ncells", C.c_int32), ("weight", C.c_int64)]


MAX_MODES = 8

_vp, _i, _i64, _u64, _u32, _f = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_uint32, C.c_float
_fp = C.POINTER(C.c_float)

# name -> (restype, argtypes); every entry point include/slam_hip.h declares
SIGNATURES = {
    "slam_abi_version": (_i, []),
    "slam_status_string": (C.c_char_p, [_i]),
    "slam_last_error": (C.c_char_p, [_vp]),
    "slam_engine_create": (_i, [_i, C.POINTER(_vp)]),
    "slam_engine_destroy": (_i, [_vp]),
    "slam_engine_set_stream": (_i, [_vp, _vp]),
    "slam_engine_sync": (_i, [_vp]),
    "slam_profile_enable": (_i, [_vp, _i]),
    "slam_profile_read": (_i, [_vp, _i, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "slam_profile_bracket_overhead": (_i, [_vp, C.POINTER(C.c_double)]),
    "slam_profile_copy_ceiling": (_i, [_vp, _vp, _vp, _i64, _i, _i, C.POINTER(C.c_double)]),
    "slam_edt_dev": (_i, [_vp, _vp, _i, _i, _i, _f, _vp]),
    "slam_edt_host": (_i, [_vp, _vp, _i, _i, _i, _f, _vp]),
    "slam_grid_upload_host": (_i, [_vp, _i, _vp, C.POINTER(GridMeta), _f, _vp]),
    "slam_grid_set_dev": (_i, [_vp, _i, _vp, C.POINTER(GridMeta)]),
    "slam_grid_set_meta": (_i, [_vp, _i, C.POINTER(GridMeta)]),
    "slam_grid_packed_state": (_i, [_vp, _i, C.POINTER(C.c_int)]),
    "slam_scan_upload_host": (_i, [_vp, _vp, _vp, _i]),
    "slam_scan_set_dev": (_i, [_vp, _vp, _vp, _i]),
    "slam_score_poses_cs_dev": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "slam_score_poses_dev": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "slam_score_poses_cs_host": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "slam_score_poses_host": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "slam_pose_hits_host": (_i, [_vp, _i, _f, _f, _f, _f, _vp, C.POINTER(C.c_int32)]),
    "slam_fastmatch_host": (_i, [_vp, _i, _fp, _fp, _fp, _vp, C.POINTER(C.c_int32), _fp]),
    "slam_motion_sample_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _fp, _fp, _u64, _u32]),
    "slam_motion_score_dev": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _fp, _fp, _u64, _u32, _vp, _vp]),
    "slam_refine_poses_dev": (_i, [_vp, _i, _vp, _vp, _vp, _i, _f, _f, _i, _vp, _vp]),
    "slam_motion_refine_dev": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _fp, _fp, _u64, _u32, _f, _f, _i, _vp,
                               _vp]),
    "slam_obs_upload_host": (_i, [_vp, _vp, _vp, _vp, _i, _i]),
    "slam_obs_set_dev": (_i, [_vp, _vp, _vp, _i]),
    "slam_logweight_ekf_dev": (_i, [_vp, _vp, _f, _i, _vp, _vp]),
    "slam_ekf_update_dev": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _vp]),
    "slam_logweight_dev": (_i, [_vp, _vp, _vp, _f, _i, _vp, _vp]),
    "slam_quantise_weights_dev": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    "slam_quantise_scan_dev": (_i, [_vp, _vp, _vp, _i, _vp]),
    "slam_offspring_from_scan_dev": (_i, [_vp, _i, _vp, _vp, _u64, _u32, _i64, _vp]),
    "slam_offspring_from_scan_sharded_dev": (_i, [_vp, _i, _vp, _i, _i, _u64, _u32, _i64, _vp]),
    "slam_prefix_sum_dev": (_i, [_vp, _vp, _i, _vp]),
    "slam_offspring_offsets_dev": (_i, [_vp, _vp, _i, _vp, _vp, _u64, _u32, _i64, _vp]),
    "slam_ancestors_dev": (_i, [_vp, _vp, _i64, _i64, _i, _vp]),
    "slam_comb_offset": (_u64, [_u64, _u32, _u64]),
    "slam_ancestors_from_scan_dev": (_i, [_vp, _i, _u64, C.c_uint32, _vp]),
    "slam_ancestors_sharded_dev": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _vp, _vp]),
    "slam_exchange_plan_host": (_i, [_vp, _i, _vp]),
    "slam_migrate_pack_dev": (_i, [_vp, _i, _i, _i, _vp, _vp, _i64, _vp, _i64, _i, _i, _vp]),
    "slam_migrate_unpack_dev": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i64, _vp, _i64, _i, _i]),
    "slam_argmax_dev": (_i, [_vp, _vp, _i, _vp, _vp]),
    "slam_gather_f32_dev": (_i, [_vp, _vp, _vp, _i, _vp]),
    "slam_gather_map_dev": (_i, [_vp, _vp, _vp, _i64, _i64, _i, _i, _i, _vp, _i]),
    "slam_mapper_create": (_i, [_vp, _i, _f, _f, C.POINTER(_vp)]),
    "slam_mapper_create_ex": (_i, [_vp, _i, _f, _f, _vp, C.POINTER(_vp)]),
    "slam_mapper_params_default": (None, [_vp]),
    "slam_mapper_destroy": (_i, [_vp]),
    "slam_mapper_first_frame": (_i, [_vp, _vp]),
    "slam_mapper_next_frame": (_i, [_vp, _vp, _fp]),
    "slam_mapper_get_map_host": (_i, [_vp, _vp, _vp, C.c_int32, C.POINTER(C.c_int32)]),
    "slam_mapper_device_view": (_i, [_vp, _vp]),
    "slam_exchange_set_capacity": (_i, [_vp, _i]),
    "slam_ekf_form_set": (_i, [_vp, _i]),
    "slam_ekf_form_counts": (_i, [_vp, _vp]),
    "slam_ekf_update_aniso_dev": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "slam_ekf_aniso_count": (_i, [_vp, _vp]),
    "slam_detections_upload_host": (_i, [_vp, _vp, _vp, _i]),
    "slam_detections_set_dev": (_i, [_vp, _vp, _vp, _i]),
    "slam_associate_dev": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _i, _vp, _i, _vp]),
    "slam_ekf_update_assoc_dev": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _vp, _i, _vp]),
    "slam_assoc_counts": (_i, [_vp, _vp]),
    "slam_associate_aniso_dev": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _f, _f, _i, _vp, _i, _vp]),
    "slam_ekf_update_assoc_aniso_dev": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp]),
    "slam_assoc_aniso_counts": (_i, [_vp, _vp]),
    "slam_detections_cov_upload_host": (_i, [_vp, _vp, _vp, _vp, _i]),
    "slam_detections_cov_set_dev": (_i, [_vp, _vp, _vp, _vp, _i]),
    "slam_detections_get_cov_host": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "slam_associate_detcov_dev": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _f, _i, _vp, _i, _vp]),
    "slam_ekf_update_assoc_detcov_dev": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp]),
    "slam_assoc_detcov_counts": (_i, [_vp, _vp]),
    "slam_landmark_evidence_dev": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "slam_evidence_init_dev": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _i, _i]),
    "slam_evidence_counts": (_i, [_vp, _vp]),
    "slam_sight_table_dev": (_i, [_vp, _i]),
    "slam_sight_table_get_host": (_i, [_vp, _vp, _vp]),
    "slam_landmark_evidence_sight_dev": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _f, _f,
                                              _vp, _vp]),
    "slam_sight_counts": (_i, [_vp, _vp]),
    "slam_fov_bound": (_f, [_f]),
    "slam_landmark_evidence_fov_dev": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _f, _f,
                                            _f, _f, _i, _vp, _vp, _vp]),
    "slam_fov_counts": (_i, [_vp, _vp]),
    "slam_landmark_merge_dev": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _i, _vp, _i, _i, _f, _vp]),
    "slam_merge_count": (_i, [_vp, _vp]),
    "slam_landmark_evidence_missed_dev": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp]),
    "slam_landmark_evidence_sight_missed_dev": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _f, _f,
                                                     _vp, _vp, _vp]),
    "slam_landmark_evidence_fov_missed_dev": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _f, _f,
                                                   _f, _f, _i, _vp, _vp, _vp, _vp]),
    "slam_assoc_weight_dev": (_i, [_vp, _vp, _vp, _i, _f, _f, _f, _vp, _vp]),
    "slam_assoc_weight_count": (_i, [_vp, _vp]),
    "slam_known_map_prepare_dev": (_i, [_vp, _vp, _i, _i, _f, _vp]),
    "slam_localise_dev": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _i, _f, _vp, _i, _vp, _vp]),
    "slam_localise_counts": (_i, [_vp, _vp]),
    "slam_localise_detcov_dev": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _i, _f, _vp, _i, _vp, _vp]),
    "slam_localise_detcov_count": (_i, [_vp, _vp]),
    "slam_localise_miss_dev": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _i, _f, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "slam_localise_detcov_miss_dev": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _i, _f, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "slam_localise_miss_count": (_i, [_vp, _vp]),
    "slam_pose_reseed_dev": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _u64, _u32, _f, _vp, _vp]),
    "slam_pose_reseed_count": (_i, [_vp, _vp]),
    "slam_pose_reseed_pairs_dev": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _u64, _u32, _f, _f, _f, _vp, _vp]),
    "slam_pose_reseed_pairs_count": (_i, [_vp, _vp]),
    "slam_detect_params_default": (None, [_vp]),
    "slam_detect_scan_dev": (_i, [_vp, _vp, _vp]),
    "slam_detect_count": (_i, [_vp, _vp]),
    "slam_detect_fit_default": (None, [_vp]),
    "slam_detect_scan_fit_dev": (_i, [_vp, _vp, _vp, _vp]),
    "slam_detect_fit_count": (_i, [_vp, _vp]),
    "slam_detections_get_host": (_i, [_vp, _vp, _vp, _vp]),
    "slam_selftest_reciprocal": (_i, [_vp, _vp, _vp]),
    "slam_frame_fusion_set": (_i, [_vp, _i]),
    "slam_frame_fusion_count": (_i, [_vp, _vp]),
    "slam_survivor_rows_set": (_i, [_vp, _i]),
    "slam_frame_front_last": (_i, [_vp, _vp]),
    "slam_ekf_inplace_form_set": (_i, [_vp, _i]),
    "slam_pf_paged_set": (_i, [_vp, _i]),
    "slam_pf_is_paged": (_i, [_vp]),
    "slam_pf_set_map_dev": (_i, [_vp, _vp, _i64, _i]),
    "slam_ekf_inplace_form_counts": (_i, [_vp, _vp]),
    "slam_resample_gate_set": (_i, [_vp, _f]),
    "slam_resample_happened_host": (_i, [_vp, C.POINTER(C.c_int)]),
    "slam_resample_heads_host": (_i, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "slam_comm_unique_id": (_i, [_vp]),
    "slam_comm_create_rccl": (_i, [_vp, _i, _i, _vp, C.POINTER(_vp)]),
    "slam_local_group_create": (_i, [_i, C.POINTER(_vp)]),
    "slam_local_group_destroy": (_i, [_vp]),
    "slam_comm_create_local": (_i, [_vp, _vp, _i, C.POINTER(_vp)]),
    "slam_comm_abort": (_i, [_vp]),
    "slam_comm_rank": (_i, [_vp]),
    "slam_comm_world": (_i, [_vp]),
    "slam_comm_destroy": (_i, [_vp]),
    "slam_pf_create_sharded": (_i, [_vp, _vp, _vp, _i, C.POINTER(_vp)]),
    "slam_pf_mean": (_i, [_vp, _f, _fp]),
    "slam_pf_spread": (_i, [_vp, _f, _fp, _fp, _fp]),
    "slam_pose_spread_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _f, _fp, _fp, _fp]),
    "slam_pf_modes": (_i, [_vp, _f, _f, _i, _i, C.POINTER(PfMode), C.POINTER(_i), C.POINTER(_i)]),
    "slam_pose_modes_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _f, _f, _i, _i, C.POINTER(PfMode), C.POINTER(_i), C.POINTER(_i),
                                 C.POINTER(_i64)]),
    "slam_pf_rows_received": (_i, [_vp]),
    "slam_pf_device_view": (_i, [_vp, _vp]),
    "slam_pf_frames_resampled": (_i64, [_vp]),
    "slam_pf_layout_changes": (_i64, [_vp]),
    "slam_pf_create": (_i, [_vp, _vp, C.POINTER(_vp)]),
    "slam_pf_destroy": (_i, [_vp]),
    "slam_pf_reset": (_i, [_vp, _fp]),
    "slam_pf_set_poses_host": (_i, [_vp, _vp, _vp, _vp]),
    "slam_pf_set_map_host": (_i, [_vp, _vp]),
    "slam_pf_step": (_i, [_vp, _i, _fp, _i]),
    "slam_pf_refine_set": (_i, [_vp, _f, _f, _i]),
    "slam_pf_meas_cov_set": (_i, [_vp, _vp]),
    "slam_pf_assoc_set": (_i, [_vp, _f, _f, _i]),
    "slam_pf_assoc_device_view": (_i, [_vp, _vp, _vp, _vp]),
    "slam_pf_assoc_cov_set": (_i, [_vp, _vp, _f, _f, _i]),
    "slam_pf_assoc_detcov_set": (_i, [_vp, _f, _f, _i]),
    "slam_pf_detect_noise_set": (_i, [_vp, _vp, _vp, _vp]),
    "slam_detect_scan_noise_dev": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "slam_detect_noise_count": (_i, [_vp, _vp]),
    "slam_pf_prune_set": (_i, [_vp, _i, _i, _i, _f]),
    "slam_pf_evidence_device_view": (_i, [_vp, _vp, _vp, _vp]),
    "slam_pf_get_evidence_host": (_i, [_vp, _vp]),
    "slam_pf_prune_sight_set": (_i, [_vp, _i, _f]),
    "slam_pf_sight_device_view": (_i, [_vp, _vp, _vp, _vp]),
    "slam_pf_prune_fov_set": (_i, [_vp, _i, _f, _f, _f]),
    "slam_pf_fov_device_view": (_i, [_vp, _vp, _vp]),
    "slam_pf_merge_set": (_i, [_vp, _f]),
    "slam_pf_merge_device_view": (_i, [_vp, _vp]),
    "slam_pf_assoc_weight_set": (_i, [_vp, _f, _f, _f, _i]),
    "slam_pf_assoc_weight_device_view": (_i, [_vp, _vp, _vp]),
    "slam_pf_known_map_set": (_i, [_vp, _vp, _i, _f, _f]),
    "slam_pf_known_map_detcov_set": (_i, [_vp, _vp, _i, _f, _f]),
    "slam_pf_known_map_device_view": (_i, [_vp, _vp, _vp, _vp]),
    "slam_pf_known_map_miss_set": (_i, [_vp, _f, _f, _i, _f, _f, _f, _i, _f]),
    "slam_pf_known_map_miss_device_view": (_i, [_vp, _vp, _vp, _vp]),
    "slam_pf_known_map_reseed": (_i, [_vp, _f, _vp]),
    "slam_pf_known_map_reseed_pairs": (_i, [_vp, _f, _f, _f, _vp]),
    "slam_pf_detect_set": (_i, [_vp, _vp]),
    "slam_pf_detect_fit_set": (_i, [_vp, _vp, _vp]),
    "slam_pf_best": (_i, [_vp, _fp, _fp, C.POINTER(C.c_int32)]),
    "slam_pf_get_poses_host": (_i, [_vp, _vp, _vp, _vp]),
    "slam_pf_get_map_host": (_i, [_vp, _vp]),
    "slam_pf_get_map_rows_host": (_i, [_vp, _vp, _i, _vp]),
    "slam_pf_paged_device_view": (_i, [_vp, _vp]),
    "slam_pf_layout": (_i, [_vp]),
    "slam_pf_split_device_view": (_i, [_vp, _vp]),
    "slam_pf_split_covx_view": (_i, [_vp, _vp]),
}

_LIB = None


def load_library() -> C.CDLL:
    """Load libslam_hip.so and bind every C-ABI symbol.  Raises if the library or a symbol is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP engine has not been built (run `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C hardware-acceleration-of-lidar-slam_amd/csrc`).  There is no CPU fallback.")
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def status_string(status: int) -> str:
    return load_library().slam_status_string(status).decode()


def _ptr(a):
    """Device pointer of a torch tensor / raw int, host pointer of a numpy array, or None."""
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data)
    return C.c_void_p(a.data_ptr())


def _np(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _f3(v):
    return (C.c_float * 3)(*[float(np.float32(x)) for x in v])


def _mode_list(modes, count):
    return [dict(pose=np.array(list(m.pose), np.float32), mass=np.float32(m.mass), cell=tuple(m.cell), ncells=int(m.ncells),
                 weight=int(m.weight)) for m in modes[:count]]


class Engine:
    """One engine per GPU / host thread (``slam_engine``)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.slam_engine_create(device, C.byref(h))
        if rc != SLAM_OK:
            raise SlamError(rc, "slam_engine_create", self.lib.slam_last_error(None).decode())
        self.h = h
        self.nbeams = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.slam_engine_destroy(self.h)
            self.h = None

    __del__ = close

    def _ck(self, rc, where):
        if rc != SLAM_OK:
            raise SlamError(rc, where, self.lib.slam_last_error(self.h).decode())

    def set_stream(self, stream_ptr: int | None):
        """stream_ptr: a hipStream_t as an integer (0 = HIP's default stream); None = the engine's own stream."""
        p = C.c_void_p(-1 & (2 ** (8 * C.sizeof(C.c_void_p)) - 1)) if stream_ptr is None else C.c_void_p(stream_ptr)
        self._ck(self.lib.slam_engine_set_stream(self.h, p), "set_stream")

    def sync(self):
        self._ck(self.lib.slam_engine_sync(self.h), "sync")

    PROF_SCORE, PROF_EDT, PROF_EKF, PROF_WEIGHTS, PROF_SCAN, PROF_ANCESTORS, PROF_PLAN, PROF_PACK, PROF_UNPACK = range(9)
    PROF_COLLECTIVES, PROF_PAGES, PROF_EKF_TAIL, PROF_MATERIALISE, PROF_COUNT = 9, 10, 11, 12, 13
    PROF_NAMES = ("score", "edt", "ekf", "weights", "scan", "ancestors", "plan", "pack", "unpack", "collectives", "pages", "ekf_tail",
                  "materialise")

    def profile_enable(self, *kernels):
        """profile_enable(PROF_EKF, ...) times those kernels; profile_enable() switches timing off."""
        mask = 0
        for k in kernels:
            mask |= 1 << k
        self._ck(self.lib.slam_profile_enable(self.h, mask), "profile_enable")

    def profile_read(self, kernel: int):
        """-> (total milliseconds, launches) of that kernel since the last read (HIP events on the engine stream)."""
        ms, n = C.c_double(0), C.c_int64(0)
        self._ck(self.lib.slam_profile_read(self.h, kernel, C.byref(ms), C.byref(n)), "profile_read")
        return ms.value, n.value

    def profile_bracket_overhead(self) -> float:
        """Milliseconds an empty event bracket measures on the engine's stream."""
        ms = C.c_double(0)
        self._ck(self.lib.slam_profile_bracket_overhead(self.h, C.byref(ms)), "profile_bracket_overhead")
        return ms.value

    def profile_copy_ceiling(self, d_src, d_dst, rows: int, plane_stride: int, reps: int = 12) -> float:
        """``slam_profile_copy_ceiling``: milliseconds of one pure copy of `rows` rows of 5 x plane_stride floats with the
        landmark update's access shape."""
        ms = C.c_double(0)
        self._ck(self.lib.slam_profile_copy_ceiling(self.h, _ptr(d_src), _ptr(d_dst), rows, plane_stride, reps, C.byref(ms)),
                 "profile_copy_ceiling")
        return ms.value

    # ---------------------------------------------------------------- host-buffer level (drop-in)
    def edt_host(self, occ: np.ndarray, rows: int, cols: int, cap: float = 10.0, out: np.ndarray | None = None):
        occ = _np(occ, np.int32)
        if out is None:
            out = np.zeros(occ.shape, np.float32)
        assert out.flags.c_contiguous and out.dtype == np.float32 and out.shape == occ.shape
        self._ck(self.lib.slam_edt_host(self.h, _ptr(occ), occ.shape[1], rows, cols, cap, _ptr(out)), "edt_host")
        return out

    def grid_upload(self, slot: int, occ: np.ndarray, meta: GridMeta, cap: float = 10.0, want_edt: bool = False):
        occ = _np(occ, np.int32)
        assert occ.ndim == 2 and occ.shape[1] == meta.ld and occ.shape[0] >= meta.rows
        out = np.zeros(occ.shape, np.float32) if want_edt else None
        self._ck(self.lib.slam_grid_upload_host(self.h, slot, _ptr(occ), C.byref(meta), cap, _ptr(out)), "grid_upload")
        return out

    def grid_set_dev(self, slot: int, d_edt, meta: GridMeta):
        self._ck(self.lib.slam_grid_set_dev(self.h, slot, _ptr(d_edt), C.byref(meta)), "grid_set_dev")
        # the engine adopts the buffer without copying it: keep the caller's array alive as long as the slot names it (a
        # temporary tensor would go back to its allocator and be handed out again under the engine's feet)
        self.__dict__.setdefault("_adopted", {})[("grid", slot)] = d_edt

    def grid_set_meta(self, slot: int, meta: GridMeta):
        self._ck(self.lib.slam_grid_set_meta(self.h, slot, C.byref(meta)), "grid_set_meta")

    def grid_packed_state(self, slot: int) -> int:
        """``slam_grid_packed_state``: 0 no verdict since the grid last changed, 1 the packed copy is in use, 2 the grid does not pack."""
        s = C.c_int(-1)
        self._ck(self.lib.slam_grid_packed_state(self.h, slot, C.byref(s)), "grid_packed_state")
        return int(s.value)

    def scan_upload(self, bx, by):
        bx, by = _np(bx, np.float32), _np(by, np.float32)
        assert bx.shape == by.shape and bx.ndim == 1
        self._ck(self.lib.slam_scan_upload_host(self.h, _ptr(bx), _ptr(by), len(bx)), "scan_upload")
        self.nbeams = len(bx)

    def scan_set_dev(self, d_bx, d_by, nbeams: int):
        self._ck(self.lib.slam_scan_set_dev(self.h, _ptr(d_bx), _ptr(d_by), nbeams), "scan_set_dev")
        self.nbeams = nbeams
        self.__dict__.setdefault("_adopted", {})["scan"] = (d_bx, d_by)

    def score_poses_cs_host(self, slot, x, y, ct, st):
        x, y, ct, st = (_np(a, np.float32) for a in (x, y, ct, st))
        score = np.empty(len(x), np.float32)
        count = np.empty(len(x), np.int32)
        self._ck(self.lib.slam_score_poses_cs_host(self.h, slot, _ptr(x), _ptr(y), _ptr(ct), _ptr(st), len(x),
                                                   _ptr(score), _ptr(count)), "score_poses_cs_host")
        return score, count

    def score_poses_host(self, slot, x, y, theta):
        x, y, theta = (_np(a, np.float32) for a in (x, y, theta))
        score = np.empty(len(x), np.float32)
        count = np.empty(len(x), np.int32)
        self._ck(self.lib.slam_score_poses_host(self.h, slot, _ptr(x), _ptr(y), _ptr(theta), len(x), _ptr(score),
                                                _ptr(count)), "score_poses_host")
        return score, count

    def pose_hits(self, slot, x, y, ct, st):
        hits = np.zeros(max(self.nbeams, 1), np.float32)
        n = C.c_int32(0)
        self._ck(self.lib.slam_pose_hits_host(self.h, slot, x, y, ct, st, _ptr(hits), C.byref(n)), "pose_hits")
        return hits[: n.value].copy(), n.value

    def fastmatch(self, slot, pose, res, hits: np.ndarray | None = None):
        """-> (pose[3], hit buffer, best_hits_size, best_score).  `hits` (float32, >= nbeams) plays the role of
        the reference's persistent FastMatchParameters.bestHits; a zeroed one is made when omitted."""
        out = (C.c_float * 3)()
        if hits is None:
            hits = np.zeros(max(self.nbeams, 1), np.float32)
        n = C.c_int32(-1)
        sc = C.c_float(0)
        self._ck(self.lib.slam_fastmatch_host(self.h, slot, _f3(pose), _f3(res), out, _ptr(hits), C.byref(n),
                                              C.byref(sc)), "fastmatch")
        return np.array(list(out), np.float32), hits, n.value, np.float32(sc.value)

    # ---------------------------------------------------------------- device level (async on the engine stream)
    def edt_dev(self, d_occ, ld, rows, cols, cap, d_out):
        self._ck(self.lib.slam_edt_dev(self.h, _ptr(d_occ), ld, rows, cols, cap, _ptr(d_out)), "edt_dev")

    def score_poses_dev(self, slot, d_x, d_y, d_th, n, d_score, d_count):
        self._ck(self.lib.slam_score_poses_dev(self.h, slot, _ptr(d_x), _ptr(d_y), _ptr(d_th), n, _ptr(d_score),
                                               _ptr(d_count)), "score_poses_dev")

    def score_poses_cs_dev(self, slot, d_x, d_y, d_ct, d_st, n, d_score, d_count):
        self._ck(self.lib.slam_score_poses_cs_dev(self.h, slot, _ptr(d_x), _ptr(d_y), _ptr(d_ct), _ptr(d_st), n,
                                                  _ptr(d_score), _ptr(d_count)), "score_poses_cs_dev")

    def motion_sample_dev(self, src, anc, dst, n, first_id, dp, sigma, seed, frame):
        """src / dst: triples (x, y, theta) of device arrays."""
        self._ck(self.lib.slam_motion_sample_dev(self.h, _ptr(src[0]), _ptr(src[1]), _ptr(src[2]), _ptr(anc),
                                                 _ptr(dst[0]), _ptr(dst[1]), _ptr(dst[2]), n, first_id, _f3(dp),
                                                 _f3(sigma), seed, frame), "motion_sample_dev")

    def motion_score_dev(self, slot, src, anc, dst, n, first_id, dp, sigma, seed, frame, d_score, d_count):
        self._ck(self.lib.slam_motion_score_dev(self.h, slot, _ptr(src[0]), _ptr(src[1]), _ptr(src[2]), _ptr(anc),
                                                _ptr(dst[0]), _ptr(dst[1]), _ptr(dst[2]), n, first_id, _f3(dp),
                                                _f3(sigma), seed, frame, _ptr(d_score), _ptr(d_count)), "motion_score_dev")

    def refine_poses_dev(self, slot, d_x, d_y, d_th, n, step_xy, step_theta, sweeps, d_score, d_count):
        """`sweeps` sweeps of the 27-pose lattice around every pose, in place; d_score / d_count: those of the final pose."""
        self._ck(self.lib.slam_refine_poses_dev(self.h, slot, _ptr(d_x), _ptr(d_y), _ptr(d_th), n, step_xy, step_theta, sweeps,
                                                _ptr(d_score), _ptr(d_count)), "refine_poses_dev")

    def motion_refine_dev(self, slot, src, anc, dst, n, first_id, dp, sigma, seed, frame, step_xy, step_theta, sweeps, d_score,
                          d_count):
        self._ck(self.lib.slam_motion_refine_dev(self.h, slot, _ptr(src[0]), _ptr(src[1]), _ptr(src[2]), _ptr(anc),
                                                 _ptr(dst[0]), _ptr(dst[1]), _ptr(dst[2]), n, first_id, _f3(dp), _f3(sigma),
                                                 seed, frame, step_xy, step_theta, sweeps, _ptr(d_score), _ptr(d_count)),
                 "motion_refine_dev")

    def obs_set_dev(self, d_zx_by_landmark, d_zy_by_landmark, nlandmarks):
        """Observation table on the device: entry l = observation of landmark l, NaN in zx = not observed."""
        self._ck(self.lib.slam_obs_set_dev(self.h, _ptr(d_zx_by_landmark), _ptr(d_zy_by_landmark), nlandmarks),
                 "obs_set_dev")
        self.__dict__.setdefault("_adopted", {})["obs"] = (d_zx_by_landmark, d_zy_by_landmark)

    def logweight_ekf_dev(self, d_score, gain, n, d_logw, d_max):
        self._ck(self.lib.slam_logweight_ekf_dev(self.h, _ptr(d_score), gain, n, _ptr(d_logw), _ptr(d_max)),
                 "logweight_ekf_dev")

    def obs_upload(self, landmark_id, zx, zy, nlandmarks):
        ids, zx, zy = _np(landmark_id, np.int32), _np(zx, np.float32), _np(zy, np.float32)
        self._ck(self.lib.slam_obs_upload_host(self.h, _ptr(ids), _ptr(zx), _ptr(zy), len(ids), nlandmarks),
                 "obs_upload")

    def ekf_update_dev(self, d_map_in, d_map_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, meas_var,
                       d_loglik):
        """Maps are one row per particle: [particle][5 planes][plane_stride] floats (include/slam_hip.h)."""
        self._ck(self.lib.slam_ekf_update_dev(self.h, _ptr(d_map_in), _ptr(d_map_out), row_stride, plane_stride, nlandmarks,
                                              _ptr(d_x), _ptr(d_y), _ptr(d_th), _ptr(d_anc), n, meas_var,
                                              _ptr(d_loglik)), "ekf_update_dev")

    def ekf_update_aniso_dev(self, d_map_in, d_map_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, meas_cov,
                             d_loglik):
        """``slam_ekf_update_aniso_dev``: ekf_update_dev with a 2x2 sensor-frame measurement covariance, meas_cov = (qxx, qxy, qyy)."""
        self._ck(self.lib.slam_ekf_update_aniso_dev(self.h, _ptr(d_map_in), _ptr(d_map_out), row_stride, plane_stride, nlandmarks,
                                                    _ptr(d_x), _ptr(d_y), _ptr(d_th), _ptr(d_anc), n, _f3(meas_cov),
                                                    _ptr(d_loglik)), "ekf_update_aniso_dev")

    def ekf_aniso_count(self) -> int:
        c = C.c_int64(0)
        self._ck(self.lib.slam_ekf_aniso_count(self.h, C.byref(c)), "ekf_aniso_count")
        return int(c.value)

    def detections_upload(self, zx, zy):
        """``slam_detections_upload_host``: the frame's detections, sensor-frame points without identity (at most 64, finite)."""
        zx, zy = _np(zx, np.float32), _np(zy, np.float32)
        assert len(zx) == len(zy)
        self._ck(self.lib.slam_detections_upload_host(self.h, _ptr(zx), _ptr(zy), len(zx)), "detections_upload")

    def detections_set_dev(self, d_zx, d_zy, ndet):
        """``slam_detections_set_dev``: the same from two device arrays, adopted and read afresh by every launch."""
        self._ck(self.lib.slam_detections_set_dev(self.h, _ptr(d_zx), _ptr(d_zy), ndet), "detections_set_dev")
        self.__dict__.setdefault("_adopted", {})["det"] = (d_zx, d_zy)

    def associate_dev(self, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, meas_var, gate, new_gate, create,
                      d_assoc, assoc_stride, d_stats):
        """``slam_associate_dev``: every particle's table uint8 [n][assoc_stride] (255 = none) and stats int32 [n][3]."""
        self._ck(self.lib.slam_associate_dev(self.h, _ptr(d_map), row_stride, plane_stride, nlandmarks, _ptr(d_x), _ptr(d_y), _ptr(d_th),
                                             _ptr(d_anc), n, meas_var, gate, new_gate, int(create), _ptr(d_assoc), assoc_stride,
                                             _ptr(d_stats)), "associate_dev")

    def ekf_update_assoc_dev(self, d_map_in, d_map_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, meas_var,
                             d_assoc, assoc_stride, d_loglik):
        """``slam_ekf_update_assoc_dev``: ekf_update_dev with particle i's observations read through its table row."""
        self._ck(self.lib.slam_ekf_update_assoc_dev(self.h, _ptr(d_map_in), _ptr(d_map_out), row_stride, plane_stride, nlandmarks,
                                                    _ptr(d_x), _ptr(d_y), _ptr(d_th), _ptr(d_anc), n, meas_var, _ptr(d_assoc),
                                                    assoc_stride, _ptr(d_loglik)), "ekf_update_assoc_dev")

    def known_map_prepare_dev(self, d_map, plane_stride, nlandmarks, meas_var, d_prepared):
        """``slam_known_map_prepare_dev``: a known map float32 [5][plane_stride] -> the prepared map [6][plane_stride]."""
        self._ck(self.lib.slam_known_map_prepare_dev(self.h, _ptr(d_map), plane_stride, nlandmarks, meas_var, _ptr(d_prepared)),
                 "known_map_prepare_dev")

    def localise_dev(self, d_prepared, plane_stride, nlandmarks, d_x, d_y, d_th, n, gate, d_assoc, assoc_stride, d_stats, d_loglik=None):
        """``slam_localise_dev``: the engine's detections against ONE prepared map per particle: stats int32 [n][3], the
        log-likelihood (d_loglik None: the engine's buffer) and, with d_assoc, the table uint8 [n][assoc_stride]."""
        self._ck(self.lib.slam_localise_dev(self.h, _ptr(d_prepared), plane_stride, nlandmarks, _ptr(d_x), _ptr(d_y), _ptr(d_th), n, gate,
                                            _ptr(d_assoc), assoc_stride, _ptr(d_stats), _ptr(d_loglik)), "localise_dev")

    def localise_counts(self):
        """-> (prepare launches, stage launches) of this engine so far."""
        c = (C.c_int64 * 2)()
        self._ck(self.lib.slam_localise_counts(self.h, c), "localise_counts")
        return int(c[0]), int(c[1])

    def localise_detcov_dev(self, d_map, plane_stride, nlandmarks, d_x, d_y, d_th, n, gate, d_assoc, assoc_stride, d_stats, d_loglik=None):
        """``slam_localise_detcov_dev``: the engine's detections AND THEIR COVARIANCES against ONE map float32 [5][plane_stride] as it
        was given, per particle: stats, log-likelihood and table as ``localise_dev``."""
        self._ck(self.lib.slam_localise_detcov_dev(self.h, _ptr(d_map), plane_stride, nlandmarks, _ptr(d_x), _ptr(d_y), _ptr(d_th), n, gate,
                                                   _ptr(d_assoc), assoc_stride, _ptr(d_stats), _ptr(d_loglik)), "localise_detcov_dev")

    def localise_detcov_count(self):
        """-> stage launches under per-detection covariances of this engine so far."""
        c = C.c_int64(0)
        self._ck(self.lib.slam_localise_detcov_count(self.h, C.byref(c)), "localise_detcov_count")
        return int(c.value)

    def localise_miss_dev(self, d_prepared, plane_stride, nlandmarks, d_x, d_y, d_th, n, gate, d_assoc, assoc_stride, d_stats, d_loglik,
                          view, d_missed, d_spared=None, d_outside=None):
        """``slam_localise_miss_dev``: ``localise_dev`` whose launch also counts the landmarks in view that no detection matched —
        view: a ``LocaliseView``; missed, spared, outside int32 [n] (the last two may be None)."""
        self._ck(self.lib.slam_localise_miss_dev(self.h, _ptr(d_prepared), plane_stride, nlandmarks, _ptr(d_x), _ptr(d_y), _ptr(d_th), n, gate,
                                                 _ptr(d_assoc), assoc_stride, _ptr(d_stats), _ptr(d_loglik),
                                                 C.byref(view) if view is not None else None, _ptr(d_missed), _ptr(d_spared),
                                                 _ptr(d_outside)), "localise_miss_dev")

    def localise_detcov_miss_dev(self, d_map, plane_stride, nlandmarks, d_x, d_y, d_th, n, gate, d_assoc, assoc_stride, d_stats, d_loglik,
                                 view, d_missed, d_spared=None, d_outside=None):
        """``slam_localise_detcov_miss_dev``: ``localise_detcov_dev`` with the counts of ``localise_miss_dev``."""
        self._ck(self.lib.slam_localise_detcov_miss_dev(self.h, _ptr(d_map), plane_stride, nlandmarks, _ptr(d_x), _ptr(d_y), _ptr(d_th), n,
                                                        gate, _ptr(d_assoc), assoc_stride, _ptr(d_stats), _ptr(d_loglik),
                                                        C.byref(view) if view is not None else None, _ptr(d_missed), _ptr(d_spared),
                                                        _ptr(d_outside)), "localise_detcov_miss_dev")

    def localise_miss_count(self):
        """-> launches of the two miss forms of the localise stage of this engine so far."""
        c = C.c_int64(0)
        self._ck(self.lib.slam_localise_miss_count(self.h, C.byref(c)), "localise_miss_count")
        return int(c.value)

    def pose_reseed_dev(self, d_map, plane_stride, nlandmarks, d_x_in, d_y_in, d_th_in, d_anc, d_x_out, d_y_out, d_th_out, n, first_id,
                        seed, frame, fraction, d_flag=None):
        """``slam_pose_reseed_dev``: a chosen fraction of n slots becomes pose proposals at which one of the engine's current
        detections coincides with one landmark of d_map (float32 [5][plane_stride], as it was given); the rest copy the pose of
        d_anc[i] (None: i, and out may be in).  d_flag uint8 [n] or None.  -> (replaced, chosen but not replaced).  Synchronises."""
        c = (C.c_int32 * 2)()
        self._ck(self.lib.slam_pose_reseed_dev(self.h, _ptr(d_map), plane_stride, nlandmarks, _ptr(d_x_in), _ptr(d_y_in), _ptr(d_th_in),
                                               _ptr(d_anc), _ptr(d_x_out), _ptr(d_y_out), _ptr(d_th_out), n, first_id, seed, frame,
                                               float(fraction), _ptr(d_flag), c), "pose_reseed_dev")
        return int(c[0]), int(c[1])

    def pose_reseed_count(self):
        """-> launches of ``pose_reseed_dev`` (the session's reseeds included) of this engine so far."""
        c = C.c_int64(0)
        self._ck(self.lib.slam_pose_reseed_count(self.h, C.byref(c)), "pose_reseed_count")
        return int(c.value)

    def pose_reseed_pairs_dev(self, d_map, plane_stride, nlandmarks, d_x_in, d_y_in, d_th_in, d_anc, d_x_out, d_y_out, d_th_out, n,
                              first_id, seed, frame, fraction, tol, min_sep, d_flag=None):
        """``slam_pose_reseed_pairs_dev``: a chosen fraction of n slots becomes pose proposals at which TWO of the engine's current
        detections coincide with two landmarks of d_map whose distance is the detections' within tol (detections closer than
        min_sep make no pair); the rest copy the pose of d_anc[i] (None: i, and out may be in).  d_flag uint8 [n] or None.
        -> (replaced, first landmark slot empty, detections too close, no partner in the map).  Synchronises."""
        c = (C.c_int32 * 4)()
        self._ck(self.lib.slam_pose_reseed_pairs_dev(self.h, _ptr(d_map), plane_stride, nlandmarks, _ptr(d_x_in), _ptr(d_y_in),
                                                     _ptr(d_th_in), _ptr(d_anc), _ptr(d_x_out), _ptr(d_y_out), _ptr(d_th_out), n, first_id,
                                                     seed, frame, float(fraction), float(tol), float(min_sep), _ptr(d_flag), c),
                 "pose_reseed_pairs_dev")
        return tuple(int(v) for v in c)

    def pose_reseed_pairs_count(self):
        """-> launches of ``pose_reseed_pairs_dev`` (the session's included) of this engine so far."""
        c = C.c_int64(0)
        self._ck(self.lib.slam_pose_reseed_pairs_count(self.h, C.byref(c)), "pose_reseed_pairs_count")
        return int(c.value)

    def assoc_counts(self):
        """-> (associate launches, assoc-update launches) of this engine so far."""
        c = (C.c_int64 * 2)()
        self._ck(self.lib.slam_assoc_counts(self.h, c), "assoc_counts")
        return int(c[0]), int(c[1])

    def associate_aniso_dev(self, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, meas_cov, gate, new_gate, create,
                            d_assoc, assoc_stride, d_stats):
        """``slam_associate_aniso_dev``: associate_dev under a 2x2 sensor-frame measurement covariance, meas_cov = (qxx, qxy, qyy)."""
        self._ck(self.lib.slam_associate_aniso_dev(self.h, _ptr(d_map), row_stride, plane_stride, nlandmarks, _ptr(d_x), _ptr(d_y),
                                                   _ptr(d_th), _ptr(d_anc), n, _f3(meas_cov), gate, new_gate, int(create), _ptr(d_assoc),
                                                   assoc_stride, _ptr(d_stats)), "associate_aniso_dev")

    def ekf_update_assoc_aniso_dev(self, d_map_in, d_map_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, meas_cov,
                                   d_assoc, assoc_stride, d_loglik):
        """``slam_ekf_update_assoc_aniso_dev``: ekf_update_aniso_dev with particle i's observations read through its table row."""
        self._ck(self.lib.slam_ekf_update_assoc_aniso_dev(self.h, _ptr(d_map_in), _ptr(d_map_out), row_stride, plane_stride, nlandmarks,
                                                          _ptr(d_x), _ptr(d_y), _ptr(d_th), _ptr(d_anc), n, _f3(meas_cov), _ptr(d_assoc),
                                                          assoc_stride, _ptr(d_loglik)), "ekf_update_assoc_aniso_dev")

    def assoc_aniso_counts(self):
        """-> (associate launches, assoc-update launches) under a 2x2 covariance of this engine so far."""
        c = (C.c_int64 * 2)()
        self._ck(self.lib.slam_assoc_aniso_counts(self.h, c), "assoc_aniso_counts")
        return int(c[0]), int(c[1])

    def detections_cov_upload(self, qxx, qxy, qyy):
        """``slam_detections_cov_upload_host``: a sensor-frame covariance Q_k = (qxx[k], qxy[k], qyy[k]) for each of the
        detections handed over last."""
        qxx, qxy, qyy = _np(qxx, np.float32), _np(qxy, np.float32), _np(qyy, np.float32)
        assert len(qxx) == len(qxy) == len(qyy)
        self._ck(self.lib.slam_detections_cov_upload_host(self.h, _ptr(qxx), _ptr(qxy), _ptr(qyy), len(qxx)), "detections_cov_upload")

    def detections_cov_set_dev(self, d_qxx, d_qxy, d_qyy, ndet):
        """``slam_detections_cov_set_dev``: the same from three device arrays, adopted and read afresh by every launch."""
        self._ck(self.lib.slam_detections_cov_set_dev(self.h, _ptr(d_qxx), _ptr(d_qxy), _ptr(d_qyy), ndet), "detections_cov_set_dev")
        self.__dict__.setdefault("_adopted", {})["detcov"] = (d_qxx, d_qxy, d_qyy)

    def detections_cov(self):
        """``slam_detections_get_cov_host``: the covariances of the current detections -> (qxx, qxy, qyy) float32 [ndet];
        synchronises."""
        q = [np.full(64, np.nan, np.float32) for _ in range(3)]
        k = C.c_int32(-1)
        self._ck(self.lib.slam_detections_get_cov_host(self.h, _ptr(q[0]), _ptr(q[1]), _ptr(q[2]), C.byref(k)), "detections_get_cov_host")
        return tuple(v[:k.value].copy() for v in q)

    def associate_detcov_dev(self, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, gate, new_gate, create,
                             d_assoc, assoc_stride, d_stats):
        """``slam_associate_detcov_dev``: associate_aniso_dev with the covariance each detection carries in the place of one Q."""
        self._ck(self.lib.slam_associate_detcov_dev(self.h, _ptr(d_map), row_stride, plane_stride, nlandmarks, _ptr(d_x), _ptr(d_y),
                                                    _ptr(d_th), _ptr(d_anc), n, gate, new_gate, int(create), _ptr(d_assoc),
                                                    assoc_stride, _ptr(d_stats)), "associate_detcov_dev")

    def ekf_update_assoc_detcov_dev(self, d_map_in, d_map_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n,
                                    d_assoc, assoc_stride, d_loglik):
        """``slam_ekf_update_assoc_detcov_dev``: ekf_update_assoc_aniso_dev with, for every landmark, the covariance of the
        detection its table entry names."""
        self._ck(self.lib.slam_ekf_update_assoc_detcov_dev(self.h, _ptr(d_map_in), _ptr(d_map_out), row_stride, plane_stride, nlandmarks,
                                                           _ptr(d_x), _ptr(d_y), _ptr(d_th), _ptr(d_anc), n, _ptr(d_assoc),
                                                           assoc_stride, _ptr(d_loglik)), "ekf_update_assoc_detcov_dev")

    def assoc_detcov_counts(self):
        """-> (associate launches, assoc-update launches) under per-detection covariances of this engine so far."""
        c = (C.c_int64 * 2)()
        self._ck(self.lib.slam_assoc_detcov_counts(self.h, c), "assoc_detcov_counts")
        return int(c[0]), int(c[1])

    def landmark_evidence_dev(self, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_anc, n, d_assoc, assoc_stride, d_ev_in,
                              d_ev_out, ev_stride, hit, miss, cmax, view_range, d_stats, d_missed=None):
        """``slam_landmark_evidence_dev``: the evidence bytes uint8 [n][ev_stride] behind a frame's associating update; pruned
        landmarks' slots in d_map become unused ones; stats int32 [n][2] = pruned, seen after pruning.  d_missed (int32 [n]: the
        slots scored as a miss): ``slam_landmark_evidence_missed_dev``."""
        if d_missed is not None:
            self._ck(self.lib.slam_landmark_evidence_missed_dev(self.h, _ptr(d_map), row_stride, plane_stride, nlandmarks, _ptr(d_x),
                                                                _ptr(d_y), _ptr(d_anc), n, _ptr(d_assoc), assoc_stride, _ptr(d_ev_in),
                                                                _ptr(d_ev_out), ev_stride, int(hit), int(miss), int(cmax), view_range,
                                                                _ptr(d_stats), _ptr(d_missed)), "landmark_evidence_missed_dev")
            return
        self._ck(self.lib.slam_landmark_evidence_dev(self.h, _ptr(d_map), row_stride, plane_stride, nlandmarks, _ptr(d_x), _ptr(d_y),
                                                     _ptr(d_anc), n, _ptr(d_assoc), assoc_stride, _ptr(d_ev_in), _ptr(d_ev_out),
                                                     ev_stride, int(hit), int(miss), int(cmax), view_range, _ptr(d_stats)),
                 "landmark_evidence_dev")

    def evidence_init_dev(self, d_map, row_stride, plane_stride, nlandmarks, nrows, d_ev, ev_stride, value):
        """``slam_evidence_init_dev``: evidence = seen ? value : 0 for the nrows rows of d_map."""
        self._ck(self.lib.slam_evidence_init_dev(self.h, _ptr(d_map), row_stride, plane_stride, nlandmarks, nrows, _ptr(d_ev), ev_stride,
                                                 int(value)), "evidence_init_dev")

    def sight_table_dev(self, bins: int):
        """``slam_sight_table_dev``: the sight table of the current scan (bins a power of two in 32 .. 1024), in the engine's buffer."""
        self._ck(self.lib.slam_sight_table_dev(self.h, int(bins)), "sight_table_dev")

    def sight_table(self):
        """``slam_sight_table_get_host``: the current sight table float32 [bins]; synchronises."""
        t, bins = np.full(1024, np.nan, np.float32), C.c_int32(0)
        self._ck(self.lib.slam_sight_table_get_host(self.h, _ptr(t), C.byref(bins)), "sight_table_get_host")
        return t[:bins.value].copy()

    def landmark_evidence_sight_dev(self, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, d_assoc, assoc_stride,
                                    d_ev_in, d_ev_out, ev_stride, hit, miss, cmax, view_range, margin, d_stats, d_spared, d_missed=None):
        """``slam_landmark_evidence_sight_dev``: landmark_evidence_dev in which a landmark behind what the engine's sight table
        holds in its direction takes no miss; spared int32 [n] = the landmarks spared one.  d_missed:
        ``slam_landmark_evidence_sight_missed_dev``."""
        if d_missed is not None:
            self._ck(self.lib.slam_landmark_evidence_sight_missed_dev(self.h, _ptr(d_map), row_stride, plane_stride, nlandmarks, _ptr(d_x),
                                                                      _ptr(d_y), _ptr(d_th), _ptr(d_anc), n, _ptr(d_assoc), assoc_stride,
                                                                      _ptr(d_ev_in), _ptr(d_ev_out), ev_stride, int(hit), int(miss),
                                                                      int(cmax), view_range, margin, _ptr(d_stats), _ptr(d_spared),
                                                                      _ptr(d_missed)), "landmark_evidence_sight_missed_dev")
            return
        self._ck(self.lib.slam_landmark_evidence_sight_dev(self.h, _ptr(d_map), row_stride, plane_stride, nlandmarks, _ptr(d_x),
                                                           _ptr(d_y), _ptr(d_th), _ptr(d_anc), n, _ptr(d_assoc), assoc_stride,
                                                           _ptr(d_ev_in), _ptr(d_ev_out), ev_stride, int(hit), int(miss), int(cmax),
                                                           view_range, margin, _ptr(d_stats), _ptr(d_spared)),
                 "landmark_evidence_sight_dev")

    def sight_counts(self):
        """-> (sight-table launches, sight evidence-stage launches) of this engine so far."""
        c = (C.c_int64 * 2)()
        self._ck(self.lib.slam_sight_counts(self.h, c), "sight_counts")
        return int(c[0]), int(c[1])

    def landmark_evidence_fov_dev(self, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, d_assoc, assoc_stride,
                                  d_ev_in, d_ev_out, ev_stride, hit, miss, cmax, view_range, margin, lo, hi, use_sight, d_stats, d_spared,
                                  d_outside, d_missed=None):
        """``slam_landmark_evidence_fov_dev``: landmark_evidence_sight_dev (use_sight) or landmark_evidence_dev in which a landmark
        due a miss whose diamond angle in the sensor frame lies outside [lo, hi] takes none; outside int32 [n] = those landmarks.
        d_missed: ``slam_landmark_evidence_fov_missed_dev``."""
        if d_missed is not None:
            self._ck(self.lib.slam_landmark_evidence_fov_missed_dev(self.h, _ptr(d_map), row_stride, plane_stride, nlandmarks, _ptr(d_x),
                                                                    _ptr(d_y), _ptr(d_th), _ptr(d_anc), n, _ptr(d_assoc), assoc_stride,
                                                                    _ptr(d_ev_in), _ptr(d_ev_out), ev_stride, int(hit), int(miss),
                                                                    int(cmax), view_range, margin, lo, hi, int(bool(use_sight)),
                                                                    _ptr(d_stats), _ptr(d_spared), _ptr(d_outside), _ptr(d_missed)),
                     "landmark_evidence_fov_missed_dev")
            return
        self._ck(self.lib.slam_landmark_evidence_fov_dev(self.h, _ptr(d_map), row_stride, plane_stride, nlandmarks, _ptr(d_x),
                                                         _ptr(d_y), _ptr(d_th), _ptr(d_anc), n, _ptr(d_assoc), assoc_stride,
                                                         _ptr(d_ev_in), _ptr(d_ev_out), ev_stride, int(hit), int(miss), int(cmax),
                                                         view_range, margin, lo, hi, int(bool(use_sight)), _ptr(d_stats),
                                                         _ptr(d_spared), _ptr(d_outside)),
                 "landmark_evidence_fov_dev")

    def fov_counts(self):
        """-> the launches of the evidence stage with a field of view of this engine so far."""
        c = C.c_int64(0)
        self._ck(self.lib.slam_fov_counts(self.h, C.byref(c)), "fov_counts")
        return int(c.value)

    def landmark_merge_dev(self, d_map, row_stride, plane_stride, nlandmarks, n, d_assoc, assoc_stride, d_ev, ev_stride, cmax, merge_gate,
                           d_stats=None):
        """``slam_landmark_merge_dev``: behind the frame's associating update and evidence stage, in place — a seen landmark the
        table does not name that lies within merge_gate of one it names is fused into it and its slot cleared (d_ev None: without
        evidence); stats int32 [n][3] = merged, refused, seen after."""
        self._ck(self.lib.slam_landmark_merge_dev(self.h, _ptr(d_map), row_stride, plane_stride, nlandmarks, n, _ptr(d_assoc), assoc_stride,
                                                  _ptr(d_ev), ev_stride, int(cmax), merge_gate, _ptr(d_stats)),
                 "landmark_merge_dev")

    def merge_count(self):
        """-> the launches of the merge stage of this engine so far."""
        c = C.c_int64(0)
        self._ck(self.lib.slam_merge_count(self.h, C.byref(c)), "merge_count")
        return int(c.value)

    def assoc_weight_dev(self, d_stats, d_missed, n, log_new, log_clutter, log_miss, d_loglik=None, d_terms=None):
        """``slam_assoc_weight_dev``: loglik[i] += created_i * log_new + dropped_i * log_clutter + missed_i * log_miss (d_stats: the
        association's int32 [n][3]; d_missed None: 0; d_loglik None: the engine's buffer; d_terms: the sum that was added)."""
        self._ck(self.lib.slam_assoc_weight_dev(self.h, _ptr(d_stats), _ptr(d_missed), n, log_new, log_clutter, log_miss, _ptr(d_loglik),
                                                _ptr(d_terms)), "assoc_weight_dev")

    def assoc_weight_count(self):
        """-> the launches of slam_assoc_weight_dev of this engine so far."""
        c = C.c_int64(0)
        self._ck(self.lib.slam_assoc_weight_count(self.h, C.byref(c)), "assoc_weight_count")
        return int(c.value)

    def detect_scan_dev(self, params: "DetectParams | None" = None, d_stats=None, **kw):
        """``slam_detect_scan_dev``: the engine's current scan -> its current detections (asynchronous; the count is picked up by
        the next associating stage or by detections()).  params: a DetectParams, or the defaults with the keywords applied."""
        p = params if params is not None else DetectParams.default(**kw)
        self._ck(self.lib.slam_detect_scan_dev(self.h, C.byref(p), _ptr(d_stats)), "detect_scan_dev")

    def detect_scan_fit_dev(self, fit: "DetectFit | tuple | None", params: "DetectParams | None" = None, d_stats=None, **kw):
        """``slam_detect_scan_fit_dev``: detect_scan_dev with every detection the centre of a circle of known radius fitted to
        its segment, and the shape test.  fit: a DetectFit, (radius, spread_tol), or None (the centroid: detect_scan_dev)."""
        p = params if params is not None else DetectParams.default(**kw)
        f = DetectFit.of(fit)
        self._ck(self.lib.slam_detect_scan_fit_dev(self.h, C.byref(p), C.byref(f) if f is not None else None, _ptr(d_stats)),
                 "detect_scan_fit_dev")

    def detect_scan_noise_dev(self, noise, fit=None, params: "DetectParams | None" = None, d_stats=None, **kw):
        """``slam_detect_scan_noise_dev``: detect_scan_fit_dev with the noise model (range_var, bearing_var, lateral_var) (None:
        exactly detect_scan_fit_dev): the detections carry covariances; d_stats: int32 [6]."""
        p = params if params is not None else DetectParams.default(**kw)
        f = DetectFit.of(fit)
        z = DetectNoise.of(noise)
        self._ck(self.lib.slam_detect_scan_noise_dev(self.h, C.byref(p), C.byref(f) if f is not None else None,
                                                     C.byref(z) if z is not None else None, _ptr(d_stats)), "detect_scan_noise_dev")

    def detect_noise_count(self) -> int:
        """Detector launches of this engine so far that ran the noise model."""
        c = C.c_int64(0)
        self._ck(self.lib.slam_detect_noise_count(self.h, C.byref(c)), "detect_noise_count")
        return c.value

    def detect_fit_count(self) -> int:
        """Detector launches of this engine so far that ran the fit."""
        c = C.c_int64(0)
        self._ck(self.lib.slam_detect_fit_count(self.h, C.byref(c)), "detect_fit_count")
        return c.value

    def detect_count(self) -> int:
        """Detector launches of this engine so far."""
        c = C.c_int64(0)
        self._ck(self.lib.slam_detect_count(self.h, C.byref(c)), "detect_count")
        return c.value

    def detections(self, full: bool = False):
        """``slam_detections_get_host``: the current detections, whatever their origin -> (zx, zy) float32 [ndet]; synchronises.
        full: -> (zx [64], zy [64], ndet), the entries from ndet on as the call returns them (0)."""
        zx, zy, k = np.full(64, np.nan, np.float32), np.full(64, np.nan, np.float32), C.c_int32(-1)
        self._ck(self.lib.slam_detections_get_host(self.h, _ptr(zx), _ptr(zy), C.byref(k)), "detections_get_host")
        return (zx, zy, k.value) if full else (zx[:k.value].copy(), zy[:k.value].copy())

    def evidence_counts(self):
        """-> (evidence launches, evidence-init launches) of this engine so far."""
        c = (C.c_int64 * 2)()
        self._ck(self.lib.slam_evidence_counts(self.h, c), "evidence_counts")
        return int(c[0]), int(c[1])

    def logweight_dev(self, d_score, d_loglik, gain, n, d_logw, d_max):
        self._ck(self.lib.slam_logweight_dev(self.h, _ptr(d_score), _ptr(d_loglik), gain, n, _ptr(d_logw), _ptr(d_max)),
                 "logweight_dev")

    def quantise_weights_dev(self, d_logw, d_max, n, d_wq, d_sum):
        self._ck(self.lib.slam_quantise_weights_dev(self.h, _ptr(d_logw), _ptr(d_max), n, _ptr(d_wq), _ptr(d_sum)),
                 "quantise_weights_dev")

    def quantise_scan_dev(self, d_logw, d_max, n, d_sum):
        self._ck(self.lib.slam_quantise_scan_dev(self.h, _ptr(d_logw), _ptr(d_max), n, _ptr(d_sum)), "quantise_scan_dev")

    def offspring_from_scan_dev(self, n, d_base, d_total, seed, frame, n_total, d_first):
        self._ck(self.lib.slam_offspring_from_scan_dev(self.h, n, _ptr(d_base), _ptr(d_total), seed, frame, n_total,
                                                       _ptr(d_first)), "offspring_from_scan_dev")

    def offspring_from_scan_sharded_dev(self, n, d_shard_totals, rank, world, seed, frame, n_total, d_first):
        self._ck(self.lib.slam_offspring_from_scan_sharded_dev(self.h, n, _ptr(d_shard_totals), rank, world, seed, frame,
                                                               n_total, _ptr(d_first)), "offspring_from_scan_sharded_dev")

    def prefix_sum_dev(self, d_wq, n, d_cdf):
        self._ck(self.lib.slam_prefix_sum_dev(self.h, _ptr(d_wq), n, _ptr(d_cdf)), "prefix_sum_dev")

    def offspring_offsets_dev(self, d_cdf, n, d_base, d_total, seed, frame, n_total, d_first):
        self._ck(self.lib.slam_offspring_offsets_dev(self.h, _ptr(d_cdf), n, _ptr(d_base), _ptr(d_total), seed, frame,
                                                     n_total, _ptr(d_first)), "offspring_offsets_dev")

    def ancestors_dev(self, d_first_all, n_total, slot0, nslots, d_anc):
        self._ck(self.lib.slam_ancestors_dev(self.h, _ptr(d_first_all), n_total, slot0, nslots, _ptr(d_anc)),
                 "ancestors_dev")

    def ancestors_from_scan_dev(self, n, seed, frame, d_anc):
        self._ck(self.lib.slam_ancestors_from_scan_dev(self.h, n, seed, frame, _ptr(d_anc)), "ancestors_from_scan_dev")

    def pose_spread_dev(self, d_x, d_y, d_theta, n, ref_theta, d_idx=None, d_carry=None):
        """``slam_pose_spread_dev``: -> (pose, cov, heading_r) of n poses in device memory, as ``PfSession.spread`` defines them.
        d_idx: a pending gather (int32, optional); d_carry: log-weight minus the largest, one float per slot (optional)."""
        pose, cov, r = (C.c_float * 3)(), (C.c_float * 6)(), C.c_float(0)
        self._ck(self.lib.slam_pose_spread_dev(self.h, _ptr(d_x), _ptr(d_y), _ptr(d_theta), _ptr(d_idx), _ptr(d_carry), n,
                                               float(ref_theta), pose, cov, C.byref(r)), "pose_spread_dev")
        return np.array(list(pose), np.float32), np.array(list(cov), np.float32), np.float32(r.value)

    def pose_modes_dev(self, d_x, d_y, d_theta, n, ref_theta, cell, hbins, max_modes, d_idx=None, d_carry=None):
        """``slam_pose_modes_dev``: -> (modes, cells, wtotal) of n poses in device memory, as ``PfSession.modes`` defines them.
        d_idx: a pending gather (int32, optional); d_carry: log-weight minus the largest, one float per slot (optional)."""
        modes, nm, cells, wt = (PfMode * MAX_MODES)(), _i(0), _i(0), _i64(0)
        self._ck(self.lib.slam_pose_modes_dev(self.h, _ptr(d_x), _ptr(d_y), _ptr(d_theta), _ptr(d_idx), _ptr(d_carry), n, float(ref_theta),
                                              float(cell), int(hbins), int(max_modes), modes, C.byref(nm), C.byref(cells), C.byref(wt)),
                 "pose_modes_dev")
        return _mode_list(modes, nm.value), cells.value, wt.value

    def argmax_dev(self, d_values, n, d_index, d_value):
        """``slam_argmax_dev``: index (int32) and value (float32) of the largest of d_values[0..n) to device memory: the lowest
        index on ties, NaN never wins, index 0 with nothing but -inf and NaN."""
        self._ck(self.lib.slam_argmax_dev(self.h, _ptr(d_values), n, _ptr(d_index), _ptr(d_value)), "argmax_dev")

    def ancestors_sharded_dev(self, d_first_all, n_total, n_local, rank, world, d_src, d_plan, d_pose_idx=None):
        """d_plan: int32[plan_words(world)] on the device: [0] anything moves, send_cnt[world], recv_cnt[world], ...
        d_pose_idx (optional): ancestor's position in an all-gather of the ranks' [x | y | theta] pose blocks."""
        self._ck(self.lib.slam_ancestors_sharded_dev(self.h, _ptr(d_first_all), n_total, n_local, rank, world,
                                                     _ptr(d_src), _ptr(d_plan), _ptr(d_pose_idx)), "ancestors_sharded_dev")

    def ekf_form_set(self, form: int):
        """-1: the engine chooses the out-of-place EKF kernel; 0: one wavefront per particle; 1 / 2: per 4 / 2 particles."""
        self._ck(self.lib.slam_ekf_form_set(self.h, int(form)), "ekf_form_set")

    def ekf_form_counts(self):
        c = (C.c_int64 * 2)()
        self._ck(self.lib.slam_ekf_form_counts(self.h, c), "ekf_form_counts")
        return int(c[0]), int(c[1])

    def selftest_reciprocal(self):
        """(mismatches, values checked) of the landmark update's fast reciprocal against IEEE division, every float in range."""
        bad, seen = C.c_int64(-1), C.c_int64(0)
        self._ck(self.lib.slam_selftest_reciprocal(self.h, C.byref(bad), C.byref(seen)), "selftest_reciprocal")
        return int(bad.value), int(seen.value)

    def frame_fusion_set(self, on: bool):
        """The front of a single-GPU frame on rows (motion + score and the landmark update) as one launch (default) or two."""
        self._ck(self.lib.slam_frame_fusion_set(self.h, 1 if on else 0), "frame_fusion_set")

    def survivor_rows_set(self, on: bool):
        """Survivor rows (``slam_survivor_rows_set``; default on): a dense split frame writes mean rows only for the particles its
        resample keeps.  Off: every frame writes every row.  Results are the same bits either way."""
        self._ck(self.lib.slam_survivor_rows_set(self.h, 1 if on else 0), "survivor_rows_set")

    def frame_front_last(self):
        """(particles per updating wavefront, lanes per pose) of the last fused front launch; (0, 0) before the first."""
        info = (C.c_int32 * 2)()
        self._ck(self.lib.slam_frame_front_last(self.h, info), "frame_front_last")
        return int(info[0]), int(info[1])

    def frame_fusion_count(self) -> int:
        c = C.c_int64(0)
        self._ck(self.lib.slam_frame_fusion_count(self.h, C.byref(c)), "frame_fusion_count")
        return int(c.value)

    def pf_paged_set(self, on: bool):
        """Sessions made from now on keep their maps as copy-on-write pages (one GPU; same results as rows)."""
        self._ck(self.lib.slam_pf_paged_set(self.h, int(bool(on))), "pf_paged_set")

    def ekf_inplace_form_set(self, form: int):
        """-1: the engine chooses the in-place EKF kernel; 0: whole rows; 1: the observed landmarks only (compact list)."""
        self._ck(self.lib.slam_ekf_inplace_form_set(self.h, int(form)), "ekf_inplace_form_set")

    def ekf_inplace_form_counts(self):
        c = (C.c_int64 * 2)()
        self._ck(self.lib.slam_ekf_inplace_form_counts(self.h, c), "ekf_inplace_form_counts")
        return int(c[0]), int(c[1])

    def resample_gate_set(self, ess_frac: float):
        self._ck(self.lib.slam_resample_gate_set(self.h, float(ess_frac)), "resample_gate_set")

    def resample_happened(self) -> bool:
        r = C.c_int(1)
        self._ck(self.lib.slam_resample_happened_host(self.h, C.byref(r)), "resample_happened")
        return bool(r.value)

    def resample_heads(self):
        """(about how many distinct ancestors the last resample stage of a population with maps left, that population's size or -1)"""
        h, n = C.c_int32(0), C.c_int32(-1)
        self._ck(self.lib.slam_resample_heads_host(self.h, C.byref(h), C.byref(n)), "resample_heads")
        return h.value, n.value

    def exchange_set_capacity(self, rows: int):
        self._ck(self.lib.slam_exchange_set_capacity(self.h, int(rows)), "exchange_set_capacity")

    def exchange_plan_host(self, world):
        """The plan of the last ancestors_sharded_dev call, delivered through mapped host memory (no copy, no sync)."""
        plan = np.zeros(plan_words(world), np.int32)
        self._ck(self.lib.slam_exchange_plan_host(self.h, world, _ptr(plan)), "exchange_plan_host")
        return plan.tolist()

    def migrate_pack_dev(self, n_local, rank, world, plan, d_pose, pose_ld, d_map, row_stride, plane_stride, nlandmarks,
                         d_out):
        plan = _np(plan, np.int32)
        self._ck(self.lib.slam_migrate_pack_dev(self.h, n_local, rank, world, _ptr(plan), _ptr(d_pose), pose_ld,
                                                _ptr(d_map), row_stride, plane_stride, nlandmarks, _ptr(d_out)),
                 "migrate_pack_dev")

    def migrate_unpack_dev(self, d_in, world, recv_cnt, n_local, d_pose, pose_ld, d_map, row_stride, plane_stride,
                           nlandmarks):
        cnt = _np(recv_cnt, np.int32)
        self._ck(self.lib.slam_migrate_unpack_dev(self.h, _ptr(d_in), world, _ptr(cnt), n_local, _ptr(d_pose), pose_ld,
                                                  _ptr(d_map), row_stride, plane_stride, nlandmarks), "migrate_unpack_dev")

    def gather_f32_dev(self, d_src, d_idx, n, d_dst):
        self._ck(self.lib.slam_gather_f32_dev(self.h, _ptr(d_src), _ptr(d_idx), n, _ptr(d_dst)), "gather_f32_dev")

    def gather_map_dev(self, d_in, d_out, in_row_stride, out_row_stride, in_plane_stride, out_plane_stride, nlandmarks,
                       d_idx, n):
        self._ck(self.lib.slam_gather_map_dev(self.h, _ptr(d_in), _ptr(d_out), in_row_stride, out_row_stride,
                                              in_plane_stride, out_plane_stride, nlandmarks, _ptr(d_idx), n),
                 "gather_map_dev")


class LocaliseView(C.Structure):
    """``slam_localise_view``: what a pose sees of a known map — view_range, the arc [lo, hi] of the diamond angle (0, 4: the whole
    circle), sight != 0: the engine's current sight table with `margin`."""

    _fields_ = [("view_range", C.c_float), ("lo", C.c_float), ("hi", C.c_float), ("sight", C.c_int32), ("margin", C.c_float)]


class DetectParams(C.Structure):
    """``slam_detect_params``: the detector's rule (include/slam_hip.h: slam_detect_scan_dev)."""

    _fields_ = [("jump", C.c_float), ("guard", C.c_float), ("max_width", C.c_float), ("max_range", C.c_float),
                ("min_points", C.c_int32), ("max_points", C.c_int32), ("wrap", C.c_int32)]

    @classmethod
    def default(cls, **kw):
        p = cls()
        load_library().slam_detect_params_default(C.byref(p))
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise TypeError(f"slam_detect_params has no field {k!r}")
            setattr(p, k, v)
        return p


class DetectNoise(C.Structure):
    """``slam_detect_noise``: the detector's noise model — variance along the line of sight, of the bearing [rad^2], and a
    range-independent one across the line of sight (slam_detect_scan_noise_dev)."""

    _fields_ = [("range_var", C.c_float), ("bearing_var", C.c_float), ("lateral_var", C.c_float)]

    @classmethod
    def of(cls, noise):
        """None, a DetectNoise or (range_var, bearing_var[, lateral_var]) -> None or a DetectNoise."""
        if noise is None or isinstance(noise, cls):
            return noise
        return cls(*noise)


class DetectFit(C.Structure):
    """``slam_detect_fit``: the poles' nominal radius and what the shape test allows beyond it (slam_detect_scan_fit_dev)."""

    _fields_ = [("radius", C.c_float), ("spread_tol", C.c_float)]

    @classmethod
    def default(cls, **kw):
        f = cls()
        load_library().slam_detect_fit_default(C.byref(f))
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise TypeError(f"slam_detect_fit has no field {k!r}")
            setattr(f, k, v)
        return f

    @classmethod
    def of(cls, fit):
        """None, a DetectFit or (radius, spread_tol) -> None or a DetectFit."""
        if fit is None or isinstance(fit, cls):
            return fit
        radius, tol = fit
        return cls(radius, tol)


class MapperParams(C.Structure):
    """``slam_mapper_params``: the reference's run-time parameters (main.c:832-839, :50, :846, :224, :943)."""

    _fields_ = [("fast_res", C.c_float * 3), ("fast_res2", C.c_float * 3), ("border", C.c_float), ("pixel", C.c_float),
                ("pixel2", C.c_float), ("key_dt", C.c_float), ("key_dr", C.c_float), ("range_min", C.c_float),
                ("usable_range", C.c_float), ("edt_cap", C.c_float), ("new_point_threshold", C.c_float)]

    @classmethod
    def default(cls):
        p = cls()
        load_library().slam_mapper_params_default(C.byref(p))
        return p

    def as_list(self):
        return list(self.fast_res) + list(self.fast_res2) + [self.border, self.pixel, self.pixel2, self.key_dt, self.key_dr,
                                                             self.range_min, self.usable_range, self.edt_cap, self.new_point_threshold]


class MapperView(C.Structure):
    """``slam_mapper_view``"""

    _fields_ = [("bx", C.c_void_p), ("by", C.c_void_p), ("tx", C.c_void_p), ("ty", C.c_void_p), ("mx", C.c_void_p),
                ("my", C.c_void_p), ("lx", C.c_void_p), ("ly", C.c_void_p), ("counts", C.c_void_p), ("occ", C.c_void_p * 2),
                ("edt", C.c_void_p * 2), ("ld", C.c_int32 * 2), ("meta", C.c_void_p), ("hits", C.c_void_p),
                ("nhits", C.c_int32), ("pose", C.c_float * 3), ("prev", C.c_float * 3), ("map_pose", C.c_float * 3),
                ("mini_updated", C.c_int32), ("frame", C.c_int32), ("map_cap", C.c_int32), ("nbeams", C.c_int32)]


LOCAL_MAP_CAP = 25000   # the reference's local-map capacity (main.c:148)


class Mapper:
    """``slam_mapper`` — the reference's frame loop with the map, the scan and the grids resident on the device."""

    def __init__(self, engine: "Engine", nbeams: int, angle_min: float, angle_inc: float, params: MapperParams | None = None):
        self.e, self.nbeams = engine, int(nbeams)
        h = C.c_void_p()
        if params is None:
            rc = engine.lib.slam_mapper_create(engine.h, nbeams, angle_min, angle_inc, C.byref(h))
        else:
            rc = engine.lib.slam_mapper_create_ex(engine.h, nbeams, angle_min, angle_inc, C.byref(params), C.byref(h))
        engine._ck(rc, "mapper_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.e.lib.slam_mapper_destroy(self.h)
            self.h = None

    def _ranges(self, ranges):
        r = _np(ranges, np.float32)
        assert r.shape == (self.nbeams,)
        return r

    def first_frame(self, ranges):
        self.e._ck(self.e.lib.slam_mapper_first_frame(self.h, _ptr(self._ranges(ranges))), "mapper_first_frame")

    def next_frame(self, ranges):
        """-> the matched pose [3]; raises SlamError (``.status``) when the frame fails."""
        pose = (C.c_float * 3)()
        self.e._ck(self.e.lib.slam_mapper_next_frame(self.h, _ptr(self._ranges(ranges)), pose), "mapper_next_frame")
        return np.array(list(pose), np.float32)

    def map(self, capacity: int | None = None, want_points: bool = True):
        """``slam_mapper_get_map_host``: -> (size, x, y).  x / y hold min(size, capacity) points; capacity None = all of
        them (two calls), want_points False = the size alone (x, y are None)."""
        n = C.c_int32(-1)
        if not want_points:
            self.e._ck(self.e.lib.slam_mapper_get_map_host(self.h, None, None, 0, C.byref(n)), "mapper_get_map")
            return n.value, None, None
        if capacity is None:
            capacity = self.map(want_points=False)[0]
        x, y = np.zeros(max(capacity, 1), np.float32), np.zeros(max(capacity, 1), np.float32)
        self.e._ck(self.e.lib.slam_mapper_get_map_host(self.h, _ptr(x), _ptr(y), capacity, C.byref(n)), "mapper_get_map")
        return n.value, x[:capacity], y[:capacity]

    def view(self):
        """dict of DeviceArray views of the mapper's own buffers and a copy of its host state (``slam_mapper_device_view``).
        Valid until the next call on the mapper; synchronise (``Engine.sync``) first."""
        v = MapperView()
        self.e._ck(self.e.lib.slam_mapper_device_view(self.h, C.byref(v)), "mapper_device_view")
        nb, cap = v.nbeams, v.map_cap
        d = {k: DeviceArray(getattr(v, k), (n,), "<f4", self)
             for k, n in (("bx", nb), ("by", nb), ("tx", nb), ("ty", nb), ("hits", nb), ("mx", cap), ("my", cap),
                          ("lx", LOCAL_MAP_CAP), ("ly", LOCAL_MAP_CAP))}
        d["counts"] = DeviceArray(v.counts, (3,), "<i4", self)
        d["occ"] = [DeviceArray(v.occ[k], (v.ld[k], v.ld[k]), "<i4", self) for k in (0, 1)]
        d["edt"] = [DeviceArray(v.edt[k], (v.ld[k], v.ld[k]), "<f4", self) for k in (0, 1)]
        d["meta"] = DeviceArray(v.meta, (2, 6), "<i4", self)   # two slam_grid_meta records as raw words
        d.update(ld=[v.ld[0], v.ld[1]], nhits=v.nhits, pose=np.array(list(v.pose), np.float32),
                 prev=np.array(list(v.prev), np.float32), map_pose=np.array(list(v.map_pose), np.float32),
                 mini_updated=v.mini_updated, frame=v.frame, map_cap=cap, nbeams=nb)
        return d


class PfConfig(C.Structure):
    """``slam_pf_config``"""

    _fields_ = [("n_particles", C.c_int32), ("n_landmarks", C.c_int32), ("sigma", C.c_float * 3),
                ("meas_var", C.c_float), ("score_gain", C.c_float), ("seed", C.c_uint64), ("resample_ess_frac", C.c_float),
                ("map_layout", C.c_int32)]


MAP_AUTO, MAP_ROWS, MAP_PAGES, MAP_SPLIT, MAP_SPLIT_PAGES = 0, 1, 2, 3, 4   # slam_map_layout
_LAYOUTS = {"auto": MAP_AUTO, "rows": MAP_ROWS, "pages": MAP_PAGES, "split": MAP_SPLIT, "split_pages": MAP_SPLIT_PAGES, None: MAP_AUTO}
_LAYOUT_NAMES = {MAP_ROWS: "rows", MAP_PAGES: "pages", MAP_SPLIT: "split", MAP_SPLIT_PAGES: "split_pages"}


COMM_ID_BYTES = 128


class PfView(C.Structure):
    """``slam_pf_view``"""

    _fields_ = [("pose", C.c_void_p), ("map", C.c_void_p), ("map_spare", C.c_void_p), ("anc", C.c_void_p), ("row_stride", C.c_int64),
                ("plane_stride", C.c_int32), ("map_rows", C.c_int32), ("score", C.c_void_p), ("logw", C.c_void_p),
                ("loglik", C.c_void_p), ("count", C.c_void_p)]


class PfSplitView(C.Structure):
    """``slam_pf_split_view``"""

    _fields_ = [("mean", C.c_void_p), ("cov", C.c_void_p), ("cls", C.c_void_p), ("live", C.c_void_p), ("live_count", C.c_void_p),
                ("plane_stride", C.c_int32), ("rows", C.c_int32)]


class PfPagedView(C.Structure):
    """``slam_pf_paged_view``"""

    _fields_ = [("pool", C.c_void_p), ("table", C.c_void_p), ("freelist", C.c_void_p), ("state", C.c_void_p),
                ("stamp", C.c_void_p), ("stamp_now", C.c_uint32), ("page_landmarks", C.c_int32),
                ("pages_per_particle", C.c_int32), ("table_rows", C.c_int32), ("npages", C.c_int64),
                ("planes", C.c_int32), ("reserved", C.c_int32), ("half_pages", C.c_int64), ("gap_floats", C.c_int64)]


class DeviceArray:
    """A device buffer owned by the engine, exposed through ``__cuda_array_interface__`` so that array libraries
    (``torch.as_tensor(a, device="cuda")``, cupy) can view it without a copy.  Plumbing only."""

    def __init__(self, ptr: int, shape, typestr: str, owner=None):
        self._owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(int(v) for v in shape), "typestr": typestr,
                                         "data": (int(ptr), False), "version": 2, "strides": None}


def comm_unique_id() -> bytes:
    """``slam_comm_unique_id``: the rendezvous token rank 0 makes and hands to the other ranks."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    rc = load_library().slam_comm_unique_id(buf)
    if rc != 0:
        raise SlamError(rc, "comm_unique_id")
    return bytes(buf)


class LocalGroup:
    """``slam_local_group``: the rendezvous of an in-process group of ranks (one host thread per rank)."""

    def __init__(self, world: int):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.slam_local_group_create(world, C.byref(h))
        if rc != 0:
            raise SlamError(rc, "local_group_create")
        self.h, self.world = h, world

    def close(self):
        if getattr(self, "h", None):
            self.lib.slam_local_group_destroy(self.h)
            self.h = None


class Comm:
    """``slam_comm``: how one rank of a sharded filter reaches the others.  ``Comm.rccl`` (one rank per GPU, RCCL over
    xGMI) or ``Comm.local`` (threads of one process).  Creation over RCCL is collective."""

    def __init__(self, engine: Engine, handle, keep=None):
        self.e, self.h, self._keep = engine, handle, keep

    @classmethod
    def rccl(cls, engine: Engine, rank: int, world: int, unique_id: bytes):
        assert len(unique_id) == COMM_ID_BYTES
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        h = C.c_void_p()
        engine._ck(engine.lib.slam_comm_create_rccl(engine.h, rank, world, buf, C.byref(h)), "comm_create_rccl")
        return cls(engine, h)

    @classmethod
    def local(cls, engine: Engine, group: LocalGroup, rank: int):
        h = C.c_void_p()
        engine._ck(engine.lib.slam_comm_create_local(engine.h, group.h, rank, C.byref(h)), "comm_create_local")
        return cls(engine, h, keep=group)

    @property
    def rank(self):
        return self.e.lib.slam_comm_rank(self.h)

    @property
    def world(self):
        return self.e.lib.slam_comm_world(self.h)

    def abort(self):
        """``slam_comm_abort``: give up, so that the other ranks fail with SLAM_ERR_COMM instead of waiting."""
        self.e._ck(self.e.lib.slam_comm_abort(self.h), "comm_abort")

    def close(self):
        if getattr(self, "h", None):
            self.e.lib.slam_comm_destroy(self.h)
            self.h = None


class PfSession:
    """``slam_pf`` — the C-level particle-filter session (what a plain C host uses).  With ``comm`` it is one rank
    of a population sharded over several GPUs (``n_particles`` = this rank's share); every call is then collective."""

    def __init__(self, engine: Engine, n_particles, n_landmarks=0, sigma=(0.01, 0.01, 0.002), meas_var=0.01,
                 score_gain=1.0, seed=1, comm: Comm | None = None, recv_capacity: int = 0, resample_ess_frac: float = 0.0,
                 map_layout: str | int | None = None):
        """map_layout: "auto" (default: the session chooses), "rows" or "pages" (``slam_map_layout``)."""
        self.e, self.n, self.L, self.comm = engine, n_particles, n_landmarks, comm
        cfg = PfConfig(n_particles, n_landmarks, (C.c_float * 3)(*sigma), meas_var, score_gain, seed, resample_ess_frac,
                       _LAYOUTS.get(map_layout, map_layout))
        h = C.c_void_p()
        if comm is None:
            engine._ck(engine.lib.slam_pf_create(engine.h, C.byref(cfg), C.byref(h)), "pf_create")
        else:
            engine._ck(engine.lib.slam_pf_create_sharded(engine.h, C.byref(cfg), comm.h, recv_capacity, C.byref(h)),
                       "pf_create_sharded")
        self.h = h

    def rows_received(self) -> int:
        return self.e.lib.slam_pf_rows_received(self.h)

    def frames_resampled(self) -> int:
        return int(self.e.lib.slam_pf_frames_resampled(self.h))

    def layout_changes(self) -> int:
        return int(self.e.lib.slam_pf_layout_changes(self.h))

    def device_view(self):
        """dict of DeviceArray views of the session's CURRENT buffers (``slam_pf_device_view``): pose [3][n], map and
        map_spare [map_rows][5][plane_stride] (None without landmarks), anc [n] (None when no gather is pending).
        They move with every step."""
        v = PfView()
        self.e._ck(self.e.lib.slam_pf_device_view(self.h, C.byref(v)), "pf_device_view")
        shape = (v.map_rows, 5, v.plane_stride)
        return {"pose": DeviceArray(v.pose, (3, self.n), "<f4", self),
                "map": DeviceArray(v.map, shape, "<f4", self) if v.map else None,
                "map_spare": DeviceArray(v.map_spare, shape, "<f4", self) if v.map_spare else None,
                "anc": DeviceArray(v.anc, (self.n,), "<i4", self) if v.anc else None,
                "score": DeviceArray(v.score, (self.n,), "<f4", self) if v.score else None,
                "logw": DeviceArray(v.logw, (self.n,), "<f4", self) if v.logw else None,
                "loglik": DeviceArray(v.loglik, (self.n,), "<f4", self) if v.loglik else None,
                "count": DeviceArray(v.count, (self.n,), "<i4", self) if v.count else None,
                "plane_stride": v.plane_stride, "row_stride": v.row_stride}

    def layout(self) -> str:
        """"rows", "pages" or "split": how the landmark maps are kept right now (``slam_pf_layout``)."""
        return _LAYOUT_NAMES[self.e.lib.slam_pf_layout(self.h)]

    def split_view(self):
        """``slam_pf_split_device_view``: means, classes, class covariance rows and the list of classes in use."""
        v = PfSplitView()
        self.e._ck(self.e.lib.slam_pf_split_device_view(self.h, C.byref(v)), "pf_split_device_view")
        return {"mean": DeviceArray(v.mean, (v.rows, 2, v.plane_stride), "<f4", self) if v.mean else None,   # None: split pages
                "cov": DeviceArray(v.cov, (v.rows, 3, v.plane_stride), "<f4", self),
                "covx": DeviceArray(self._split_covx(), (v.rows, 2, v.plane_stride), "<f4", self),
                "cls": DeviceArray(v.cls, (v.rows,), "<i4", self), "live": DeviceArray(v.live, (v.rows,), "<i4", self),
                "live_count": DeviceArray(v.live_count, (1,), "<i4", self), "plane_stride": v.plane_stride}

    def _split_covx(self):
        p = C.c_void_p()
        self.e._ck(self.e.lib.slam_pf_split_covx_view(self.h, C.byref(p)), "pf_split_covx_view")
        return p.value

    def paged_view(self):
        """``slam_pf_paged_device_view``: the page pool, tables, stamps and free list of a session that is on pages."""
        v = PfPagedView()
        self.e._ck(self.e.lib.slam_pf_paged_device_view(self.h, C.byref(v)), "pf_paged_device_view")
        P, nb = int(v.npages), v.pages_per_particle
        if v.planes == 2:   # split pages: two buffers of half_pages pages of [2][page_landmarks] floats, gap_floats apart
            H, pf_ = int(v.half_pages), 2 * v.page_landmarks
            pool = [DeviceArray(v.pool + 4 * k * (H * pf_ + int(v.gap_floats)), (H, 2, v.page_landmarks), "<f4", self) for k in (0, 1)]
        else:
            pool = DeviceArray(v.pool, (P, 5, v.page_landmarks), "<f4", self)
        return {"pool": pool, "planes": v.planes, "half_pages": int(v.half_pages),
                "table": DeviceArray(v.table, (v.table_rows, nb), "<i4", self),
                "freelist": DeviceArray(v.freelist, (P,), "<i4", self), "state": DeviceArray(v.state, (4,), "<i4", self),
                "stamp": DeviceArray(v.stamp, (P,), "<i4", self), "stamp_now": int(v.stamp_now),
                "page_landmarks": v.page_landmarks, "pages_per_particle": nb, "table_rows": v.table_rows, "npages": P}

    def close(self):
        if getattr(self, "h", None):
            self.e.lib.slam_pf_destroy(self.h)
            self.h = None

    def reset(self, pose):
        self.e._ck(self.e.lib.slam_pf_reset(self.h, _f3(pose)), "pf_reset")

    def set_poses(self, x, y, th):
        x, y, th = (_np(a, np.float32) for a in (x, y, th))
        self.e._ck(self.e.lib.slam_pf_set_poses_host(self.h, _ptr(x), _ptr(y), _ptr(th)), "pf_set_poses")

    def set_map(self, rows):
        """rows: float32 [n_particles][5][n_landmarks] (mu_x, mu_y, P_xx, P_xy, P_yy)"""
        rows = _np(rows, np.float32)
        assert rows.shape == (self.n, 5, self.L)
        self.e._ck(self.e.lib.slam_pf_set_map_host(self.h, _ptr(rows)), "pf_set_map")

    def set_map_dev(self, d_rows, row_stride: int, plane_stride: int):
        """Maps from device memory: rows [n_particles][5][plane_stride] floats, row_stride floats apart (asynchronous)."""
        self.e._ck(self.e.lib.slam_pf_set_map_dev(self.h, _ptr(d_rows), int(row_stride), int(plane_stride)), "pf_set_map_dev")

    def is_paged(self) -> bool:
        return bool(self.e.lib.slam_pf_is_paged(self.h))

    def step(self, slot, dp, use_observations=False):
        self.e._ck(self.e.lib.slam_pf_step(self.h, slot, _f3(dp), 1 if use_observations else 0), "pf_step")

    def refine_set(self, step_xy: float, step_theta: float, sweeps: int):
        """sweeps in 1..16: every frame refines its motion samples on the 27-pose lattice; 0 switches it off."""
        self.e._ck(self.e.lib.slam_pf_refine_set(self.h, step_xy, step_theta, sweeps), "pf_refine_set")

    def meas_cov_set(self, meas_cov):
        """``slam_pf_meas_cov_set``: (qxx, qxy, qyy) of the sensor-frame measurement covariance; rows sessions only;
        (meas_var, 0, meas_var) switches back to the isotropic update."""
        self.e._ck(self.e.lib.slam_pf_meas_cov_set(self.h, _f3(meas_cov)), "pf_meas_cov_set")

    def assoc_set(self, gate: float, new_gate: float = 0.0, create: bool = True):
        """``slam_pf_assoc_set``: gate > 0: frames associate the engine's detections themselves (single-GPU rows sessions only);
        gate = 0 switches it off."""
        self.e._ck(self.e.lib.slam_pf_assoc_set(self.h, gate, new_gate, 1 if create else 0), "pf_assoc_set")

    def assoc_detcov_set(self, gate: float, new_gate: float = 0.0, create: bool = True):
        """``slam_pf_assoc_detcov_set``: association under the covariance each detection carries (Engine.detections_cov_upload
        behind every hand-over of detections)."""
        self.e._ck(self.e.lib.slam_pf_assoc_detcov_set(self.h, gate, new_gate, 1 if create else 0), "pf_assoc_detcov_set")

    def assoc_cov_set(self, meas_cov, gate: float, new_gate: float = 0.0, create: bool = True):
        """``slam_pf_assoc_cov_set``: association under the 2x2 sensor-frame covariance (qxx, qxy, qyy) — covariance and gates in one
        switch; (meas_var, 0, meas_var) is exactly assoc_set(gate, new_gate, create)."""
        self.e._ck(self.e.lib.slam_pf_assoc_cov_set(self.h, _f3(meas_cov), gate, new_gate, 1 if create else 0), "pf_assoc_cov_set")

    def known_map_set(self, rows, gate: float = 0.0, log_clutter: float = 0.0):
        """``slam_pf_known_map_set``: rows float32 [5][L] (mx, my, P_xx, P_xy, P_yy; P_xx < 0: no landmark): observing frames
        localise in this ONE map (sessions with n_landmarks == 0 on one GPU); rows None switches it off."""
        if rows is None:
            self.e._ck(self.e.lib.slam_pf_known_map_set(self.h, None, 0, 0.0, 0.0), "pf_known_map_set")
            return
        rows = _np(rows, np.float32)
        assert rows.ndim == 2 and rows.shape[0] == 5
        self.e._ck(self.e.lib.slam_pf_known_map_set(self.h, _ptr(rows), rows.shape[1], gate, log_clutter), "pf_known_map_set")

    def known_map_detcov_set(self, rows, gate: float = 0.0, log_clutter: float = 0.0):
        """``slam_pf_known_map_detcov_set``: ``known_map_set`` for the form of the stage that weighs every detection under its own
        covariance (uploaded with the detections, or the detector's noise model); rows None switches it off."""
        if rows is None:
            self.e._ck(self.e.lib.slam_pf_known_map_detcov_set(self.h, None, 0, 0.0, 0.0), "pf_known_map_detcov_set")
            return
        rows = _np(rows, np.float32)
        assert rows.ndim == 2 and rows.shape[0] == 5
        self.e._ck(self.e.lib.slam_pf_known_map_detcov_set(self.h, _ptr(rows), rows.shape[1], gate, log_clutter), "pf_known_map_detcov_set")

    def known_map_view(self):
        """``slam_pf_known_map_device_view``: the prepared map float32 [6][L rounded up to 32] (None while the mode is off and under
        ``known_map_detcov_set``), L, and
        the last stage's stats int32 [n][3] = matched, 0, dropped."""
        p, st, L = C.c_void_p(), C.c_void_p(), C.c_int32(0)
        self.e._ck(self.e.lib.slam_pf_known_map_device_view(self.h, C.byref(p), C.byref(L), C.byref(st)), "pf_known_map_device_view")
        Lp = (L.value + 31) // 32 * 32
        return {"prepared": DeviceArray(p.value, (6, Lp), "<f4", self) if p.value else None, "nlandmarks": L.value,
                "stats": DeviceArray(st.value, (self.n, 3), "<i4", self)}

    def known_map_miss_set(self, log_miss: float, view_range: float, fov=None, sight=None):
        """``slam_pf_known_map_miss_set`` (only while a known map is set): observing frames also count the landmarks in view that no
        detection matched and charge log_miss for each.  fov: None (the whole circle) or (angle_min, angle_max, edge); sight: None
        or (bins, margin); view_range = 0 switches it off."""
        on, (a0, a1, edge) = (1, fov) if fov is not None else (0, (0.0, 0.0, 0.0))
        bins, margin = sight if sight is not None else (0, 0.0)
        self.e._ck(self.e.lib.slam_pf_known_map_miss_set(self.h, log_miss, view_range, on, a0, a1, edge, int(bins), margin), "pf_known_map_miss_set")

    def known_map_miss_view(self):
        """``slam_pf_known_map_miss_device_view``: the last miss stage's missed, spared and outside counts, int32 [n] each."""
        m, s, o = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.e._ck(self.e.lib.slam_pf_known_map_miss_device_view(self.h, C.byref(m), C.byref(s), C.byref(o)), "pf_known_map_miss_device_view")
        return {k: DeviceArray(v.value, (self.n,), "<i4", self) for k, v in (("missed", m), ("spared", s), ("outside", o))}

    def known_map_reseed(self, fraction: float):
        """``slam_pf_known_map_reseed`` (between frames, while a known map is set): the pending resample and pose proposals from
        the engine's current detections for `fraction` of the slots, in one launch.  -> (replaced, chosen but not replaced).
        ``best`` is refused until the next ``step``; two calls with no step between them draw the same slots."""
        c = (C.c_int32 * 2)()
        self.e._ck(self.e.lib.slam_pf_known_map_reseed(self.h, float(fraction), c), "pf_known_map_reseed")
        return int(c[0]), int(c[1])

    def known_map_reseed_pairs(self, fraction: float, tol: float, min_sep: float):
        """``slam_pf_known_map_reseed_pairs`` (between frames, while a known map is set): as ``known_map_reseed``, with proposals
        from pairs of detections whose heading the lidar fixes.  -> (replaced, first landmark slot empty, detections too close,
        no partner in the map).  ``best`` is refused until the next ``step``."""
        c = (C.c_int32 * 4)()
        self.e._ck(self.e.lib.slam_pf_known_map_reseed_pairs(self.h, float(fraction), float(tol), float(min_sep), c), "pf_known_map_reseed_pairs")
        return tuple(int(v) for v in c)

    def assoc_view(self):
        """``slam_pf_assoc_device_view``: the last frame's table uint8 [n][stride] and stats int32 [n][3], indexed like score."""
        a, st, stride = C.c_void_p(), C.c_void_p(), C.c_int32(0)
        self.e._ck(self.e.lib.slam_pf_assoc_device_view(self.h, C.byref(a), C.byref(stride), C.byref(st)), "pf_assoc_device_view")
        return {"assoc": DeviceArray(a.value, (self.n, stride.value), "|u1", self), "stats": DeviceArray(st.value, (self.n, 3), "<i4", self),
                "assoc_stride": stride.value}

    def prune_set(self, hit: int, miss: int = 1, cmax: int = 1, view_range: float = 1.0):
        """``slam_pf_prune_set``: existence evidence and pruning of clutter landmarks behind every associating update (only while
        association is on); hit = 0 switches it off."""
        self.e._ck(self.e.lib.slam_pf_prune_set(self.h, int(hit), int(miss), int(cmax), view_range), "pf_prune_set")

    def prune_sight_set(self, bins: int, margin: float = 0.3):
        """``slam_pf_prune_sight_set``: the pruning's evidence stage with line of sight (only while association is on; in force
        while pruning is); bins = 0 switches it off."""
        self.e._ck(self.e.lib.slam_pf_prune_sight_set(self.h, int(bins), margin), "pf_prune_sight_set")

    def sight_view(self):
        """``slam_pf_sight_device_view``: the engine's sight table float32 [1024] (the first `bins` in use), the bins in force and
        the last stage's spared counts int32 [n]."""
        t, sp, bins = C.c_void_p(), C.c_void_p(), C.c_int32(0)
        self.e._ck(self.e.lib.slam_pf_sight_device_view(self.h, C.byref(t), C.byref(bins), C.byref(sp)), "pf_sight_device_view")
        return {"table": DeviceArray(t.value, (1024,), "<f4", self), "bins": bins.value, "spared": DeviceArray(sp.value, (self.n,), "<i4", self)}

    def prune_fov_set(self, on: bool, angle_min: float = -2.351831, angle_max: float = 2.351831, edge: float = 0.0):
        """``slam_pf_prune_fov_set``: the pruning's evidence stage with a field of view [angle_min + edge, angle_max - edge] (only
        while association is on; in force while pruning is); on = False switches it off."""
        self.e._ck(self.e.lib.slam_pf_prune_fov_set(self.h, int(bool(on)), angle_min, angle_max, edge), "pf_prune_fov_set")

    def fov_view(self):
        """``slam_pf_fov_device_view``: the bounds (lo, hi) in force as float32 and the last stage's outside counts int32 [n]."""
        b, out = (C.c_float * 2)(), C.c_void_p()
        self.e._ck(self.e.lib.slam_pf_fov_device_view(self.h, b, C.byref(out)), "pf_fov_device_view")
        return {"bounds": (np.float32(b[0]), np.float32(b[1])), "outside": DeviceArray(out.value, (self.n,), "<i4", self)}

    def merge_set(self, merge_gate: float):
        """``slam_pf_merge_set``: every observing frame merges duplicate landmarks behind its update and evidence stage (only
        while association is on); merge_gate = 0 switches it off."""
        self.e._ck(self.e.lib.slam_pf_merge_set(self.h, merge_gate), "pf_merge_set")

    def merge_view(self):
        """``slam_pf_merge_device_view``: the last stage's stats int32 [n][3] = merged, refused, seen after."""
        st = C.c_void_p()
        self.e._ck(self.e.lib.slam_pf_merge_device_view(self.h, C.byref(st)), "pf_merge_device_view")
        return DeviceArray(st.value, (self.n, 3), "<i4", self)

    def assoc_weight_set(self, log_new: float = 0.0, log_clutter: float = 0.0, log_miss: float = 0.0, on: bool = True):
        """``slam_pf_assoc_weight_set``: every observing frame adds created * log_new + dropped * log_clutter + missed * log_miss
        to its log-likelihood in front of the weights (only while association is on; each constant finite and <= 0)."""
        self.e._ck(self.e.lib.slam_pf_assoc_weight_set(self.h, log_new, log_clutter, log_miss, int(bool(on))), "pf_assoc_weight_set")

    def assoc_weight_view(self):
        """``slam_pf_assoc_weight_device_view``: of the last frame that ran the stage -> (missed int32 [n] or None while pruning is
        off, terms float32 [n])."""
        ms, tm = C.c_void_p(), C.c_void_p()
        self.e._ck(self.e.lib.slam_pf_assoc_weight_device_view(self.h, C.byref(ms), C.byref(tm)), "pf_assoc_weight_device_view")
        return (DeviceArray(ms.value, (self.n,), "<i4", self) if ms.value else None), DeviceArray(tm.value, (self.n,), "<f4", self)

    def detect_set(self, params: "DetectParams | None | bool" = True, **kw):
        """``slam_pf_detect_set``: observing frames make their detections from the engine's scan (only while association is on).
        params: a DetectParams; True: the defaults with the keywords applied; None / False: off."""
        if params is None or params is False:
            self.e._ck(self.e.lib.slam_pf_detect_set(self.h, None), "pf_detect_set")
            return
        p = DetectParams.default(**kw) if params is True else params
        self.e._ck(self.e.lib.slam_pf_detect_set(self.h, C.byref(p)), "pf_detect_set")

    def detect_noise_set(self, noise, fit=None, params: "DetectParams | None | bool" = True, **kw):
        """``slam_pf_detect_noise_set``: detect_fit_set with the noise model (range_var, bearing_var, lateral_var): the detector's
        detections carry covariances (None: detect_fit_set)."""
        if params is None or params is False:
            self.e._ck(self.e.lib.slam_pf_detect_noise_set(self.h, None, None, None), "pf_detect_noise_set")
            return
        p = DetectParams.default(**kw) if params is True else params
        f, z = DetectFit.of(fit), DetectNoise.of(noise)
        self.e._ck(self.e.lib.slam_pf_detect_noise_set(self.h, C.byref(p), C.byref(f) if f is not None else None,
                                                       C.byref(z) if z is not None else None), "pf_detect_noise_set")

    def detect_fit_set(self, fit: "DetectFit | tuple | None", params: "DetectParams | None | bool" = True, **kw):
        """``slam_pf_detect_fit_set``: detect_set with the fit (a DetectFit or (radius, spread_tol); None: detect_set)."""
        if params is None or params is False:
            self.e._ck(self.e.lib.slam_pf_detect_fit_set(self.h, None, None), "pf_detect_fit_set")
            return
        p = DetectParams.default(**kw) if params is True else params
        f = DetectFit.of(fit)
        self.e._ck(self.e.lib.slam_pf_detect_fit_set(self.h, C.byref(p), C.byref(f) if f is not None else None), "pf_detect_fit_set")

    def evidence_view(self):
        """``slam_pf_evidence_device_view``: the current evidence uint8 [n][stride] (indexed like the maps: before the pending
        gather) and the last stage's stats int32 [n][2]."""
        a, st, stride = C.c_void_p(), C.c_void_p(), C.c_int32(0)
        self.e._ck(self.e.lib.slam_pf_evidence_device_view(self.h, C.byref(a), C.byref(stride), C.byref(st)), "pf_evidence_device_view")
        return {"ev": DeviceArray(a.value, (self.n, stride.value), "|u1", self), "stats": DeviceArray(st.value, (self.n, 2), "<i4", self),
                "ev_stride": stride.value}

    def evidence(self):
        """``slam_pf_get_evidence_host``: uint8 [n][n_landmarks], the pending gather applied."""
        ev = np.empty((self.n, self.L), np.uint8)
        self.e._ck(self.e.lib.slam_pf_get_evidence_host(self.h, _ptr(ev)), "pf_get_evidence")
        return ev

    def best(self):
        pose = (C.c_float * 3)()
        lw, idx = C.c_float(0), C.c_int32(0)
        self.e._ck(self.e.lib.slam_pf_best(self.h, pose, C.byref(lw), C.byref(idx)), "pf_best")
        return np.array(list(pose), np.float32), np.float32(lw.value), idx.value

    def mean(self, ref_theta: float):
        """``slam_pf_mean``: posterior mean of the current population (heading averaged on the circle around ref_theta):
        the plain mean of equally weighted particles, the weighted mean after a frame the resample gate kept."""
        pose = (C.c_float * 3)()
        self.e._ck(self.e.lib.slam_pf_mean(self.h, float(ref_theta), pose), "pf_mean")
        return np.array(list(pose), np.float32)

    def modes(self, ref_theta: float, cell: float, hbins: int = 16, max_modes: int = 4):
        """``slam_pf_modes``: -> (modes, cells).  modes: the heaviest clusters of the cloud, heaviest first, each a dict with pose
        (float32 [3]), mass (float32, its share of the population's weight), cell (the centre: ix, iy, heading bin), ncells and
        weight; cells: the number of distinct occupied cells.  cell: the cell's size in metres (at least the size of a settled
        cloud); hbins: heading bins, 1 or 4 .. 64; max_modes: 1 .. 8.  One GPU only.  No policy: what to do with it is yours."""
        modes, nm, cells = (PfMode * MAX_MODES)(), _i(0), _i(0)
        self.e._ck(self.e.lib.slam_pf_modes(self.h, float(ref_theta), float(cell), int(hbins), int(max_modes), modes, C.byref(nm),
                                            C.byref(cells)), "pf_modes")
        return _mode_list(modes, nm.value), cells.value

    def spread(self, ref_theta: float):
        """``slam_pf_spread``: -> (pose, cov, heading_r).  pose: ``mean(ref_theta)``, bit for bit; cov: float32 [6] = xx, xy, yy,
        xs, ys, ss, the covariance of the population over (x, y, sin(theta - pose[2])) about that mean; heading_r: the length of
        the mean heading vector (1: one heading).  A small spread says the particles agree, not that they are right."""
        pose, cov, r = (C.c_float * 3)(), (C.c_float * 6)(), C.c_float(0)
        self.e._ck(self.e.lib.slam_pf_spread(self.h, float(ref_theta), pose, cov, C.byref(r)), "pf_spread")
        return np.array(list(pose), np.float32), np.array(list(cov), np.float32), np.float32(r.value)

    def poses(self):
        x, y, th = (np.empty(self.n, np.float32) for _ in range(3))
        self.e._ck(self.e.lib.slam_pf_get_poses_host(self.h, _ptr(x), _ptr(y), _ptr(th)), "pf_get_poses")
        return np.stack([x, y, th])

    def maps(self):
        m = np.empty((self.n, 5, self.L), np.float32)
        self.e._ck(self.e.lib.slam_pf_get_map_host(self.h, _ptr(m)), "pf_get_map")
        return m

    def map_rows(self, particles):
        """``slam_pf_get_map_rows_host``: the maps of the chosen current particles, [len][5][n_landmarks]."""
        sel = _np(particles, np.int32)
        m = np.empty((len(sel), 5, self.L), np.float32)
        self.e._ck(self.e.lib.slam_pf_get_map_rows_host(self.h, _ptr(sel), len(sel), _ptr(m)), "pf_get_map_rows")
        return m


def plan_words(world: int) -> int:
    """int32 words of the exchange plan slam_ancestors_sharded_dev writes (SLAM_PLAN_WORDS in slam_hip.h)."""
    return 1 + 3 * world


def comb_offset(seed: int, frame: int, total: int) -> int:
    return int(load_library().slam_comb_offset(seed, frame, total))


def fov_bound(angle: float):
    """``slam_fov_bound``: the diamond angle in [0, 4] of the direction `angle` (radians) -> numpy float32; needs no GPU."""
    return np.float32(load_library().slam_fov_bound(float(angle)))


def grid_meta(rows, cols, ld, pixel, min_x, min_y) -> GridMeta:
    return GridMeta(int(rows), int(cols), int(ld), float(np.float32(pixel)), float(np.float32(min_x)),
                    float(np.float32(min_y)))
