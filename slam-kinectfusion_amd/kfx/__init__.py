"""kfx — Python binding of libkfx.so (the MI355X KinectFusion hot path).

`KinectFusion` mirrors the reference's `kf::kinectfusion` (kinectfusion.h:31-73):
pipeline(color, depth) / reset() / getCurCameraPose() / pose_record /
frame_count, plus the stage seams of include/kfx.h used by the parity tests.

There is no CPU fallback: constructing a KinectFusion without the HIP library or
without a GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from .abi import (FERN_DTYPE, KFX_FRAME_CUR, KFX_FRAME_PREV, KFX_OK, KFX_TRACKING_LOST, Fern, FernParams, IcpQuality,
                  IcpResult, Intrinsics, KeyframeMatch, Params, Pose, RecoverParams, RecoverReport, RelocResult,
                  default_params, fptr, i16ptr, i64ptr, u8ptr, u16ptr)

__all__ = ["KinectFusion", "KfxError", "Dataset", "png_info", "png_read_bgr8", "png_read_depth", "parse_intr",
           "comm_unique_id", "pipeline_group", "slab_balance", "write_ply", "write_ply_attr", "write_ply_mesh_attr",
           "write_ply_mesh_indexed", "write_ppm", "shift_for_pose", "quality_figures", "quality_chunk", "icp_multi_chunk", "Keyframes", "fern_table", "keyframes_search_chunk", "IcpQuality", "IcpResult", "VIEW_KINDS", "VERTEX_DTYPE", "BRICK_DTYPE", "BrickStore", "lib", "build", "LIB_PATH", "Intrinsics", "Params", "Pose",
           "default_params", "KFX_FRAME_CUR", "KFX_FRAME_PREV", "KFX_OK", "KFX_TRACKING_LOST", "EXPORTS"]

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("KFX_LIB_PATH") or os.path.join(_PKG, "lib", "libkfx.so")  # override: tuning runs

# every symbol include/kfx.h declares
EXPORTS = [
    "kfx_abi_version", "kfx_last_error", "kfx_default_params", "kfx_create", "kfx_destroy", "kfx_reset",
    "kfx_pipeline", "kfx_pipeline_u16", "kfx_stage_frames", "kfx_pipeline_staged", "kfx_synchronize",
    "kfx_set_graph_mode", "kfx_set_frame_overlap", "kfx_set_kernel_timing", "kfx_get_kernel_timing", "kfx_get_kernel_timing_ex", "kfx_set_icp_persistent", "kfx_debug_force_icp_stall", "kfx_debug_force_index64", "kfx_debug_icp_band_ms", "kfx_get_icp_trace", "kfx_get_cur_camera_pose", "kfx_get_frame_count", "kfx_get_pose_record",
    "kfx_write_poses_txt", "kfx_get_frame_maps", "kfx_set_frame_maps", "kfx_download_tsdf",
    "kfx_upload_tsdf", "kfx_download_volume_soa", "kfx_stage_preprocess", "kfx_stage_icp_accumulate",
    "kfx_stage_icp", "kfx_stage_integrate", "kfx_stage_raycast", "kfx_set_profiling", "kfx_get_stage_ms",
    "kfx_integrate_counts", "kfx_integrate_stats", "kfx_raycast_stats", "kfx_download_columns", "kfx_pipeline_async", "kfx_pipeline_async_u16", "kfx_register_host_buffer", "kfx_unregister_host_buffer", "kfx_slab_mask_payload", "kfx_slab_expand", "kfx_set_icp_allreduce", "kfx_create_slab", "kfx_create_slab_cuts", "kfx_slice_work", "kfx_slice_work_parts", "kfx_slice_work_at", "kfx_get_graph_mode", "kfx_get_graph_note", "kfx_slab_balance", "kfx_slab_info", "kfx_comm_get_unique_id", "kfx_comm_init",
    "kfx_pipeline_group", "kfx_slab_frame_local", "kfx_slab_frame_finish", "kfx_render", "kfx_volume_checksum", "kfx_extract_points", "kfx_write_ply", "kfx_save_pointcloud",
    "kfx_extract_mesh", "kfx_write_ply_mesh", "kfx_get_extract_ms", "kfx_set_extract_passes", "kfx_get_extract_passes", "kfx_set_slab_bound",
    "kfx_extract_points_attr", "kfx_extract_mesh_attr", "kfx_write_ply_attr", "kfx_write_ply_mesh_attr",
    "kfx_save_pointcloud_attr", "kfx_save_mesh_attr",
    "kfx_render_view", "kfx_get_view_ms", "kfx_write_ppm",
    "kfx_shift_volume", "kfx_evict_points", "kfx_get_volume_origin", "kfx_get_volume_pose", "kfx_get_shift_ms",
    "kfx_shift_for_pose",
    "kfx_evict_bricks", "kfx_restore_bricks", "kfx_get_stream_ms", "kfx_brick_store_create", "kfx_brick_store_destroy",
    "kfx_brick_store_put", "kfx_brick_store_count", "kfx_brick_store_take_window",
    "kfx_world_points_attr", "kfx_world_mesh_attr", "kfx_get_world_ms", "kfx_brick_store_copy", "kfx_world_bricks",
    "kfx_save_world_mesh",
    "kfx_extract_mesh_indexed", "kfx_world_mesh_indexed", "kfx_get_indexed_ms", "kfx_write_ply_mesh_indexed",
    "kfx_save_mesh_indexed", "kfx_save_world_mesh_indexed",
    "kfx_world_view_load", "kfx_world_view", "kfx_get_world_view_ms", "kfx_save_world_view",
    "kfx_debug_count_settled", "kfx_debug_get_settled", "kfx_debug_get_hidden", "kfx_debug_int_tiles",
    "kfx_debug_get_icp_sums", "kfx_debug_cap_icp_blocks", "kfx_debug_extract_units", "kfx_debug_scan",
    "kfx_debug_get_icp_step",
    "kfx_stage_icp_residuals", "kfx_score_poses", "kfx_frame_quality", "kfx_score_view", "kfx_get_quality_ms",
    "kfx_quality_figures", "kfx_quality_chunk",
    "kfx_icp_multi", "kfx_track_view", "kfx_resume_at", "kfx_icp_multi_chunk", "kfx_get_icp_multi_ms",
    "kfx_fern_table", "kfx_keyframes_create", "kfx_keyframes_destroy", "kfx_keyframes_get_table", "kfx_keyframes_count",
    "kfx_encode_frame", "kfx_keyframes_add", "kfx_keyframes_put", "kfx_keyframes_consider", "kfx_keyframes_get",
    "kfx_keyframes_search", "kfx_keyframes_search_chunk", "kfx_keyframes_export", "kfx_keyframes_import",
    "kfx_get_keyframe_ms", "kfx_relocalise", "kfx_pipeline_recover",
    "kfx_dataset_open", "kfx_dataset_info", "kfx_dataset_read", "kfx_dataset_close", "kfx_png_info",
    "kfx_png_read_bgr8", "kfx_png_read_depth", "kfx_parse_intr",
]


class KfxError(RuntimeError):
    pass


_lib = None


def build() -> str:
    subprocess.run(["make", "-s", "-j8", "-C", _PKG], check=True)
    return LIB_PATH


def lib():
    """Load libkfx.so (raises if it has not been built — no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KfxError(f"{LIB_PATH} missing: run `make -C {_PKG}` (or __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    P, i, f = C.POINTER, C.c_int, C.c_float
    vp = C.c_void_p
    sig = {
        "kfx_abi_version": ([], i),
        "kfx_last_error": ([], C.c_char_p),
        "kfx_default_params": ([P(Params)], i),
        "kfx_create": ([P(Intrinsics), P(Params), i, P(vp)], i),
        "kfx_destroy": ([vp], i),
        "kfx_reset": ([vp], i),
        "kfx_pipeline": ([vp, P(C.c_uint8), P(f)], i),
        "kfx_pipeline_u16": ([vp, P(C.c_uint8), P(C.c_uint16)], i),
        "kfx_stage_frames": ([vp, i, P(C.c_uint8), P(f)], i),
        "kfx_pipeline_staged": ([vp, i], i),
        "kfx_synchronize": ([vp], i),
        "kfx_set_graph_mode": ([vp, i], i),
        "kfx_set_frame_overlap": ([vp, i], i),
        "kfx_set_kernel_timing": ([vp, i, i], i),
        "kfx_get_kernel_timing": ([vp, P(C.c_float), P(C.c_int)], i),
        "kfx_get_kernel_timing_ex": ([vp, P(C.c_float), P(C.c_int)], i),
        "kfx_set_icp_persistent": ([vp, i], i),
        "kfx_debug_force_icp_stall": ([vp], i),
        "kfx_debug_force_index64": ([vp, i], i),
        "kfx_debug_count_settled": ([vp, i], i),
        "kfx_debug_int_tiles": ([vp, i], i),
        "kfx_debug_get_settled": ([vp, P(C.c_uint64)], i),
        "kfx_debug_get_hidden": ([vp, P(C.c_uint64)], i),
        "kfx_debug_icp_band_ms": ([vp, i, i, i, P(C.c_float)], i),
        "kfx_debug_get_icp_sums": ([vp, P(C.c_int64)], i),
        "kfx_debug_cap_icp_blocks": ([vp, i, P(C.c_int32)], i),
        "kfx_debug_get_icp_step": ([vp, P(C.c_double)], i),
        "kfx_debug_extract_units": ([vp, i], i),
        "kfx_debug_scan": ([vp, P(C.c_uint32), C.c_int64, P(C.c_uint64), P(C.c_uint64)], i),
        "kfx_get_icp_trace": ([vp, P(C.c_uint64), i], i),
        "kfx_get_cur_camera_pose": ([vp, P(Pose)], i),
        "kfx_get_frame_count": ([vp, P(i)], i),
        "kfx_get_pose_record": ([vp, P(Pose), i, P(i)], i),
        "kfx_write_poses_txt": ([vp, C.c_char_p], i),
        "kfx_get_frame_maps": ([vp, i, i, P(f), P(f), P(f)], i),
        "kfx_set_frame_maps": ([vp, i, i, P(f), P(f)], i),
        "kfx_download_tsdf": ([vp, vp], i),
        "kfx_upload_tsdf": ([vp, vp], i),
        "kfx_download_volume_soa": ([vp, P(C.c_int16), P(C.c_int16), P(C.c_uint8)], i),
        "kfx_stage_preprocess": ([vp, P(C.c_uint8), P(f)], i),
        "kfx_stage_icp_accumulate": ([vp, i, P(Pose), P(C.c_int64)], i),
        "kfx_stage_icp": ([vp, P(Pose)], i),
        "kfx_stage_integrate": ([vp, P(Pose), P(C.c_int64), P(C.c_int64)], i),
        "kfx_stage_raycast": ([vp, P(Pose), P(f)], i),
        "kfx_set_profiling": ([vp, i], i),
        "kfx_get_stage_ms": ([vp, P(f)], i),
        "kfx_integrate_counts": ([vp, P(C.c_int64), P(C.c_int64)], i),
        "kfx_integrate_stats": ([vp, P(C.c_int64)], i),
        "kfx_raycast_stats": ([vp, P(C.c_int64)], i),
        "kfx_pipeline_async": ([vp, P(C.c_uint8), P(f)], i),
        "kfx_slab_mask_payload": ([P(C.c_uint32), P(C.c_uint32), P(C.c_uint32), C.c_int64], i),
        "kfx_set_icp_allreduce": ([vp, i], i),
        "kfx_slab_expand": ([P(C.c_uint32), P(Intrinsics), P(Pose), P(f), P(f), P(f)], i),
        "kfx_pipeline_async_u16": ([vp, P(C.c_uint8), P(C.c_uint16)], i),
        "kfx_register_host_buffer": ([vp, vp, C.c_size_t], i),
        "kfx_unregister_host_buffer": ([vp, vp], i),
        "kfx_download_columns": ([vp, P(C.c_int32), i, P(C.c_int16), P(C.c_int16), P(C.c_uint32)], i),
        "kfx_create_slab": ([P(Intrinsics), P(Params), i, i, i, P(vp)], i),
        "kfx_create_slab_cuts": ([P(Intrinsics), P(Params), i, i, i, P(i), P(vp)], i),
        "kfx_slice_work": ([vp, P(C.c_uint8), P(f), P(C.c_int64)], i),
        "kfx_slice_work_parts": ([vp, P(C.c_uint8), P(f), P(C.c_int64), P(C.c_int64)], i),
        "kfx_slice_work_at": ([vp, P(C.c_uint8), P(f), P(Pose), P(C.c_int64), P(C.c_int64), P(C.c_int64)], i),
        "kfx_get_graph_mode": ([vp, P(i)], i),
        "kfx_get_graph_note": ([vp], C.c_char_p),
        "kfx_slab_balance": ([P(C.c_int64), i, i, P(i)], i),
        "kfx_slab_info": ([vp, P(i), P(i), P(i), P(i)], i),
        "kfx_comm_get_unique_id": ([P(C.c_uint8)], i),
        "kfx_comm_init": ([vp, P(C.c_uint8)], i),
        "kfx_pipeline_group": ([P(vp), i, P(C.c_uint8), P(f)], i),
        "kfx_slab_frame_local": ([vp, P(C.c_uint8), P(f), P(C.c_uint32), P(C.c_uint32)], i),
        "kfx_slab_frame_finish": ([vp, P(C.c_uint32)], i),
        "kfx_extract_points": ([vp, P(f), C.c_int64, P(C.c_int64)], i),
        "kfx_render": ([vp, i, P(C.c_uint8)], i),
        "kfx_render_view": ([vp, P(Intrinsics), P(Pose), i, P(C.c_uint8), P(f), P(f), P(f)], i),
        "kfx_get_view_ms": ([vp, P(f)], i),
        "kfx_write_ppm": ([C.c_char_p, P(C.c_uint8), i, i], i),
        "kfx_shift_volume": ([vp, P(i)], i),
        "kfx_evict_points": ([vp, P(i), vp, C.c_int64, P(C.c_int64)], i),
        "kfx_get_volume_origin": ([vp, P(i)], i),
        "kfx_get_volume_pose": ([vp, P(Pose)], i),
        "kfx_get_shift_ms": ([vp, P(f)], i),
        "kfx_shift_for_pose": ([P(Params), P(Pose), P(Pose), f, P(i)], i),
        "kfx_evict_bricks": ([vp, P(i), vp, C.c_int64, P(C.c_int64)], i),
        "kfx_restore_bricks": ([vp, vp, C.c_int64, P(C.c_int64)], i),
        "kfx_get_stream_ms": ([vp, P(f)], i),
        "kfx_brick_store_create": ([P(vp)], i),
        "kfx_brick_store_destroy": ([vp], i),
        "kfx_brick_store_put": ([vp, vp, C.c_int64], i),
        "kfx_brick_store_count": ([vp, P(C.c_int64)], i),
        "kfx_brick_store_take_window": ([vp, P(i), P(i), vp, C.c_int64, P(C.c_int64)], i),
        "kfx_world_points_attr": ([vp, vp, C.c_int64, vp, C.c_int64, P(C.c_int64)], i),
        "kfx_world_mesh_attr": ([vp, vp, C.c_int64, vp, C.c_int64, P(C.c_int64)], i),
        "kfx_get_world_ms": ([vp, P(f)], i),
        "kfx_brick_store_copy": ([vp, vp, C.c_int64, P(C.c_int64)], i),
        "kfx_world_bricks": ([vp, vp, vp, C.c_int64, P(C.c_int64)], i),
        "kfx_save_world_mesh": ([vp, vp, C.c_char_p, C.c_int64], i),
        "kfx_extract_mesh_indexed": ([vp, vp, C.c_int64, vp, C.c_int64, P(C.c_int64), P(C.c_int64)], i),
        "kfx_world_mesh_indexed": ([vp, vp, C.c_int64, vp, C.c_int64, vp, C.c_int64, P(C.c_int64), P(C.c_int64)], i),
        "kfx_get_indexed_ms": ([vp, P(f)], i),
        "kfx_write_ply_mesh_indexed": ([C.c_char_p, vp, C.c_int64, vp, C.c_int64], i),
        "kfx_save_mesh_indexed": ([vp, C.c_char_p], i),
        "kfx_save_world_mesh_indexed": ([vp, vp, C.c_char_p], i),
        "kfx_world_view_load": ([vp, vp, C.c_int64, P(i), P(i)], i),
        "kfx_world_view": ([vp, P(Intrinsics), P(Pose), i, P(C.c_uint8), P(f), P(f), P(f)], i),
        "kfx_get_world_view_ms": ([vp, P(f)], i),
        "kfx_save_world_view": ([vp, vp, P(Intrinsics), P(Pose), i, C.c_char_p], i),
        "kfx_volume_checksum": ([vp, P(C.c_uint64)], i),
        "kfx_write_ply": ([C.c_char_p, P(f), C.c_int64], i),
        "kfx_save_pointcloud": ([vp, C.c_char_p, C.c_int64], i),
        "kfx_extract_mesh": ([vp, P(f), C.c_int64, P(C.c_int64)], i),
        "kfx_get_extract_ms": ([vp, P(f)], i),
        "kfx_set_extract_passes": ([vp, i], i),
        "kfx_set_slab_bound": ([vp, i], i),
        "kfx_get_extract_passes": ([vp, P(i)], i),
        "kfx_write_ply_mesh": ([C.c_char_p, P(f), C.c_int64], i),
        "kfx_extract_points_attr": ([vp, vp, C.c_int64, P(C.c_int64)], i),
        "kfx_extract_mesh_attr": ([vp, vp, C.c_int64, P(C.c_int64)], i),
        "kfx_write_ply_attr": ([C.c_char_p, vp, C.c_int64], i),
        "kfx_write_ply_mesh_attr": ([C.c_char_p, vp, C.c_int64], i),
        "kfx_save_pointcloud_attr": ([vp, C.c_char_p, C.c_int64], i),
        "kfx_save_mesh_attr": ([vp, C.c_char_p, C.c_int64], i),
        "kfx_stage_icp_residuals": ([vp, i, P(Pose), P(f), P(C.c_uint8), P(IcpQuality)], i),
        "kfx_score_poses": ([vp, i, P(Pose), C.c_int64, P(IcpQuality)], i),
        "kfx_frame_quality": ([vp, i, P(f), P(C.c_uint8), P(IcpQuality)], i),
        "kfx_score_view": ([vp, i, P(Pose), P(f), P(C.c_uint8), P(IcpQuality)], i),
        "kfx_get_quality_ms": ([vp, P(f)], i),
        "kfx_quality_figures": ([P(IcpQuality), P(C.c_double), P(C.c_double)], i),
        "kfx_quality_chunk": ([i, i, C.c_int64], i),
        "kfx_icp_multi": ([vp, P(Pose), C.c_int64, P(IcpResult), P(IcpQuality)], i),
        "kfx_track_view": ([vp, P(Pose), P(Pose), C.c_int64, P(IcpResult), P(Pose), P(IcpQuality)], i),
        "kfx_resume_at": ([vp, P(Pose)], i),
        "kfx_icp_multi_chunk": ([i, i, C.c_int64], i),
        "kfx_get_icp_multi_ms": ([vp, P(f)], i),
        "kfx_fern_table": ([P(Intrinsics), i, P(FernParams), vp], i),
        "kfx_keyframes_create": ([vp, P(FernParams), vp, P(vp)], i),
        "kfx_keyframes_destroy": ([vp], i),
        "kfx_keyframes_get_table": ([vp, vp], i),
        "kfx_keyframes_count": ([vp, P(C.c_int64)], i),
        "kfx_encode_frame": ([vp, vp, P(C.c_uint64)], i),
        "kfx_keyframes_add": ([vp, vp, P(Pose), P(C.c_int32)], i),
        "kfx_keyframes_put": ([vp, P(Pose), P(C.c_uint64), P(C.c_int32)], i),
        "kfx_keyframes_consider": ([vp, vp, C.c_int32, P(C.c_int32), P(KeyframeMatch)], i),
        "kfx_keyframes_get": ([vp, C.c_int32, P(Pose), P(C.c_uint64)], i),
        "kfx_keyframes_search": ([vp, vp, P(C.c_uint64), C.c_int64, i, vp], i),
        "kfx_keyframes_search_chunk": ([C.c_int64, C.c_int64], i),
        "kfx_keyframes_export": ([vp, vp, C.c_int64, P(C.c_int64)], i),
        "kfx_keyframes_import": ([vp, vp, C.c_int64, P(vp)], i),
        "kfx_get_keyframe_ms": ([vp, P(f)], i),
        "kfx_relocalise": ([vp, vp, i, P(Pose), C.c_int64, C.c_double, P(RelocResult)], i),
        "kfx_pipeline_recover": ([vp, vp, P(C.c_uint8), P(f), P(RecoverParams), P(RecoverReport)], i),
        "kfx_dataset_open": ([C.c_char_p, P(vp)], i),
        "kfx_dataset_info": ([vp, P(Intrinsics), P(i), P(i)], i),
        "kfx_dataset_read": ([vp, i, P(C.c_uint8), P(f)], i),
        "kfx_dataset_close": ([vp], i),
        "kfx_png_info": ([C.c_char_p, P(i), P(i), P(i), P(i)], i),
        "kfx_png_read_bgr8": ([C.c_char_p, P(C.c_uint8), i, i], i),
        "kfx_png_read_depth": ([C.c_char_p, P(f), i, i], i),
        "kfx_parse_intr": ([C.c_char_p, P(f)], i),
    }
    for name, (args, res) in sig.items():
        try:
            fn = getattr(L, name)
        except AttributeError:  # an older build (A/B timing runs); calling it raises then
            continue
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L


def _check(rc: int, what: str, ok=(KFX_OK,)) -> int:
    if rc not in ok:
        raise KfxError(f"{what} failed ({rc}): {lib().kfx_last_error().decode(errors='replace')}")
    return rc


def slab_mask_payload(key_local: np.ndarray, key_min: np.ndarray, payload: np.ndarray) -> np.ndarray:
    """Host side of the slab combine (kfx_slab_mask_payload): payload (4, n)
    u32 with the pixels this slab lost cleared (returns a copy)."""
    u32p = C.POINTER(C.c_uint32)
    kl = np.ascontiguousarray(key_local, np.uint32).ravel()
    km = np.ascontiguousarray(key_min, np.uint32).ravel()
    pay = np.ascontiguousarray(payload, np.uint32).copy()
    _check(lib().kfx_slab_mask_payload(kl.ctypes.data_as(u32p), km.ctypes.data_as(u32p), pay.ctypes.data_as(u32p),
                                       kl.size), "kfx_slab_mask_payload")
    return pay


def slab_expand(payload: np.ndarray, intr, cam2vol: Pose, Rinv: np.ndarray):
    """Host side of the slab combine (kfx_slab_expand): level-0 (vmap, nmap)."""
    pay = np.ascontiguousarray(payload, np.uint32)
    I = Intrinsics.from_any(intr)
    vmap = np.zeros((I.height, I.width, 3), np.float32)
    nmap = np.zeros_like(vmap)
    R = np.ascontiguousarray(Rinv, np.float32).reshape(9)
    _check(lib().kfx_slab_expand(pay.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(I), C.byref(cam2vol), fptr(R),
                                 fptr(vmap), fptr(nmap)), "kfx_slab_expand")
    return vmap, nmap


def write_ply(path: str, xyz: np.ndarray):
    """kinectfusion::savePointcloud's ASCII PLY for an (N, 3) float32 array."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    _check(lib().kfx_write_ply(path.encode(), fptr(xyz), xyz.shape[0]), "kfx_write_ply")


VIEW_KINDS = {"phong": 0, "normal": 1, "color": 2}  # KFX_VIEW_*


def write_ppm(path: str, bgr: np.ndarray):
    """Binary PPM (P6, RGB) of an (H, W, 3) uint8 image in the ABI's BGR order."""
    img = np.ascontiguousarray(bgr, np.uint8)
    assert img.ndim == 3 and img.shape[2] == 3
    _check(lib().kfx_write_ppm(path.encode(), img.ctypes.data_as(C.POINTER(C.c_uint8)), img.shape[1], img.shape[0]),
           "kfx_write_ppm")


def quality_figures(q: IcpQuality) -> tuple:
    """kfx_quality_figures: (fitness, rmse) of a record, both float (host only)."""
    a, b = C.c_double(), C.c_double()
    _check(lib().kfx_quality_figures(C.byref(q), C.byref(a), C.byref(b)), "kfx_quality_figures")
    return a.value, b.value


def quality_chunk(width: int, height: int, n: int) -> int:
    """kfx_quality_chunk: poses one block of a score_poses batch of n walks at a width x height level."""
    return _check(lib().kfx_quality_chunk(int(width), int(height), int(n)), "kfx_quality_chunk",
                  ok=range(1, 17))


def icp_multi_chunk(width: int, height: int, n: int) -> int:
    """kfx_icp_multi_chunk: poses one block of an icp_multi batch of n walks at a width x height level."""
    return _check(lib().kfx_icp_multi_chunk(int(width), int(height), int(n)), "kfx_icp_multi_chunk",
                  ok=range(1, 17))


def keyframes_search_chunk(n_keyframes: int, q: int) -> int:
    """kfx_keyframes_search_chunk: queries one block walks in a search of q codes over n keyframes."""
    return _check(lib().kfx_keyframes_search_chunk(int(n_keyframes), int(q)), "kfx_keyframes_search_chunk",
                  ok=tuple(range(1, 17)))


def _fern_params(m=512, seed=2013, depth_mm=(400, 4000)) -> FernParams:
    return FernParams(int(m), int(depth_mm[0]), int(depth_mm[1]), int(seed))


def fern_table(intr, pyramid_height: int = 3, m: int = 512, seed: int = 2013, depth_mm=(400, 4000)) -> np.ndarray:
    """kfx_fern_table (host only): the generated table as a FERN_DTYPE array of m records."""
    out = np.zeros(max(int(m), 0) if 0 <= int(m) <= 4096 else 0, FERN_DTYPE)
    buf = np.zeros(max(out.size, 1), FERN_DTYPE)
    I, fp = Intrinsics.from_any(intr), _fern_params(m, seed, depth_mm)
    _check(lib().kfx_fern_table(C.byref(I), int(pyramid_height), C.byref(fp), buf.ctypes.data), "kfx_fern_table")
    return buf[:out.size].copy()


class Keyframes:
    """kfx_keyframes: the device-resident keyframe store of a KinectFusion context.  Codes are
    uint64 arrays of m / 16 words, matches (id, distance) pairs in match order."""

    def __init__(self, kf: "KinectFusion", m: int = 512, seed: int = 2013, depth_mm=(400, 4000), table=None,
                 _handle=None):
        self.kf = kf
        if _handle is not None:
            self._h = _handle
        else:
            h = C.c_void_p()
            t = None if table is None else np.ascontiguousarray(table, FERN_DTYPE)
            fp = _fern_params(m if t is None else t.size, seed, depth_mm)
            _check(lib().kfx_keyframes_create(kf._h, C.byref(fp), None if t is None else t.ctypes.data, C.byref(h)),
                   "kfx_keyframes_create")
            self._h = h
        self.m = int(self.table().size)
        self.words = self.m // 16

    @staticmethod
    def load(kf: "KinectFusion", blob: bytes) -> "Keyframes":
        """kfx_keyframes_import."""
        h = C.c_void_p()
        b = np.frombuffer(bytes(blob), np.uint8)
        _check(lib().kfx_keyframes_import(kf._h, b.ctypes.data if b.size else None, b.size, C.byref(h)),
               "kfx_keyframes_import")
        return Keyframes(kf, _handle=h)

    def close(self):
        if getattr(self, "_h", None):
            lib().kfx_keyframes_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __len__(self):
        n = C.c_int64()
        _check(lib().kfx_keyframes_count(self._h, C.byref(n)), "kfx_keyframes_count")
        return int(n.value)

    def table(self) -> np.ndarray:
        probe = np.zeros(1024, FERN_DTYPE)
        probe["x"] = -7
        _check(lib().kfx_keyframes_get_table(self._h, probe.ctypes.data), "kfx_keyframes_get_table")
        return probe[:int(np.count_nonzero(probe["x"] != -7))].copy()

    def encode(self) -> np.ndarray:
        code = np.zeros(self.words, np.uint64)
        _check(lib().kfx_encode_frame(self.kf._h, self._h, code.ctypes.data_as(C.POINTER(C.c_uint64))), "kfx_encode_frame")
        return code

    def add(self, cam_pose=None) -> int:
        P = None if cam_pose is None else (cam_pose if isinstance(cam_pose, Pose) else Pose.from_matrix(cam_pose))
        k = C.c_int32(-1)
        _check(lib().kfx_keyframes_add(self.kf._h, self._h, None if P is None else C.byref(P), C.byref(k)),
               "kfx_keyframes_add")
        return int(k.value)

    def put(self, cam_pose, code) -> int:
        P = cam_pose if isinstance(cam_pose, Pose) else Pose.from_matrix(cam_pose)
        c = np.ascontiguousarray(code, np.uint64)
        if c.size != self.words:
            raise ValueError("a code has m / 16 words")
        k = C.c_int32(-1)
        _check(lib().kfx_keyframes_put(self._h, C.byref(P), c.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(k)),
               "kfx_keyframes_put")
        return int(k.value)

    def consider(self, min_distance: int) -> tuple:
        """kfx_keyframes_consider: (new id or -1, (nearest id, distance) before the add)."""
        k, m = C.c_int32(-1), KeyframeMatch(-1, -1)
        _check(lib().kfx_keyframes_consider(self.kf._h, self._h, int(min_distance), C.byref(k), C.byref(m)),
               "kfx_keyframes_consider")
        return int(k.value), (int(m.id), int(m.distance))

    def get(self, k: int) -> tuple:
        P, code = Pose(), np.zeros(self.words, np.uint64)
        _check(lib().kfx_keyframes_get(self._h, int(k), C.byref(P), code.ctypes.data_as(C.POINTER(C.c_uint64))),
               "kfx_keyframes_get")
        return P, code

    def search(self, codes=None, k: int = 4) -> np.ndarray:
        """kfx_keyframes_search: (q, k, 2) int32 of (id, distance) in match order, -1 in unused slots.
        codes: (q, m / 16) uint64, or None for the frame's own code (q = 1)."""
        if codes is None:
            c, q = None, 1
        else:
            c = np.ascontiguousarray(codes, np.uint64).reshape(-1, self.words)
            q = c.shape[0]
        out = np.full((max(q, 1), max(int(k), 1), 2), -9, np.int32)
        _check(lib().kfx_keyframes_search(self.kf._h, self._h,
                                          None if c is None or q == 0 else c.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          q, int(k), out.ctypes.data), "kfx_keyframes_search")
        return out[:q]

    def export(self) -> bytes:
        n = C.c_int64()
        _check(lib().kfx_keyframes_export(self._h, None, 0, C.byref(n)), "kfx_keyframes_export")
        b = np.zeros(n.value, np.uint8)
        _check(lib().kfx_keyframes_export(self._h, b.ctypes.data, b.size, C.byref(n)), "kfx_keyframes_export")
        return b.tobytes()


def shift_for_pose(params: Params, volume_pose, cam_pose, ahead_m: float) -> tuple:
    """kfx_shift_for_pose: the (sx, sy, sz) voxel shift (multiples of 8) that centres the
    volume at `volume_pose` on the point ahead_m metres along the +z of camera-to-world
    `cam_pose` (4x4 matrices or Pose).  Host only."""
    V = volume_pose if isinstance(volume_pose, Pose) else Pose.from_matrix(volume_pose)
    K = cam_pose if isinstance(cam_pose, Pose) else Pose.from_matrix(cam_pose)
    s = (C.c_int * 3)()
    _check(lib().kfx_shift_for_pose(C.byref(params), C.byref(V), C.byref(K), float(ahead_m), s), "kfx_shift_for_pose")
    return tuple(int(x) for x in s)


# kfx_vertex (include/kfx.h): position, unit normal, colour in the ABI's BGR order + a (255: coloured)
VERTEX_DTYPE = [("xyz", "<f4", 3), ("normal", "<f4", 3), ("bgra", "u1", 4)]


def write_ply_attr(path: str, verts: np.ndarray):
    """ASCII PLY (x y z nx ny nz red green blue) of an (N,) VERTEX_DTYPE array."""
    v = np.ascontiguousarray(verts, np.dtype(VERTEX_DTYPE)).ravel()
    _check(lib().kfx_write_ply_attr(path.encode(), v.ctypes.data_as(C.c_void_p), v.shape[0]), "kfx_write_ply_attr")


def write_ply_mesh_attr(path: str, tris: np.ndarray):
    """ASCII PLY of an (N, 3) VERTEX_DTYPE triangle soup: 3N attributed vertices, N faces."""
    t = np.ascontiguousarray(tris, np.dtype(VERTEX_DTYPE)).reshape(-1, 3)
    _check(lib().kfx_write_ply_mesh_attr(path.encode(), t.ctypes.data_as(C.c_void_p), t.shape[0]),
           "kfx_write_ply_mesh_attr")


def write_ply_mesh_indexed(path: str, verts: np.ndarray, tris: np.ndarray):
    """ASCII PLY of an indexed mesh: (V,) VERTEX_DTYPE vertices and (T, 3) uint32 faces."""
    v = np.ascontiguousarray(verts, np.dtype(VERTEX_DTYPE)).ravel()
    t = np.ascontiguousarray(tris, np.uint32).reshape(-1, 3)
    _check(lib().kfx_write_ply_mesh_indexed(path.encode(), v.ctypes.data_as(C.c_void_p) if len(v) else None, len(v),
                                            t.ctypes.data_as(C.c_void_p) if len(t) else None, len(t)),
           "kfx_write_ply_mesh_indexed")


def png_info(path: str) -> tuple:
    """(width, height, channels, bit_depth) of a PNG file."""
    w, h, c, b = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _check(lib().kfx_png_info(path.encode(), C.byref(w), C.byref(h), C.byref(c), C.byref(b)), "kfx_png_info")
    return w.value, h.value, c.value, b.value


def png_read_bgr8(path: str) -> np.ndarray:
    """imread(path, IMREAD_COLOR): (H, W, 3) uint8 BGR."""
    w, h, _, _ = png_info(path)
    out = np.empty((h, w, 3), np.uint8)
    _check(lib().kfx_png_read_bgr8(path.encode(), out.ctypes.data_as(C.POINTER(C.c_uint8)), w, h),
           "kfx_png_read_bgr8")
    return out


def png_read_depth(path: str) -> np.ndarray:
    """imread(path, IMREAD_UNCHANGED).convertTo(CV_32F): (H, W) float32."""
    w, h, _, _ = png_info(path)
    out = np.empty((h, w), np.float32)
    _check(lib().kfx_png_read_depth(path.encode(), fptr(out), w, h), "kfx_png_read_depth")
    return out


def parse_intr(path: str) -> tuple:
    """intr.txt (depth_sensor.cpp:22-35): (fx, cx, fy, cy, c)."""
    out = (C.c_float * 5)()
    _check(lib().kfx_parse_intr(path.encode(), out), "kfx_parse_intr")
    return tuple(out)


class Dataset:
    """depth_sensor's DATASET mode (depth_sensor.cpp:11-46, 186-196) over the C-ABI:
    frames as kinectfusion::pipeline receives them (BGR uint8, depth float mm)."""

    def __init__(self, path: str):
        h = C.c_void_p()
        _check(lib().kfx_dataset_open(path.encode(), C.byref(h)), "kfx_dataset_open")
        self._h = h
        intr, n, has = Intrinsics(), C.c_int(), C.c_int()
        _check(lib().kfx_dataset_info(self._h, C.byref(intr), C.byref(n), C.byref(has)), "kfx_dataset_info")
        self.intrinsics, self.n_frames, self.has_intr = intr, n.value, bool(has.value)

    def __len__(self):
        return self.n_frames

    def read(self, index: int):
        w, hgt = self.intrinsics.width, self.intrinsics.height
        bgr = np.empty((hgt, w, 3), np.uint8)
        dep = np.empty((hgt, w), np.float32)
        _check(lib().kfx_dataset_read(self._h, int(index), bgr.ctypes.data_as(C.POINTER(C.c_uint8)), fptr(dep)),
               "kfx_dataset_read")
        return bgr, dep

    def close(self):
        if self._h:
            lib().kfx_dataset_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# kfx_brick (3600 bytes): the world brick coordinate and the brick's tsdf, weight and colour in
# the device order of a brick, index 64*dz + 8*dy + dx
BRICK_DTYPE = np.dtype([("b", "<i4", 3), ("reserved", "<i4"), ("tsdf", "<i2", 512), ("weight", "u1", 512),
                        ("rgb", "u1", (512, 4))])
assert BRICK_DTYPE.itemsize == 3600


def _bricks(bricks) -> np.ndarray:
    return np.ascontiguousarray(bricks, BRICK_DTYPE).ravel()


class BrickStore:
    """The host-only brick store (kfx_brick_store_*): bricks outside the window, keyed by their
    world coordinate.  Needs the library, not a GPU."""

    def __init__(self):
        h = C.c_void_p()
        _check(lib().kfx_brick_store_create(C.byref(h)), "kfx_brick_store_create")
        self._h = h

    def put(self, bricks):
        """Copy (N,) BRICK_DTYPE bricks in; a coordinate already held is replaced."""
        a = _bricks(bricks)
        _check(lib().kfx_brick_store_put(self._h, a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a)),
               "kfx_brick_store_put")

    def __len__(self):
        n = C.c_int64()
        _check(lib().kfx_brick_store_count(self._h, C.byref(n)), "kfx_brick_store_count")
        return int(n.value)

    def take_window(self, origin, dims) -> np.ndarray:
        """Remove and return the bricks inside the window of voxel `origin` (multiples of 8) and
        `dims`, ascending (b[2], b[1], b[0])."""
        o = (C.c_int * 3)(*[int(x) for x in origin])
        d = (C.c_int * 3)(*[int(x) for x in dims])
        n = C.c_int64()
        _check(lib().kfx_brick_store_take_window(self._h, o, d, None, 0, C.byref(n)), "kfx_brick_store_take_window")
        out = np.zeros(int(n.value), BRICK_DTYPE)
        if len(out):
            _check(lib().kfx_brick_store_take_window(self._h, o, d, out.ctypes.data_as(C.c_void_p), len(out),
                                                     C.byref(n)), "kfx_brick_store_take_window")
        return out

    def copy(self) -> np.ndarray:
        """All bricks of the store, ascending (b[2], b[1], b[0]); nothing is removed."""
        n = C.c_int64()
        _check(lib().kfx_brick_store_copy(self._h, None, 0, C.byref(n)), "kfx_brick_store_copy")
        out = np.zeros(int(n.value), BRICK_DTYPE)
        if len(out):
            _check(lib().kfx_brick_store_copy(self._h, out.ctypes.data_as(C.c_void_p), len(out), C.byref(n)),
                   "kfx_brick_store_copy")
        return out

    def close(self):
        if self._h:
            lib().kfx_brick_store_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_ply_mesh(path: str, tris: np.ndarray):
    """ASCII PLY of an (N, 3, 3) float32 triangle soup."""
    t = np.ascontiguousarray(tris, np.float32)
    _check(lib().kfx_write_ply_mesh(path.encode(), fptr(t), t.shape[0]), "kfx_write_ply_mesh")


def comm_unique_id() -> bytes:
    """RCCL unique id (128 bytes) for kfx_comm_init; made on rank 0 and
    broadcast to the other ranks by the launcher."""
    buf = (C.c_uint8 * 128)()
    _check(lib().kfx_comm_get_unique_id(buf), "kfx_comm_get_unique_id")
    return bytes(buf)


def slab_balance(slice_work, world: int) -> list:
    """kfx_slab_balance: world + 1 slab cuts (multiples of 8) minimising the
    largest slab's stored-range work for a per-slice work histogram."""
    w = np.ascontiguousarray(slice_work, np.int64)
    cu = (C.c_int * (world + 1))()
    _check(lib().kfx_slab_balance(i64ptr(w), int(w.size), int(world), cu), "kfx_slab_balance")
    return list(cu)


def _trim(out: np.ndarray, n: int) -> np.ndarray:
    """The first n items of a cap-sized output buffer: a copy when n is well
    below the cap (a view would keep the whole cap-sized allocation alive)."""
    return out[:n].copy() if 2 * n < len(out) else out[:n]


def pipeline_group(members, color: np.ndarray, depth: np.ndarray) -> int:
    """One pipeline() frame over all Z-slabs held in this process
    (members[k] = slab k of len(members))."""
    color = np.ascontiguousarray(color, np.uint8)
    d = np.ascontiguousarray(depth, np.float32)
    hs = (C.c_void_p * len(members))(*[m._h for m in members])
    rc = lib().kfx_pipeline_group(hs, len(members), u8ptr(color), fptr(d))
    return _check(rc, "kfx_pipeline_group", ok=(KFX_OK, KFX_TRACKING_LOST))


class KinectFusion:
    """kf::kinectfusion over the C-ABI.  Images: depth (H,W) float32/uint16 mm,
    colour (H,W,3) uint8 BGR."""

    def __init__(self, intr, params: Params | None = None, device: int = 0, slab=None, cuts=None):
        """slab=(rank, world): this instance owns Z-slab `rank` of `world`
        (kfx_create_slab; with cuts, world + 1 slice boundaries:
        kfx_create_slab_cuts); combine through comm_init (one process per GPU)
        or pipeline_group (all slabs in this process)."""
        self.intr = Intrinsics.from_any(intr)
        self.params = params if params is not None else default_params()
        h = C.c_void_p()
        if slab is None:
            _check(lib().kfx_create(C.byref(self.intr), C.byref(self.params), device, C.byref(h)), "kfx_create")
        else:
            rank, world = slab
            if cuts is None:
                _check(lib().kfx_create_slab(C.byref(self.intr), C.byref(self.params), device, int(rank), int(world),
                                             C.byref(h)), "kfx_create_slab")
            else:
                cu = (C.c_int * (world + 1))(*[int(x) for x in cuts])
                _check(lib().kfx_create_slab_cuts(C.byref(self.intr), C.byref(self.params), device, int(rank),
                                                  int(world), cu, C.byref(h)), "kfx_create_slab_cuts")
        self._h = h
        self.slab = slab
        X, Y, Z = (int(d) for d in self.params.volu_dims)
        self.dims = (X, Y, Z)
        self.nvox = X * Y * Z

    def close(self):
        if getattr(self, "_h", None):
            lib().kfx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- kf::kinectfusion ------------------------------------------------
    def pipeline(self, color: np.ndarray, depth: np.ndarray) -> int:
        """Returns KFX_OK or KFX_TRACKING_LOST (reset applied, frame dropped)."""
        color = np.ascontiguousarray(color, np.uint8)
        if depth.dtype == np.uint16:
            d = np.ascontiguousarray(depth)
            rc = lib().kfx_pipeline_u16(self._h, u8ptr(color), u16ptr(d))
        else:
            d = np.ascontiguousarray(depth, np.float32)
            rc = lib().kfx_pipeline(self._h, u8ptr(color), fptr(d))
        return _check(rc, "kfx_pipeline", ok=(KFX_OK, KFX_TRACKING_LOST))

    def reset(self):
        _check(lib().kfx_reset(self._h), "kfx_reset")

    def getCurCameraPose(self) -> np.ndarray:
        p = Pose()
        _check(lib().kfx_get_cur_camera_pose(self._h, C.byref(p)), "kfx_get_cur_camera_pose")
        return p.matrix()

    @property
    def frame_count(self) -> int:
        n = C.c_int()
        _check(lib().kfx_get_frame_count(self._h, C.byref(n)), "kfx_get_frame_count")
        return n.value

    @property
    def pose_record(self) -> np.ndarray:
        n = C.c_int()
        _check(lib().kfx_get_pose_record(self._h, None, 0, C.byref(n)), "kfx_get_pose_record")
        buf = (Pose * max(n.value, 1))()
        _check(lib().kfx_get_pose_record(self._h, buf, n.value, C.byref(n)), "kfx_get_pose_record")
        return np.stack([buf[i].matrix() for i in range(n.value)])

    def write_poses_txt(self, path: str):
        _check(lib().kfx_write_poses_txt(self._h, path.encode()), "kfx_write_poses_txt")

    # ---- device-resident frames ------------------------------------------
    def stage_frames(self, colors: np.ndarray, depths: np.ndarray):
        colors = np.ascontiguousarray(colors, np.uint8)
        depths = np.ascontiguousarray(depths, np.float32)
        _check(lib().kfx_stage_frames(self._h, depths.shape[0], u8ptr(colors), fptr(depths)), "kfx_stage_frames")

    def pipeline_staged(self, idx: int):
        _check(lib().kfx_pipeline_staged(self._h, int(idx)), "kfx_pipeline_staged")

    def pipeline_async(self, color, depth_mm):
        """Queue a host frame (f32 or u16 depth, mm) without waiting for the GPU
        (kfx_pipeline_async); tracking status comes with synchronize()."""
        color = np.ascontiguousarray(color, np.uint8)
        if np.asarray(depth_mm).dtype == np.uint16:
            d = np.ascontiguousarray(depth_mm, np.uint16)
            _check(lib().kfx_pipeline_async_u16(self._h, u8ptr(color), d.ctypes.data_as(C.POINTER(C.c_uint16))),
                   "kfx_pipeline_async_u16")
        else:
            d = np.ascontiguousarray(depth_mm, np.float32)
            _check(lib().kfx_pipeline_async(self._h, u8ptr(color), fptr(d)), "kfx_pipeline_async")

    def register_host_buffer(self, arr: np.ndarray):
        """Page-lock a C-contiguous array: pipeline_async then uploads frames in
        it without a host copy (keep it unchanged until synchronize())."""
        assert arr.flags["C_CONTIGUOUS"]
        _check(lib().kfx_register_host_buffer(self._h, arr.ctypes.data, arr.nbytes), "kfx_register_host_buffer")

    def unregister_host_buffer(self, arr: np.ndarray):
        _check(lib().kfx_unregister_host_buffer(self._h, arr.ctypes.data), "kfx_unregister_host_buffer")

    def synchronize(self) -> int:
        """Wait for queued frames; KFX_OK, or KFX_TRACKING_LOST if one of the
        frames completed since the last status check was dropped (reset)."""
        return _check(lib().kfx_synchronize(self._h), "kfx_synchronize", ok=(KFX_OK, KFX_TRACKING_LOST))

    def set_graph_mode(self, mode):
        """0/False eager, 1/True (default) graphs, 2 overlapped frames also
        replay ICP + integrate + raycast as a graph (kfx.h kfx_set_graph_mode)."""
        _check(lib().kfx_set_graph_mode(self._h, int(mode)), "kfx_set_graph_mode")

    def graph_mode(self) -> int:
        """The graph mode in effect (kfx_get_graph_mode: lowered where RCCL
        refused stream capture)."""
        m = C.c_int()
        _check(lib().kfx_get_graph_mode(self._h, C.byref(m)), "kfx_get_graph_mode")
        return m.value

    def graph_note(self) -> str:
        """Why graph mode 2 was lowered (RCCL / capture error text), or ""."""
        return (lib().kfx_get_graph_note(self._h) or b"").decode(errors="replace")

    def set_kernel_timing(self, every: int, max_samples: int = 1024):
        """Bracket every `every`-th pipelined frame with HIP events (0 = off)."""
        _check(lib().kfx_set_kernel_timing(self._h, int(every), int(max_samples)), "kfx_set_kernel_timing")

    def kernel_timing(self) -> dict:
        """Mean ms of ICP / integrate / raycast (+ slab combine) over the sampled
        frames, and of the local raycast and the combine apart (resets the samples)."""
        a, n = (C.c_float * 4)(), C.c_int()
        _check(lib().kfx_get_kernel_timing_ex(self._h, a, C.byref(n)), "kfx_get_kernel_timing_ex")
        return {"icp": a[0], "integrate": a[1], "raycast": a[2] + a[3], "raycast_local": a[2],
                "combine": a[3], "samples": n.value}

    def set_frame_overlap(self, on: bool):
        """Overlap staged frames' preprocess with the previous frame's tracking."""
        _check(lib().kfx_set_frame_overlap(self._h, int(on)), "kfx_set_frame_overlap")

    def set_icp_allreduce(self, on: bool):
        """Slab contexts: shard the ICP sums over the ranks (all-reduced per iteration)."""
        _check(lib().kfx_set_icp_allreduce(self._h, int(on)), "kfx_set_icp_allreduce")

    def set_icp_persistent(self, on) -> bool:
        """Persistent ICP: False = one launch per iteration, True = one persistent
        launch, 2 = persistent through a cooperative launch; returns whether the
        persistent kernel is usable here."""
        r = lib().kfx_set_icp_persistent(self._h, int(on))
        _check(min(r, 0), "kfx_set_icp_persistent")
        return bool(r)

    def debug_force_icp_stall(self):
        """Test hook: the next tracked frame's persistent-ICP barrier never completes."""
        _check(lib().kfx_debug_force_icp_stall(self._h), "kfx_debug_force_icp_stall")

    def debug_force_index64(self, on=True):
        """Test hook: integrate / raycast take the 64-bit-index kernels (the
        >= 2^31-voxel path) at any volume size."""
        _check(lib().kfx_debug_force_index64(self._h, int(on)), "kfx_debug_force_index64")

    def debug_count_settled(self, on=True):
        """Debug hook: integrate counts the settled bricks its waves skip."""
        _check(lib().kfx_debug_count_settled(self._h, int(on)), "kfx_debug_count_settled")

    def debug_int_tiles(self, on=True) -> bool:
        """Debug switch: integrate's per-frame tile kernel on / off (off: every wave
        computes its own prologue); returns whether it is in use."""
        r = lib().kfx_debug_int_tiles(self._h, int(on))
        _check(min(r, 0), "kfx_debug_int_tiles")
        return bool(r)

    def debug_get_settled(self):
        """(bricks whose settled byte is set, bricks skipped by the last integrate)."""
        out = (C.c_uint64 * 2)()
        _check(lib().kfx_debug_get_settled(self._h, out), "kfx_debug_get_settled")
        return int(out[0]), int(out[1])

    def debug_get_hidden(self):
        """(bricks the last integrate skipped as hidden, those among them that hang
        over an end of their tile's interval); armed by debug_count_settled."""
        out = (C.c_uint64 * 2)()
        _check(lib().kfx_debug_get_hidden(self._h, out), "kfx_debug_get_hidden")
        return int(out[0]), int(out[1])

    def debug_get_icp_sums(self) -> np.ndarray:
        """The 27 int64 sums of the last ICP iteration that ran, whichever kernel ran it."""
        s = np.zeros(27, np.int64)
        _check(lib().kfx_debug_get_icp_sums(self._h, i64ptr(s)), "kfx_debug_get_icp_sums")
        return s

    def debug_get_icp_step(self) -> np.ndarray:
        """The six doubles (rotation vector, translation) of the last ICP iteration that solved."""
        x = (C.c_double * 6)()
        _check(lib().kfx_debug_get_icp_step(self._h, x), "kfx_debug_get_icp_step")
        return np.array(x[:], np.float64)

    def debug_cap_icp_blocks(self, cap: int = 0) -> dict:
        """Plan the persistent ICP as if at most `cap` blocks were co-resident
        (0: the device's own figure; < 0: change nothing); returns the plan in effect: usable,
        stride, nblocks, launch (0 none, 1 plain, 2 cooperative, 3 the sharded loop of stage_icp) and per level
        span / groups / ppl."""
        a = (C.c_int32 * 16)()
        r = lib().kfx_debug_cap_icp_blocks(self._h, int(cap), a)
        _check(min(r, 0), "kfx_debug_cap_icp_blocks")
        n = a[2]
        return {"usable": bool(r), "stride": int(a[0]), "nblocks": int(a[1]), "launch": int(a[3]),
                "span": [int(a[4 + 3 * l]) for l in range(n)], "groups": [int(a[5 + 3 * l]) for l in range(n)],
                "ppl": [int(a[6 + 3 * l]) for l in range(n)]}

    def debug_icp_plan(self) -> dict:
        """The persistent ICP's plan in effect (debug_cap_icp_blocks without a change)."""
        return self.debug_cap_icp_blocks(-1)

    def debug_extract_units(self, units: int = 0) -> int:
        """Force `units` (1, 2, 4, ..., 64) units per wave in every extraction sweep of this
        context (0: the automatic rule); returns the figure the next extraction uses."""
        r = lib().kfx_debug_extract_units(self._h, int(units))
        _check(min(r, 0), "kfx_debug_extract_units")
        return r

    def debug_scan(self, counts: np.ndarray):
        """The extraction's exclusive offset scan of uint32 counts on the device:
        ((n,) uint64 offsets, total)."""
        cnt = np.ascontiguousarray(counts, np.uint32)
        off = np.empty(len(cnt), np.uint64)
        tot = C.c_uint64()
        _check(lib().kfx_debug_scan(self._h, cnt.ctypes.data_as(C.POINTER(C.c_uint32)), len(cnt),
                                    off.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(tot)), "kfx_debug_scan")
        return off, int(tot.value)

    def debug_icp_band_ms(self, rank, world, reps=5) -> float:
        """Device ms of the sharded ICP's launches for band rank of world (no
        all-reduces; the tracking state is restored afterwards)."""
        ms = C.c_float()
        _check(lib().kfx_debug_icp_band_ms(self._h, int(rank), int(world), int(reps), C.byref(ms)),
               "kfx_debug_icp_band_ms")
        return float(ms.value)

    def icp_trace(self):
        """(iterations, 5) s_memrealtime stamps of the last persistent-ICP frame."""
        import numpy as np
        out = np.zeros((64, 12), np.uint64)
        n = _check(lib().kfx_get_icp_trace(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), 64),
                   "kfx_get_icp_trace", ok=tuple(range(65)))
        return out[:n]

    def set_profiling(self, on: bool):
        _check(lib().kfx_set_profiling(self._h, int(on)), "kfx_set_profiling")

    def stage_ms(self) -> dict:
        a = (C.c_float * 5)()
        _check(lib().kfx_get_stage_ms(self._h, a), "kfx_get_stage_ms")
        return dict(zip(["preprocess", "icp", "integrate", "raycast", "total"], a[:]))

    def integrate_counts(self):
        a, b = C.c_int64(), C.c_int64()
        _check(lib().kfx_integrate_counts(self._h, C.byref(a), C.byref(b)), "kfx_integrate_counts")
        return a.value, b.value

    def integrate_stats(self) -> dict:
        """Work of the last frame's integrate: updated / coloured / visited / gathered voxels."""
        a = (C.c_int64 * 8)()
        _check(lib().kfx_integrate_stats(self._h, a), "kfx_integrate_stats")
        return dict(zip(["updated", "colored", "visited", "gathered", "wave_batches"], a[:5]))

    def raycast_stats(self) -> dict:
        """Work of the last frame's raycast (re-run, nothing written)."""
        a = (C.c_int64 * 8)()
        _check(lib().kfx_raycast_stats(self._h, a), "kfx_raycast_stats")
        return dict(zip(["rays", "skip_lookups", "skipped_samples", "blocked_lookups", "batches",
                         "normal_candidates", "ref_uniq_voxels", "ref_reads"], a[:8]))

    def volume_checksum(self) -> tuple:
        """(hash sum mod 2^64, voxels with weight > 0) over the owned slices."""
        out = (C.c_uint64 * 2)()
        _check(lib().kfx_volume_checksum(self._h, out), "kfx_volume_checksum")
        return int(out[0]), int(out[1])

    def render(self, kind: str = "phong") -> np.ndarray:
        """getRenderMap(PHONG / NORMAL): (H, W, 3) uint8 from the last raycast."""
        out = np.empty((self.intr.height, self.intr.width, 3), np.uint8)
        _check(lib().kfx_render(self._h, 0 if kind == "phong" else 1, out.ctypes.data_as(C.POINTER(C.c_uint8))),
               "kfx_render")
        return out

    def _view(self, name: str, intr, pose, kind: str, maps: bool):
        I = Intrinsics.from_any(intr)
        P = pose if isinstance(pose, Pose) else Pose.from_matrix(pose)
        h, w = max(I.height, 0), max(I.width, 0)
        out = np.zeros((h, w, 3), np.uint8)
        vm = np.zeros((h, w, 3), np.float32) if maps else None
        nm = np.zeros((h, w, 3), np.float32) if maps else None
        ts = np.zeros((h, w), np.float32) if maps else None
        _check(getattr(lib(), name)(self._h, C.byref(I), C.byref(P), VIEW_KINDS[kind],
                                    out.ctypes.data_as(C.POINTER(C.c_uint8)), fptr(vm) if maps else None,
                                    fptr(nm) if maps else None, fptr(ts) if maps else None), name)
        return (out, vm, nm, ts) if maps else out

    def render_view(self, intr, pose, kind: str = "phong", maps: bool = False):
        """kfx_render_view: the volume as it stands seen from camera-to-world
        `pose` (4x4 matrix or Pose) through `intr` (any size and focal lengths);
        kind "phong", "normal" or "color" (the fused colour, BGR).  Returns the
        (H, W, 3) uint8 image, with maps=True (image, vmap, nmap, ts): the
        view's (H, W, 3) float32 vertex and normal maps and the (H, W) float32
        distance along each ray (0: no surface).  Tracking state is untouched."""
        return self._view("kfx_render_view", intr, pose, kind, maps)

    def view_ms(self) -> float:
        """Device milliseconds of the last render_view launch (HIP events)."""
        ms = C.c_float()
        _check(lib().kfx_get_view_ms(self._h, C.byref(ms)), "kfx_get_view_ms")
        return float(ms.value)

    # ---- ICP residuals and tracking quality ----------------
    def _quality(self, name: str, level: int, args: tuple, maps: bool):
        g = self.intr.level(level)
        res = np.zeros((g.height, g.width), np.float32) if maps else None
        lab = np.zeros((g.height, g.width), np.uint8) if maps else None
        q = IcpQuality()
        _check(getattr(lib(), name)(self._h, int(level), *args, fptr(res) if maps else None,
                                    u8ptr(lab) if maps else None, C.byref(q)), name)
        return (q, res, lab) if maps else q

    def stage_icp_residuals(self, level: int, pose, maps: bool = True):
        """kfx_stage_icp_residuals: CUR against PREV maps of `level` under the
        relative `pose`.  Returns (IcpQuality, residual (h, w) float32, label
        (h, w) uint8), or with maps=False the record alone (no per-pixel stores)."""
        P = pose if isinstance(pose, Pose) else Pose.from_matrix(pose)
        return self._quality("kfx_stage_icp_residuals", level, (C.byref(P),), maps)

    def frame_quality(self, level: int = 0, maps: bool = False):
        """kfx_frame_quality: the last frame's maps against the model raycast from its pose (identity)."""
        return self._quality("kfx_frame_quality", level, (), maps)

    def score_view(self, level: int, cam_pose, maps: bool = False):
        """kfx_score_view: CUR maps of `level` against the volume seen from the world pose cam_pose."""
        P = cam_pose if isinstance(cam_pose, Pose) else Pose.from_matrix(cam_pose)
        return self._quality("kfx_score_view", level, (C.byref(P),), maps)

    def score_poses(self, level: int, poses) -> list:
        """kfx_score_poses: one IcpQuality per relative pose (Pose or 4x4), one launch."""
        ps = [p if isinstance(p, Pose) else Pose.from_matrix(p) for p in poses]
        arr = (Pose * max(len(ps), 1))(*ps)
        out = (IcpQuality * max(len(ps), 1))()
        _check(lib().kfx_score_poses(self._h, int(level), arr, len(ps), out), "kfx_score_poses")
        return list(out)[:len(ps)]

    def quality_ms(self) -> dict:
        """Device ms of the last residual launch or batch, and of the view raycast in front of it (0: none)."""
        a = (C.c_float * 2)()
        _check(lib().kfx_get_quality_ms(self._h, a), "kfx_get_quality_ms")
        return {"residuals": float(a[0]), "view": float(a[1])}

    # ---- multi-start ICP, tracking against a view, resuming --
    def icp_multi(self, starts, quality: bool = False):
        """kfx_icp_multi: the coarse-to-fine ICP loop of CUR against PREV from every start (Pose or 4x4) in
        one batch.  Returns one IcpResult per start, or with quality=True (results, records): the level-0
        IcpQuality of each pose reached."""
        ps = [p if isinstance(p, Pose) else Pose.from_matrix(p) for p in starts]
        arr = (Pose * max(len(ps), 1))(*ps)
        out = (IcpResult * max(len(ps), 1))()
        q = (IcpQuality * max(len(ps), 1))() if quality else None
        _check(lib().kfx_icp_multi(self._h, arr, len(ps), out, q), "kfx_icp_multi")
        res = list(out)[:len(ps)]
        return (res, list(q)[:len(ps)]) if quality else res

    def track_view(self, cam_pose, starts, quality: bool = False):
        """kfx_track_view: the same loop against the volume seen from the world pose cam_pose.  Returns
        (results, world) with world[k] = cam_pose * results[k].pose as Pose, and the records behind them
        with quality=True."""
        V = cam_pose if isinstance(cam_pose, Pose) else Pose.from_matrix(cam_pose)
        ps = [p if isinstance(p, Pose) else Pose.from_matrix(p) for p in starts]
        arr = (Pose * max(len(ps), 1))(*ps)
        out = (IcpResult * max(len(ps), 1))()
        world = (Pose * max(len(ps), 1))()
        q = (IcpQuality * max(len(ps), 1))() if quality else None
        _check(lib().kfx_track_view(self._h, C.byref(V), arr, len(ps), out, world, q), "kfx_track_view")
        res, wl = list(out)[:len(ps)], list(world)[:len(ps)]
        return (res, wl, list(q)[:len(ps)]) if quality else (res, wl)

    def resume_at(self, cam_pose):
        """kfx_resume_at: the next frame tracks from the world pose cam_pose against the volume as it stands."""
        V = cam_pose if isinstance(cam_pose, Pose) else Pose.from_matrix(cam_pose)
        _check(lib().kfx_resume_at(self._h, C.byref(V)), "kfx_resume_at")

    # ---- relocalisation -------------------------------------
    def relocalise(self, keyframes: "Keyframes", k: int = 4, starts=None, min_fitness: float = 0.5) -> RelocResult:
        """kfx_relocalise: retrieve the k nearest keyframes, track against each one's view from every start
        (None: the identity), pick the best.  result.status is KFX_OK or KFX_TRACKING_LOST."""
        out = RelocResult()
        if starts is None:
            arr, n = None, 1
        else:
            ps = [p if isinstance(p, Pose) else Pose.from_matrix(p) for p in starts]
            arr, n = (Pose * max(len(ps), 1))(*ps), len(ps)
        _check(lib().kfx_relocalise(self._h, keyframes._h, int(k), arr, n, float(min_fitness), C.byref(out)),
               "kfx_relocalise", ok=(KFX_OK, KFX_TRACKING_LOST))
        return out

    def pipeline_recover(self, keyframes: "Keyframes", color: np.ndarray, depth: np.ndarray, params=None) -> tuple:
        """kfx_pipeline_recover: (status, RecoverReport); params a RecoverParams or None for the defaults."""
        color = np.ascontiguousarray(color, np.uint8)
        d = np.ascontiguousarray(depth, np.float32)
        rep = RecoverReport()
        rc = lib().kfx_pipeline_recover(self._h, keyframes._h, u8ptr(color), fptr(d),
                                        None if params is None else C.byref(params), C.byref(rep))
        return _check(rc, "kfx_pipeline_recover", ok=(KFX_OK, KFX_TRACKING_LOST)), rep

    def keyframe_ms(self) -> dict:
        """Device ms of the last frame encode and the last keyframe search."""
        a = (C.c_float * 2)()
        _check(lib().kfx_get_keyframe_ms(self._h, a), "kfx_get_keyframe_ms")
        return {"encode": float(a[0]), "search": float(a[1])}

    def icp_multi_ms(self) -> dict:
        """Device ms of the last icp_multi / track_view: the view raycasts, the loop, the final scoring (0: none)."""
        a = (C.c_float * 3)()
        _check(lib().kfx_get_icp_multi_ms(self._h, a), "kfx_get_icp_multi_ms")
        return {"view": float(a[0]), "loop": float(a[1]), "score": float(a[2])}

    # ---- moving volume ------------------------------------
    def shift_volume(self, shift):
        """kfx_shift_volume: move the volume's contents by `shift` = (sx, sy, sz) voxels
        (multiples of 8) in place, and the volume pose with them; None passes a null shift."""
        s = None if shift is None else (C.c_int * 3)(*[int(x) for x in shift])
        _check(lib().kfx_shift_volume(self._h, s), "kfx_shift_volume")

    def evict_points(self, shift, cap: int = 10_000_000) -> np.ndarray:
        """kfx_evict_points: the items of extract_points_attr that `shift` would drop,
        (N,) VERTEX_DTYPE in the same order; the volume is unchanged."""
        s = None if shift is None else (C.c_int * 3)(*[int(x) for x in shift])
        n = C.c_int64()
        out = np.empty(max(cap, 0), np.dtype(VERTEX_DTYPE))
        _check(lib().kfx_evict_points(self._h, s, out.ctypes.data_as(C.c_void_p) if cap > 0 else None, max(cap, 0),
                                      C.byref(n)), "kfx_evict_points")
        return _trim(out, min(n.value, max(cap, 0)))

    def evict_count(self, shift) -> int:
        """Items evict_points(shift) would return (count pass only)."""
        s = (C.c_int * 3)(*[int(x) for x in shift])
        n = C.c_int64()
        _check(lib().kfx_evict_points(self._h, s, None, 0, C.byref(n)), "kfx_evict_points")
        return n.value

    @property
    def volume_origin(self) -> tuple:
        """The accumulated shift in voxels (kfx_get_volume_origin)."""
        o = (C.c_int * 3)()
        _check(lib().kfx_get_volume_origin(self._h, o), "kfx_get_volume_origin")
        return tuple(int(x) for x in o)

    @property
    def volume_pose(self) -> np.ndarray:
        """The volume pose in effect, 4x4 (kfx_get_volume_pose)."""
        p = Pose()
        _check(lib().kfx_get_volume_pose(self._h, C.byref(p)), "kfx_get_volume_pose")
        return p.matrix()

    def shift_ms(self) -> dict:
        """Device ms of the last evict_points and the last shift_volume (HIP events)."""
        a = (C.c_float * 2)()
        _check(lib().kfx_get_shift_ms(self._h, a), "kfx_get_shift_ms")
        return {"evict": a[0], "shift": a[1]}

    def evict_bricks(self, shift, cap: int | None = None) -> np.ndarray:
        """kfx_evict_bricks: the non-empty bricks `shift` would drop, (N,) BRICK_DTYPE ascending
        (b[2], b[1], b[0]); the volume is unchanged.  cap None: all of them (a count pass first)."""
        s = None if shift is None else (C.c_int * 3)(*[int(x) for x in shift])
        if cap is None:
            cap = self.evict_brick_count(shift)
        n = C.c_int64()
        out = np.zeros(max(cap, 0), BRICK_DTYPE)
        _check(lib().kfx_evict_bricks(self._h, s, out.ctypes.data_as(C.c_void_p) if cap > 0 else None, max(cap, 0),
                                      C.byref(n)), "kfx_evict_bricks")
        return _trim(out, min(n.value, max(cap, 0)))

    def evict_brick_count(self, shift) -> int:
        """Bricks evict_bricks(shift) would return (count and scan only)."""
        s = None if shift is None else (C.c_int * 3)(*[int(x) for x in shift])
        n = C.c_int64()
        _check(lib().kfx_evict_bricks(self._h, s, None, 0, C.byref(n)), "kfx_evict_bricks")
        return int(n.value)

    def restore_bricks(self, bricks) -> int:
        """kfx_restore_bricks: write the (N,) BRICK_DTYPE bricks whose coordinate lies in the
        current window over the volume; returns how many were written."""
        a = _bricks(bricks)
        n = C.c_int64()
        _check(lib().kfx_restore_bricks(self._h, a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a),
                                        C.byref(n)), "kfx_restore_bricks")
        return int(n.value)

    def stream_ms(self) -> dict:
        """Device ms of the last evict_bricks and the last restore_bricks (HIP events)."""
        a = (C.c_float * 2)()
        _check(lib().kfx_get_stream_ms(self._h, a), "kfx_get_stream_ms")
        return {"evict_bricks": a[0], "restore_bricks": a[1]}

    # ---- world map ------------------------------------------
    def _world(self, bricks, cap: int, mesh: bool) -> np.ndarray:
        a = _bricks(bricks)
        name = "kfx_world_mesh_attr" if mesh else "kfx_world_points_attr"
        n = C.c_int64()
        cap = max(int(cap), 0)
        out = np.empty((cap, 3) if mesh else cap, np.dtype(VERTEX_DTYPE))
        _check(getattr(lib(), name)(self._h, a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a),
                                    out.ctypes.data_as(C.c_void_p) if cap > 0 else None, cap, C.byref(n)), name)
        return _trim(out, min(n.value, cap))

    def world_points(self, bricks, cap: int = 10_000_000) -> np.ndarray:
        """kfx_world_points_attr: the attributed points of the (N,) BRICK_DTYPE world `bricks`
        (strictly ascending (b[2], b[1], b[0])), (M,) VERTEX_DTYPE."""
        return self._world(bricks, cap, False)

    def world_mesh(self, bricks, cap: int = 50_000_000) -> np.ndarray:
        """kfx_world_mesh_attr: the attributed triangles of the world `bricks`, (M, 3) VERTEX_DTYPE."""
        return self._world(bricks, cap, True)

    def world_count(self, bricks, mesh: bool = False) -> int:
        """Points (or triangles) the world `bricks` holds (table, count and scan only)."""
        a = _bricks(bricks)
        name = "kfx_world_mesh_attr" if mesh else "kfx_world_points_attr"
        n = C.c_int64()
        _check(getattr(lib(), name)(self._h, a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a), None, 0,
                                    C.byref(n)), name)
        return int(n.value)

    def world_bricks(self, store: "BrickStore | None" = None) -> np.ndarray:
        """kfx_world_bricks: the window's non-empty bricks merged with the store's (the window's
        win), (N,) BRICK_DTYPE ascending; store and volume are unchanged."""
        h = store._h if store is not None else None
        n = C.c_int64()
        _check(lib().kfx_world_bricks(self._h, h, None, 0, C.byref(n)), "kfx_world_bricks")
        out = np.zeros(int(n.value), BRICK_DTYPE)
        if len(out):
            _check(lib().kfx_world_bricks(self._h, h, out.ctypes.data_as(C.c_void_p), len(out), C.byref(n)),
                   "kfx_world_bricks")
        return out

    def save_world_mesh(self, path: str, store: "BrickStore | None" = None, cap: int = 0):
        """kfx_save_world_mesh: the world's attributed mesh (window and store) as an ASCII PLY."""
        _check(lib().kfx_save_world_mesh(self._h, store._h if store is not None else None, path.encode(), cap),
               "kfx_save_world_mesh")

    def world_ms(self) -> dict:
        """Device ms of the last world_points / world_mesh / world_count: the neighbour table,
        count + scan, emit (HIP events; without the upload of the records)."""
        a = (C.c_float * 3)()
        _check(lib().kfx_get_world_ms(self._h, a), "kfx_get_world_ms")
        return {"table": a[0], "count": a[1], "emit": a[2]}

    # ---- world view -------------------------------------------
    def world_view_load(self, bricks, box=None):
        """kfx_world_view_load: make the (N,) BRICK_DTYPE world `bricks` the one world_view renders
        (a snapshot; an empty list unloads).  box = (origin, dims) in world voxels, None: the list's
        bounding box padded by one brick on every side."""
        a = _bricks(bricks)
        o = d = None
        if box is not None:
            o, d = (None if q is None else (C.c_int * 3)(*[int(x) for x in q]) for q in box)
        _check(lib().kfx_world_view_load(self._h, a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a), o, d),
               "kfx_world_view_load")

    def world_view(self, intr, pose, kind: str = "phong", maps: bool = False):
        """kfx_world_view: render_view of the loaded world (same arguments, same return shapes)."""
        return self._view("kfx_world_view", intr, pose, kind, maps)

    def world_view_ms(self) -> dict:
        """Device ms of the last world_view_load (without the upload) and the last world_view (HIP events)."""
        a = (C.c_float * 2)()
        _check(lib().kfx_get_world_view_ms(self._h, a), "kfx_get_world_view_ms")
        return {"load": a[0], "render": a[1]}

    def save_world_view(self, path: str, intr, pose, kind: str = "color", store: "BrickStore | None" = None):
        """kfx_save_world_view: window plus store seen from `pose` through `intr`, as a binary PPM."""
        I = Intrinsics.from_any(intr)
        P = pose if isinstance(pose, Pose) else Pose.from_matrix(pose)
        _check(lib().kfx_save_world_view(self._h, store._h if store is not None else None, C.byref(I), C.byref(P),
                                         VIEW_KINDS[kind], path.encode()), "kfx_save_world_view")

    # ---- indexed mesh ----------------------------------------
    def _indexed(self, call, fill: bool):
        """call(verts, cap_verts, tris, cap_tris, n_verts, n_tris): size, then (fill) fill."""
        nv, nt = C.c_int64(), C.c_int64()
        call(None, 0, None, 0, C.byref(nv), C.byref(nt))
        if not fill:
            return int(nv.value), int(nt.value)
        verts, tris = np.empty(int(nv.value), np.dtype(VERTEX_DTYPE)), np.empty((int(nt.value), 3), np.uint32)
        if len(verts):
            call(verts.ctypes.data_as(C.c_void_p), len(verts), tris.ctypes.data_as(C.c_void_p) if len(tris) else None,
                 len(tris), C.byref(nv), C.byref(nt))
            assert (nv.value, nt.value) == (len(verts), len(tris))
        return verts, tris

    def _window_indexed(self, *a):
        _check(lib().kfx_extract_mesh_indexed(self._h, *a), "kfx_extract_mesh_indexed")

    def extract_mesh_indexed(self):
        """kfx_extract_mesh_indexed: (verts (V,) VERTEX_DTYPE, tris (T, 3) uint32); verts[tris] is
        extract_mesh_attr()'s soup, each vertex (grid edge) stored once."""
        return self._indexed(self._window_indexed, True)

    def indexed_count(self) -> tuple:
        """(vertices, triangles) of extract_mesh_indexed, count and scans only."""
        return self._indexed(self._window_indexed, False)

    def world_mesh_indexed(self, bricks):
        """kfx_world_mesh_indexed: extract_mesh_indexed of the world `bricks` ((N,) BRICK_DTYPE)."""
        a = _bricks(bricks)

        def call(*rest):
            _check(lib().kfx_world_mesh_indexed(self._h, a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a), *rest),
                   "kfx_world_mesh_indexed")
        return self._indexed(call, True)

    def indexed_ms(self) -> dict:
        """Device ms of the last extract_mesh_indexed / world_mesh_indexed / indexed_count: the
        world's neighbour table (0 in the window form), counts + scans, vertex emit, index emit."""
        a = (C.c_float * 4)()
        _check(lib().kfx_get_indexed_ms(self._h, a), "kfx_get_indexed_ms")
        return {"table": a[0], "count": a[1], "verts": a[2], "tris": a[3]}

    def save_mesh_indexed(self, path: str):
        _check(lib().kfx_save_mesh_indexed(self._h, path.encode()), "kfx_save_mesh_indexed")

    def save_world_mesh_indexed(self, path: str, store: "BrickStore | None" = None):
        """kfx_save_world_mesh_indexed: the world's indexed mesh (window and store) as an ASCII PLY."""
        _check(lib().kfx_save_world_mesh_indexed(self._h, store._h if store is not None else None, path.encode()),
               "kfx_save_world_mesh_indexed")

    def extract_mesh(self, cap: int = 50_000_000) -> np.ndarray:
        """Marching-cubes triangles, (N, 3, 3) float32 world coordinates (canonical order)."""
        # one call into a cap-sized buffer (the library's single-pass path;
        # np.empty pages are touched only where triangles are written)
        n = C.c_int64()
        out = np.empty((max(cap, 0), 3, 3), np.float32)
        _check(lib().kfx_extract_mesh(self._h, fptr(out) if cap > 0 else None, max(cap, 0), C.byref(n)),
               "kfx_extract_mesh")
        return _trim(out, min(n.value, max(cap, 0)))

    # ---- point cloud (kinectfusion::extracePointcloud / savePointcloud) ---
    def extract_points(self, cap: int = 10_000_000) -> np.ndarray:
        """(N, 3) float32 zero-crossing points in world coordinates (canonical order)."""
        n = C.c_int64()
        out = np.empty((max(cap, 0), 3), np.float32)
        _check(lib().kfx_extract_points(self._h, fptr(out) if cap > 0 else None, max(cap, 0), C.byref(n)),
               "kfx_extract_points")
        return _trim(out, min(n.value, max(cap, 0)))

    def extract_points_attr(self, cap: int = 10_000_000) -> np.ndarray:
        """extract_points with a unit normal and the fused colour per point: (N,) VERTEX_DTYPE,
        item i = point i of extract_points (same order, total and cap prefix)."""
        n = C.c_int64()
        out = np.empty(max(cap, 0), np.dtype(VERTEX_DTYPE))
        _check(lib().kfx_extract_points_attr(self._h, out.ctypes.data_as(C.c_void_p) if cap > 0 else None,
                                             max(cap, 0), C.byref(n)), "kfx_extract_points_attr")
        return _trim(out, min(n.value, max(cap, 0)))

    def extract_mesh_attr(self, cap: int = 50_000_000) -> np.ndarray:
        """extract_mesh with a unit normal and the fused colour per vertex: (N, 3) VERTEX_DTYPE."""
        n = C.c_int64()
        out = np.empty((max(cap, 0), 3), np.dtype(VERTEX_DTYPE))
        _check(lib().kfx_extract_mesh_attr(self._h, out.ctypes.data_as(C.c_void_p) if cap > 0 else None,
                                           max(cap, 0), C.byref(n)), "kfx_extract_mesh_attr")
        return _trim(out, min(n.value, max(cap, 0)))

    def extract_count(self, mesh: bool = False, attr: bool = False) -> int:
        """Points (or triangles) the volume holds, without extracting them (count pass only);
        attr: through the _attr call (the same total)."""
        n = C.c_int64()
        name = ("kfx_extract_mesh" if mesh else "kfx_extract_points") + ("_attr" if attr else "")
        _check(getattr(lib(), name)(self._h, None, 0, C.byref(n)), name)
        return n.value

    def set_slab_bound(self, mode: int):
        """Z-slab raycast bounded by the previous frame's model (1), off (0, default),
        or bounded without margin (2, tests); results identical."""
        _check(lib().kfx_set_slab_bound(self._h, int(mode)), "kfx_set_slab_bound")

    def set_extract_passes(self, passes: int):
        """1: single-pass extraction (default); 2: count + scan + emit passes."""
        _check(lib().kfx_set_extract_passes(self._h, int(passes)), "kfx_set_extract_passes")

    def extract_ms(self) -> dict:
        """Device ms of the last extract_points / extract_mesh: the volume pass, the offset
        scan, and the pool copy (one volume read, passes = 1) or the emit pass (passes = 2)."""
        a = (C.c_float * 3)()
        _check(lib().kfx_get_extract_ms(self._h, a), "kfx_get_extract_ms")
        n = C.c_int()
        _check(lib().kfx_get_extract_passes(self._h, C.byref(n)), "kfx_get_extract_passes")
        return {"count": a[0], "scan": a[1], "emit": a[2], "passes": n.value}

    def save_pointcloud(self, path: str, cap: int = 0):
        _check(lib().kfx_save_pointcloud(self._h, path.encode(), cap), "kfx_save_pointcloud")

    def save_pointcloud_attr(self, path: str, cap: int = 0):
        _check(lib().kfx_save_pointcloud_attr(self._h, path.encode(), cap), "kfx_save_pointcloud_attr")

    def save_mesh_attr(self, path: str, cap: int = 0):
        _check(lib().kfx_save_mesh_attr(self._h, path.encode(), cap), "kfx_save_mesh_attr")

    # ---- Z-slab sharding -------------------------------------------------
    def slab_info(self):
        """(zb, zn, own0, own1): stored slices [zb, zb+zn), owned [own0, own1)."""
        a = [C.c_int() for _ in range(4)]
        _check(lib().kfx_slab_info(self._h, *[C.byref(x) for x in a]), "kfx_slab_info")
        return tuple(x.value for x in a)

    def slab_frame_local(self, color: np.ndarray, depth: np.ndarray):
        """Slab frame up to the local raycast (kfx_slab_frame_local): returns this
        slab's (keys (n,) u32, payload (4, n) u32) for an exchange by the caller."""
        color = np.ascontiguousarray(color, np.uint8)
        d = np.ascontiguousarray(depth, np.float32)
        n = self.intr.width * self.intr.height
        keys = np.zeros(n, np.uint32)
        pay = np.zeros((4, n), np.uint32)
        u32p = C.POINTER(C.c_uint32)
        _check(lib().kfx_slab_frame_local(self._h, u8ptr(color), fptr(d), keys.ctypes.data_as(u32p),
                                          pay.ctypes.data_as(u32p)), "kfx_slab_frame_local")
        return keys, pay

    def slab_frame_finish(self, payload: np.ndarray) -> int:
        """Finish the frame from the MAX-combined payload (kfx_slab_frame_finish)."""
        pay = np.ascontiguousarray(payload, np.uint32)
        rc = lib().kfx_slab_frame_finish(self._h, pay.ctypes.data_as(C.POINTER(C.c_uint32)))
        return _check(rc, "kfx_slab_frame_finish", ok=(KFX_OK, KFX_TRACKING_LOST))

    def slice_work(self, color: np.ndarray, depth: np.ndarray) -> np.ndarray:
        """(Z,) int64: per global slice, the estimated integrate cost of this
        frame at the first frame's pose (kfx_slice_work; slab balancing)."""
        color = np.ascontiguousarray(color, np.uint8)
        d = np.ascontiguousarray(depth, np.float32)
        out = np.zeros(self.dims[2], np.int64)
        _check(lib().kfx_slice_work(self._h, u8ptr(color), fptr(d), i64ptr(out)), "kfx_slice_work")
        return out

    def slice_work_at(self, color: np.ndarray, depth: np.ndarray, cam_pose=None):
        """(work, cover, updated), each (Z,) int64 (kfx_slice_work_at): the
        frame seen from cam_pose (4x4 camera-to-world; None = identity)."""
        color = np.ascontiguousarray(color, np.uint8)
        d = np.ascontiguousarray(depth, np.float32)
        work, cover, upd = (np.zeros(self.dims[2], np.int64) for _ in range(3))
        cam = None if cam_pose is None else C.byref(Pose.from_matrix(cam_pose))
        _check(lib().kfx_slice_work_at(self._h, u8ptr(color), fptr(d), cam, i64ptr(work), i64ptr(cover),
                                       i64ptr(upd)), "kfx_slice_work_at")
        return work, cover, upd

    def slice_work_parts(self, color: np.ndarray, depth: np.ndarray):
        """(cover, updated), each (Z,) int64 (kfx_slice_work_parts): voxel
        slots integrate's waves visit, and voxels whose depth test passes."""
        color = np.ascontiguousarray(color, np.uint8)
        d = np.ascontiguousarray(depth, np.float32)
        cover = np.zeros(self.dims[2], np.int64)
        upd = np.zeros(self.dims[2], np.int64)
        _check(lib().kfx_slice_work_parts(self._h, u8ptr(color), fptr(d), i64ptr(cover), i64ptr(upd)),
               "kfx_slice_work_parts")
        return cover, upd

    def comm_init(self, uid: bytes):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        _check(lib().kfx_comm_init(self._h, buf), "kfx_comm_init")

    # ---- frames / volume -------------------------------------------------
    def frame_maps(self, which: int, level: int):
        li = self.intr.level(level)
        d = np.zeros((li.height, li.width), np.float32)
        v = np.zeros((li.height, li.width, 3), np.float32)
        n = np.zeros_like(v)
        _check(lib().kfx_get_frame_maps(self._h, which, level, fptr(d), fptr(v), fptr(n)), "kfx_get_frame_maps")
        return d, v, n

    def set_frame_maps(self, which: int, level: int, vmap: np.ndarray, nmap: np.ndarray):
        v = np.ascontiguousarray(vmap, np.float32)
        n = np.ascontiguousarray(nmap, np.float32)
        _check(lib().kfx_set_frame_maps(self._h, which, level, fptr(v), fptr(n)), "kfx_set_frame_maps")

    def download_tsdf(self) -> np.ndarray:
        """Reference 8-byte records as a structured array (x fastest)."""
        rec = np.zeros(self.nvox, dtype=np.dtype([("tsdf", "<i2"), ("weight", "<i2"), ("rgb", "u1", 3),
                                                  ("pad", "u1")]))
        _check(lib().kfx_download_tsdf(self._h, rec.ctypes.data_as(C.c_void_p)), "kfx_download_tsdf")
        return rec

    def upload_tsdf(self, rec: np.ndarray):
        rec = np.ascontiguousarray(rec)
        assert rec.nbytes == 8 * self.nvox
        _check(lib().kfx_upload_tsdf(self._h, rec.ctypes.data_as(C.c_void_p)), "kfx_upload_tsdf")

    def volume_soa(self):
        t = np.zeros(self.nvox, np.int16)
        w = np.zeros(self.nvox, np.int16)
        c = np.zeros(4 * self.nvox, np.uint8)
        _check(lib().kfx_download_volume_soa(self._h, i16ptr(t), i16ptr(w), u8ptr(c)), "kfx_download_volume_soa")
        return t, w, c

    def download_columns(self, cols):
        """(tsdf, weight, rgb u8x4) of (x, y) columns over the owned slices, shape (n, nz)."""
        cols = np.ascontiguousarray(cols, np.int32).reshape(-1, 2)
        n = cols.shape[0]
        _, _, o0, o1 = self.slab_info()
        t = np.zeros((n, o1 - o0), np.int16)
        w = np.zeros((n, o1 - o0), np.int16)
        c = np.zeros((n, o1 - o0), np.uint32)
        _check(lib().kfx_download_columns(self._h, cols.ctypes.data_as(C.POINTER(C.c_int32)), n, i16ptr(t),
                                          i16ptr(w), c.ctypes.data_as(C.POINTER(C.c_uint32))),
               "kfx_download_columns")
        return t, w, c.view(np.uint8).reshape(n, o1 - o0, 4)

    # ---- stage seams -----------------------------------------------------
    def stage_preprocess(self, color, depth_mm):
        color = np.ascontiguousarray(color, np.uint8)
        d = np.ascontiguousarray(depth_mm, np.float32)
        _check(lib().kfx_stage_preprocess(self._h, u8ptr(color), fptr(d)), "kfx_stage_preprocess")

    def stage_icp_accumulate(self, level: int, pose: Pose) -> np.ndarray:
        s = np.zeros(27, np.int64)
        _check(lib().kfx_stage_icp_accumulate(self._h, level, C.byref(pose), i64ptr(s)), "kfx_stage_icp_accumulate")
        return s

    def stage_icp(self):
        p = Pose()
        rc = _check(lib().kfx_stage_icp(self._h, C.byref(p)), "kfx_stage_icp", ok=(KFX_OK, KFX_TRACKING_LOST))
        return rc, p

    def stage_integrate(self, vol2cam: Pose, counts: bool = True):
        a, b = C.c_int64(), C.c_int64()
        _check(lib().kfx_stage_integrate(self._h, C.byref(vol2cam), C.byref(a) if counts else None,
                                         C.byref(b) if counts else None), "kfx_stage_integrate")
        return a.value, b.value

    def stage_raycast(self, cam2vol: Pose, Rinv: np.ndarray):
        R = np.ascontiguousarray(Rinv, np.float32).reshape(9)
        _check(lib().kfx_stage_raycast(self._h, C.byref(cam2vol), fptr(R)), "kfx_stage_raycast")
