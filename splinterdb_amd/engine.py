"""Python host mirror of SplinterDB's routing_filter.h API over the MI355X engine's C ABI.

Names, argument meaning and errors follow the reference interface
(src/routing_filter.h:32-192): `routing_config_init`, `routing_filter_add`,
`routing_filter_lookup`, `routing_filter_get_next_value`, `routing_filter_is_value_found`,
`routing_filter_max_fingerprints`, `routing_filter_estimate_unique_keys_from_count`,
`routing_filter_space_use_bytes`. Errors raise `PlatformStatusError` carrying the
platform_status code (ENOMEM / EINVAL / ENODEV).

The compute runs only in librf_amd.so (hand-written HIP kernels for gfx950). There is
no CPU fallback: without the library or a HIP device every call raises.
"""
import ctypes
import os
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librf_amd.so")

STATUS_OK = 0
STATUS_NO_MEMORY = 12
STATUS_NO_DEVICE = 19
STATUS_BAD_PARAM = 22
STATUS_NO_SPACE = 28  # RF_AMD_ENOSPC: an edit that exceeds a range map's room
MAX_FILTERS = 32  # src/routing_filter.h:25
ROUTING_NOT_FOUND = 0xFFFF  # src/routing_filter.h:26

# symbols the C ABI (include/rf_amd.h) exports
EXPORTED = [
    "rf_amd_engine_create", "rf_amd_engine_destroy", "rf_amd_last_error",
    "rf_amd_batch_create", "rf_amd_batch_destroy", "rf_amd_batch_build_keys",
    "rf_amd_batch_build_var_keys", "rf_amd_batch_build_hashes", "rf_amd_batch_probe_keys",
    "rf_amd_batch_probe_var_keys", "rf_amd_batch_probe_hashes", "rf_amd_batch_info",
    "rf_amd_batch_probe_keys_runs", "rf_amd_batch_probe_hashes_runs",
    "rf_amd_batch_read_image", "rf_amd_batch_read_image_async", "rf_amd_batch_image_ptrs", "rf_amd_batch_num_filters",
    "rf_amd_batch_set_timing", "rf_amd_batch_timings", "rf_amd_batch_timings_back", 
    "rf_amd_debug_read_lines", "rf_amd_debug_rebuild_lines", "rf_amd_debug_phase_buffer", "rf_amd_diag_lookup_stats",
    "rf_amd_debug_probe_floor",
    "rf_amd_host_alloc", "rf_amd_host_free", "rf_amd_engine_fence", "rf_amd_engine_fence_wait",
    "rf_amd_host_register", "rf_amd_host_unregister", "rf_amd_batch_place_image", "rf_amd_engine_set_pool_limit",
    "rf_amd_lookup_submit", "rf_amd_lookup_wait", "rf_amd_lookup_reap", "rf_amd_lookup_server_stats",
    "rf_amd_build_id",
    "rf_amd_filter_add", "rf_amd_filter_lookup_hashes", "rf_amd_filter_lookup_keys",
    "rf_amd_image_free",
    "rf_amd_max_fingerprints", "rf_amd_estimate_unique_keys_from_count",
    "rf_amd_space_use_bytes",
    "rf_amd_estimate_unique_fp", "rf_amd_batch_estimate_unique_fp", "rf_amd_estimate_unique_keys",
    "rf_amd_lookup_async", "rf_amd_lookup_async_poll", "rf_amd_lookup_async_wait",
    "rf_amd_lookup_async_free", "rf_amd_filter_verify", "rf_amd_filter_print",
    "rf_amd_hash_keys", "rf_amd_hash_var_keys",
    "rf_amd_batch_export", "rf_amd_batch_import", "rf_amd_route_scratch_bytes", "rf_amd_route_probes", "rf_amd_batch_probe_pairs", "rf_amd_unroute_found",
    "rf_amd_batch_build_hashes_host", "rf_amd_batch_probe_hashes_host", "rf_amd_engine_pool_stats",
    "rf_amd_filter_print_abs", "rf_amd_batch_infos", "rf_amd_batch_destroy_on", "rf_amd_probe_many_hashes_host",
    "rf_amd_probe_filters_host", "rf_amd_engine_pool_trim", "rf_amd_engine_stream", "rf_amd_engine_sync",
    "rf_amd_batch_device_bytes", "rf_amd_batch_trim", "rf_amd_batch_stage_begin", "rf_amd_batch_stage_build",
    "rf_amd_batch_stage_abort", "rf_amd_lookup_server_error", "rf_amd_lookup_server_failed",
    "rf_amd_lookup_server_set_times", "rf_amd_diag_lookup_server_kill", "rf_amd_diag_lookup_ring",
    "rf_amd_batch_create_runs", "rf_amd_filter_add_runs", "rf_amd_diag_k4_bitmap_builds",
    "rf_amd_filter_set_create", "rf_amd_filter_set_destroy", "rf_amd_filter_set_num_members",
    "rf_amd_filter_set_probe_keys", "rf_amd_filter_set_probe_hashes",
    "rf_amd_found_compact_scratch_bytes", "rf_amd_found_compact",
    "rf_amd_filter_set_probe_var_keys", "rf_amd_batch_probe_var_keys_runs", "rf_amd_filter_lookup_var_keys",
    "rf_amd_diag_fanout_max_blocks", "rf_amd_diag_lookup_paths", "rf_amd_diag_part16_builds",
    "rf_amd_diag_dense_line_filters", "rf_amd_diag_k4_packed_builds",
    "rf_amd_filter_set_probe_keys_ragged", "rf_amd_filter_set_probe_var_keys_ragged",
    "rf_amd_filter_set_probe_hashes_ragged",
    "rf_amd_filter_set_create_cap", "rf_amd_filter_set_capacity", "rf_amd_filter_set_update",
    "rf_amd_filter_set_destroy_on",
    "rf_amd_range_map_create", "rf_amd_range_map_destroy", "rf_amd_range_map_destroy_on",
    "rf_amd_range_map_num_ranges", "rf_amd_range_map_max_list", "rf_amd_range_route_scratch_bytes",
    "rf_amd_range_map_route_keys", "rf_amd_range_map_route_var_keys",
    "rf_amd_diag_range_tile", "rf_amd_diag_range_lds_ranges",
    "rf_amd_range_map_create_segments", "rf_amd_range_map_num_segments", "rf_amd_range_map_update_segments",
    "rf_amd_diag_range_seg_launch_ids", "rf_amd_diag_range_seg_thread_ids",
    "rf_amd_range_map_create_segments_room", "rf_amd_range_map_split", "rf_amd_range_map_set_paths",
    "rf_amd_diag_range_splice_words",
    "rf_amd_found_per_key_scratch_bytes", "rf_amd_found_per_key", "rf_amd_found_per_key_ragged",
    "rf_amd_diag_per_key_tile",
    "rf_amd_filter_set_exists_keys", "rf_amd_filter_set_exists_var_keys", "rf_amd_filter_set_exists_hashes",
    "rf_amd_filter_set_exists_keys_ragged", "rf_amd_filter_set_exists_var_keys_ragged",
    "rf_amd_filter_set_exists_hashes_ragged",
    "rf_amd_found_by_branch_scratch_bytes", "rf_amd_found_by_branch",
    "rf_amd_diag_by_branch_tile", "rf_amd_diag_by_branch_passes",
    "rf_amd_found_advance_scratch_bytes", "rf_amd_found_advance",
]
ROUTE_MAX_WORLD = 16
FOUND_COMPACT_TILE = 4096  # found words per workgroup of rf_amd_found_compact (FC_TILE)
ASYNC_STATUS_RUNNING = 0  # src/platform_linux/async.h:137-140
ASYNC_STATUS_DONE = 1
CALLBACK_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p)


class PlatformStatusError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"platform_status {code}: {msg}")
        self.code = code


class RfConfig(ctypes.Structure):
    _fields_ = [("fingerprint_size", ctypes.c_uint32), ("log_index_size", ctypes.c_uint32),
                ("seed", ctypes.c_uint32), ("page_size", ctypes.c_uint32),
                ("pages_per_extent", ctypes.c_uint32)]


class RfFilterInfo(ctypes.Structure):
    _fields_ = [("num_fingerprints", ctypes.c_uint32), ("num_unique", ctypes.c_uint32),
                ("value_size", ctypes.c_uint32), ("num_indices", ctypes.c_uint32),
                ("num_pages", ctypes.c_uint32), ("error", ctypes.c_uint32)]


class RfImage(ctypes.Structure):
    _fields_ = [("info", RfFilterInfo), ("pages", ctypes.POINTER(ctypes.c_uint8)),
                ("slots", ctypes.POINTER(ctypes.c_uint64))]


class RangeRoom(ctypes.Structure):
    """rf_amd_range_room: what a range map that follows splits may grow to"""
    _fields_ = [("ranges", ctypes.c_uint32), ("bound_bytes", ctypes.c_uint64),
                ("path_entries", ctypes.c_uint64), ("list_ids", ctypes.c_uint64),
                ("max_list", ctypes.c_uint32)]


_lib = None


def check_build_id(L, path):
    """a library built from other sources than the tree's (a stale prebuilt .so, e.g. the
    diagnostics build left behind by an earlier round) fails loudly instead of running"""
    from . import build as _b
    L.rf_amd_build_id.restype = ctypes.c_char_p
    got = L.rf_amd_build_id().decode()
    try:
        want = _b.source_id()
    except OSError:  # sources absent: nothing to compare with
        return
    if got != want:
        raise RuntimeError(f"{path} was built from other sources (build id {got}, tree {want}): "
                           "rebuild it (python -c 'import __graft_entry__ as g; g.build()')")


def load_library(build_if_missing=True):
    """Load librf_amd.so (building it in-tree with hipcc if absent)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("RF_AMD_LIB", LIB_PATH)  # e.g. the phase-stamp diagnostics build
    if not os.path.exists(path):
        if not build_if_missing or path != LIB_PATH:
            raise PlatformStatusError(STATUS_NO_DEVICE, f"{path} missing (run build)")
        from . import build as _b
        _b.build()
    L = ctypes.CDLL(path)
    check_build_id(L, path)
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    L.rf_amd_last_error.restype = ctypes.c_char_p
    L.rf_amd_engine_create.argtypes = [i32, ctypes.POINTER(vp)]
    L.rf_amd_engine_destroy.argtypes = [vp]
    L.rf_amd_engine_destroy.restype = None
    L.rf_amd_batch_create.argtypes = [vp, ctypes.POINTER(RfConfig), u32, vp, vp, vp, vp,
                                      ctypes.POINTER(vp)]
    L.rf_amd_batch_create_runs.argtypes = [vp, ctypes.POINTER(RfConfig), u32, vp, vp, vp, vp, vp,
                                           ctypes.POINTER(vp)]
    L.rf_amd_batch_destroy.argtypes = [vp]
    L.rf_amd_batch_destroy.restype = None
    L.rf_amd_batch_build_keys.argtypes = [vp, vp, u32, vp]
    L.rf_amd_batch_build_var_keys.argtypes = [vp, vp, vp, vp]
    L.rf_amd_batch_build_hashes.argtypes = [vp, vp, vp]
    L.rf_amd_batch_probe_keys.argtypes = [vp, vp, u32, vp, u64, vp, vp]
    L.rf_amd_batch_probe_var_keys.argtypes = [vp, vp, vp, vp, u64, vp, vp]
    L.rf_amd_batch_probe_hashes.argtypes = [vp, vp, vp, u64, vp, vp]
    L.rf_amd_batch_probe_keys_runs.argtypes = [vp, vp, u32, ctypes.POINTER(u64), vp, vp]
    L.rf_amd_batch_probe_hashes_runs.argtypes = [vp, vp, ctypes.POINTER(u64), vp, vp]
    L.rf_amd_batch_info.argtypes = [vp, u32, ctypes.POINTER(RfFilterInfo)]
    L.rf_amd_batch_read_image.argtypes = [vp, u32, vp, u64, vp, u32]
    L.rf_amd_batch_read_image_async.argtypes = [vp, u32, vp, u64, vp, u32, vp]
    L.rf_amd_batch_image_ptrs.argtypes = [vp, u32, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.rf_amd_batch_set_timing.argtypes = [vp, i32]
    L.rf_amd_batch_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_float), u32]
    L.rf_amd_batch_timings_back.argtypes = [vp, u32, ctypes.POINTER(ctypes.c_float), u32]
    L.rf_amd_debug_read_lines.argtypes = [vp, vp, u64, ctypes.POINTER(u64)]
    L.rf_amd_debug_rebuild_lines.argtypes = [vp]
    L.rf_amd_debug_phase_buffer.argtypes = [vp, u32]
    L.rf_amd_debug_probe_floor.argtypes = [vp, vp, u32, vp, vp, vp]
    L.rf_amd_diag_lookup_stats.argtypes = [vp, ctypes.c_int]
    L.rf_amd_diag_lookup_paths.argtypes = [vp, ctypes.c_int]
    L.rf_amd_lookup_submit.argtypes = [vp, vp, u32, u32, vp, ctypes.POINTER(u64)]
    L.rf_amd_lookup_wait.argtypes = [vp, u64, ctypes.POINTER(u64)]
    L.rf_amd_lookup_reap.argtypes = [vp, vp, vp, u64]
    L.rf_amd_lookup_reap.restype = u64
    L.rf_amd_lookup_server_stats.argtypes = [vp, vp]
    L.rf_amd_lookup_server_error.argtypes = [vp]
    L.rf_amd_lookup_server_failed.argtypes = [vp, vp, u64]
    L.rf_amd_lookup_server_failed.restype = u64
    L.rf_amd_lookup_server_set_times.argtypes = [vp, u64, u64]
    L.rf_amd_diag_lookup_server_kill.argtypes = [vp, i32, u32]
    L.rf_amd_diag_lookup_ring.argtypes = [vp]
    L.rf_amd_diag_k4_bitmap_builds.argtypes = []
    L.rf_amd_diag_k4_bitmap_builds.restype = u64
    L.rf_amd_diag_dense_line_filters.argtypes = []
    L.rf_amd_diag_dense_line_filters.restype = u64
    L.rf_amd_diag_part16_builds.argtypes = []
    L.rf_amd_diag_part16_builds.restype = u64
    L.rf_amd_diag_k4_packed_builds.argtypes = []
    L.rf_amd_diag_k4_packed_builds.restype = u64
    L.rf_amd_batch_num_filters.argtypes = [vp]
    L.rf_amd_batch_num_filters.restype = u32
    L.rf_amd_filter_add.argtypes = [vp, ctypes.POINTER(RfConfig), ctypes.POINTER(RfImage),
                                    ctypes.POINTER(RfImage), vp, u64, ctypes.c_uint16]
    L.rf_amd_filter_add_runs.argtypes = [vp, ctypes.POINTER(RfConfig), ctypes.POINTER(RfImage),
                                         ctypes.POINTER(RfImage), vp, vp, vp, u32]
    L.rf_amd_filter_lookup_hashes.argtypes = [vp, ctypes.POINTER(RfConfig),
                                              ctypes.POINTER(RfImage), vp, u64, vp]
    L.rf_amd_filter_lookup_keys.argtypes = [vp, ctypes.POINTER(RfConfig), ctypes.POINTER(RfImage),
                                            vp, u32, u64, vp]
    L.rf_amd_image_free.argtypes = [ctypes.POINTER(RfImage)]
    L.rf_amd_image_free.restype = None
    L.rf_amd_max_fingerprints.argtypes = [ctypes.POINTER(RfConfig)]
    L.rf_amd_max_fingerprints.restype = u64
    L.rf_amd_estimate_unique_keys_from_count.argtypes = [ctypes.POINTER(RfConfig), u64]
    L.rf_amd_estimate_unique_keys_from_count.restype = u32
    L.rf_amd_space_use_bytes.argtypes = [ctypes.POINTER(RfConfig), u32]
    L.rf_amd_space_use_bytes.restype = u64
    L.rf_amd_estimate_unique_fp.argtypes = [vp, ctypes.POINTER(RfConfig), vp, u64,
                                            ctypes.POINTER(u32)]
    L.rf_amd_batch_estimate_unique_fp.argtypes = [vp, vp, u64, ctypes.POINTER(u32)]
    L.rf_amd_estimate_unique_keys.argtypes = [ctypes.POINTER(RfFilterInfo), ctypes.POINTER(RfConfig)]
    L.rf_amd_estimate_unique_keys.restype = u32
    L.rf_amd_lookup_async.argtypes = [vp, vp, u32, vp, u64, vp, CALLBACK_FN, vp, vp,
                                      ctypes.POINTER(vp)]
    L.rf_amd_lookup_async_poll.argtypes = [vp]
    L.rf_amd_lookup_async_wait.argtypes = [vp]
    L.rf_amd_lookup_async_free.argtypes = [vp]
    L.rf_amd_lookup_async_free.restype = None
    L.rf_amd_filter_verify.argtypes = [vp, ctypes.POINTER(RfConfig), ctypes.POINTER(RfImage), vp, u32,
                                       u64, ctypes.c_uint16, ctypes.POINTER(u64)]
    L.rf_amd_filter_print.argtypes = [ctypes.POINTER(RfConfig), ctypes.POINTER(RfImage), vp]
    L.rf_amd_hash_keys.argtypes = [vp, ctypes.POINTER(RfConfig), vp, u32, u64, vp, vp]
    L.rf_amd_hash_var_keys.argtypes = [vp, ctypes.POINTER(RfConfig), vp, vp, u64, vp, vp]
    L.rf_amd_batch_export.argtypes = [vp, vp, u64, vp, u64, vp]
    L.rf_amd_batch_import.argtypes = [vp, ctypes.POINTER(RfConfig), u32, ctypes.POINTER(RfFilterInfo), vp, vp,
                                      i32, ctypes.POINTER(vp)]
    L.rf_amd_route_scratch_bytes.argtypes = [u64, u32]
    L.rf_amd_route_scratch_bytes.restype = u64
    L.rf_amd_route_probes.argtypes = [vp, vp, vp, u64, vp, u32, u32, vp, vp, vp, ctypes.POINTER(u64), vp]
    L.rf_amd_batch_probe_pairs.argtypes = [vp, vp, u64, vp, vp]
    L.rf_amd_unroute_found.argtypes = [vp, vp, vp, u64, vp, vp]
    L.rf_amd_batch_build_hashes_host.argtypes = [vp, vp]
    L.rf_amd_batch_probe_hashes_host.argtypes = [vp, vp, vp, u64, vp]
    L.rf_amd_engine_pool_stats.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.rf_amd_filter_print_abs.argtypes = [ctypes.POINTER(RfConfig), ctypes.POINTER(RfImage), u64, vp, vp]
    L.rf_amd_batch_infos.argtypes = [vp, ctypes.POINTER(RfFilterInfo), vp]
    L.rf_amd_batch_destroy_on.argtypes = [vp, vp]
    L.rf_amd_probe_many_hashes_host.argtypes = [vp, vp, vp, vp, u32, vp, vp]
    L.rf_amd_probe_filters_host.argtypes = [vp, vp, vp, u32, vp, vp, u64, vp]
    L.rf_amd_engine_pool_trim.argtypes = [vp, u64]
    L.rf_amd_engine_stream.argtypes = [vp]
    L.rf_amd_engine_stream.restype = vp
    L.rf_amd_engine_sync.argtypes = [vp]
    L.rf_amd_batch_device_bytes.argtypes = [vp]
    L.rf_amd_batch_device_bytes.restype = u64
    L.rf_amd_batch_trim.argtypes = [vp, vp]
    L.rf_amd_batch_stage_begin.argtypes = [vp, ctypes.POINTER(vp)]
    L.rf_amd_batch_stage_build.argtypes = [vp]
    L.rf_amd_batch_stage_abort.argtypes = [vp]
    L.rf_amd_batch_stage_abort.restype = None
    L.rf_amd_filter_set_create.argtypes = [vp, vp, vp, u32, ctypes.POINTER(vp)]
    L.rf_amd_filter_set_destroy.argtypes = [vp]
    L.rf_amd_filter_set_destroy.restype = None
    L.rf_amd_filter_set_num_members.argtypes = [vp]
    L.rf_amd_filter_set_num_members.restype = u32
    L.rf_amd_filter_set_create_cap.argtypes = [vp, vp, vp, u32, u32, ctypes.POINTER(vp)]
    L.rf_amd_filter_set_capacity.argtypes = [vp]
    L.rf_amd_filter_set_capacity.restype = u32
    L.rf_amd_filter_set_update.argtypes = [vp, vp, vp, vp, u32, vp]
    L.rf_amd_filter_set_destroy_on.argtypes = [vp, vp]
    L.rf_amd_filter_set_probe_keys.argtypes = [vp, vp, u32, vp, u32, u64, vp, vp]
    L.rf_amd_filter_set_probe_hashes.argtypes = [vp, vp, vp, u32, u64, vp, vp]
    L.rf_amd_found_compact_scratch_bytes.argtypes = [u64]
    L.rf_amd_found_compact_scratch_bytes.restype = u64
    L.rf_amd_found_compact.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp]
    L.rf_amd_filter_set_probe_var_keys.argtypes = [vp, vp, vp, vp, u32, u64, vp, vp]
    L.rf_amd_batch_probe_var_keys_runs.argtypes = [vp, vp, vp, ctypes.POINTER(u64), vp, vp]
    L.rf_amd_filter_lookup_var_keys.argtypes = [vp, ctypes.POINTER(RfConfig), ctypes.POINTER(RfImage),
                                                vp, vp, u64, vp]
    L.rf_amd_filter_set_probe_keys_ragged.argtypes = [vp, vp, u32, vp, vp, u64, vp, vp]
    L.rf_amd_filter_set_probe_var_keys_ragged.argtypes = [vp, vp, vp, vp, vp, u64, vp, vp]
    L.rf_amd_filter_set_probe_hashes_ragged.argtypes = [vp, vp, vp, vp, u64, vp, vp]
    L.rf_amd_filter_set_exists_keys.argtypes = L.rf_amd_filter_set_probe_keys.argtypes
    L.rf_amd_filter_set_exists_hashes.argtypes = L.rf_amd_filter_set_probe_hashes.argtypes
    L.rf_amd_filter_set_exists_var_keys.argtypes = L.rf_amd_filter_set_probe_var_keys.argtypes
    L.rf_amd_filter_set_exists_keys_ragged.argtypes = L.rf_amd_filter_set_probe_keys_ragged.argtypes
    L.rf_amd_filter_set_exists_var_keys_ragged.argtypes = L.rf_amd_filter_set_probe_var_keys_ragged.argtypes
    L.rf_amd_filter_set_exists_hashes_ragged.argtypes = L.rf_amd_filter_set_probe_hashes_ragged.argtypes
    L.rf_amd_diag_fanout_max_blocks.argtypes = [u32]
    L.rf_amd_range_map_create.argtypes = [vp, u32, vp, vp, vp, vp, ctypes.POINTER(vp)]
    L.rf_amd_range_map_destroy.argtypes = [vp]
    L.rf_amd_range_map_destroy.restype = None
    L.rf_amd_range_map_destroy_on.argtypes = [vp, vp]
    L.rf_amd_range_map_num_ranges.argtypes = [vp]
    L.rf_amd_range_map_num_ranges.restype = u32
    L.rf_amd_range_map_max_list.argtypes = [vp]
    L.rf_amd_range_map_max_list.restype = u32
    L.rf_amd_range_route_scratch_bytes.argtypes = [u64]
    L.rf_amd_range_route_scratch_bytes.restype = u64
    L.rf_amd_range_map_route_keys.argtypes = [vp, vp, u32, u64, vp, vp, vp, u64, vp, vp, vp]
    L.rf_amd_range_map_route_var_keys.argtypes = [vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp]
    L.rf_amd_diag_range_tile.argtypes = []
    L.rf_amd_diag_range_tile.restype = u32
    L.rf_amd_diag_range_lds_ranges.argtypes = []
    L.rf_amd_diag_range_lds_ranges.restype = u32
    L.rf_amd_range_map_create_segments.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, ctypes.POINTER(vp)]
    L.rf_amd_range_map_num_segments.argtypes = [vp]
    L.rf_amd_range_map_num_segments.restype = u32
    L.rf_amd_range_map_update_segments.argtypes = [vp, vp, vp, vp, u32, vp]
    L.rf_amd_diag_range_seg_launch_ids.argtypes = []
    L.rf_amd_diag_range_seg_launch_ids.restype = u32
    L.rf_amd_diag_range_seg_thread_ids.argtypes = []
    L.rf_amd_diag_range_seg_thread_ids.restype = u32
    L.rf_amd_range_map_create_segments_room.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp, vp, vp,
                                                        ctypes.POINTER(RangeRoom), ctypes.POINTER(vp)]
    L.rf_amd_range_map_split.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp]
    L.rf_amd_range_map_set_paths.argtypes = [vp, u32, u32, vp, vp, vp]
    L.rf_amd_diag_range_splice_words.argtypes = []
    L.rf_amd_diag_range_splice_words.restype = u32
    L.rf_amd_found_per_key_scratch_bytes.argtypes = [u64]
    L.rf_amd_found_per_key_scratch_bytes.restype = u64
    L.rf_amd_found_per_key.argtypes = [vp, vp, vp, u32, u64, vp, vp, vp, u64, vp, vp, vp]
    L.rf_amd_found_per_key_ragged.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp]
    L.rf_amd_diag_per_key_tile.argtypes = []
    L.rf_amd_diag_per_key_tile.restype = u32
    L.rf_amd_found_by_branch_scratch_bytes.argtypes = [u64, u32]
    L.rf_amd_found_by_branch_scratch_bytes.restype = u64
    L.rf_amd_found_by_branch.argtypes = [vp, vp, vp, vp, u64, u32, vp, vp, vp, vp, u64, vp, vp, vp]
    L.rf_amd_diag_by_branch_tile.argtypes = []
    L.rf_amd_diag_by_branch_tile.restype = u32
    L.rf_amd_diag_by_branch_passes.argtypes = [u32]
    L.rf_amd_diag_by_branch_passes.restype = u32
    L.rf_amd_found_advance_scratch_bytes.argtypes = [u64]
    L.rf_amd_found_advance_scratch_bytes.restype = u64
    L.rf_amd_found_advance.argtypes = [vp, vp, vp, u64, u64, u32, u32, vp, vp, vp, vp, u64, vp, vp, vp]
    L.rf_amd_host_alloc.argtypes = [vp, u64, ctypes.POINTER(vp)]
    L.rf_amd_host_free.argtypes = [vp, vp]
    L.rf_amd_host_free.restype = None
    L.rf_amd_batch_place_image.argtypes = [vp, u32, vp, u32, u32, u32, i32, u32, vp]
    L.rf_amd_host_register.argtypes = [vp, vp, u64]
    L.rf_amd_host_unregister.argtypes = [vp, vp]
    L.rf_amd_engine_fence.argtypes = [vp, ctypes.POINTER(u64)]
    L.rf_amd_engine_fence_wait.argtypes = [vp, u64]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise PlatformStatusError(rc, load_library().rf_amd_last_error().decode())


# ---- routing_config (src/routing_filter.h:32-58) --------------------------------------
@dataclass
class RoutingConfig:
    fingerprint_size: int = 26
    log_index_size: int = 8
    seed: int = 42
    page_size: int = 4096
    pages_per_extent: int = 32

    @property
    def index_size(self):
        return 1 << self.log_index_size

    def c(self):
        return RfConfig(self.fingerprint_size, self.log_index_size, self.seed, self.page_size,
                        self.pages_per_extent)


def routing_config_init(fingerprint_size=26, log_index_size=8, seed=42, page_size=4096,
                        pages_per_extent=32):
    """routing_config_init (src/routing_filter.h:42-58); the key_hash argument of the
    reference is ignored there too -- hashing is XXH32 with `seed`."""
    return RoutingConfig(fingerprint_size, log_index_size, seed, page_size, pages_per_extent)


class Engine:
    """One HIP device + stream. Raises PlatformStatusError(ENODEV) without a GPU."""

    def __init__(self, device=0):
        L = load_library()
        h = ctypes.c_void_p()
        _check(L.rf_amd_engine_create(device, ctypes.byref(h)))
        self.h = h
        self.device = device

    def pool_stats(self):
        """device-memory pool of the engine's batches: bytes held, hits, misses"""
        v = [ctypes.c_uint64() for _ in range(3)]
        _check(load_library().rf_amd_engine_pool_stats(self.h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("pooled_bytes", "hits", "misses"), (x.value for x in v)))

    def close(self):
        if self.h:
            load_library().rf_amd_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_engine = None


def default_engine():
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine(0)
    return _default_engine


# ---- routing_filter descriptor + image -----------------------------------------------
@dataclass
class RoutingFilter:
    """routing_filter (src/routing_filter.h:66-72) plus its relocatable page image:
    pages = num_pages * page_size bytes, slots[i] = data_page_no * page_size + offset."""
    num_fingerprints: int
    num_unique: int
    value_size: int
    num_indices: int
    num_pages: int
    pages: np.ndarray
    slots: np.ndarray

    def _c(self):
        img = RfImage()
        img.info = RfFilterInfo(self.num_fingerprints, self.num_unique, self.value_size,
                                self.num_indices, self.num_pages, 0)
        self._pages_c = np.ascontiguousarray(self.pages, dtype=np.uint8)
        self._slots_c = np.ascontiguousarray(self.slots, dtype=np.uint64)
        img.pages = self._pages_c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        img.slots = self._slots_c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        return img


NULL_ROUTING_FILTER = None


def routing_filter_add(cfg: RoutingConfig, old_filter, new_fp_arr, value=0, engine=None):
    """routing_filter_add (src/routing_filter.h:78-85): 32-bit key hashes in, new filter
    out. new_fp_arr is not modified (the reference shifts/sorts it in place)."""
    eng = engine or default_engine()
    L = load_library()
    fps = np.ascontiguousarray(new_fp_arr, dtype=np.uint32)
    out = RfImage()
    old_c = old_filter._c() if old_filter is not None else None
    _check(L.rf_amd_filter_add(eng.h, ctypes.byref(cfg.c()),
                               ctypes.byref(old_c) if old_c is not None else None,
                               ctypes.byref(out), fps.ctypes.data if fps.size else None,
                               fps.size, value))
    try:
        info = out.info
        npg = info.num_pages * cfg.page_size
        pages = np.ctypeslib.as_array(out.pages, shape=(npg,)).copy()
        slots = np.ctypeslib.as_array(out.slots, shape=(info.num_indices,)).copy()
    finally:
        L.rf_amd_image_free(ctypes.byref(out))
    return RoutingFilter(info.num_fingerprints, info.num_unique, info.value_size,
                         info.num_indices, info.num_pages, pages, slots)


def _image_out(L, cfg, out):
    """an rf_amd_image the library allocated, copied into a RoutingFilter and freed"""
    try:
        info = out.info
        npg = info.num_pages * cfg.page_size
        pages = np.ctypeslib.as_array(out.pages, shape=(npg,)).copy()
        slots = np.ctypeslib.as_array(out.slots, shape=(info.num_indices,)).copy()
    finally:
        L.rf_amd_image_free(ctypes.byref(out))
    return RoutingFilter(info.num_fingerprints, info.num_unique, info.value_size,
                         info.num_indices, info.num_pages, pages, slots)


def routing_filter_add_runs(cfg: RoutingConfig, old_filter, fp_arrs, values, engine=None):
    """A chain of routing_filter_add calls in one build (rf_amd_filter_add_runs): run j adds the
    32-bit key hashes fp_arrs[j] with values[j] (strictly increasing) onto the result of run
    j - 1, run 0 onto old_filter (or None). Returns the chain's last filter -- the one
    maplet_compaction_task (src/trunk.c:3815-3868) keeps."""
    eng = engine or default_engine()
    L = load_library()
    fps = [np.ascontiguousarray(a, dtype=np.uint32) for a in fp_arrs]
    k = len(fps)
    ptrs = (ctypes.c_void_p * max(1, k))(*[(a.ctypes.data if a.size else None) for a in fps])
    lens = np.ascontiguousarray([a.size for a in fps], dtype=np.uint64)
    vals = np.ascontiguousarray(values, dtype=np.uint16)
    if vals.size != k:
        raise PlatformStatusError(STATUS_BAD_PARAM, "one value per run")
    out = RfImage()
    old_c = old_filter._c() if old_filter is not None else None
    _check(L.rf_amd_filter_add_runs(eng.h, ctypes.byref(cfg.c()),
                                    ctypes.byref(old_c) if old_c is not None else None,
                                    ctypes.byref(out), ctypes.cast(ptrs, ctypes.c_void_p), lens.ctypes.data,
                                    vals.ctypes.data, k))
    return _image_out(L, cfg, out)


def routing_filter_lookup_hashes(cfg: RoutingConfig, filt, hashes, engine=None):
    eng = engine or default_engine()
    L = load_library()
    h = np.ascontiguousarray(hashes, dtype=np.uint32)
    out = np.zeros(h.size, dtype=np.uint64)
    fc = filt._c() if filt is not None else None
    _check(L.rf_amd_filter_lookup_hashes(eng.h, ctypes.byref(cfg.c()),
                                         ctypes.byref(fc) if fc is not None else None,
                                         h.ctypes.data, h.size, out.ctypes.data))
    return out


def routing_filter_lookup_keys(cfg: RoutingConfig, filt, keys: np.ndarray, engine=None):
    """Fixed-length keys (n x key_len uint8) hashed and probed on the GPU."""
    eng = engine or default_engine()
    L = load_library()
    k = np.ascontiguousarray(keys, dtype=np.uint8)
    if k.ndim == 1:
        k = k.reshape(1, -1)
    out = np.zeros(k.shape[0], dtype=np.uint64)
    fc = filt._c() if filt is not None else None
    _check(L.rf_amd_filter_lookup_keys(eng.h, ctypes.byref(cfg.c()),
                                       ctypes.byref(fc) if fc is not None else None,
                                       k.ctypes.data, k.shape[1], k.shape[0], out.ctypes.data))
    return out


def routing_filter_lookup_var_keys(cfg: RoutingConfig, filt, data, offs, engine=None):
    """Variable-length keys in host memory, key i = data[offs[i]:offs[i+1]] (n + 1 offsets),
    hashed and probed on the GPU; only data[offs[0]:offs[n]] is copied in."""
    eng = engine or default_engine()
    L = load_library()
    d = np.ascontiguousarray(data, dtype=np.uint8)
    o = np.ascontiguousarray(offs, dtype=np.uint64)
    n = max(o.size - 1, 0)
    out = np.zeros(n, dtype=np.uint64)
    fc = filt._c() if filt is not None else None
    _check(L.rf_amd_filter_lookup_var_keys(eng.h, ctypes.byref(cfg.c()),
                                           ctypes.byref(fc) if fc is not None else None,
                                           d.ctypes.data, o.ctypes.data, n, out.ctypes.data))
    return out


def routing_filter_lookup(cfg: RoutingConfig, filt, key: bytes, engine=None):
    """routing_filter_lookup (src/routing_filter.h:87-92) for one key; returns found_values."""
    arr = np.frombuffer(bytes(key), dtype=np.uint8)
    return int(routing_filter_lookup_keys(cfg, filt, arr, engine)[0])


def _c_int_shl1(v: int) -> int:
    """`1 << v` on a 32-bit C int as the reference's x86-64 build evaluates it, widened to
    uint64: the shift count is taken mod 32 (`shl %cl`), and 1 << 31 is INT_MIN, which
    sign-extends. (Values >= 31 are UB in C; this is the code gcc emits for them.)"""
    sh = v & 31
    return 0xFFFFFFFF80000000 if sh == 31 else 1 << sh


def routing_filter_get_next_value(found_values: int, last_value: int) -> int:
    """src/routing_filter.h:94-105: `uint64 mask = (1 << last_value) - 1` is int arithmetic
    (INT_MIN - 1 wraps to INT_MAX), so last_value >= 31 does not mask the way a 64-bit
    shift would."""
    if last_value != ROUTING_NOT_FOUND:
        m = _c_int_shl1(last_value)
        mask = 0x7FFFFFFF if m == 0xFFFFFFFF80000000 else m - 1
        found_values &= mask
    if found_values == 0:
        return ROUTING_NOT_FOUND
    return found_values.bit_length() - 1


def routing_filter_is_value_found(found_values: int, value: int) -> bool:
    """src/routing_filter.h:107-111: `found_values & (1 << value)` with an int shift."""
    return (found_values & _c_int_shl1(value)) != 0


def routing_filter_max_fingerprints(cfg: RoutingConfig) -> int:
    return load_library().rf_amd_max_fingerprints(ctypes.byref(cfg.c()))


def routing_filter_estimate_unique_keys_from_count(cfg: RoutingConfig, num_unique: int) -> int:
    return load_library().rf_amd_estimate_unique_keys_from_count(ctypes.byref(cfg.c()), num_unique)


def routing_filter_estimate_unique_keys(filt: RoutingFilter, cfg: RoutingConfig) -> int:
    """src/routing_filter.h:165-167, .c:1141-1146."""
    info = RfFilterInfo(filt.num_fingerprints, filt.num_unique, filt.value_size,
                        filt.num_indices, filt.num_pages, 0)
    return load_library().rf_amd_estimate_unique_keys(ctypes.byref(info), ctypes.byref(cfg.c()))


def routing_filter_estimate_unique_fp(cfg: RoutingConfig, filters, engine=None) -> int:
    """routing_filter_estimate_unique_fp (src/routing_filter.h:169-175, .c:702-848) over
    host images; None entries are NULL_ROUTING_FILTER. Returns num_unique_fp."""
    eng = engine or default_engine()
    arr = (RfImage * max(1, len(filters)))()
    keep = []
    for i, f in enumerate(filters):
        if f is None:
            arr[i] = RfImage()
        else:
            arr[i] = f._c()
            keep.append(f)
    out = ctypes.c_uint32(0)
    _check(load_library().rf_amd_estimate_unique_fp(eng.h, ctypes.byref(cfg.c()), ctypes.addressof(arr),
                                                    len(filters), ctypes.byref(out)))
    return out.value


def batch_estimate_unique_fp(members) -> int:
    """estimate_unique_fp over device-resident filters: members = [(FilterBatch, f) or None]."""
    n = len(members)
    hs = (ctypes.c_void_p * max(1, n))()
    idx = np.zeros(max(1, n), dtype=np.uint32)
    for i, m in enumerate(members):
        if m is not None:
            hs[i] = m[0].h.value
            idx[i] = m[1]
    out = ctypes.c_uint32(0)
    _check(load_library().rf_amd_batch_estimate_unique_fp(ctypes.addressof(hs), idx.ctypes.data, n,
                                                          ctypes.byref(out)))
    return out.value


def routing_filter_verify(cfg: RoutingConfig, filt, keys: np.ndarray, value: int, engine=None) -> int:
    """routing_filter_verify (src/routing_filter.c:1163-1183) over fixed-length keys: raises
    PlatformStatusError(EINVAL) if a key does not find `value` (the reference asserts)."""
    eng = engine or default_engine()
    k = np.ascontiguousarray(keys, dtype=np.uint8)
    if k.ndim == 1:
        k = k.reshape(1, -1)
    missing = ctypes.c_uint64(0)
    fc = filt._c() if filt is not None else None
    rc = load_library().rf_amd_filter_verify(eng.h, ctypes.byref(cfg.c()),
                                             ctypes.byref(fc) if fc is not None else None,
                                             k.ctypes.data, k.shape[1], k.shape[0], value,
                                             ctypes.byref(missing))
    if rc:
        err = PlatformStatusError(rc, load_library().rf_amd_last_error().decode())
        err.num_missing = missing.value
        raise err
    return 0


def routing_filter_print(cfg: RoutingConfig, filt, path=None) -> str:
    """routing_filter_print (src/routing_filter.c:1260-1286); returns the text."""
    import tempfile
    libc = ctypes.CDLL(None)
    libc.fopen.restype = ctypes.c_void_p
    libc.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    libc.fclose.argtypes = [ctypes.c_void_p]
    fd, tmp = tempfile.mkstemp(suffix=".txt")
    os.close(fd)
    fh = libc.fopen((path or tmp).encode(), b"w")
    try:
        fc = filt._c()
        _check(load_library().rf_amd_filter_print(ctypes.byref(cfg.c()), ctypes.byref(fc), fh))
    finally:
        libc.fclose(fh)
    with open(path or tmp) as t:
        text = t.read()
    os.unlink(tmp)
    return text


def hash_keys(cfg: RoutingConfig, d_keys, key_len, n, d_hashes, stream=None, engine=None):
    """XXH32 of n device-resident fixed-length keys (data_key_hash) into d_hashes, on the GPU."""
    eng = engine or default_engine()
    _check(load_library().rf_amd_hash_keys(eng.h, ctypes.byref(cfg.c()), _dptr(d_keys), key_len, n,
                                           _dptr(d_hashes), _stream(stream)))


def hash_var_keys(cfg: RoutingConfig, d_bytes, d_offsets, n, d_hashes, stream=None, engine=None):
    eng = engine or default_engine()
    _check(load_library().rf_amd_hash_var_keys(eng.h, ctypes.byref(cfg.c()), _dptr(d_bytes), _dptr(d_offsets), n,
                                               _dptr(d_hashes), _stream(stream)))


def route_scratch_bytes(n, world):
    return int(load_library().rf_amd_route_scratch_bytes(n, world))


def route_probes(d_hashes, d_filter_id, n, d_route, num_filters, world, d_pairs, d_perm, d_scratch,
                 stream=None, engine=None):
    """Stable partition of n probes by owning rank (rf_amd_route_probes); returns the
    per-rank pair counts (list of `world` ints)."""
    eng = engine or default_engine()
    counts = (ctypes.c_uint64 * max(1, world))()
    _check(load_library().rf_amd_route_probes(eng.h, _dptr(d_hashes), _dptr(d_filter_id), n, _dptr(d_route),
                                              num_filters, world, _dptr(d_pairs), _dptr(d_perm),
                                              _dptr(d_scratch), counts, _stream(stream)))
    return [int(c) for c in counts[:world]]


def unroute_found(d_back, d_perm, n, d_found, stream=None, engine=None):
    eng = engine or default_engine()
    _check(load_library().rf_amd_unroute_found(eng.h, _dptr(d_back), _dptr(d_perm), n, _dptr(d_found),
                                               _stream(stream)))


class LookupAsync:
    """routing_filter_lookup_async (src/routing_filter.h:130-155) for a batch of host keys
    against a built FilterBatch: poll() returns ASYNC_STATUS_RUNNING / ASYNC_STATUS_DONE;
    callback() (optional, no arguments) runs once the results are in `found`."""

    def __init__(self, batch, keys: np.ndarray, filter_id=None, callback=None, stream=None):
        k = np.ascontiguousarray(keys, dtype=np.uint8)
        if k.ndim == 1:
            k = k.reshape(1, -1)
        self.found = np.zeros(k.shape[0], dtype=np.uint64)
        self._fid = None if filter_id is None else np.ascontiguousarray(filter_id, dtype=np.uint32)
        self._cb = CALLBACK_FN(lambda _arg: callback()) if callback else CALLBACK_FN()
        self.batch = batch
        self.h = ctypes.c_void_p()
        _check(load_library().rf_amd_lookup_async(
            batch.h, k.ctypes.data, k.shape[1], None if self._fid is None else self._fid.ctypes.data,
            k.shape[0], self.found.ctypes.data, self._cb, None, stream, ctypes.byref(self.h)))

    def poll(self) -> int:
        return load_library().rf_amd_lookup_async_poll(self.h)

    def wait(self) -> np.ndarray:
        _check(load_library().rf_amd_lookup_async_wait(self.h))
        return self.found

    def close(self):
        if self.h:
            load_library().rf_amd_lookup_async_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def routing_filter_space_use_bytes(cfg: RoutingConfig, filt: RoutingFilter) -> int:
    if filt is None:
        return 0
    return load_library().rf_amd_space_use_bytes(ctypes.byref(cfg.c()), filt.num_pages)


# ---- batched device-resident engine -----------------------------------------------------
def _stream(stream):
    """The caller's stream: explicit handle, else torch's current stream when torch has a
    live HIP context and uses a non-default stream, else None (the engine's blocking
    stream, which is ordered with the legacy null stream)."""
    if stream is not None:
        return stream
    import sys
    t = sys.modules.get("torch")
    if t is not None and t.cuda.is_initialized():
        h = t.cuda.current_stream().cuda_stream
        return h or None
    return None


def _hptr(x):
    """Address of a numpy array, torch tensor or int."""
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return _dptr(x)


def _dptr(x):
    """Device pointer of a torch tensor (or an int address)."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    return x.data_ptr()


class FilterBatch:
    """F independent filters built in one launch sequence on the device.

    num_new[f] inputs feed filter f (runs concatenated in filter order); old=[(batch, i)
    or None] merges a previously built filter (incremental routing_filter_add)."""

    def __init__(self, cfg: RoutingConfig, num_new, values=None, old=None, engine=None):
        self.engine = engine or default_engine()
        self.cfg = cfg
        L = load_library()
        nn = np.ascontiguousarray(num_new, dtype=np.uint32)
        self.F = nn.size
        vals = np.ascontiguousarray(values if values is not None else np.zeros(self.F),
                                    dtype=np.uint16)
        self.num_new = nn
        self.values = vals
        self._keep = [nn, vals]
        ob_arr = oi_arr = None
        if old is not None:
            ob_arr = (ctypes.c_void_p * self.F)(*[(o[0].h.value if o else None) for o in old])
            oi_arr = np.ascontiguousarray([(o[1] if o else 0) for o in old], dtype=np.uint32)
            self._keep += [ob_arr, oi_arr, [o[0] for o in old if o]]
        h = ctypes.c_void_p()
        _check(L.rf_amd_batch_create(self.engine.h, ctypes.byref(cfg.c()), self.F,
                                     nn.ctypes.data, vals.ctypes.data,
                                     ctypes.cast(ob_arr, ctypes.c_void_p) if ob_arr is not None else None,
                                     oi_arr.ctypes.data if oi_arr is not None else None,
                                     ctypes.byref(h)))
        self.h = h

    @classmethod
    def chained(cls, cfg: RoutingConfig, runs, old=None, engine=None):
        """A chained batch (rf_amd_batch_create_runs): filter f is the end of the chain of
        routing_filter_add calls runs[f] = [(count, value), ...] (values strictly increasing),
        onto old[f] = (batch, i) or None, built in one build. The build calls take the inputs
        concatenated filter-major, run-minor."""
        self = cls.__new__(cls)
        self.engine = engine or default_engine()
        self.cfg = cfg
        self.F = len(runs)
        nr = np.ascontiguousarray([len(r) for r in runs], dtype=np.uint32)
        rl = np.ascontiguousarray([c for r in runs for c, _ in r], dtype=np.uint32)
        rv = np.ascontiguousarray([v for r in runs for _, v in r], dtype=np.uint16)
        self.num_new = np.array([sum(c for c, _ in r) for r in runs], dtype=np.uint32)
        self.values = np.array([(r[-1][1] if len(r) else 0) for r in runs], dtype=np.uint16)
        self._keep = [nr, rl, rv]
        ob_arr = oi_arr = None
        if old is not None:
            ob_arr = (ctypes.c_void_p * self.F)(*[(o[0].h.value if o else None) for o in old])
            oi_arr = np.ascontiguousarray([(o[1] if o else 0) for o in old], dtype=np.uint32)
            self._keep += [ob_arr, oi_arr, [o[0] for o in old if o]]
        h = ctypes.c_void_p()
        _check(load_library().rf_amd_batch_create_runs(
            self.engine.h, ctypes.byref(cfg.c()), self.F, nr.ctypes.data, rl.ctypes.data, rv.ctypes.data,
            ctypes.cast(ob_arr, ctypes.c_void_p) if ob_arr is not None else None,
            oi_arr.ctypes.data if oi_arr is not None else None, ctypes.byref(h)))
        self.h = h
        return self

    @classmethod
    def imported(cls, cfg: RoutingConfig, infos, d_pages, d_slots, device_resident=True, engine=None):
        """A built, probe-only batch from packed images (rf_amd_batch_import); infos: one
        RfFilterInfo per filter."""
        self = cls.__new__(cls)
        self.engine = engine or default_engine()
        self.cfg = cfg
        self.F = len(infos)
        arr = (RfFilterInfo * max(1, self.F))(*infos)
        self._keep = [arr]
        h = ctypes.c_void_p()
        _check(load_library().rf_amd_batch_import(self.engine.h, ctypes.byref(cfg.c()), self.F, arr,
                                                  _hptr(d_pages), _hptr(d_slots), 1 if device_resident else 0,
                                                  ctypes.byref(h)))
        self.h = h
        return self

    def export(self, d_pages, d_slots, stream=None):
        """Pack every filter's pages and slots (device tensors sized by export_sizes())."""
        _check(load_library().rf_amd_batch_export(self.h, _dptr(d_pages), d_pages.numel() * d_pages.element_size(),
                                                  _dptr(d_slots), d_slots.numel(), _stream(stream)))

    def export_sizes(self):
        """(infos, total page bytes, total index slots) of the packed export."""
        infos = [self.info(f) for f in range(self.F)]
        return infos, sum(i.num_pages for i in infos) * self.cfg.page_size, sum(i.num_indices for i in infos)

    def close(self, stream=None):
        """release the batch; with `stream`, stream-ordered (rf_amd_batch_destroy_on: every
        use of the batch must be ordered before the stream's current end), else after a
        device synchronisation"""
        if getattr(self, "h", None):
            if stream is not None:
                _check(load_library().rf_amd_batch_destroy_on(self.h, _stream(stream)))
            else:
                load_library().rf_amd_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def build_keys(self, d_keys, key_len, stream=None):
        _check(load_library().rf_amd_batch_build_keys(self.h, _dptr(d_keys), key_len, _stream(stream)))

    def build_var_keys(self, d_bytes, d_offsets, stream=None):
        _check(load_library().rf_amd_batch_build_var_keys(self.h, _dptr(d_bytes), _dptr(d_offsets),
                                                          _stream(stream)))

    def build_hashes(self, d_hashes, stream=None):
        _check(load_library().rf_amd_batch_build_hashes(self.h, _dptr(d_hashes), _stream(stream)))

    def probe_keys(self, d_keys, key_len, d_filter_id, n, d_found, stream=None):
        _check(load_library().rf_amd_batch_probe_keys(self.h, _dptr(d_keys), key_len,
                                                      _dptr(d_filter_id), n, _dptr(d_found), _stream(stream)))

    def probe_var_keys(self, d_bytes, d_offsets, d_filter_id, n, d_found, stream=None):
        _check(load_library().rf_amd_batch_probe_var_keys(self.h, _dptr(d_bytes), _dptr(d_offsets),
                                                          _dptr(d_filter_id), n, _dptr(d_found),
                                                          _stream(stream)))

    def probe_hashes(self, d_hashes, d_filter_id, n, d_found, stream=None):
        _check(load_library().rf_amd_batch_probe_hashes(self.h, _dptr(d_hashes), _dptr(d_filter_id),
                                                        n, _dptr(d_found), _stream(stream)))

    def probe_keys_runs(self, d_keys, key_len, counts, d_found, stream=None):
        """Probes grouped by filter: counts[f] probes of filter f, in filter order."""
        c = (ctypes.c_uint64 * self.F)(*[int(x) for x in counts])
        _check(load_library().rf_amd_batch_probe_keys_runs(self.h, _dptr(d_keys), key_len, c, _dptr(d_found),
                                                           _stream(stream)))

    def probe_hashes_runs(self, d_hashes, counts, d_found, stream=None):
        c = (ctypes.c_uint64 * self.F)(*[int(x) for x in counts])
        _check(load_library().rf_amd_batch_probe_hashes_runs(self.h, _dptr(d_hashes), c, _dptr(d_found),
                                                             _stream(stream)))

    def probe_var_keys_runs(self, d_bytes, d_offsets, counts, d_found, stream=None):
        """probe_keys_runs for variable-length keys (bytes and sum(counts) + 1 offsets)"""
        c = (ctypes.c_uint64 * self.F)(*[int(x) for x in counts])
        _check(load_library().rf_amd_batch_probe_var_keys_runs(self.h, _dptr(d_bytes), _dptr(d_offsets), c,
                                                               _dptr(d_found), _stream(stream)))

    def probe_floor(self, d_in, key_len, counts, d_out, stream=None):
        """The probe's memory floor (rf_amd_debug_probe_floor): the fast path's traffic over the
        same runs with the arithmetic removed; d_out gets no lookup results."""
        c = (ctypes.c_uint64 * self.F)(*[int(x) for x in counts])
        _check(load_library().rf_amd_debug_probe_floor(self.h, _dptr(d_in), key_len, c, _dptr(d_out),
                                                       _stream(stream)))

    def probe_pairs(self, d_pairs, n, d_found, stream=None):
        """Probes given as (local filter id << 32 | hash) u64 pairs (routed probes, route.py)."""
        _check(load_library().rf_amd_batch_probe_pairs(self.h, _dptr(d_pairs), n, _dptr(d_found),
                                                       _stream(stream)))

    # fresh builds: partition = fused hash + coarse-bucket partition (K1+K3); count_scan and
    # scatter = the spill fallback (near zero unless a coarse bucket overflowed); incremental
    # builds: partition = K1 count, count_scan = K2, scatter = K3. assemble includes the
    # probe lines.
    STAGES = ["partition", "count_scan", "scatter", "cb_sort", "cb_sort_big", "layout",
              "assemble", "build_total", "probe"]

    def set_timing(self, enable=True, sets=1, probe_only=False):
        """Per-stage HIP-event timing; `sets` rounds (build + probe) kept in a ring.
        probe_only: record only the probe's two events (the build stages read -1)."""
        n = sets if enable else 0
        _check(load_library().rf_amd_batch_set_timing(self.h, -n if probe_only else n))

    def debug_lines(self) -> np.ndarray:
        """The batch's device-only probe lines (diagnostics), as an (N, 64) uint8 array."""
        L, n = load_library(), ctypes.c_uint64(0)
        _check(L.rf_amd_debug_read_lines(self.h, None, 0, ctypes.byref(n)))
        out = np.zeros((n.value, 64), dtype=np.uint8)
        _check(L.rf_amd_debug_read_lines(self.h, out.ctypes.data, out.nbytes, ctypes.byref(n)))
        return out

    def debug_rebuild_lines(self):
        """Re-cut the probe lines from the images with the image-upload kernel (diagnostics)."""
        _check(load_library().rf_amd_debug_rebuild_lines(self.h))

    def timings(self, back=0):
        """Per-stage milliseconds of a build / probe round (HIP events on the launch stream);
        back = 0 is the latest round, up to sets - 1 (set_timing)."""
        arr = (ctypes.c_float * len(self.STAGES))()
        _check(load_library().rf_amd_batch_timings_back(self.h, back, arr, len(self.STAGES)))
        return dict(zip(self.STAGES, [float(x) for x in arr]))

    def info(self, f):
        out = RfFilterInfo()
        _check(load_library().rf_amd_batch_info(self.h, f, ctypes.byref(out)))
        return out

    def infos(self, stream=None):
        """every filter's RfFilterInfo (one synchronisation: with `stream`, the build's
        stream, or the whole device)"""
        arr = (RfFilterInfo * self.F)()
        _check(load_library().rf_amd_batch_infos(self.h, arr, _stream(stream)))
        return list(arr)

    def read_image_async(self, f, h_pages, h_slots, stream=None):
        """D2H of filter f's pages/slots into (pinned) host tensors sized by the caller."""
        _check(load_library().rf_amd_batch_read_image_async(
            self.h, f, h_pages.data_ptr(), h_pages.numel(), h_slots.data_ptr(), h_slots.numel(),
            _stream(stream)))

    def image(self, f) -> RoutingFilter:
        inf = self.info(f)
        if inf.error:
            raise PlatformStatusError(STATUS_BAD_PARAM, f"filter {f} error bits {inf.error:#x}")
        pages = np.zeros(inf.num_pages * self.cfg.page_size, dtype=np.uint8)
        slots = np.zeros(inf.num_indices, dtype=np.uint64)
        _check(load_library().rf_amd_batch_read_image(self.h, f, pages.ctypes.data, pages.size,
                                                      slots.ctypes.data, slots.size))
        return RoutingFilter(inf.num_fingerprints, inf.num_unique, inf.value_size,
                             inf.num_indices, inf.num_pages, pages, slots)


# ---- multi-get: filter sets, fan-out probes, candidate lists -----------------------------
def found_candidates(found: np.ndarray) -> np.ndarray:
    """Host mirror of rf_amd_found_compact: the set bits of the found_values words as records
    index << 8 | value (uint64), index ascending and, within a word, value descending -- the
    order in which routing_filter_get_next_value hands a word's values out."""
    w = np.ascontiguousarray(found).reshape(-1).view(np.uint64)
    nz = np.flatnonzero(w)
    if nz.size == 0:
        return np.zeros(0, dtype=np.uint64)
    # byte-wise big-endian view: unpackbits then lists bit 63 first
    bits = np.unpackbits(w[nz].astype(">u8").view(np.uint8).reshape(-1, 8), axis=1)
    row, col = np.nonzero(bits)  # row-major: value = 63 - col descends within a word
    return (nz[row].astype(np.uint64) << np.uint64(8)) | (np.uint64(63) - col.astype(np.uint64))


def ragged_pair_keys(offsets, pair_index) -> np.ndarray:
    """Host mirror of the ragged multi-get's record-to-key step: the key that owns each pair,
    pair_index being relative to offsets[0] as rf_amd_found_compact's record indices are after
    a ragged probe (record >> 8). offsets: the n + 1 non-decreasing pair offsets; the key of
    pair p is the last k with offsets[k] <= p, so empty lists own nothing."""
    off = np.ascontiguousarray(offsets).reshape(-1).view(np.uint64).astype(np.int64)
    p = np.asarray(pair_index).astype(np.int64) + off[0]
    return np.searchsorted(off, p, side="right").astype(np.int64) - 1


def found_compact_scratch_bytes(m) -> int:
    return int(load_library().rf_amd_found_compact_scratch_bytes(m))


_compact_scratch = {}  # (engine, stream) -> the scratch of the last found_compact issued there


def found_compact(d_found, m, d_cand, d_count, stream=None, engine=None):
    """rf_amd_found_compact: the candidate records of d_found[:m] into d_cand (capacity: its
    length; None: count only) and their total number into d_count (a device uint64 / int64 of
    one element), asynchronously. The scratch is a torch buffer kept until the next call on the
    same stream."""
    import torch
    eng = engine or default_engine()
    st = _stream(stream)
    ref = d_found if hasattr(d_found, "device") else d_count
    scratch = torch.empty(found_compact_scratch_bytes(m) // 8, dtype=torch.int64, device=ref.device)
    cap = 0 if d_cand is None else d_cand.numel()
    _check(load_library().rf_amd_found_compact(eng.h, _dptr(d_found), m, _dptr(d_cand), cap, _dptr(d_count),
                                               scratch.data_ptr(), st))
    _compact_scratch[(id(eng), st)] = scratch


def found_per_key_host(found, member, member_off):
    """Host mirror of rf_amd_found_per_key_ragged: found and member indexed by the absolute pair,
    member_off the n + 1 non-decreasing pair offsets (member_off[0] any value). Returns (key_off
    uint64[n + 1], cand uint64[total], cand_key int64[total]): cand = member id << 8 | value in
    found_candidates' order over the pairs [member_off[0], member_off[n]), key i owning
    cand[key_off[i] : key_off[i + 1]], cand_key the key of every record."""
    off = np.ascontiguousarray(member_off).reshape(-1).view(np.uint64).astype(np.int64)
    first, last = int(off[0]), int(off[-1])
    rec = found_candidates(np.ascontiguousarray(found).reshape(-1).view(np.uint64)[first:last])
    pair = (rec >> np.uint64(8)).astype(np.int64)
    ids = np.ascontiguousarray(member).reshape(-1).view(np.uint32)[first:last].astype(np.uint64)
    cand = (ids[pair] << np.uint64(8)) | (rec & np.uint64(0xFF))
    cand_key = ragged_pair_keys(off, pair)
    key_off = np.zeros(off.size, dtype=np.uint64)
    np.cumsum(np.bincount(cand_key, minlength=off.size - 1).astype(np.uint64), out=key_off[1:])
    return key_off, cand, cand_key


def found_per_key_host_fixed(found, member, K):
    """Host mirror of rf_amd_found_per_key: the pair of (key i, slot j) is i * K + j; member None:
    the id is the slot. Returns what found_per_key_host does."""
    w = np.ascontiguousarray(found).reshape(-1).view(np.uint64)
    n = w.size // K
    if member is None:
        member = np.tile(np.arange(K, dtype=np.uint32), n)
    return found_per_key_host(w, member, np.arange(n + 1, dtype=np.uint64) * np.uint64(K))


def found_per_key_scratch_bytes(n) -> int:
    return int(load_library().rf_amd_found_per_key_scratch_bytes(n))


def diag_per_key_tile() -> int:
    """keys per tile of found_per_key / found_per_key_ragged (rf_amd_diag_per_key_tile)"""
    return int(load_library().rf_amd_diag_per_key_tile())


_per_key_scratch = {}  # (engine, stream) -> the scratch of the last found_per_key issued there


def _found_per_key(call, n, d_key_off, d_cand, d_cand_key, d_count, stream, engine):
    import torch
    eng = engine or default_engine()
    st = _stream(stream)
    scratch = torch.empty(found_per_key_scratch_bytes(n) // 8, dtype=torch.int64, device=d_count.device)
    cap = 0 if d_cand is None else d_cand.numel()
    if d_cand_key is not None and d_cand_key.numel() < cap:
        raise ValueError("d_cand_key is shorter than d_cand")
    _check(call(eng.h, n, _dptr(d_key_off), _dptr(d_cand), _dptr(d_cand_key), cap, _dptr(d_count),
                scratch.data_ptr(), st))
    _per_key_scratch[(id(eng), st)] = scratch


def found_per_key(d_found, d_member, K, n, d_key_off, d_cand, d_cand_key, d_count, stream=None, engine=None):
    """rf_amd_found_per_key: the words d_found[:n * K] of a fixed-K probe to d_key_off (n + 1),
    the records member id << 8 | value in d_cand (capacity: its length; None: offsets and count
    only), their keys in d_cand_key (None: not written) and their total number in d_count,
    asynchronously. d_member None: the id is the slot. The scratch is a torch buffer kept until
    the next call on the same stream."""
    L = load_library()
    _found_per_key(lambda e, *a: L.rf_amd_found_per_key(e, _dptr(d_found), _dptr(d_member), K, *a),
                   n, d_key_off, d_cand, d_cand_key, d_count, stream, engine)


def found_per_key_ragged(d_found, d_member, d_member_off, n, d_key_off, d_cand, d_cand_key, d_count, stream=None,
                         engine=None):
    """rf_amd_found_per_key_ragged: found_per_key after a ragged probe, with the probe's d_found
    (a tensor or the address the probe took), d_member and d_member_off"""
    L = load_library()
    _found_per_key(lambda e, *a: L.rf_amd_found_per_key_ragged(e, _dptr(d_found), _dptr(d_member),
                                                               _dptr(d_member_off), *a),
                   n, d_key_off, d_cand, d_cand_key, d_count, stream, engine)


def by_branch_sort_key(cand, num_members):
    """the 32-bit sort key of rf_amd_found_by_branch for every record: ((c >> 8) & (2^mb - 1)) << 6
    | (c & 63), mb the bit width of num_members - 1"""
    if not 1 <= num_members <= 1 << 26:
        raise ValueError("num_members outside [1, 2^26]")
    c = np.ascontiguousarray(cand).reshape(-1).view(np.uint64)
    mask = np.uint64((1 << (num_members - 1).bit_length()) - 1)
    return ((((c >> np.uint64(8)) & mask) << np.uint64(6)) | (c & np.uint64(63))).astype(np.uint32)


def found_by_branch_host(cand, num_members, cand_key=None):
    """Host mirror of rf_amd_found_by_branch over all of cand (the caller slices the first
    min(count, cap) records): a numpy stable argsort on the sort key. Returns (order uint32[m],
    order_key uint64[m] or None, branch uint64[runs], branch_off uint64[runs + 1]): order[t] = the
    position in cand of the record at grouped position t, order_key = cand_key[order], branch[u]
    the record of run u's first element, the run being order[branch_off[u] : branch_off[u + 1]]."""
    c = np.ascontiguousarray(cand).reshape(-1).view(np.uint64)
    key = by_branch_sort_key(c, num_members)
    order = np.argsort(key, kind="stable").astype(np.uint32)
    skey = key[order]
    heads = np.flatnonzero(np.concatenate(([True], skey[1:] != skey[:-1]))) if c.size else np.zeros(0, np.int64)
    order_key = None
    if cand_key is not None:
        order_key = np.ascontiguousarray(cand_key).reshape(-1).view(np.uint64)[order]
    branch_off = np.concatenate((heads, [c.size])).astype(np.uint64)
    return order, order_key, c[order[heads]], branch_off


def found_by_branch_scratch_bytes(cap, num_members) -> int:
    return int(load_library().rf_amd_found_by_branch_scratch_bytes(cap, num_members))


def diag_by_branch_tile() -> int:
    """records per tile of found_by_branch (rf_amd_diag_by_branch_tile)"""
    return int(load_library().rf_amd_diag_by_branch_tile())


def diag_by_branch_passes(num_members) -> int:
    """digit passes of found_by_branch's sort (rf_amd_diag_by_branch_passes)"""
    return int(load_library().rf_amd_diag_by_branch_passes(num_members))


_by_branch_scratch = {}  # (engine, stream) -> the scratch of the last found_by_branch issued there


def found_by_branch(d_cand, d_cand_key, d_count, cap, num_members, d_order, d_order_key, d_branch, d_branch_off,
                    branch_cap, d_num_branches, stream=None, engine=None):
    """rf_amd_found_by_branch: the first min(d_count, cap) records of d_cand, as a found_per_key
    call left them, grouped by branch, asynchronously: d_order (int32 / uint32, cap elements), the
    optional d_order_key (with d_cand_key; both None: not produced), the first branch_cap runs in
    d_branch and d_branch_off (branch_cap + 1 elements) and the true number of runs in
    d_num_branches. The scratch is a torch buffer kept until the next call on the same stream."""
    import torch
    eng = engine or default_engine()
    st = _stream(stream)
    if cap and d_order.numel() < cap:
        raise ValueError("d_order is shorter than cap")
    if d_order_key is not None and d_order_key.numel() < cap:
        raise ValueError("d_order_key is shorter than cap")
    if branch_cap and (d_branch.numel() < branch_cap or d_branch_off.numel() < branch_cap + 1):
        raise ValueError("d_branch / d_branch_off are shorter than branch_cap / branch_cap + 1")
    scratch = torch.empty(found_by_branch_scratch_bytes(cap, num_members) // 8, dtype=torch.int64,
                          device=d_count.device)
    _check(load_library().rf_amd_found_by_branch(eng.h, _dptr(d_cand), _dptr(d_cand_key), _dptr(d_count), cap,
                                                 num_members, _dptr(d_order), _dptr(d_order_key), _dptr(d_branch),
                                                 _dptr(d_branch_off), branch_cap, _dptr(d_num_branches),
                                                 scratch.data_ptr(), st))
    _by_branch_scratch[(id(eng), st)] = scratch


ADVANCE_FIRST = 1  # RF_AMD_ADVANCE_FIRST: the cursors count as 0 and are not read; they are written
ADVANCE_MAX_TAKE = 65535 * 64  # the records one key takes in one call at most (PER_KEY_MAX_KEY_CANDS)


def found_advance_host(key_off, cand, cand_cap, width, done, cursor, out_cap):
    """Host mirror of rf_amd_found_advance: key_off the n + 1 record offsets and cand the records
    of a found_per_key call, cand_cap the capacity that call was given, done n bytes or None
    (every key open), cursor n uint32 or None (RF_AMD_ADVANCE_FIRST: all 0). Returns (out_cand
    uint64[w], out_key uint64[w], count, new_cursor uint32[n]) with w = min(count, out_cap) the
    records written and count the true total."""
    off = np.ascontiguousarray(key_off).reshape(-1).view(np.uint64).astype(np.int64)
    n = off.size - 1
    c = np.ascontiguousarray(cand).reshape(-1).view(np.uint64)
    cur = np.zeros(n, dtype=np.int64) if cursor is None else \
        np.ascontiguousarray(cursor).reshape(-1).view(np.uint32).astype(np.int64)
    if not 1 <= width < 1 << 32:
        raise ValueError("width outside [1, 2^32)")
    a = off[:-1] + cur
    e = np.minimum(off[1:], cand_cap)
    take = np.clip(np.minimum(e - a, min(width, ADVANCE_MAX_TAKE)), 0, None)
    if done is not None:
        take[np.ascontiguousarray(done).reshape(-1).view(np.uint8) != 0] = 0
    pos = np.cumsum(take) - take  # key i's first output position
    count = int(take.sum())
    wr = np.clip(out_cap - pos, 0, take)  # the records of key i below out_cap
    new_cursor = cur + wr
    out_key = np.repeat(np.arange(n, dtype=np.int64), wr)
    src = np.arange(out_key.size, dtype=np.int64) - pos[out_key] + a[out_key]
    return c[src], out_key.astype(np.uint64), count, new_cursor.astype(np.uint32)


def found_advance_scratch_bytes(n) -> int:
    return int(load_library().rf_amd_found_advance_scratch_bytes(n))


_advance_scratch = {}  # (engine, stream) -> the scratch of the last found_advance issued there


def found_advance(d_key_off, d_cand, cand_cap, n, width, flags, d_done, d_cursor, d_out_cand, d_out_key, out_cap,
                  d_out_count, stream=None, engine=None):
    """rf_amd_found_advance: for every key that is not done (d_done uint8[n] or None) the next
    `width` records of d_cand behind its cursor (d_cursor int32 / uint32[n]; flags ADVANCE_FIRST:
    taken as 0) into d_out_cand and d_out_key (None: not written), both of out_cap elements, the
    true total into d_out_count, the cursors advanced by what was written, asynchronously.
    d_key_off, d_cand and cand_cap are a found_per_key call's. The scratch is a torch buffer kept
    until the next call on the same stream."""
    import torch
    eng = engine or default_engine()
    st = _stream(stream)
    for name, buf in (("d_out_cand", d_out_cand), ("d_out_key", d_out_key)):
        if buf is not None and not isinstance(buf, int) and buf.numel() < out_cap:
            raise ValueError(f"{name} is shorter than out_cap")
    scratch = torch.empty(found_advance_scratch_bytes(n) // 8, dtype=torch.int64, device=d_out_count.device)
    _check(load_library().rf_amd_found_advance(eng.h, _dptr(d_key_off), _dptr(d_cand), cand_cap, n, width, flags,
                                               _dptr(d_done), _dptr(d_cursor), _dptr(d_out_cand), _dptr(d_out_key),
                                               out_cap, _dptr(d_out_count), scratch.data_ptr(), st))
    _advance_scratch[(id(eng), st)] = scratch


class LookupSteps:
    """A multi-get with the early exit of the reference's loop (FilterSet.lookup_steps): every
    step() hands out the next `width` records of each key that is still open."""

    def __init__(self, fset, per_key_result, width=1, stream=None):
        import torch
        if not 1 <= width < 1 << 32:
            raise ValueError("width outside [1, 2^32)")
        self.fset, self.width, self.stream = fset, width, stream
        self.d_key_off, self.d_cand, count, _ = per_key_result
        self.n = self.d_key_off.numel() - 1
        self.cand_cap = min(count, self.d_cand.numel())
        dev = self.d_key_off.device
        # a step hands out at most width records per key and never more than there are: no cut
        self.out_cap = max(1, min(self.cand_cap, self.n * width))
        self.d_cursor = torch.empty(max(1, self.n), dtype=torch.int32, device=dev)  # the first step writes it
        self.d_out_cand = torch.empty(self.out_cap, dtype=torch.int64, device=dev)
        self.d_out_key = torch.empty(self.out_cap, dtype=torch.int64, device=dev)
        self.d_out_count = torch.empty(1, dtype=torch.int64, device=dev)
        self.d_order = torch.empty(self.out_cap, dtype=torch.int32, device=dev)
        self.d_order_key = torch.empty(self.out_cap, dtype=torch.int64, device=dev)
        self.d_runs = torch.empty(1, dtype=torch.int64, device=dev)
        self.branch_cap = max(1, min(self.out_cap, 64 * fset.num_members))
        self.steps = 0

    def _sync(self):
        if self.stream is not None:  # a raw handle torch's own copy is not ordered with
            import torch
            torch.cuda.ExternalStream(self.stream).synchronize()

    def step(self, d_done=None, by_branch=True):
        """One advance: d_done (uint8 / bool [n], or None) marks the keys whose lookup is
        complete. Returns (d_out_cand, d_out_key, count, group): the count records handed out and
        their keys, in batch order, and with by_branch what FilterSet.group_by_branch returns
        for them, (d_order, d_order_key, d_branch, d_branch_off, runs), else None -- the grouping
        is issued behind the advance and reads its count on the device. count == 0: the multi-get
        has finished. The tensors are views of buffers that the next step overwrites."""
        import torch
        eng = self.fset.engine
        found_advance(self.d_key_off, self.d_cand, self.cand_cap, self.n, self.width,
                      0 if self.steps else ADVANCE_FIRST, d_done, self.d_cursor, self.d_out_cand, self.d_out_key,
                      self.out_cap, self.d_out_count, self.stream, eng)
        self.steps += 1
        group = None
        while by_branch:
            d_branch = torch.empty(self.branch_cap, dtype=torch.int64, device=self.d_out_cand.device)
            d_branch_off = torch.empty(self.branch_cap + 1, dtype=torch.int64, device=self.d_out_cand.device)
            found_by_branch(self.d_out_cand, self.d_out_key, self.d_out_count, self.out_cap, self.fset.num_members,
                            self.d_order, self.d_order_key, d_branch, d_branch_off, self.branch_cap, self.d_runs,
                            self.stream, eng)
            self._sync()
            runs = int(self.d_runs.item())
            if runs <= self.branch_cap:
                group = (d_branch, d_branch_off, runs)
                break
            self.branch_cap = runs  # ids at or above num_members: only the grouping is repeated
        self._sync()
        count = int(self.d_out_count.item())
        if group is not None:
            d_branch, d_branch_off, runs = group
            group = (self.d_order[:count], self.d_order_key[:count], d_branch[:runs], d_branch_off[:runs + 1], runs)
        return self.d_out_cand[:count], self.d_out_key[:count], count, group


_exists_routed_csr = {}  # (engine, stream) -> the CSR of the last exists_routed issued there


class _Unfiltered:
    """RF_AMD_MEMBER_UNFILTERED: a bundle without a maplet that holds one branch
    (src/trunk.c:6020-6022); every key finds value 0 in it"""

    def __repr__(self):
        return "UNFILTERED"


UNFILTERED = _Unfiltered()
EXISTS_FILTER_HIT = 1  # RF_AMD_EXISTS_FILTER_HIT: some filter of the key's list found a value
EXISTS_UNFILTERED = 2  # RF_AMD_EXISTS_UNFILTERED: the list holds an unfiltered member
KIND_FILTER, KIND_NULL, KIND_UNFILTERED = 0, 1, 2  # what a set's slot holds (exists_host's kinds)


def exists_host(words, kinds, member, member_off):
    """Host mirror of rf_amd_filter_set_exists_*_ragged: words[p] = the oracle's found word of
    pair p where its member is a filter (not read elsewhere), kinds[g] = KIND_* of member g of
    the set, member and member_off the call's, all indexed by the absolute pair (member_off[0]
    any value). An id >= len(kinds) adds nothing, as a NULL member. Returns the n bytes: bit 0
    when a filter of the key's list has a non-zero word, bit 1 when the list holds an unfiltered
    member."""
    off = np.ascontiguousarray(member_off).reshape(-1).view(np.uint64).astype(np.int64)
    first, last, n = int(off[0]), int(off[-1]), off.size - 1
    ids = np.ascontiguousarray(member).reshape(-1).view(np.uint32)[first:last].astype(np.int64)
    kinds = np.asarray(kinds, dtype=np.int64).reshape(-1)
    ok = ids < kinds.size
    kind = np.where(ok, kinds[np.where(ok, ids, 0)] if kinds.size else KIND_NULL, KIND_NULL)
    w = np.ascontiguousarray(words).reshape(-1).view(np.uint64)[first:last]
    bits = np.where((kind == KIND_FILTER) & (w != 0), EXISTS_FILTER_HIT, 0) | \
        np.where(kind == KIND_UNFILTERED, EXISTS_UNFILTERED, 0)
    key = np.repeat(np.arange(n), np.diff(off))
    out = np.zeros(n, dtype=np.uint8)
    for b in (EXISTS_FILTER_HIT, EXISTS_UNFILTERED):
        out[np.unique(key[(bits & b) != 0])] |= np.uint8(b)
    return out


def exists_host_fixed(words, kinds, member, K):
    """Host mirror of rf_amd_filter_set_exists_{keys,var_keys,hashes}: the pair of (key i, slot
    j) is i * K + j; member None: the id is the slot. Returns what exists_host does."""
    w = np.ascontiguousarray(words).reshape(-1).view(np.uint64)
    n = w.size // K
    if member is None:
        member = np.tile(np.arange(K, dtype=np.uint32), n)
    return exists_host(w, kinds, member, np.arange(n + 1, dtype=np.uint64) * np.uint64(K))


def diag_fanout_max_blocks(blocks: int):
    """rf_amd_diag_fanout_max_blocks: cap the fan-out probe's grid (diagnostics, process-wide)
    so that every wave takes several 64-key chunks; 0 restores the default"""
    _check(load_library().rf_amd_diag_fanout_max_blocks(int(blocks)))


class FilterSet:
    """A resident table of filters of any batches (rf_amd_filter_set): members = [(FilterBatch,
    index), None (a bundle with no branch) or UNFILTERED (a bundle without a maplet that holds one
    branch: every key's word is 1)]. The member batches must outlive the set's last probe.
    capacity (None: the number of members) is the room update() has: the slots past the members
    start empty."""

    def __init__(self, members, engine=None, capacity=None):
        self.engine = engine or default_engine()
        n = len(members)
        hs, idx = self._member_arrays(members)
        h = ctypes.c_void_p()
        if capacity is None:
            _check(load_library().rf_amd_filter_set_create(self.engine.h, ctypes.addressof(hs), idx.ctypes.data, n,
                                                           ctypes.byref(h)))
        else:
            _check(load_library().rf_amd_filter_set_create_cap(self.engine.h, ctypes.addressof(hs), idx.ctypes.data,
                                                               n, int(capacity), ctypes.byref(h)))
        self.h = h
        self.num_members = n
        self._members = list(members) + [None] * (self.capacity - n)  # slot -> (batch, index), None or UNFILTERED
        self._keep = self._batches(self._members)

    @staticmethod
    def _batches(members):
        return [m[0] for m in members if m is not None and m is not UNFILTERED]

    @staticmethod
    def _member_arrays(members):
        n = len(members)
        hs = (ctypes.c_void_p * max(1, n))()
        idx = np.zeros(max(1, n), dtype=np.uint32)
        for i, m in enumerate(members):
            if m is UNFILTERED:
                hs[i] = 1  # RF_AMD_MEMBER_UNFILTERED
            elif m is not None:
                hs[i] = m[0].h.value
                idx[i] = m[1]
        return hs, idx

    @property
    def capacity(self):
        return load_library().rf_amd_filter_set_capacity(self.h)

    def update(self, ids, members, stream=None):
        """rf_amd_filter_set_update: slot ids[i] becomes members[i] -- (FilterBatch, index),
        UNFILTERED, or None to clear it -- in stream order, without a host wait (the caller orders the members'
        builds before the call, on the same stream or with an event). An id named twice: the
        last entry wins. num_members follows the call. Returns what slot ids[i] held before the
        call, entry by entry; the set references the new batches afterwards and the replaced ones
        no longer, so the caller keeps the returned members alive until the last probe ordered
        before the update has run (dropping a FilterBatch synchronises the device, which is safe;
        FilterBatch.close(stream) after the update is the release without a wait)."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        members = list(members)
        if len(members) != ids.size:
            raise ValueError("ids and members differ in length")
        hs, idx = self._member_arrays(members)
        L = load_library()
        _check(L.rf_amd_filter_set_update(self.h, ids.ctypes.data if ids.size else None,
                                          ctypes.addressof(hs) if ids.size else None, idx.ctypes.data, ids.size,
                                          _stream(stream)))
        replaced = [self._members[int(i)] for i in ids]
        for i, m in zip(ids, members):
            self._members[int(i)] = m
        self._keep = self._batches(self._members)
        self.num_members = L.rf_amd_filter_set_num_members(self.h)
        return replaced

    def close(self):
        if getattr(self, "h", None):
            load_library().rf_amd_filter_set_destroy(self.h)
            self.h = None

    def close_on(self, stream):
        """rf_amd_filter_set_destroy_on: release the set in stream order (every probe and update
        of it must be ordered before the current end of `stream`), without a wait"""
        if getattr(self, "h", None):
            _check(load_library().rf_amd_filter_set_destroy_on(self.h, _stream(stream)))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def probe_keys(self, d_keys, key_len, d_member, K, n, d_found, stream=None):
        """key i in members d_member[i*K : i*K+K] (None: every member, K = num_members) into
        d_found[i*K : i*K+K]; each key is read and hashed once"""
        _check(load_library().rf_amd_filter_set_probe_keys(self.h, _dptr(d_keys), key_len, _dptr(d_member), K, n,
                                                           _dptr(d_found), _stream(stream)))

    def probe_hashes(self, d_hashes, d_member, K, n, d_found, stream=None):
        _check(load_library().rf_amd_filter_set_probe_hashes(self.h, _dptr(d_hashes), _dptr(d_member), K, n,
                                                             _dptr(d_found), _stream(stream)))

    def probe_var_keys(self, d_bytes, d_offsets, d_member, K, n, d_found, stream=None):
        """probe_keys for variable-length keys: key i is d_bytes[d_offsets[i] : d_offsets[i+1]]
        (n + 1 uint64 byte offsets)"""
        _check(load_library().rf_amd_filter_set_probe_var_keys(self.h, _dptr(d_bytes), _dptr(d_offsets),
                                                               _dptr(d_member), K, n, _dptr(d_found),
                                                               _stream(stream)))

    def multiget(self, d_keys, key_len, d_member, K, n, cap=None, stream=None):
        """probe_keys + found_compact: returns (d_cand, count), the first `count` records of
        d_cand being the candidates key * K + slot << 8 | value in order. One synchronisation;
        a second compaction and synchronisation when the candidates outnumber `cap` (default:
        one per key)."""
        import torch
        d_found = torch.empty(n * K, dtype=torch.int64, device=d_keys.device)
        self.probe_keys(d_keys, key_len, d_member, K, n, d_found, stream)
        return self._compact_found(d_found, n, K, cap, stream)

    def multiget_var(self, d_bytes, d_offsets, d_member, K, n, cap=None, stream=None):
        """multiget for variable-length keys (probe_var_keys + found_compact)"""
        import torch
        d_found = torch.empty(n * K, dtype=torch.int64, device=d_offsets.device)
        self.probe_var_keys(d_bytes, d_offsets, d_member, K, n, d_found, stream)
        return self._compact_found(d_found, n, K, cap, stream)

    def probe_keys_ragged(self, d_keys, key_len, d_member, d_member_off, n, d_found, stream=None):
        """key i in members d_member[d_member_off[i] : d_member_off[i+1]] (n + 1 uint64 pair
        offsets, at most 65,535 ids per key) into d_found at the same positions; each key is
        read and hashed once, and nothing outside the offsets' range is written"""
        _check(load_library().rf_amd_filter_set_probe_keys_ragged(self.h, _dptr(d_keys), key_len, _dptr(d_member),
                                                                  _dptr(d_member_off), n, _dptr(d_found),
                                                                  _stream(stream)))

    def probe_var_keys_ragged(self, d_bytes, d_offsets, d_member, d_member_off, n, d_found, stream=None):
        """probe_keys_ragged for variable-length keys (d_offsets: n + 1 uint64 byte offsets)"""
        _check(load_library().rf_amd_filter_set_probe_var_keys_ragged(self.h, _dptr(d_bytes), _dptr(d_offsets),
                                                                      _dptr(d_member), _dptr(d_member_off), n,
                                                                      _dptr(d_found), _stream(stream)))

    def probe_hashes_ragged(self, d_hashes, d_member, d_member_off, n, d_found, stream=None):
        _check(load_library().rf_amd_filter_set_probe_hashes_ragged(self.h, _dptr(d_hashes), _dptr(d_member),
                                                                    _dptr(d_member_off), n, _dptr(d_found),
                                                                    _stream(stream)))

    # ---- existence multi-get (rf_amd_filter_set_exists_*): the probes' arguments with d_exists, n
    # bytes (uint8, any alignment), in d_found's place; d_exists[i] = EXISTS_FILTER_HIT when a filter
    # of key i's list found a value | EXISTS_UNFILTERED when the list holds an unfiltered member
    def exists_keys(self, d_keys, key_len, d_member, K, n, d_exists, stream=None):
        _check(load_library().rf_amd_filter_set_exists_keys(self.h, _dptr(d_keys), key_len, _dptr(d_member), K, n,
                                                            _dptr(d_exists), _stream(stream)))

    def exists_hashes(self, d_hashes, d_member, K, n, d_exists, stream=None):
        _check(load_library().rf_amd_filter_set_exists_hashes(self.h, _dptr(d_hashes), _dptr(d_member), K, n,
                                                              _dptr(d_exists), _stream(stream)))

    def exists_var_keys(self, d_bytes, d_offsets, d_member, K, n, d_exists, stream=None):
        _check(load_library().rf_amd_filter_set_exists_var_keys(self.h, _dptr(d_bytes), _dptr(d_offsets),
                                                                _dptr(d_member), K, n, _dptr(d_exists),
                                                                _stream(stream)))

    def exists_keys_ragged(self, d_keys, key_len, d_member, d_member_off, n, d_exists, stream=None):
        _check(load_library().rf_amd_filter_set_exists_keys_ragged(self.h, _dptr(d_keys), key_len, _dptr(d_member),
                                                                   _dptr(d_member_off), n, _dptr(d_exists),
                                                                   _stream(stream)))

    def exists_var_keys_ragged(self, d_bytes, d_offsets, d_member, d_member_off, n, d_exists, stream=None):
        _check(load_library().rf_amd_filter_set_exists_var_keys_ragged(self.h, _dptr(d_bytes), _dptr(d_offsets),
                                                                       _dptr(d_member), _dptr(d_member_off), n,
                                                                       _dptr(d_exists), _stream(stream)))

    def exists_hashes_ragged(self, d_hashes, d_member, d_member_off, n, d_exists, stream=None):
        _check(load_library().rf_amd_filter_set_exists_hashes_ragged(self.h, _dptr(d_hashes), _dptr(d_member),
                                                                     _dptr(d_member_off), n, _dptr(d_exists),
                                                                     _stream(stream)))

    def exists_routed(self, range_map, d_keys, key_len, n, stream=None):
        """RangeMap.route_keys + exists_keys_ragged, from raw device keys: the n bytes (a uint8
        tensor). No host read: the route call's CSR goes to the existence call as it is."""
        return self._exists_routed(n, stream, range_map.route_keys(d_keys, key_len, n, stream=stream),
                                   lambda *a: self.exists_keys_ragged(d_keys, key_len, *a))

    def exists_var_routed(self, range_map, d_bytes, d_offsets, n, stream=None):
        """exists_routed for variable-length keys (route_var_keys + exists_var_keys_ragged)"""
        return self._exists_routed(n, stream, range_map.route_var_keys(d_bytes, d_offsets, n, stream=stream),
                                   lambda *a: self.exists_var_keys_ragged(d_bytes, d_offsets, *a))

    def _exists_routed(self, n, stream, routed, exists):
        import torch
        _, d_off, d_member, _ = routed
        if d_member.numel() == 0:  # a map whose lists are all empty
            return torch.zeros(n, dtype=torch.uint8, device=d_off.device)
        d_exists = torch.empty(n, dtype=torch.uint8, device=d_off.device)
        exists(d_member, d_off, n, d_exists, stream)
        # the CSR is read in stream order: kept until the next call on the same stream
        _exists_routed_csr[(id(self.engine), _stream(stream))] = (d_off, d_member)
        return d_exists

    def multiget_ragged(self, d_keys, key_len, d_member, d_member_off, n, cap=None, stream=None):
        """probe_keys_ragged + found_compact over the pairs: returns (d_cand, count, d_key). The
        first `count` records of d_cand are the candidates pair << 8 | value in order, pair
        being relative to d_member_off[0]; d_key[j] is the key of record j. The pair count is
        read from the offsets once; then as multiget."""
        return self._multiget_ragged(d_member_off, n, cap, stream,
                                     lambda d_found: self.probe_keys_ragged(d_keys, key_len, d_member, d_member_off,
                                                                            n, d_found, stream))

    def multiget_var_ragged(self, d_bytes, d_offsets, d_member, d_member_off, n, cap=None, stream=None):
        """multiget_ragged for variable-length keys (probe_var_keys_ragged + found_compact)"""
        return self._multiget_ragged(d_member_off, n, cap, stream,
                                     lambda d_found: self.probe_var_keys_ragged(d_bytes, d_offsets, d_member,
                                                                                d_member_off, n, d_found, stream))

    def _probe_ragged(self, d_member_off, n, probe):
        """the found words of a ragged multi-get: (d_found, first pair, number of pairs)"""
        import torch
        first, last = (int(x) for x in d_member_off[[0, n]].tolist()) if n else (0, 0)  # the one read
        m = last - first
        # the m words of the pairs alone: the probe indexes from d_member_off[0] and writes
        # nothing below it, so it takes the address that word 0 would have
        d_found = torch.empty(m, dtype=torch.int64, device=d_member_off.device)
        if m:
            probe(d_found.data_ptr() - 8 * first)
        return d_found, first, m

    def _multiget_ragged(self, d_member_off, n, cap, stream, probe):
        import torch
        d_found, first, m = self._probe_ragged(d_member_off, n, probe)
        d_cand, count = self._compact_found(d_found, m, 1, max(1, n) if cap is None else cap, stream)
        d_key = torch.searchsorted(d_member_off[:n + 1].view(torch.int64), (d_cand[:count] >> 8) + first,
                                   right=True) - 1
        return d_cand, count, d_key

    def multiget_routed(self, range_map, d_keys, key_len, n, cap=None, stream=None):
        """RangeMap.route_keys + probe_keys_ragged + found_compact, from raw device keys: returns
        (d_cand, count, d_key) as multiget_ragged does, the pairs being those of the route call's
        CSR (first offset 0). One 8-byte read of the pair count sizes d_found, in the place of
        multiget_ragged's read of the offsets; then as multiget."""
        return self._multiget_routed(
            n, cap, stream, lambda: range_map.route_keys(d_keys, key_len, n, stream=stream),
            lambda d_member, d_off, d_found: self.probe_keys_ragged(d_keys, key_len, d_member, d_off, n, d_found,
                                                                    stream))

    def multiget_var_routed(self, range_map, d_bytes, d_offsets, n, cap=None, stream=None):
        """multiget_routed for variable-length keys (route_var_keys + probe_var_keys_ragged)"""
        return self._multiget_routed(
            n, cap, stream, lambda: range_map.route_var_keys(d_bytes, d_offsets, n, stream=stream),
            lambda d_member, d_off, d_found: self.probe_var_keys_ragged(d_bytes, d_offsets, d_member, d_off, n,
                                                                        d_found, stream))

    def _probe_routed(self, stream, route, probe):
        """route and ragged probe of a routed multi-get: (d_found, d_member_off, d_member, pairs)"""
        import torch
        d_range, d_off, d_member, d_total = route()
        if stream is not None:  # a raw handle torch's own copy is not ordered with
            torch.cuda.ExternalStream(stream).synchronize()
        m = int(d_total.item())  # the one read
        d_found = torch.empty(m, dtype=torch.int64, device=d_off.device)
        if m:
            probe(d_member, d_off, d_found)
        return d_found, d_off, d_member, m

    def _multiget_routed(self, n, cap, stream, route, probe):
        import torch
        d_found, d_off, d_member, m = self._probe_routed(stream, route, probe)
        d_cand, count = self._compact_found(d_found, m, 1, max(1, n) if cap is None else cap, stream)
        d_key = torch.searchsorted(d_off[:n + 1], d_cand[:count] >> 8, right=True) - 1
        return d_cand, count, d_key

    # ---- the same probes with the key-aware compaction in the place of found_compact + searchsorted:
    # (d_key_off int64[n + 1], d_cand, count, d_cand_key), the first `count` records of d_cand being
    # member id << 8 | value, key i owning d_cand[d_key_off[i] : d_key_off[i + 1]] and d_cand_key[j]
    # being the key of record j. cap as in multiget.
    def multiget_per_key(self, d_keys, key_len, d_member, K, n, cap=None, stream=None):
        """probe_keys + found_per_key (d_member None: every member, the id is the slot)"""
        import torch
        d_found = torch.empty(n * K, dtype=torch.int64, device=d_keys.device)
        self.probe_keys(d_keys, key_len, d_member, K, n, d_found, stream)
        return self._per_key_tail(n, cap, stream, d_found.device,
                                  lambda *a: found_per_key(d_found, d_member, K, n, *a, stream, self.engine))

    def multiget_var_per_key(self, d_bytes, d_offsets, d_member, K, n, cap=None, stream=None):
        """multiget_per_key for variable-length keys"""
        import torch
        d_found = torch.empty(n * K, dtype=torch.int64, device=d_offsets.device)
        self.probe_var_keys(d_bytes, d_offsets, d_member, K, n, d_found, stream)
        return self._per_key_tail(n, cap, stream, d_found.device,
                                  lambda *a: found_per_key(d_found, d_member, K, n, *a, stream, self.engine))

    def multiget_ragged_per_key(self, d_keys, key_len, d_member, d_member_off, n, cap=None, stream=None):
        """probe_keys_ragged + found_per_key_ragged"""
        return self._per_key_ragged(d_member, d_member_off, n, cap, stream,
                                    lambda d_found: self.probe_keys_ragged(d_keys, key_len, d_member, d_member_off,
                                                                           n, d_found, stream))

    def multiget_var_ragged_per_key(self, d_bytes, d_offsets, d_member, d_member_off, n, cap=None, stream=None):
        """multiget_ragged_per_key for variable-length keys"""
        return self._per_key_ragged(d_member, d_member_off, n, cap, stream,
                                    lambda d_found: self.probe_var_keys_ragged(d_bytes, d_offsets, d_member,
                                                                               d_member_off, n, d_found, stream))

    def _per_key_ragged(self, d_member, d_member_off, n, cap, stream, probe):
        d_found, first, m = self._probe_ragged(d_member_off, n, probe)
        at = d_found.data_ptr() - 8 * first  # the probe's d_found: indexed by the absolute pair
        return self._per_key_tail(n, cap, stream, d_found.device,
                                  lambda *a: found_per_key_ragged(at, d_member, d_member_off, n, *a, stream,
                                                                  self.engine))

    def multiget_routed_per_key(self, range_map, d_keys, key_len, n, cap=None, stream=None):
        """RangeMap.route_keys + probe_keys_ragged + found_per_key_ragged, from raw device keys"""
        return self._per_key_routed(
            n, cap, stream, lambda: range_map.route_keys(d_keys, key_len, n, stream=stream),
            lambda d_member, d_off, d_found: self.probe_keys_ragged(d_keys, key_len, d_member, d_off, n, d_found,
                                                                    stream))

    def multiget_var_routed_per_key(self, range_map, d_bytes, d_offsets, n, cap=None, stream=None):
        """multiget_routed_per_key for variable-length keys"""
        return self._per_key_routed(
            n, cap, stream, lambda: range_map.route_var_keys(d_bytes, d_offsets, n, stream=stream),
            lambda d_member, d_off, d_found: self.probe_var_keys_ragged(d_bytes, d_offsets, d_member, d_off, n,
                                                                        d_found, stream))

    def _per_key_routed(self, n, cap, stream, route, probe):
        d_found, d_off, d_member, m = self._probe_routed(stream, route, probe)
        return self._per_key_tail(n, cap, stream, d_off.device,
                                  lambda *a: found_per_key_ragged(d_found, d_member, d_off, n, *a, stream,
                                                                  self.engine))

    def _per_key_tail(self, n, cap, stream, dev, compact):
        """the per-key multi-get's tail: compact(d_key_off, d_cand, d_cand_key, d_count) once, and
        once more into larger buffers when the candidates outnumber cap (default: one per key)"""
        import torch
        d_count = torch.zeros(1, dtype=torch.int64, device=dev)
        d_key_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        size = max(1, n) if cap is None else cap
        while True:
            d_cand = torch.empty(size, dtype=torch.int64, device=dev)
            d_cand_key = torch.empty(size, dtype=torch.int64, device=dev)
            compact(d_key_off, d_cand, d_cand_key, d_count)
            if stream is not None:  # a raw handle torch's own copy is not ordered with
                torch.cuda.ExternalStream(stream).synchronize()
            count = int(d_count.item())
            if count <= size:
                return d_key_off, d_cand, count, d_cand_key
            size = count

    def group_by_branch(self, per_key_result, stream=None):
        """found_by_branch on what a multiget_*_per_key method returned, (d_key_off, d_cand, count,
        d_cand_key), with this set's num_members: returns (d_order int32[count], d_order_key
        int64[count], d_branch int64[runs], d_branch_off int64[runs + 1], runs). Run u is the
        records d_cand[d_order[d_branch_off[u] : d_branch_off[u + 1]]] of the branch d_branch[u],
        in batch order, and d_order_key their keys. The branch table is sized for 64 branches per
        member, at most one per record; only this step is repeated, into a larger table, when the
        branches outnumber it (ids at or above num_members can make them)."""
        return self._group_by_branch(per_key_result, stream, None)

    def _group_by_branch(self, per_key_result, stream, branch_cap):
        """group_by_branch with the first branch table of branch_cap runs (None: the default)"""
        import contextlib

        import torch
        _, d_cand, count, d_cand_key = per_key_result
        dev = d_cand.device
        # *d_count is read on the device: its fill runs on the stream of the launches
        on = torch.cuda.stream(torch.cuda.ExternalStream(stream)) if stream is not None else contextlib.nullcontext()
        with on:
            d_count = torch.full((1,), count, dtype=torch.int64, device=dev)
        d_runs = torch.empty(1, dtype=torch.int64, device=dev)  # every call writes it: no fill to order
        # never empty: no records is still a buffer, so that the key pointers are both non-NULL
        d_order = torch.empty(max(1, count), dtype=torch.int32, device=dev)
        d_order_key = torch.empty(max(1, count), dtype=torch.int64, device=dev)
        keyed = d_cand_key.numel() > 0  # a per-key call with cap 0 left no key buffer: then neither side's
        size = max(1, min(count, 64 * self.num_members)) if branch_cap is None else branch_cap
        while True:
            d_branch = torch.empty(size, dtype=torch.int64, device=dev)
            d_branch_off = torch.empty(size + 1, dtype=torch.int64, device=dev)
            found_by_branch(d_cand, d_cand_key if keyed else None, d_count, count, self.num_members, d_order,
                            d_order_key if keyed else None, d_branch, d_branch_off, size, d_runs, stream,
                            self.engine)
            if stream is not None:  # a raw handle torch's own copy is not ordered with
                torch.cuda.ExternalStream(stream).synchronize()
            runs = int(d_runs.item())
            if runs <= size:
                return d_order[:count], d_order_key[:count], d_branch[:runs], d_branch_off[:runs + 1], runs
            size = runs

    def lookup_steps(self, per_key_result, width=1, stream=None):
        """The early exit of the reference's lookup loop (src/trunk.c:6085) over what a
        multiget_*_per_key method returned: a LookupSteps whose step(d_done=None, by_branch=True)
        runs one found_advance -- the next `width` records of every key not marked in d_done --
        and, with by_branch, found_by_branch behind it. The consumer walks the runs, marks the
        keys that met a definitive message and steps again until the count is 0."""
        return LookupSteps(self, per_key_result, width, stream)

    def _compact_found(self, d_found, n, K, cap, stream):
        """the multi-get's tail: the candidates of d_found[:n * K] as (d_cand, count)"""
        import torch
        dev = d_found.device
        d_count = torch.zeros(1, dtype=torch.int64, device=dev)
        d_cand = torch.empty(max(1, n) if cap is None else cap, dtype=torch.int64, device=dev)
        def read_count():
            if stream is not None:  # a raw handle torch's own copy is not ordered with
                torch.cuda.ExternalStream(stream).synchronize()
            return int(d_count.item())

        found_compact(d_found, n * K, d_cand, d_count, stream, self.engine)
        count = read_count()
        if count > d_cand.numel():
            d_cand = torch.empty(count, dtype=torch.int64, device=dev)
            found_compact(d_found, n * K, d_cand, d_count, stream, self.engine)
            count = read_count()
        return d_cand, count


# ---- range maps: multi-get keys routed to their member lists -----------------------------
def range_route_host(boundaries, lists, keys):
    """Host mirror of a route call (rf_amd_range_map_route_*): boundaries = the R - 1 boundary
    keys as `bytes`, strictly ascending; lists = the R id sequences; keys = n `bytes`. Key i's
    range is the number of boundaries <= it -- bisect_right, Python's `bytes` order being
    slice_lex_cmp's (unsigned bytes over the common length, then the shorter first). Returns
    (range uint32[n], member_off uint64[n + 1], member uint32[total], total)."""
    import bisect
    boundaries = [bytes(b) for b in boundaries]
    if len(lists) != len(boundaries) + 1:
        raise ValueError("R lists take R - 1 boundaries")
    rng = np.fromiter((bisect.bisect_right(boundaries, bytes(k)) for k in keys), dtype=np.uint32, count=len(keys))
    llen = np.array([len(x) for x in lists], dtype=np.int64)
    loff = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum(llen, out=loff[1:])
    flat = np.fromiter((i for x in lists for i in x), dtype=np.uint32, count=int(loff[-1]))
    cnt = llen[rng]
    off = np.zeros(len(keys) + 1, dtype=np.uint64)
    np.cumsum(cnt.astype(np.uint64), out=off[1:])
    total = int(off[-1])
    # pair p of key i is id p - off[i] of its range's list
    key = np.repeat(np.arange(len(keys), dtype=np.int64), cnt)
    src = loff[rng][key] + (np.arange(total, dtype=np.int64) - off[:-1].astype(np.int64)[key])
    return rng, off, flat[src], total


def diag_range_tile() -> int:
    """keys per scan tile of a route call (rf_amd_diag_range_tile)"""
    return int(load_library().rf_amd_diag_range_tile())


def diag_range_lds_ranges() -> int:
    """the largest R whose boundary prefixes the route kernel searches in LDS
    (rf_amd_diag_range_lds_ranges); a map with more ranges takes the kernel's other instance"""
    return int(load_library().rf_amd_diag_range_lds_ranges())


def range_route_scratch_bytes(n) -> int:
    return int(load_library().rf_amd_range_route_scratch_bytes(n))


def diag_range_seg_launch_ids() -> int:
    """the ids one launch of RangeMap.update_segments carries when it holds one list
    (rf_amd_diag_range_seg_launch_ids): a list of one id more is cut into two pieces"""
    return int(load_library().rf_amd_diag_range_seg_launch_ids())


def diag_range_seg_thread_ids() -> int:
    """the longest list of a range that the flatten of an update expands by a single thread
    (rf_amd_diag_range_seg_thread_ids); a longer one takes a wave"""
    return int(load_library().rf_amd_diag_range_seg_thread_ids())


def range_segment_lists(paths, seg_lists):
    """The R flat lists of a map made from segments, as range_route_host and RangeMap take them:
    range r's list is the concatenation of seg_lists[s] for s in paths[r], in path order."""
    seg_lists = [[int(i) for i in x] for x in seg_lists]
    return [[i for s in path for i in seg_lists[s]] for path in paths]


def diag_range_splice_words() -> int:
    """the 32-bit words of new elements one launch of RangeMap.split / set_paths carries
    (rf_amd_diag_range_splice_words): see range_splice_words"""
    return int(load_library().rf_amd_diag_range_splice_words())


def range_splice_words(boundaries, paths) -> int:
    """the argument words the new elements of a split (set_paths: no boundaries) take: four per
    boundary, one per four boundary bytes, two per path and one per path entry. An edit of at
    most diag_range_splice_words() words is one splice launch."""
    return (4 * len(boundaries) + (sum(len(b) for b in boundaries) + 3) // 4 + 2 * len(paths)
            + sum(len(p) for p in paths))


def range_split_host(boundaries, paths, r, new_boundaries, new_paths):
    """Host model of RangeMap.split as list surgery: the (boundaries, paths) of the map after
    range r has become len(new_paths) ranges. Feed the result to range_segment_lists and
    range_route_host."""
    if len(new_boundaries) != len(new_paths) - 1:
        raise ValueError("m pieces take m - 1 boundaries")
    boundaries, paths = [bytes(b) for b in boundaries], [list(p) for p in paths]
    return (boundaries[:r] + [bytes(b) for b in new_boundaries] + boundaries[r:],
            paths[:r] + [list(p) for p in new_paths] + paths[r + 1:])


def range_set_paths_host(paths, first, new_paths):
    """Host model of RangeMap.set_paths: the paths after those of [first, first + len(new_paths))
    have been replaced"""
    paths = [list(p) for p in paths]
    return paths[:first] + [list(p) for p in new_paths] + paths[first + len(new_paths):]


def _csr(seqs, dtype):
    """(flat array of `dtype` with one spare element, uint64 offsets) of a list of sequences"""
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(np.array([len(x) for x in seqs], dtype=np.uint64), out=off[1:])
    flat = np.fromiter((i for x in seqs for i in x), dtype=dtype, count=int(off[-1]))
    return np.ascontiguousarray(np.append(flat, dtype(0))), off


_route_scratch = {}  # (engine, stream) -> the scratch of the last route call issued there


class RangeMap:
    """A resident table of R key ranges and their member lists (rf_amd_range_map):
    boundaries = the R - 1 boundary keys as `bytes`, strictly ascending in `bytes` order; lists =
    R sequences of member ids (of whatever FilterSet the caller probes), each of at most 65,535.
    Range r holds the keys k with boundaries[r-1] <= k < boundaries[r]. A map made this way is
    immutable; one made by from_segments follows the trunk through update_segments, and one made
    there with room= follows node splits through split and set_paths. num_ranges is the current R."""

    def __init__(self, boundaries, lists, engine=None):
        self.engine = engine or default_engine()
        boundaries = [bytes(b) for b in boundaries]
        R = len(lists)
        if R != len(boundaries) + 1:
            raise ValueError("R lists take R - 1 boundaries")
        boff = np.zeros(max(R, 1), dtype=np.uint64)
        np.cumsum(np.array([len(b) for b in boundaries], dtype=np.uint64), out=boff[1:R])
        bbytes = np.frombuffer(b"".join(boundaries) + b"\0", dtype=np.uint8)
        loff = np.zeros(R + 1, dtype=np.uint64)
        np.cumsum(np.array([len(x) for x in lists], dtype=np.uint64), out=loff[1:])
        flat = np.fromiter((i for x in lists for i in x), dtype=np.uint32, count=int(loff[-1]))
        flat = np.ascontiguousarray(np.append(flat, np.uint32(0)))
        h = ctypes.c_void_p()
        _check(load_library().rf_amd_range_map_create(self.engine.h, R, bbytes.ctypes.data, boff.ctypes.data,
                                                      flat.ctypes.data, loff.ctypes.data, ctypes.byref(h)))
        self.h = h
        self.num_ranges = R
        self.num_segments = 0
        self.max_list = int(load_library().rf_amd_range_map_max_list(h))

    @staticmethod
    def _bound_arrays(boundaries, R):
        boundaries = [bytes(b) for b in boundaries]
        if R != len(boundaries) + 1:
            raise ValueError("R ranges take R - 1 boundaries")
        boff = np.zeros(max(R, 1), dtype=np.uint64)
        np.cumsum(np.array([len(b) for b in boundaries], dtype=np.uint64), out=boff[1:R])
        return np.frombuffer(b"".join(boundaries) + b"\0", dtype=np.uint8), boff

    @classmethod
    def from_segments(cls, boundaries, paths, seg_lists, seg_caps=None, engine=None, room=None):
        """rf_amd_range_map_create_segments: R = len(paths) ranges; paths[r] = range r's segment
        ids, root to leaf; seg_lists[s] = segment s's initial ids; seg_caps[s] = the ids it has
        room for (None: its initial length). Range r's list is the concatenation of its path's
        segments' current lists (range_segment_lists); max_list is the largest sum of a path's
        capacities, which no update can exceed.
        room (rf_amd_range_map_create_segments_room): a RangeRoom or a dict of its fields --
        ranges, bound_bytes, path_entries, list_ids, max_list -- the most the map may grow to by
        split and set_paths; max_list is then room's."""
        self = cls.__new__(cls)
        self.h = None
        self.engine = engine or default_engine()
        R, S = len(paths), len(seg_lists)
        bbytes, boff = cls._bound_arrays(boundaries, R)
        path, poff = _csr(paths, np.uint32)
        ids, soff = _csr(seg_lists, np.uint32)
        caps = [len(x) for x in seg_lists] if seg_caps is None else seg_caps
        if len(caps) != S:
            raise ValueError("seg_caps and seg_lists differ in length")
        caps = np.ascontiguousarray(np.append(np.asarray(caps, dtype=np.uint32), np.uint32(0)))
        h = ctypes.c_void_p()
        args = (self.engine.h, R, bbytes.ctypes.data, boff.ctypes.data, path.ctypes.data, poff.ctypes.data, S,
                caps.ctypes.data, ids.ctypes.data, soff.ctypes.data)
        if room is None:
            _check(load_library().rf_amd_range_map_create_segments(*args, ctypes.byref(h)))
        else:
            room = room if isinstance(room, RangeRoom) else RangeRoom(**room)
            if R == 1:  # the map every trunk starts as: no boundary arrays at all
                args = args[:2] + (None, None) + args[4:]
            _check(load_library().rf_amd_range_map_create_segments_room(*args, ctypes.byref(room), ctypes.byref(h)))
        self.h = h
        self.num_ranges = R
        self.num_segments = int(load_library().rf_amd_range_map_num_segments(h))
        self.max_list = int(load_library().rf_amd_range_map_max_list(h))
        return self

    def update_segments(self, ids, lists, stream=None):
        """rf_amd_range_map_update_segments: segment ids[i]'s list becomes lists[i], in stream
        order and without a host wait -- a route call queued on `stream` before the call sees the
        old lists, one queued after it the new ones. An id named twice: the last entry wins. The
        caller orders other streams and serialises calls on one map."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        lists = list(lists)
        if len(lists) != ids.size:
            raise ValueError("ids and lists differ in length")
        flat, off = _csr(lists, np.uint32)
        _check(load_library().rf_amd_range_map_update_segments(
            self.h, ids.ctypes.data if ids.size else None, flat.ctypes.data if ids.size else None,
            off.ctypes.data if ids.size else None, ids.size, _stream(stream)))

    def split(self, range, boundaries, paths, stream=None):
        """rf_amd_range_map_split on a map made with room: range `range` becomes len(paths)
        ranges cut by the len(paths) - 1 new `boundaries` (strictly inside the range, ascending),
        with those paths; one path and no boundary replaces the range's path only. In stream
        order and without a host wait, like update_segments: a route call queued before it sees
        the old table and range numbers, one queued after it the new. num_ranges is the new R on
        return. A call that exceeds the room raises with code STATUS_NO_SPACE and changes nothing."""
        paths = list(paths)
        boundaries = [bytes(b) for b in boundaries]
        if paths and len(boundaries) != len(paths) - 1:
            raise ValueError("m pieces take m - 1 boundaries")
        boff = np.zeros(len(boundaries) + 1, dtype=np.uint64)
        np.cumsum(np.array([len(b) for b in boundaries], dtype=np.uint64), out=boff[1:])
        bbytes = np.frombuffer(b"".join(boundaries) + b"\0", dtype=np.uint8)
        path, poff = _csr(paths, np.uint32)
        _check(load_library().rf_amd_range_map_split(self.h, range, len(paths), bbytes.ctypes.data, boff.ctypes.data,
                                                     path.ctypes.data, poff.ctypes.data, _stream(stream)))
        self.num_ranges = int(load_library().rf_amd_range_map_num_ranges(self.h))

    def set_paths(self, first, paths, stream=None):
        """rf_amd_range_map_set_paths on a map made with room: the paths of ranges [first, first +
        len(paths)) are replaced, in stream order like split -- an index split's outcome, or over
        all ranges a new root level"""
        paths = list(paths)
        path, poff = _csr(paths, np.uint32)
        _check(load_library().rf_amd_range_map_set_paths(self.h, first, len(paths), path.ctypes.data,
                                                         poff.ctypes.data, _stream(stream)))

    def close(self):
        if getattr(self, "h", None):
            load_library().rf_amd_range_map_destroy(self.h)
            self.h = None

    def close_on(self, stream):
        """rf_amd_range_map_destroy_on: release the map in stream order (every route call on it
        must be ordered before the current end of `stream`), without a wait. What the route
        calls wrote stays valid: it is a copy."""
        if getattr(self, "h", None):
            _check(load_library().rf_amd_range_map_destroy_on(self.h, _stream(stream)))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _route(self, call, n, pair_cap, stream, device):
        import torch
        st = _stream(stream)
        cap = n * self.max_list if pair_cap is None else int(pair_cap)
        d_range = torch.empty(n, dtype=torch.int32, device=device)
        d_off = torch.empty(n + 1, dtype=torch.int64, device=device)
        d_member = torch.empty(cap, dtype=torch.int32, device=device)
        d_total = torch.empty(1, dtype=torch.int64, device=device)
        scratch = torch.empty(range_route_scratch_bytes(n) // 8, dtype=torch.int64, device=device)
        _check(call(d_range.data_ptr() if n else None, d_off.data_ptr(), d_member.data_ptr() if cap else None, cap,
                    d_total.data_ptr(), scratch.data_ptr(), st))
        _route_scratch[(id(self.engine), st)] = scratch
        return d_range, d_off, d_member, d_total

    def route_keys(self, d_keys, key_len, n, pair_cap=None, stream=None):
        """rf_amd_range_map_route_keys: n fixed-length device keys to (d_range int32[n],
        d_member_off int64[n + 1], d_member int32[pair_cap], d_total int64[1]), asynchronously:
        key i's range, and the CSR of the ranges' lists that probe_keys_ragged reads. pair_cap
        None: n * the map's longest list, which never overflows; the offsets and the total are
        the true values whatever pair_cap is."""
        L = load_library()
        return self._route(lambda *a: L.rf_amd_range_map_route_keys(self.h, _dptr(d_keys), key_len, n, *a),
                           n, pair_cap, stream, getattr(d_keys, "device", "cuda"))

    def route_var_keys(self, d_bytes, d_offsets, n, pair_cap=None, stream=None):
        """route_keys for variable-length keys: key i is d_bytes[d_offsets[i] : d_offsets[i+1]]"""
        L = load_library()
        return self._route(lambda *a: L.rf_amd_range_map_route_var_keys(self.h, _dptr(d_bytes), _dptr(d_offsets),
                                                                        n, *a),
                           n, pair_cap, stream, getattr(d_offsets, "device", "cuda"))
