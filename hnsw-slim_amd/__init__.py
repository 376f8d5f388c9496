"""hnsw_slim_amd -- thin ctypes binding over the C ABI (include/hnsw_slim_amd.h) of the MI355X-native
HNSW / HNSW-Slim batched search engine.  Used by tests/ and bench.py; the drop-in surface for C++
callers is hnsw-slim_amd/hnswlib/hnswlib_amd.h.

There is no CPU search path here: if the HIP library is missing or no device is visible, index
loading / searching raises (fails loudly) instead of falling back.
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HS_LIB", os.path.join(_HERE, "libhnsw_slim_amd.so"))  # HS_LIB: diagnostic builds only

HS_KIND_HNSW, HS_KIND_SLIM, HS_KIND_SLIMQ = 0, 1, 2
HS_METRIC_L2, HS_METRIC_IP = 0, 1
HS_MODE_SLIM_IDS, HS_MODE_PQ = 0, 1
HS_ROWS_F32, HS_ROWS_F16, HS_ROWS_U8 = 0, 1, 2   # hs_row_format (narrow rows: Index.set_row_format)
HS_OK, HS_ERR_IO, HS_ERR_CORRUPT, HS_ERR_NOMEM, HS_ERR_INVALID, HS_ERR_UNSUPPORTED, HS_ERR_DEVICE, HS_ERR_CAPACITY = range(8)

EXPORTS = [
    "hs_last_error", "hs_device_count", "hs_index_load", "hs_index_load_mem", "hs_index_free", "hs_set_ef", "hs_index_info",
    "hs_set_capacity", "hs_set_exact_order", "hs_search_batch", "hs_search_batch_dev", "hs_search_check", "hs_search_batch_raw", "hs_search_batch_filtered", "hs_labels",
    "hs_build_hnsw", "hs_build_hnsw_labeled", "hs_convert_slim", "hs_rabitq_rotate", "hs_rabitq_quantize_data", "hs_rabitq_prepare_query",
    "hs_rabitq_estimate", "hs_convert_slimq", "hs_rabitq_default_tconst", "hs_slimq_set_dataset", "hs_slimq_set_tconst", "hs_slimq_get_tconst",
    "hs_slimq_search_batch", "hs_slimq_search_batch_dev", "hs_slimq_trace", "hs_slimq_prepare_debug", "hs_brute_force", "hs_brute_force_dev",
    "hs_search_batch_async", "hs_host_alloc", "hs_host_free", "hs_comm_init", "hs_comm_free", "hs_comm_size", "hs_search_batch_sharded",
    "hs_comm_results_dev", "hs_convert_slim_gpu", "hs_index_patch", "hs_index_from_host_arrays", "hs_build_rabitq_hnsw",
    "hs_convert_slimq_graph", "hs_host_device_pointer", "hs_index_set_row_format", "hs_index_row_format", "hs_rows_representable",
    "hs_index_set_f32_resident", "hs_index_f32_resident", "hs_rows_to_narrow", "hs_index_load_narrow",
    "hs_filter_row_words", "hs_filter_pack", "hs_filter_set_create", "hs_filter_set_free", "hs_filter_set_write", "hs_filter_set_write_bits",
    "hs_filter_set_write_dev", "hs_filter_set_read", "hs_filter_set_info", "hs_search_batch_filter_set", "hs_search_batch_filter_set_dev",
    "hs_index_exact_search", "hs_index_exact_search_dev",
    "hs_index_add_points", "hs_index_seed_levels", "hs_index_mark_deleted", "hs_index_save", "hs_index_get_row", "hs_index_capacity",
    "hs_index_deleted_count", "hs_hnsw_resume",
    "hs_index_set_replace_deleted", "hs_index_upsert_points", "hs_index_resize", "hs_hnsw_replay",
    "hs_queue_create", "hs_queue_free", "hs_queue_submit", "hs_queue_submit_dev", "hs_queue_flush", "hs_queue_wait",
    "hs_queue_join_stream", "hs_queue_drain", "hs_queue_info",
    "hs_build_hnsw_batched", "hs_build_schedule",
    "hs_index_add_points_batched", "hs_hnsw_resume_batched", "hs_debug_batched_add_changed",
    "hs_build_rabitq_hnsw_batched", "hs_debug_rq_raw_dist",
    "hs_convert_slimq_graph_gpu", "hs_convert_slimq_gpu", "hs_convert_hnsw_to_slimq", "hs_debug_rq_quantize_rows",
    "hs_build_rabitq_hnsw_batched_mem", "hs_graph_load", "hs_graph_save", "hs_graph_info", "hs_graph_free", "hs_graph_convert_slimq",
    "hs_slimq_index_from_rows", "hs_slimq_index_save", "hs_debug_slimq_arrays", "hs_debug_slimq_arrays_host",
]


class HsError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(msg)
        self.status = status


class HsSlimqConvertStats(ctypes.Structure):
    _fields_ = [("graph_used_gpu", ctypes.c_int), ("records_used_gpu", ctypes.c_int), ("graph_kernel_ms", ctypes.c_double),
                ("records_kernel_ms", ctypes.c_double), ("graph_ms", ctypes.c_double), ("records_ms", ctypes.c_double),
                ("total_ms", ctypes.c_double)]


class HsSlimqParams(ctypes.Structure):   # hs_slimq_params
    _fields_ = [("threshold_level", ctypes.c_int), ("top_degree_percent0", ctypes.c_float), ("top_degree_percent", ctypes.c_float),
                ("top_degree_M0", ctypes.c_size_t), ("low_degree_m0", ctypes.c_size_t), ("top_degree_M", ctypes.c_size_t),
                ("low_degree_m", ctypes.c_size_t), ("centroids", ctypes.c_void_p), ("num_cluster", ctypes.c_size_t),
                ("cluster_ids", ctypes.c_void_p), ("flip_seed", ctypes.c_uint64)]


class HsInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint64), ("dim", ctypes.c_uint64), ("kind", ctypes.c_int32), ("metric", ctypes.c_int32),
                ("maxlevel", ctypes.c_int32), ("threshold_level", ctypes.c_int32), ("enterpoint", ctypes.c_uint32),
                ("has_deleted", ctypes.c_int32), ("n_edges", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64),
                ("max_degree0", ctypes.c_uint64), ("index_size", ctypes.c_uint64)]


_i32, _u32, _u64 = ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64
HS_PLAN_FLAT, HS_PLAN_LEAN, HS_PLAN_FAST, HS_PLAN_STRICT = range(4)   # hs_plan_family
PLAN_KERNELS = {None: 0, "lean": 1, "fast": 2}                       # hs_plan_kernel (HS_KERNEL)


class HsPlanDiag(ctypes.Structure):   # hs_plan_diag: the diagnostic environment knobs
    _fields_ = [("kernel", _i32), ("lean_forced", _i32), ("lean_min_ef", _u32), ("order", _i32), ("flat", _i32), ("vis16", _i32),
                ("flat_waves_per_cu", _i32), ("zero_copy", _i32), ("verbose", _i32), ("slimq_fused", _i32)]


class HsPlanIn(ctypes.Structure):     # hs_plan_in: everything the launch plan of a search may depend on
    _fields_ = [("n", _u64), ("dim", _u64), ("has_tile0", _i32), ("has_uptile", _i32), ("maxlevel", _i32), ("threshold_level", _i32),
                ("has_deleted", _i32), ("kind", _i32), ("ef", _u64), ("k", _u64), ("nq", _u64), ("mode", _i32),
                ("user_cand_cap", _u32), ("user_hash_slots", _u32), ("grow_cand", _u32), ("grow_hash", _u32),
                ("exact_order", _i32), ("want_raw", _i32), ("has_filter", _i32), ("row_fmt", _i32), ("f32_resident", _i32),
                ("has_dup0", _i32), ("diag", HsPlanDiag)]


class HsPlanOut(ctypes.Structure):    # hs_plan_out
    _fields_ = [("family", _i32), ("rows", _i32), ("split", _i32), ("skip_order", _i32), ("ef", _u32), ("mark_ep", _u32),
                ("cand_cap", _u32), ("hash_slots", _u32), ("vis_bits", _u32), ("hash_fill_shift", _u32), ("flat", _u32), ("lds_bytes", _u32),
                ("fl_nb", _u32), ("fl_mul", _u32), ("fl_sh", _u32), ("fl_bits", _u32), ("fl_ok", _u32),
                ("rerun_rows", _i32), ("rerun_select_mask", _u32), ("rerun_cand_cap", _u32), ("rerun_hash_slots", _u32),
                ("spill_stride", _u32), ("log_cap", _u32), ("hop_cap", _u32), ("name", ctypes.c_char_p)]


class HsQueueInfo(ctypes.Structure):  # struct hs_queue_info
    _fields_ = [("submitted", _u64), ("launches", _u64), ("pending", _u64), ("in_flight", _u64), ("largest_launch", _u64),
                ("device_bytes", _u64)]


class HsBatchBuildOpts(ctypes.Structure):    # hs_batch_build_opts
    _fields_ = [("device", _i32), ("threads", _i32), ("grow_div", _u64), ("batch_max", _u64), ("scratch_ids", _u64)]


class HsBatchBuildStats(ctypes.Structure):   # hs_batch_build_stats
    _fields_ = [("used_gpu", _i32), ("reserved", _u32), ("batches", _u64), ("flagged_rows", _u64), ("kernel_ms", ctypes.c_double),
                ("total_ms", ctypes.c_double)]


class HsSlimqPipelineStats(ctypes.Structure):   # hs_slimq_pipeline_stats
    _fields_ = [("build", HsBatchBuildStats), ("convert", HsSlimqConvertStats), ("resident_ms", ctypes.c_double),
                ("tile_kernel_ms", ctypes.c_double), ("total_ms", ctypes.c_double)]


class HsFastShape(ctypes.Structure):  # hs_fast_shape
    _fields_ = [("d16", _i32), ("slots", _i32), ("wb", _i32)]


def build_library(force=False):
    """Compile the HIP extension in-tree (hipcc --offload-arch=gfx950)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-C", _HERE, "libhnsw_slim_amd.so"] + (["-B"] if force else []))
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HsError(HS_ERR_DEVICE, f"{LIB_PATH} is missing: build it with `make -C hnsw-slim_amd` "
                      "(__graft_entry__.build()); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    vp, sz, ci, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
    L.hs_last_error.restype = ctypes.c_char_p
    L.hs_device_count.restype = ci
    L.hs_index_load.argtypes = [ctypes.c_char_p, ci, ci, sz, sz, ci, ctypes.POINTER(vp)]
    L.hs_index_load_mem.argtypes = [ctypes.c_char_p, sz, ci, ci, sz, sz, ci, ctypes.POINTER(vp)]
    L.hs_index_patch.argtypes = [vp, ctypes.c_char_p, sz, ci]
    L.hs_index_from_host_arrays.argtypes = [ci, ci, sz, sz, vp, vp, vp, vp, vp, vp, u32, ctypes.c_int32, ctypes.c_int32, ci, ctypes.POINTER(vp)]
    L.hs_index_free.argtypes = [vp]
    L.hs_index_free.restype = None
    L.hs_set_ef.argtypes = [vp, sz]
    L.hs_index_info.argtypes = [vp, ctypes.POINTER(HsInfo)]
    L.hs_index_set_row_format.argtypes = [vp, ci]
    L.hs_index_row_format.argtypes = [vp]
    L.hs_rows_representable.argtypes = [vp, sz, sz, ci, ctypes.POINTER(ctypes.c_uint64)]
    L.hs_index_set_f32_resident.argtypes = [vp, ci]
    L.hs_index_f32_resident.argtypes = [vp]
    L.hs_rows_to_narrow.argtypes = [vp, sz, sz, ci, vp, ctypes.POINTER(ctypes.c_uint64)]
    L.hs_index_load_narrow.argtypes = [ctypes.c_char_p, ci, ci, sz, sz, ci, ci, ctypes.POINTER(vp)]
    L.hs_last_kernel.argtypes = [vp]
    L.hs_last_kernel.restype = ctypes.c_char_p
    L.hs_set_capacity.argtypes = [vp, u32, u32]
    L.hs_set_exact_order.argtypes = [vp, ci]
    L.hs_search_batch.argtypes = [vp, vp, sz, sz, ci, vp, vp, vp, vp, vp]
    L.hs_search_batch_dev.argtypes = [vp, vp, sz, sz, ci, vp, vp, vp, vp, vp, vp]
    L.hs_search_check.argtypes = [vp, vp]
    L.hs_debug_heap_ops.argtypes = [vp, sz, ci, u32, vp, vp, vp]
    if "HS_LIB" not in os.environ or hasattr(L, "hs_debug_search_plan"):   # (a baseline build in an A/B run may predate these two)
        L.hs_debug_search_plan.argtypes = [ctypes.POINTER(HsPlanIn), ctypes.POINTER(HsPlanOut)]
        L.hs_debug_plan_input.argtypes = [vp, sz, sz, ci, ci, ctypes.POINTER(HsPlanIn)]
    if "HS_LIB" not in os.environ or hasattr(L, "hs_debug_fast_shape"):
        L.hs_debug_fast_shape.argtypes = [ci, _u64, _u64, _u64, ci, ctypes.POINTER(HsFastShape)]
    L.hs_search_batch_async.argtypes = [vp, vp, sz, sz, ci, vp, vp, vp, vp, vp, vp]
    L.hs_host_alloc.restype = vp
    L.hs_host_alloc.argtypes = [sz]
    L.hs_host_free.restype = None
    L.hs_host_free.argtypes = [vp]
    L.hs_comm_init.argtypes = [ci, vp, ctypes.POINTER(vp)]
    L.hs_comm_free.restype = None
    L.hs_comm_free.argtypes = [vp]
    L.hs_comm_size.argtypes = [vp]
    L.hs_search_batch_sharded.argtypes = [vp, vp, vp, sz, sz, ci, vp, vp, vp, vp]
    L.hs_search_batch_sharded_async.argtypes = [vp, vp, vp, sz, sz, ci, vp, vp, vp, vp, ci]
    L.hs_comm_check.argtypes = [vp, vp, ci]
    L.hs_comm_slots.argtypes = [vp]
    L.hs_comm_results_dev.argtypes = [vp, ci, vp, vp, vp, vp]
    L.hs_search_batch_raw.argtypes = [vp, vp, sz, sz, ci, vp, vp, vp, vp]
    L.hs_search_batch_filtered.argtypes = [vp, vp, sz, sz, vp, vp, vp, vp, vp]
    L.hs_labels.argtypes = [vp, vp]
    L.hs_filter_row_words.restype = sz
    L.hs_filter_row_words.argtypes = [sz]
    L.hs_filter_pack.argtypes = [vp, sz, sz, vp]
    L.hs_filter_set_create.argtypes = [vp, sz, ctypes.POINTER(vp)]
    L.hs_filter_set_free.restype = None
    L.hs_filter_set_free.argtypes = [vp]
    L.hs_filter_set_write.argtypes = [vp, sz, sz, vp]
    L.hs_filter_set_write_bits.argtypes = [vp, sz, sz, vp]
    L.hs_filter_set_write_dev.argtypes = [vp, sz, sz, vp, vp]
    L.hs_filter_set_read.argtypes = [vp, sz, vp]
    L.hs_filter_set_info.argtypes = [vp, vp, vp, vp, vp]
    L.hs_search_batch_filter_set.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp, vp]
    L.hs_search_batch_filter_set_dev.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp, vp, vp]
    L.hs_index_exact_search.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp]
    if "HS_LIB" not in os.environ or hasattr(L, "hs_queue_create"):   # (a baseline build in an A/B run may predate the queue)
        pu64 = ctypes.POINTER(ctypes.c_uint64)
        L.hs_queue_create.argtypes = [vp, sz, ci, sz, ci, vp, ctypes.POINTER(vp)]
        L.hs_queue_free.restype = None
        L.hs_queue_free.argtypes = [vp]
        L.hs_queue_submit.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, pu64]
        L.hs_queue_submit_dev.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, pu64]
        L.hs_queue_flush.argtypes = [vp]
        L.hs_queue_wait.argtypes = [vp, ctypes.c_uint64]
        L.hs_queue_join_stream.argtypes = [vp, ctypes.c_uint64, vp]
        L.hs_queue_drain.argtypes = [vp]
        L.hs_queue_info.argtypes = [vp, ctypes.POINTER(HsQueueInfo)]
    L.hs_index_exact_search_dev.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp, vp]
    L.hs_index_add_points.argtypes = [vp, vp, vp, sz, ci]
    L.hs_index_seed_levels.argtypes = [vp, sz, sz]
    L.hs_index_mark_deleted.argtypes = [vp, vp, sz, ci]
    L.hs_index_save.argtypes = [vp, ctypes.c_char_p]
    L.hs_index_get_row.argtypes = [vp, ctypes.c_uint64, vp]
    L.hs_index_capacity.restype = sz
    L.hs_index_capacity.argtypes = [vp]
    L.hs_index_deleted_count.restype = sz
    L.hs_index_deleted_count.argtypes = [vp]
    L.hs_hnsw_resume.argtypes = [ctypes.c_char_p, ci, sz, sz, vp, vp, sz, sz, sz, ci, ctypes.c_char_p]
    L.hs_index_set_replace_deleted.argtypes = [vp, ci]
    L.hs_index_upsert_points.argtypes = [vp, vp, vp, vp, sz]
    L.hs_index_resize.argtypes = [vp, sz]
    L.hs_hnsw_replay.argtypes = [ctypes.c_char_p, ci, sz, sz, ci, vp, sz, vp, ctypes.c_char_p]
    L.hs_build_hnsw.argtypes = [vp, sz, sz, ci, sz, sz, ctypes.c_char_p, sz, ci, ctypes.c_char_p]
    L.hs_build_hnsw_labeled.argtypes = [vp, vp, sz, sz, ci, sz, sz, ctypes.c_char_p, sz, ci, ctypes.c_char_p]
    if "HS_LIB" not in os.environ or hasattr(L, "hs_build_hnsw_batched"):   # (a baseline build in an A/B run may predate these)
        L.hs_build_hnsw_batched.argtypes = [vp, vp, sz, sz, ci, sz, sz, ctypes.c_char_p, sz, ctypes.POINTER(HsBatchBuildOpts), ctypes.c_char_p,
                                            ctypes.POINTER(HsBatchBuildStats)]
        L.hs_build_schedule.argtypes = [sz, sz, ctypes.c_char_p, sz, sz, sz, sz, vp, vp, vp, ctypes.POINTER(sz)]
    if "HS_LIB" not in os.environ or hasattr(L, "hs_index_add_points_batched"):
        L.hs_index_add_points_batched.argtypes = [vp, vp, vp, sz, ctypes.POINTER(HsBatchBuildOpts), ctypes.POINTER(HsBatchBuildStats)]
        L.hs_debug_batched_add_changed.argtypes = [vp, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(sz)]
        L.hs_hnsw_resume_batched.argtypes = [ctypes.c_char_p, ci, sz, sz, vp, vp, sz, sz, sz, ctypes.POINTER(HsBatchBuildOpts), ctypes.c_char_p,
                                             ctypes.POINTER(HsBatchBuildStats)]
    L.hs_convert_slim.argtypes = [ctypes.c_char_p, ci, sz, ci, ctypes.c_float, ctypes.c_float, sz, sz, sz, sz, ci, ctypes.c_char_p]
    L.hs_convert_slimq_graph.argtypes = L.hs_convert_slim.argtypes
    L.hs_host_device_pointer.restype = ctypes.c_void_p
    L.hs_host_device_pointer.argtypes = [vp]
    L.hs_build_rabitq_hnsw.argtypes = [vp, sz, sz, ci, sz, sz, sz, ci, ctypes.c_char_p]
    if "HS_LIB" not in os.environ or hasattr(L, "hs_build_rabitq_hnsw_batched"):   # (a baseline build in an A/B run may predate these)
        L.hs_build_rabitq_hnsw_batched.argtypes = [vp, sz, sz, ci, sz, sz, sz, ctypes.POINTER(HsBatchBuildOpts), ctypes.c_char_p,
                                                   ctypes.POINTER(HsBatchBuildStats)]
        L.hs_debug_rq_raw_dist.argtypes = [vp, vp, sz, sz, ci, ci, vp]
    L.hs_convert_slim_gpu.argtypes = [ctypes.c_char_p, ci, sz, ci, ctypes.c_float, ctypes.c_float, sz, sz, sz, sz, ci, ci, ctypes.c_char_p,
                                      ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_double)]
    L.hs_convert_slimq.argtypes = [ctypes.c_char_p, ci, sz, vp, sz, vp, ctypes.c_uint64, ci, ctypes.c_char_p]
    if "HS_LIB" not in os.environ or hasattr(L, "hs_convert_hnsw_to_slimq"):   # (a baseline build in an A/B run may predate these)
        L.hs_convert_slimq_graph_gpu.argtypes = L.hs_convert_slim_gpu.argtypes
        L.hs_convert_slimq_gpu.argtypes = [ctypes.c_char_p, ci, sz, vp, sz, vp, ctypes.c_uint64, ci, ci, ctypes.c_char_p, ctypes.POINTER(ci),
                                           ctypes.POINTER(ctypes.c_double)]
        L.hs_convert_hnsw_to_slimq.argtypes = [ctypes.c_char_p, ci, sz, ci, ctypes.c_float, ctypes.c_float, sz, sz, sz, sz, vp, sz, vp, ctypes.c_uint64,
                                               ci, ci, ctypes.c_char_p, ctypes.POINTER(HsSlimqConvertStats)]
        L.hs_debug_rq_quantize_rows.argtypes = [sz, ci, vp, vp, sz, vp, sz, vp, ci, vp, vp, vp, vp]
    if "HS_LIB" not in os.environ or hasattr(L, "hs_graph_convert_slimq"):   # (a baseline build in an A/B run may predate these)
        pu64, pu32 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
        L.hs_build_rabitq_hnsw_batched_mem.argtypes = [vp, sz, sz, ci, sz, sz, sz, ctypes.POINTER(HsBatchBuildOpts), ctypes.POINTER(vp),
                                                       ctypes.POINTER(HsBatchBuildStats)]
        L.hs_graph_load.argtypes = [ctypes.c_char_p, ci, sz, ctypes.POINTER(vp)]
        L.hs_graph_save.argtypes = [vp, ctypes.c_char_p]
        L.hs_graph_info.argtypes = [vp, pu64, pu64, ctypes.POINTER(ci), pu64, pu64, ctypes.POINTER(ci)]
        L.hs_graph_free.argtypes = [vp]
        L.hs_graph_free.restype = None
        L.hs_graph_convert_slimq.argtypes = [vp, ctypes.POINTER(HsSlimqParams), ci, ci, ctypes.c_char_p, ci, ci, ctypes.POINTER(vp),
                                             ctypes.POINTER(HsSlimqConvertStats)]
        L.hs_slimq_index_from_rows.argtypes = [vp, sz, sz, ci, sz, sz, sz, ctypes.POINTER(HsBatchBuildOpts), ctypes.POINTER(HsSlimqParams), ci, ci,
                                               ctypes.POINTER(vp), ctypes.POINTER(HsSlimqPipelineStats)]
        L.hs_slimq_index_save.argtypes = [vp, ctypes.c_char_p]
        L.hs_debug_slimq_arrays.argtypes = [vp, ci, vp, sz, ctypes.POINTER(sz), pu32, pu32]
        L.hs_debug_slimq_arrays_host.argtypes = [ctypes.c_char_p, ci, sz, ci, ci, vp, sz, ctypes.POINTER(sz), pu32, pu32]
    if "HS_LIB" not in os.environ or hasattr(L, "hs_slim_convert_diff"):   # (a baseline build in an A/B run may predate these)
        psz = ctypes.POINTER(sz)
        L.hs_slim_convert_diff.argtypes = [vp, vp, ctypes.c_float, ctypes.c_float, sz, sz, sz, sz, ci, ctypes.POINTER(vp), ctypes.POINTER(ci),
                                           ctypes.POINTER(ctypes.c_double)]
        L.hs_slim_diff_info.argtypes = [vp, psz, psz, psz, psz]
        L.hs_slim_diff_ids.argtypes = [vp, vp, vp]
        L.hs_slim_diff_stream.argtypes = [vp, vp, vp, sz, psz]
        L.hs_slim_diff_next.argtypes = [vp, vp, sz, ci, vp, sz, psz, psz, psz, ctypes.POINTER(ci)]
        L.hs_slim_diff_free.argtypes = [vp]
        L.hs_slim_diff_free.restype = None
        L.hs_slim_index_save.argtypes = [vp, ctypes.c_char_p]
        L.hs_slim_convert_diff_files.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ci, sz, ci, ctypes.c_float, ctypes.c_float, sz, sz, sz, sz, ci,
                                                 ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(vp)]
    L.hs_rabitq_default_tconst.restype = ctypes.c_double
    L.hs_rabitq_default_tconst.argtypes = [sz, ctypes.c_uint64]
    L.hs_slimq_set_dataset.argtypes = [vp, vp, sz, sz]
    L.hs_slimq_set_tconst.argtypes = [vp, ctypes.c_double]
    L.hs_slimq_get_tconst.restype = ctypes.c_double
    L.hs_slimq_get_tconst.argtypes = [vp]
    L.hs_slimq_search_batch.argtypes = [vp, vp, sz, sz, vp, vp, vp, vp]
    L.hs_slimq_search_batch_dev.argtypes = [vp, vp, sz, sz, vp, vp, vp, vp, vp]
    L.hs_slimq_trace.argtypes = [vp, vp, sz, sz, vp, sz, vp]
    L.hs_slimq_prepare_debug.argtypes = [vp, vp, sz, vp]
    L.hs_brute_force.argtypes = [vp, sz, sz, ci, vp, vp, sz, sz, ci, vp, vp, vp]
    L.hs_brute_force_dev.argtypes = [vp, vp, sz, sz, ci, vp, sz, sz, vp, vp, vp, vp]
    L.hs_rabitq_rotate.argtypes = [sz, vp, vp, sz, vp]
    L.hs_rabitq_quantize_data.argtypes = [sz, ci, vp, sz, vp, vp, vp]
    L.hs_rabitq_prepare_query.argtypes = [sz, ctypes.c_double, vp, sz, vp, vp]
    L.hs_rabitq_estimate.argtypes = [sz, vp, vp, sz, vp, vp, vp, vp, sz, vp]
    _lib = L
    return L


def _check(rc):
    if rc != HS_OK:
        raise HsError(rc, lib().hs_last_error().decode())


def device_count():
    return lib().hs_device_count()


def build_hnsw(base, out_path, metric=HS_METRIC_L2, M=16, ef_construction=200, branching_factor="4", seed=100, threads=1, labels=None):
    """HierarchicalNSW ctor + addPoint loop (labels = row index unless given) + saveIndex, on the CPU (harness)."""
    base = np.ascontiguousarray(base, np.float32)
    if labels is not None:
        lab = np.ascontiguousarray(labels, np.uint64)
        if lab.shape != (base.shape[0],):
            raise HsError(HS_ERR_INVALID, "labels: one per row")
        _check(lib().hs_build_hnsw_labeled(base.ctypes.data, lab.ctypes.data, base.shape[0], base.shape[1], metric, M, ef_construction,
                                           str(branching_factor).encode(), seed, threads, out_path.encode()))
        return
    _check(lib().hs_build_hnsw(base.ctypes.data, base.shape[0], base.shape[1], metric, M, ef_construction,
                               str(branching_factor).encode(), seed, threads, out_path.encode()))


def build_hnsw_batched(base, out_path, metric=HS_METRIC_L2, M=16, ef_construction=200, branching_factor="4", seed=100, device=-1, threads=1,
                       grow_div=0, batch_max=0, scratch_ids=0, labels=None):
    """hs_build_hnsw_batched: batched addPoint on HIP device `device`, or on the host twin (device=-1, `threads` workers);
    both write the same file, and batch_max=1 writes build_hnsw(threads=1)'s.  Returns the stats as a dict: used_gpu, batches,
    flagged_rows, kernel_ms, total_ms."""
    base = np.ascontiguousarray(base, np.float32)
    if base.ndim != 2:
        raise HsError(HS_ERR_INVALID, "base: rows x dim")
    lab = None
    if labels is not None:
        lab = np.ascontiguousarray(labels, np.uint64)
        if lab.shape != (base.shape[0],):
            raise HsError(HS_ERR_INVALID, "labels: one per row")
    opts = HsBatchBuildOpts(device, threads, grow_div, batch_max, scratch_ids)
    st = HsBatchBuildStats()
    _check(lib().hs_build_hnsw_batched(base.ctypes.data, lab.ctypes.data if lab is not None else None, base.shape[0], base.shape[1], metric, M,
                                       ef_construction, str(branching_factor).encode(), seed, ctypes.byref(opts), out_path.encode(),
                                       ctypes.byref(st)))
    return {"used_gpu": bool(st.used_gpu), "batches": int(st.batches), "flagged_rows": int(st.flagged_rows), "kernel_ms": st.kernel_ms,
            "total_ms": st.total_ms}


def build_schedule(n, M=16, branching_factor="4", seed=100, grow_div=0, batch_max=0):
    """hs_build_schedule (host only): the batches build_hnsw_batched inserts n rows in -- their sizes, and the entry point (0xFFFFFFFF:
    none yet) and top level (-1) before each."""
    nb = ctypes.c_size_t(0)
    bf = str(branching_factor).encode()
    _check(lib().hs_build_schedule(n, M, bf, seed, grow_div, batch_max, 0, None, None, None, ctypes.byref(nb)))
    sizes, eps, tops = np.zeros(nb.value, np.uint32), np.zeros(nb.value, np.uint32), np.zeros(nb.value, np.int32)
    _check(lib().hs_build_schedule(n, M, bf, seed, grow_div, batch_max, nb.value, sizes.ctypes.data, eps.ctypes.data, tops.ctypes.data,
                                   ctypes.byref(nb)))
    return {"sizes": sizes, "entry_points": eps, "top_levels": tops}


def hnsw_resume(in_path, out_path, rows, labels, dim=None, metric=HS_METRIC_L2, max_elements=0, seed=100, drawn=0, threads=1):
    """hs_hnsw_resume (host only): load `in_path` with room for `max_elements`, put the level generator where a build with `seed`
    that has added `drawn` points left it, addPoint(rows[i], labels[i]) for every row, saveIndex(out_path)."""
    r = np.ascontiguousarray(rows, np.float32)
    r = r.reshape(-1, dim) if r.ndim != 2 else r
    lab = np.ascontiguousarray(labels, np.uint64)
    if lab.shape != (r.shape[0],):
        raise HsError(HS_ERR_INVALID, "labels: one per row")
    _check(lib().hs_hnsw_resume(in_path.encode(), metric, r.shape[1] if dim is None else dim, max_elements, r.ctypes.data,
                                lab.ctypes.data, r.shape[0], seed, drawn, threads, out_path.encode()))


def _batch_stats(st):
    return {"used_gpu": bool(st.used_gpu), "batches": int(st.batches), "flagged_rows": int(st.flagged_rows), "kernel_ms": st.kernel_ms,
            "total_ms": st.total_ms}


def hnsw_resume_batched(in_path, out_path, rows, labels, dim=None, metric=HS_METRIC_L2, max_elements=0, seed=100, drawn=0, device=-1, threads=1,
                        grow_div=0, batch_max=0, scratch_ids=0):
    """hs_hnsw_resume_batched (host only): hnsw_resume with the rows added in the batched order, continued from the
    loaded graph; always the host twin (`device` is accepted and not used).  Returns the stats dict of build_hnsw_batched."""
    r = np.ascontiguousarray(rows, np.float32)
    r = r.reshape(-1, dim) if r.ndim != 2 else r
    lab = np.ascontiguousarray(labels, np.uint64)
    if lab.shape != (r.shape[0],):
        raise HsError(HS_ERR_INVALID, "labels: one per row")
    opts = HsBatchBuildOpts(device, threads, grow_div, batch_max, scratch_ids)
    st = HsBatchBuildStats()
    _check(lib().hs_hnsw_resume_batched(in_path.encode(), metric, r.shape[1] if dim is None else dim, max_elements, r.ctypes.data,
                                        lab.ctypes.data, r.shape[0], seed, drawn, ctypes.byref(opts), out_path.encode(), ctypes.byref(st)))
    return _batch_stats(st)


HS_OP_ADD, HS_OP_MARK, HS_OP_UNMARK, HS_OP_RESIZE = range(4)   # operation kinds of hs_hnsw_replay


def hnsw_replay(in_path, out_path, ops, rows, dim, metric=HS_METRIC_L2, max_elements=0, allow_replace_deleted=False):
    """hs_hnsw_replay (host only): load `in_path`, apply `ops` -- rows of four uint64 {kind, label or new capacity, replace flag,
    row index into `rows`} -- through the reference's addPoint / markDelete / unmarkDelete / resizeIndex, saveIndex(out_path)."""
    o = np.ascontiguousarray(ops, np.uint64).reshape(-1, 4)
    r = np.ascontiguousarray(rows, np.float32).reshape(-1, dim)
    adds = o[o[:, 0] == HS_OP_ADD]
    if adds.size and int(adds[:, 3].max()) >= r.shape[0]:
        raise HsError(HS_ERR_INVALID, "hnsw_replay: an operation names a row beyond `rows`")
    _check(lib().hs_hnsw_replay(in_path.encode(), metric, dim, max_elements, 1 if allow_replace_deleted else 0, o.ctypes.data, o.shape[0],
                                r.ctypes.data, out_path.encode()))


def convert_slim(hnsw_path, out_path, dim, metric=HS_METRIC_L2, threshold_level=0, top_degree_percent0=0.02,
                 top_degree_percent=0.02, top_degree_M0=32, low_degree_m0=8, top_degree_M=16, low_degree_m=4, threads=1):
    """HierarchicalNSWSlim::convertFromHNSW + saveIndex, on the CPU (harness)."""
    _check(lib().hs_convert_slim(hnsw_path.encode(), metric, dim, threshold_level, top_degree_percent0, top_degree_percent,
                                 top_degree_M0, low_degree_m0, top_degree_M, low_degree_m, threads, out_path.encode()))


def build_rabitq_hnsw(base, out_path, metric=HS_METRIC_L2, M=32, ef_construction=128, seed=100, threads=1):
    """rabitqlib::hnsw::HierarchicalNSW::construct's edges (the graph HNSW-SlimQ converts from; defaults =
    hnsw_slimq_strategy.h:106-108), saved in hnswlib's layout.  CPU harness."""
    base = np.ascontiguousarray(base, np.float32)
    _check(lib().hs_build_rabitq_hnsw(base.ctypes.data, base.shape[0], base.shape[1], metric, M, ef_construction, seed, threads,
                                      out_path.encode()))


def build_rabitq_hnsw_batched(base, out_path, metric=HS_METRIC_L2, M=32, ef_construction=128, seed=100, device=-1, threads=1, grow_div=0,
                              batch_max=0, scratch_ids=0):
    """hs_build_rabitq_hnsw_batched: build_rabitq_hnsw's graph from the batched insertion order on HIP device `device`,
    or on the host twin (device=-1, `threads` workers); both write the same file, and batch_max=1 writes build_rabitq_hnsw(threads=1)'s.
    Returns the stats dict of build_hnsw_batched."""
    base = np.ascontiguousarray(base, np.float32)
    if base.ndim != 2:
        raise HsError(HS_ERR_INVALID, "base: rows x dim")
    opts = HsBatchBuildOpts(device, threads, grow_div, batch_max, scratch_ids)
    st = HsBatchBuildStats()
    _check(lib().hs_build_rabitq_hnsw_batched(base.ctypes.data, base.shape[0], base.shape[1], metric, M, ef_construction, seed, ctypes.byref(opts),
                                              out_path.encode(), ctypes.byref(st)))
    return {"used_gpu": bool(st.used_gpu), "batches": int(st.batches), "flagged_rows": int(st.flagged_rows), "kernel_ms": st.kernel_ms,
            "total_ms": st.total_ms}


def rq_raw_dist(a, b, metric=HS_METRIC_L2, device=-1):
    """hs_debug_rq_raw_dist: rabitqlib's raw distance of rows a[i] and b[i] -- the host recipe (device=-1) or the wavefront recipe of
    the build kernels on a HIP device.  Returns float32[n_pairs]."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.ndim != 2 or a.shape != b.shape:
        raise HsError(HS_ERR_INVALID, "a, b: n_pairs x dim each")
    out = np.empty(a.shape[0], np.float32)
    _check(lib().hs_debug_rq_raw_dist(a.ctypes.data, b.ctypes.data, a.shape[0], a.shape[1], metric, device, out.ctypes.data))
    return out


def convert_slimq_graph(hnsw_path, out_path, dim, metric=HS_METRIC_L2, threshold_level=0, top_degree_percent0=0.02,
                        top_degree_percent=0.02, top_degree_M0=32, low_degree_m0=8, top_degree_M=16, low_degree_m=4, threads=1):
    """HierarchicalNSWSlimQ::convertFromHNSW's graph passes (its own PruneByHeuristic) -> Slim-layout file for convert_slimq."""
    _check(lib().hs_convert_slimq_graph(hnsw_path.encode(), metric, dim, threshold_level, top_degree_percent0, top_degree_percent,
                                        top_degree_M0, low_degree_m0, top_degree_M, low_degree_m, threads, out_path.encode()))


def convert_slim_gpu(hnsw_path, out_path, dim, metric=HS_METRIC_L2, threshold_level=0, top_degree_percent0=0.02,
                     top_degree_percent=0.02, top_degree_M0=32, low_degree_m0=8, top_degree_M=16, low_degree_m=4, device=0, threads=8):
    """convertFromHNSW with the per-list work on the GPU; returns (used_gpu, kernel_ms).  Same bytes as convert_slim."""
    used, ms = ctypes.c_int(0), ctypes.c_double(0.0)
    _check(lib().hs_convert_slim_gpu(hnsw_path.encode(), metric, dim, threshold_level, top_degree_percent0, top_degree_percent,
                                     top_degree_M0, low_degree_m0, top_degree_M, low_degree_m, device, threads, out_path.encode(),
                                     ctypes.byref(used), ctypes.byref(ms)))
    return bool(used.value), ms.value


def convert_slimq_graph_gpu(hnsw_path, out_path, dim, metric=HS_METRIC_L2, threshold_level=0, top_degree_percent0=0.02,
                            top_degree_percent=0.02, top_degree_M0=32, low_degree_m0=8, top_degree_M=16, low_degree_m=4, device=0, threads=8):
    """convert_slimq_graph with the per-list work on the GPU; returns (used_gpu, kernel_ms).  Same bytes as convert_slimq_graph."""
    used, ms = ctypes.c_int(0), ctypes.c_double(0.0)
    _check(lib().hs_convert_slimq_graph_gpu(hnsw_path.encode(), metric, dim, threshold_level, top_degree_percent0, top_degree_percent,
                                            top_degree_M0, low_degree_m0, top_degree_M, low_degree_m, device, threads, out_path.encode(),
                                            ctypes.byref(used), ctypes.byref(ms)))
    return bool(used.value), ms.value


class SlimDiff:
    """What one convertFromHNSWWithDiff call found (hs_slim_diff_*): the changed old nodes and the new nodes, the whole stream of
    the std::ostream overload, and genPatch with its cursors.  `index`: the Slim Index the diff was made on, None for a diff of
    slim_convert_diff_files (which owns its Slim image)."""

    def __init__(self, handle, index, used_gpu=False, kernel_ms=0.0):
        self._h, self._ix, self.used_gpu, self.kernel_ms = handle, index, used_gpu, kernel_ms

    def _slim(self):
        return self._ix._h if self._ix is not None else None

    def close(self):
        if self._h:
            lib().hs_slim_diff_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        v = [ctypes.c_size_t(0) for _ in range(4)]
        _check(lib().hs_slim_diff_info(self._h, *[ctypes.byref(x) for x in v]))
        return dict(count=v[0].value, n_old=v[1].value, n_new=v[2].value, n_reprune=v[3].value)

    def ids(self):
        """(changed old ids, new ids), both ascending."""
        i = self.info()
        old, new = np.empty(i["n_old"], np.uint32), np.empty(i["n_new"], np.uint32)
        _check(lib().hs_slim_diff_ids(self._h, old.ctypes.data, new.ctypes.data))
        return old, new

    def stream(self):
        """The whole stream (new records without rows): what Index.patch(.., to_add=False) takes."""
        n = ctypes.c_size_t(0)
        rc = lib().hs_slim_diff_stream(self._h, self._slim(), None, 0, ctypes.byref(n))
        if rc not in (HS_OK, HS_ERR_CAPACITY):
            _check(rc)
        buf = ctypes.create_string_buffer(max(n.value, 1))
        _check(lib().hs_slim_diff_stream(self._h, self._slim(), buf, n.value, ctypes.byref(n)))
        return buf.raw[:n.value]

    def next(self, limit, to_add=False, cap=None):
        """One genPatch call -> (bytes for Index.patch(.., to_add), old_written, new_written, finished).  cap: the buffer size to
        offer (default: ask first); too small raises HsError(HS_ERR_CAPACITY) and the cursors stay."""
        n, ow, nw, fin = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_int(0)
        if cap is None:
            rc = lib().hs_slim_diff_next(self._h, self._slim(), limit, 1 if to_add else 0, None, 0, ctypes.byref(n), None, None, None)
            if rc not in (HS_OK, HS_ERR_CAPACITY):
                _check(rc)
            cap = n.value
        buf = ctypes.create_string_buffer(max(cap, 1))
        _check(lib().hs_slim_diff_next(self._h, self._slim(), limit, 1 if to_add else 0, buf, cap, ctypes.byref(n), ctypes.byref(ow),
                                       ctypes.byref(nw), ctypes.byref(fin)))
        return buf.raw[:n.value], ow.value, nw.value, bool(fin.value)


def slim_convert_diff_files(old_slim_path, hnsw_path, out_slim_path, dim, metric=HS_METRIC_L2, threshold_level=0, top_degree_percent0=0.02,
                            top_degree_percent=0.02, top_degree_M0=32, low_degree_m0=8, top_degree_M=16, low_degree_m=4, threads=1,
                            out_stream_path=None):
    """hs_slim_convert_diff_files (host only): convertFromHNSWWithDiff of the Slim file `old_slim_path` (None: an empty Slim index)
    from the vanilla file `hnsw_path`; writes the new Slim file (and the whole stream when asked) and returns the SlimDiff."""
    h = ctypes.c_void_p()
    _check(lib().hs_slim_convert_diff_files(None if old_slim_path is None else old_slim_path.encode(), hnsw_path.encode(), metric, dim,
                                            threshold_level, top_degree_percent0, top_degree_percent, top_degree_M0, low_degree_m0,
                                            top_degree_M, low_degree_m, threads, out_slim_path.encode(),
                                            None if out_stream_path is None else out_stream_path.encode(), ctypes.byref(h)))
    return SlimDiff(h, None)


def rows_representable(rows, fmt):
    """hs_rows_representable (host only): None when every value of `rows` (n x dim fp32) is exactly representable in the row
    format `fmt` (HS_ROWS_U8: integers 0..255; HS_ROWS_F16: finite fp16 values), else the index of the first row that is not."""
    r = np.ascontiguousarray(rows, np.float32)
    r = r.reshape(r.shape[0], -1) if r.ndim != 2 else r
    bad = ctypes.c_uint64(0)
    _check(lib().hs_rows_representable(r.ctypes.data, r.shape[0], r.shape[1], int(fmt), ctypes.byref(bad)))
    return None if bad.value == r.shape[0] else int(bad.value)


def rows_to_narrow(rows, fmt, out=None):
    """hs_rows_to_narrow (host only): `rows` (n x dim fp32, dim % 16 == 0) in the row format `fmt` and the lane-major layout of the
    device copy -- (narrow, first_bad): narrow is n x dim uint8 (HS_ROWS_U8) or float16 (HS_ROWS_F16), first_bad None when every
    value is representable, else the first row that is not (nothing is written from there on; `out`, when given, is the array
    that is filled)."""
    r = np.ascontiguousarray(rows, np.float32)
    r = r.reshape(r.shape[0], -1) if r.ndim != 2 else r
    dt = np.uint8 if int(fmt) == HS_ROWS_U8 else np.float16
    if out is None:
        out = np.zeros(r.shape, dt)
    assert out.dtype == dt and out.shape == r.shape and out.flags.c_contiguous
    bad = ctypes.c_uint64(0)
    _check(lib().hs_rows_to_narrow(r.ctypes.data, r.shape[0], r.shape[1], int(fmt), out.ctypes.data, ctypes.byref(bad)))
    return out, (None if bad.value == r.shape[0] else int(bad.value))


def filter_row_words(n):
    """hs_filter_row_words: 32-bit words per bitmap row of a filter set over n ids (ceil(n / 32) rounded up to a multiple of 4)."""
    return int(lib().hs_filter_row_words(int(n)))


def filter_pack(allowed):
    """hs_filter_pack (host only): allowed (nf x n, or n: one filter; non-zero = allowed) -> uint32 words nf x filter_row_words(n),
    bit i & 31 of word i >> 5, padding bits zero."""
    a = np.ascontiguousarray(allowed, np.uint8)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    nf, n = a.shape
    out = np.empty((nf, filter_row_words(n)), np.uint32)
    _check(lib().hs_filter_pack(a.ctypes.data, n, nf, out.ctypes.data))
    return out


class FilterSet:
    """hs_filter_set: nf filters over the internal ids of one index, resident on its device as bitmaps.  Index.search_filter_set
    names the set and one filter per query; queries under different filters run in one launch."""

    def __init__(self, index, nf):
        self._h = ctypes.c_void_p()
        _check(lib().hs_filter_set_create(index._h, int(nf), ctypes.byref(self._h)))

    @classmethod
    def create(cls, index, nf):
        return cls(index, nf)

    def close(self):
        if self._h:
            lib().hs_filter_set_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        v = [ctypes.c_uint64(0) for _ in range(4)]
        _check(lib().hs_filter_set_info(self._h, *[ctypes.byref(x) for x in v]))
        return dict(nf=v[0].value, n=v[1].value, row_words=v[2].value, device_bytes=v[3].value)

    def write(self, first, allowed_bytes):
        """Rows first.. from host bytes (count x n, or n: one row; non-zero = allowed), packed on the device."""
        a = np.ascontiguousarray(allowed_bytes, np.uint8)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        if a.shape[1] != self.info()["n"]:
            raise HsError(HS_ERR_INVALID, f"rows of {a.shape[1]} bytes for a filter set over {self.info()['n']} ids")
        _check(lib().hs_filter_set_write(self._h, int(first), a.shape[0], a.ctypes.data))

    def write_bits(self, first, words):
        """Rows first.. from host words in filter_pack's layout (count x row_words uint32)."""
        w = np.ascontiguousarray(words, np.uint32)
        w = w.reshape(1, -1) if w.ndim == 1 else w
        if w.shape[1] != self.info()["row_words"]:
            raise HsError(HS_ERR_INVALID, f"rows of {w.shape[1]} words for a filter set of {self.info()['row_words']}-word rows")
        _check(lib().hs_filter_set_write_bits(self._h, int(first), w.shape[0], w.ctypes.data))

    def write_dev(self, first, torch_tensor, stream=0):
        """Rows first.. from a contiguous torch bool / uint8 tensor on the set's device (count x n, or n); asynchronous on `stream`."""
        t = torch_tensor
        if t.element_size() != 1 or not t.is_contiguous():
            raise HsError(HS_ERR_INVALID, "write_dev takes a contiguous bool / uint8 tensor")
        count, n = (1, t.shape[0]) if t.dim() == 1 else (t.shape[0], t.shape[1])
        if n != self.info()["n"]:
            raise HsError(HS_ERR_INVALID, f"rows of {n} bytes for a filter set over {self.info()['n']} ids")
        _check(lib().hs_filter_set_write_dev(self._h, int(first), count, t.data_ptr(), stream))

    def read(self, f):
        """Row f unpacked: n uint8 (0 / 1)."""
        out = np.empty(self.info()["n"], np.uint8)
        _check(lib().hs_filter_set_read(self._h, int(f), out.ctypes.data))
        return out


class QueueTicket:
    """One submission to a SearchQueue: its ticket id and the arrays its answers land in (host submissions: numpy arrays owned
    here, valid after SearchQueue.wait; device submissions: the caller's tensors, kept alive here)."""

    def __init__(self, id, labels=None, dists=None, cnt=None, stats=None, keep=None, device=False):
        self.id, self.labels, self.dists, self.cnt, self.stats, self._keep, self.device = id, labels, dists, cnt, stats, keep, device

    def result(self):
        return dict(labels=self.labels, dists=self.dists, cnt=self.cnt, stats=self.stats)


class SearchQueue:
    """hs_queue: small submissions from any thread, coalesced into one search launch per flush on a resident HNSW / Slim index;
    every query's answer is bit for bit Index.search_ids / search_pq / search_filter_set of that query.  mode: HS_MODE_SLIM_IDS
    (labels uint32, as search_ids) or HS_MODE_PQ (labels uint64 + dists + cnt, as search_pq); with a FilterSet `fs`, HS_MODE_PQ and
    one filter index per query.  The calls release the GIL: Python threads block in wait() side by side."""

    def __init__(self, index, k, mode, max_queries=8192, slots=2, fs=None):
        self._h = ctypes.c_void_p()
        self.k, self.mode, self.dim, self._index, self._fs = int(k), int(mode), index.dim, index, fs
        self._out = {}   # outstanding tickets by id: the queue holds the addresses of their arrays until their launch is done
        _check(lib().hs_queue_create(index._h, self.k, self.mode, int(max_queries), int(slots), None if fs is None else fs._h,
                                     ctypes.byref(self._h)))

    def close(self):
        if self._h:
            lib().hs_queue_free(self._h)   # drains first
            self._h = ctypes.c_void_p()
            self._out.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def submit(self, queries, filter_of_query=None, want_dists=False, want_stats=False):
        """Host rows (nq x dim; pageable is fine: copied before this returns; a view of a PinnedArray is read in place and must stay
        unchanged until wait) -> QueueTicket.  HS_MODE_SLIM_IDS: labels uint32 nq x k,
        cnt, dists when asked; HS_MODE_PQ: labels uint64, dists, cnt; stats (nq x 4) when asked."""
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, self.dim)
        nq, k, ids = q.shape[0], self.k, self.mode == HS_MODE_SLIM_IDS
        foq = None if filter_of_query is None else np.ascontiguousarray(filter_of_query, np.uint32)
        if foq is not None and foq.shape != (nq,):
            raise HsError(HS_ERR_INVALID, "filter_of_query: one filter index per query")
        labels = np.empty((nq, k), np.uint32 if ids else np.uint64)
        dists = np.empty((nq, k), np.float32) if (want_dists or not ids) else None
        cnt = np.empty(nq, np.uint32)
        stats = np.empty((nq, 4), np.uint32) if want_stats else None
        t = ctypes.c_uint64(0)
        _check(lib().hs_queue_submit(self._h, q.ctypes.data, nq, None if foq is None else foq.ctypes.data,
                                     labels.ctypes.data if ids else None, None if ids else labels.ctypes.data,
                                     None if dists is None else dists.ctypes.data, cnt.ctypes.data,
                                     None if stats is None else stats.ctypes.data, ctypes.byref(t)))
        return self._hold(QueueTicket(t.value, labels, dists, cnt, stats, keep=(q, foq)))

    def submit_dev(self, d_queries, d_labels, d_dists=None, d_counts=None, d_stats=None, d_filter_of_query=None, stream=0):
        """Device tensors (torch, on the index's device; queries f32 nq x dim, contiguous rows, any 4-byte alignment; labels int32
        nq x k in HS_MODE_SLIM_IDS, int64 in HS_MODE_PQ; dists f32 nq x k; counts int32 nq; stats int32 nq x 4; filter indices
        int32 nq) -> QueueTicket.  The queue's launch waits for what `stream` holds at this moment."""
        if not d_queries.is_contiguous():
            raise HsError(HS_ERR_INVALID, "submit_dev takes contiguous rows")
        nq, ids = d_queries.shape[0], self.mode == HS_MODE_SLIM_IDS
        ptr = lambda x: None if x is None else x.data_ptr()
        t = ctypes.c_uint64(0)
        _check(lib().hs_queue_submit_dev(self._h, d_queries.data_ptr(), nq, ptr(d_filter_of_query), ptr(d_labels) if ids else None,
                                         None if ids else ptr(d_labels), ptr(d_dists), ptr(d_counts), ptr(d_stats), stream, ctypes.byref(t)))
        return self._hold(QueueTicket(t.value, d_labels, d_dists, d_counts, d_stats, keep=(d_queries, d_filter_of_query), device=True))

    def _hold(self, ticket):
        self._out[ticket.id] = ticket   # a caller may drop the ticket: its arrays live until wait / drain / close
        return ticket

    def flush(self):
        """Enqueue one launch for everything pending; does not wait for it."""
        _check(lib().hs_queue_flush(self._h))

    def wait(self, ticket):
        """Block until the ticket's answers are in its arrays (flushing if it is still pending) -> dict(labels, dists, cnt, stats).
        Raises the status of the ticket's launch.  A ticket is waited once."""
        try:
            _check(lib().hs_queue_wait(self._h, ticket.id))   # (returns only once the ticket's launch is done, whatever its status)
        finally:
            self._out.pop(ticket.id, None)
        return ticket.result()

    def join_stream(self, ticket, stream=0):
        """Device tickets: `stream` waits for the ticket's launch, the host does not.  The ticket still wants its wait (or a drain)."""
        _check(lib().hs_queue_join_stream(self._h, ticket.id, stream))

    def drain(self):
        ids = list(self._out)   # the tickets this drain completes (later ones stay held)
        try:
            _check(lib().hs_queue_drain(self._h))
        finally:
            for i in ids:
                self._out.pop(i, None)

    def info(self):
        i = HsQueueInfo()
        _check(lib().hs_queue_info(self._h, ctypes.byref(i)))
        return {f: int(getattr(i, f)) for f, _ in HsQueueInfo._fields_}


def plan_input(kernel=None, lean_min_ef=None, order=-1, flat=1, vis16=1, flat_waves_per_cu=0, **fields):
    """An hs_plan_in with the knobs unset and a bare 1M x 128 Slim index (tiles present, fp32 rows resident) searched with ef 70,
    k 10, 10 000 queries, in HS_MODE_PQ; `fields` overrides members by name, the leading arguments are the knobs as the
    environment spells them (kernel: None | "lean" | "fast"; lean_min_ef: None = unset)."""
    p = HsPlanIn(n=1_000_000, dim=128, has_tile0=1, has_uptile=1, maxlevel=3, threshold_level=0, has_deleted=0, kind=HS_KIND_SLIM,
                 ef=70, k=10, nq=10_000, mode=HS_MODE_PQ, row_fmt=HS_ROWS_F32, f32_resident=1)
    p.diag = HsPlanDiag(kernel=PLAN_KERNELS[kernel], lean_forced=lean_min_ef is not None, lean_min_ef=64 if lean_min_ef is None else lean_min_ef,
                        order=order, flat=flat, vis16=vis16, flat_waves_per_cu=flat_waves_per_cu, zero_copy=0, verbose=0, slimq_fused=1)
    for name, v in fields.items():
        assert hasattr(p, name), name
        setattr(p, name, int(v))
    return p


def debug_search_plan(inp):
    """hs_debug_search_plan (host only): the launch plan for an HsPlanIn, as a dict of hs_plan_out's members (name: str)."""
    out = HsPlanOut()
    _check(lib().hs_debug_search_plan(ctypes.byref(inp), ctypes.byref(out)))
    d = {f: getattr(out, f) for f, _ in HsPlanOut._fields_}
    d["name"] = out.name.decode()
    return d


def debug_fast_shape(metric, dim, ef, k, bare=True):
    """hs_debug_fast_shape (host only): the instantiation of hs::fast_kernel the launchers pick for a call, as dict(d16, slots, wb)."""
    out = HsFastShape()
    _check(lib().hs_debug_fast_shape(int(metric), int(dim), int(ef), int(k), int(bool(bare)), ctypes.byref(out)))
    return {f: getattr(out, f) for f, _ in HsFastShape._fields_}


def debug_plan_input(index, k, nq, has_filter=False, want_raw=False):
    """hs_debug_plan_input: the HsPlanIn of a search of nq queries on a live index, knobs from this process's environment."""
    p = HsPlanIn()
    _check(lib().hs_debug_plan_input(index._h, int(k), int(nq), int(bool(has_filter)), int(bool(want_raw)), ctypes.byref(p)))
    return p


def debug_heap_ops(ops, wave_pop=True, lds_slots=1024):
    """hs_debug_heap_ops: ops = [(0, dist, id) | (1, 0, 0), ...] -> (heap [(dist, id)], pops [(dist, id)]) from the device."""
    n = len(ops)
    arr = np.zeros((max(n, 1), 3), np.uint32)
    for i, (kind, d, idv) in enumerate(ops):
        arr[i] = (kind, np.float32(d).view(np.uint32), idv)
    heap = np.zeros((n + 2, 2), np.uint32)
    pops = np.zeros((n + 2, 2), np.uint32)
    cnt = np.zeros(2, np.uint32)
    _check(lib().hs_debug_heap_ops(arr.ctypes.data, n, 1 if wave_pop else 0, lds_slots, heap.ctypes.data, pops.ctypes.data, cnt.ctypes.data))
    f = lambda a, m: [(float(a[i, 0:1].view(np.float32)[0]), int(a[i, 1])) for i in range(m)]
    return f(heap, int(cnt[0])), f(pops, int(cnt[1]))


def brute_force(base, queries, k, metric=HS_METRIC_L2, labels=None, device=0):
    """hnswlib::BruteforceSearch::searchKnn for a batch: (labels, dists) nq x k, ascending by (dist, label)."""
    b = np.ascontiguousarray(base, np.float32)
    q = np.ascontiguousarray(queries, np.float32)
    lab = None if labels is None else np.ascontiguousarray(labels, np.uint64)
    ol = np.empty((q.shape[0], k), np.uint64)
    od = np.empty((q.shape[0], k), np.float32)
    oc = np.empty(q.shape[0], np.uint32)
    _check(lib().hs_brute_force(b.ctypes.data, b.shape[0], b.shape[1], metric, None if lab is None else lab.ctypes.data, q.ctypes.data,
                                q.shape[0], k, device, ol.ctypes.data, od.ctypes.data, oc.ctypes.data))
    return ol, od, oc


def brute_force_dev(d_base, d_queries, k, d_labels_out, d_dists_out, metric=HS_METRIC_L2, d_counts=None, stream=0):
    """Device tensors (torch): base n x d, queries nq x d, outputs int64 / float32 nq x k."""
    _check(lib().hs_brute_force_dev(d_base.data_ptr(), None, d_base.shape[0], d_base.shape[1], metric, d_queries.data_ptr(),
                                    d_queries.shape[0], k, d_labels_out.data_ptr(), d_dists_out.data_ptr(),
                                    d_counts.data_ptr() if d_counts is not None else None, stream))


def convert_slimq(slim_path, metric, dim, centroids, out_path, cluster_ids=None, flip_seed=1, threads=8):
    c = np.ascontiguousarray(centroids, np.float32).reshape(-1, dim)
    cid = None if cluster_ids is None else np.ascontiguousarray(cluster_ids, np.uint32)
    _check(lib().hs_convert_slimq(slim_path.encode(), metric, dim, c.ctypes.data, c.shape[0], None if cid is None else cid.ctypes.data,
                                  flip_seed, threads, out_path.encode()))


def convert_slimq_gpu(slim_path, metric, dim, centroids, out_path, cluster_ids=None, flip_seed=1, device=0, threads=8):
    """convert_slimq with the rotation and quantisation of the rows on a HIP device; returns (used_gpu, kernel_ms).  Same bytes."""
    c = np.ascontiguousarray(centroids, np.float32).reshape(-1, dim)
    cid = None if cluster_ids is None else np.ascontiguousarray(cluster_ids, np.uint32)
    used, ms = ctypes.c_int(0), ctypes.c_double(0.0)
    _check(lib().hs_convert_slimq_gpu(slim_path.encode(), metric, dim, c.ctypes.data, c.shape[0], None if cid is None else cid.ctypes.data,
                                      flip_seed, device, threads, out_path.encode(), ctypes.byref(used), ctypes.byref(ms)))
    return bool(used.value), ms.value


def convert_hnsw_to_slimq(hnsw_path, out_path, dim, centroids, metric=HS_METRIC_L2, cluster_ids=None, flip_seed=1, threshold_level=0,
                          top_degree_percent0=0.02, top_degree_percent=0.02, top_degree_M0=32, low_degree_m0=8, top_degree_M=16,
                          low_degree_m=4, device=-1, threads=8):
    """HierarchicalNSWSlimQ::convertFromHNSW in one call, HNSW file in, SlimQ file out, no intermediate file: the bytes of
    convert_slimq_graph + convert_slimq.  device=-1: on host threads; device>=0: both steps on that HIP device.  Returns the stats as
    a dict (graph_used_gpu, records_used_gpu, graph_kernel_ms, records_kernel_ms, graph_ms, records_ms, total_ms)."""
    c = np.ascontiguousarray(centroids, np.float32).reshape(-1, dim)
    cid = None if cluster_ids is None else np.ascontiguousarray(cluster_ids, np.uint32)
    st = HsSlimqConvertStats()
    _check(lib().hs_convert_hnsw_to_slimq(hnsw_path.encode(), metric, dim, threshold_level, top_degree_percent0, top_degree_percent,
                                          top_degree_M0, low_degree_m0, top_degree_M, low_degree_m, c.ctypes.data, c.shape[0],
                                          None if cid is None else cid.ctypes.data, flip_seed, device, threads, out_path.encode(),
                                          ctypes.byref(st)))
    return {k: getattr(st, k) for k, _ in HsSlimqConvertStats._fields_}


class Graph:
    """hs_graph: an HNSW graph in host memory, what saveIndex would write (build_rabitq_hnsw_batched_mem, Graph.load)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def load(cls, path, dim, metric=HS_METRIC_L2):
        h = ctypes.c_void_p()
        _check(lib().hs_graph_load(path.encode(), metric, dim, ctypes.byref(h)))
        return cls(h)

    def save(self, path):
        _check(lib().hs_graph_save(self._h, path.encode()))

    def info(self):
        n, dim, M, efc = (ctypes.c_uint64() for _ in range(4))
        metric, maxlevel = ctypes.c_int(), ctypes.c_int()
        _check(lib().hs_graph_info(self._h, ctypes.byref(n), ctypes.byref(dim), ctypes.byref(metric), ctypes.byref(M), ctypes.byref(efc),
                                   ctypes.byref(maxlevel)))
        return dict(n=n.value, dim=dim.value, metric=metric.value, M=M.value, ef_construction=efc.value, maxlevel=maxlevel.value)

    def close(self):
        if self._h:
            lib().hs_graph_free(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def build_rabitq_hnsw_batched_mem(base, metric=HS_METRIC_L2, M=32, ef_construction=128, seed=100, device=-1, threads=1, grow_div=0,
                                  batch_max=0, scratch_ids=0):
    """hs_build_rabitq_hnsw_batched_mem: build_rabitq_hnsw_batched without its file.  Returns (Graph, stats dict); Graph.save writes the
    bytes build_rabitq_hnsw_batched writes."""
    base = np.ascontiguousarray(base, np.float32)
    if base.ndim != 2:
        raise HsError(HS_ERR_INVALID, "base: rows x dim")
    opts = HsBatchBuildOpts(device, threads, grow_div, batch_max, scratch_ids)
    st = HsBatchBuildStats()
    h = ctypes.c_void_p()
    _check(lib().hs_build_rabitq_hnsw_batched_mem(base.ctypes.data, base.shape[0], base.shape[1], metric, M, ef_construction, seed,
                                                  ctypes.byref(opts), ctypes.byref(h), ctypes.byref(st)))
    return Graph(h), {"used_gpu": bool(st.used_gpu), "batches": int(st.batches), "flagged_rows": int(st.flagged_rows),
                      "kernel_ms": st.kernel_ms, "total_ms": st.total_ms}


def _slimq_params(dim, centroids, cluster_ids, flip_seed, threshold_level, top_degree_percent0, top_degree_percent, top_degree_M0, low_degree_m0,
                  top_degree_M, low_degree_m):
    """(hs_slimq_params, the arrays it points into -- keep them alive for the call)"""
    c = np.ascontiguousarray(centroids, np.float32).reshape(-1, dim)
    cid = None if cluster_ids is None else np.ascontiguousarray(cluster_ids, np.uint32)
    p = HsSlimqParams(threshold_level, top_degree_percent0, top_degree_percent, top_degree_M0, low_degree_m0, top_degree_M, low_degree_m,
                      c.ctypes.data, c.shape[0], None if cid is None else cid.ctypes.data, flip_seed)
    return p, (c, cid)


def _stats_dict(st):
    return {k: getattr(st, k) for k, _ in type(st)._fields_}


def _adopt_index(h, dim, metric, device):
    ix = Index.__new__(Index)
    ix._h = h
    ix.kind, ix.dim, ix.metric, ix.device, ix.ef = HS_KIND_SLIMQ, dim, metric, device, 10
    return ix


def graph_convert_slimq(graph, centroids, out_path=None, want_index=False, with_dataset=False, convert_device=-1, index_device=0,
                        cluster_ids=None, flip_seed=1, threshold_level=0, top_degree_percent0=0.02, top_degree_percent=0.02,
                        top_degree_M0=32, low_degree_m0=8, top_degree_M=16, low_degree_m=4, threads=8):
    """hs_graph_convert_slimq: convertFromHNSW of an in-memory Graph into a SlimQ file (out_path), a resident Index (want_index; its
    fused tiles gathered on the device, with_dataset: the graph's own rows as its re-rank dataset) or both.  Returns (Index or None,
    the stats dict of convert_hnsw_to_slimq)."""
    gi = graph.info()
    p, keep = _slimq_params(gi["dim"], centroids, cluster_ids, flip_seed, threshold_level, top_degree_percent0, top_degree_percent,
                            top_degree_M0, low_degree_m0, top_degree_M, low_degree_m)
    st = HsSlimqConvertStats()
    h = ctypes.c_void_p()
    _check(lib().hs_graph_convert_slimq(graph._h, ctypes.byref(p), convert_device, threads, None if out_path is None else out_path.encode(),
                                        index_device, 1 if with_dataset else 0, ctypes.byref(h) if want_index else None, ctypes.byref(st)))
    del keep
    return (_adopt_index(h, gi["dim"], gi["metric"], index_device) if want_index else None), _stats_dict(st)


def slimq_index_from_rows(base, centroids, metric=HS_METRIC_L2, M=32, ef_construction=128, seed=100, device=0, threads=8, with_dataset=True,
                          grow_div=0, batch_max=0, scratch_ids=0, cluster_ids=None, flip_seed=1, threshold_level=0,
                          top_degree_percent0=0.02, top_degree_percent=0.02, top_degree_M0=32, low_degree_m0=8, top_degree_M=16,
                          low_degree_m=4):
    """hs_slimq_index_from_rows: rows in, resident SlimQ Index out -- the batched rabitqlib build, convertFromHNSW and the tile
    assembly on HIP device `device`, no file written or read.  Returns (Index, stats dict with 'build' and 'convert' dicts,
    resident_ms, tile_kernel_ms, total_ms)."""
    base = np.ascontiguousarray(base, np.float32)
    if base.ndim != 2:
        raise HsError(HS_ERR_INVALID, "base: rows x dim")
    dim = base.shape[1]
    p, keep = _slimq_params(dim, centroids, cluster_ids, flip_seed, threshold_level, top_degree_percent0, top_degree_percent, top_degree_M0,
                            low_degree_m0, top_degree_M, low_degree_m)
    opts = HsBatchBuildOpts(device, threads, grow_div, batch_max, scratch_ids)
    st = HsSlimqPipelineStats()
    h = ctypes.c_void_p()
    _check(lib().hs_slimq_index_from_rows(base.ctypes.data, base.shape[0], dim, metric, M, ef_construction, seed, ctypes.byref(opts),
                                          ctypes.byref(p), threads, 1 if with_dataset else 0, ctypes.byref(h), ctypes.byref(st)))
    del keep
    return _adopt_index(h, dim, metric, device), dict(build=_stats_dict(st.build), convert=_stats_dict(st.convert), resident_ms=st.resident_ms,
                                                      tile_kernel_ms=st.tile_kernel_ms, total_ms=st.total_ms)


def debug_slimq_arrays_host(slimq_path, dim, which, metric=HS_METRIC_L2, fused=True):
    """hs_debug_slimq_arrays_host: rec (which=0), ftile (1) or uptile (2) of a SlimQ file by the host statement of the layout alone.
    Returns (uint32 words, stride, row_words); an array the index would not have comes back empty with stride 0."""
    words, st, rw = ctypes.c_size_t(), ctypes.c_uint32(), ctypes.c_uint32()
    args = (slimq_path.encode(), metric, dim, 1 if fused else 0, which)
    _check(lib().hs_debug_slimq_arrays_host(*args, None, 0, ctypes.byref(words), ctypes.byref(st), ctypes.byref(rw)))
    out = np.empty(words.value, np.uint32)
    _check(lib().hs_debug_slimq_arrays_host(*args, out.ctypes.data, out.size, ctypes.byref(words), ctypes.byref(st), ctypes.byref(rw)))
    return out, st.value, rw.value


def debug_rq_quantize_rows(dim, metric, flips, rows, centroids, cluster_ids=None, device=-1, want_rotated=True):
    """hs_debug_rq_quantize_rows: the data-side quantiser alone on explicit flip bytes -- the host recipe (device=-1) or the kernels of
    convert_slimq_gpu.  Returns (rotated n x padded or None, cluster uint32[n], codes uint64[n x padded/64], factors float32[n x 3])."""
    padded = (dim + 63) // 64 * 64
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, dim)
    c = np.ascontiguousarray(centroids, np.float32).reshape(-1, dim)
    flips = np.ascontiguousarray(flips, np.uint8)
    if flips.size != 4 * padded // 8:
        raise HsError(HS_ERR_INVALID, "flips: 4 * padded / 8 bytes")
    cid = None if cluster_ids is None else np.ascontiguousarray(cluster_ids, np.uint32)
    n = rows.shape[0]
    rot = np.empty((n, padded), np.float32) if want_rotated else None
    cl, codes, fac = np.empty(n, np.uint32), np.empty((n, padded // 64), np.uint64), np.empty((n, 3), np.float32)
    _check(lib().hs_debug_rq_quantize_rows(dim, metric, flips.ctypes.data, rows.ctypes.data, n, c.ctypes.data, c.shape[0],
                                           None if cid is None else cid.ctypes.data, device, None if rot is None else rot.ctypes.data,
                                           cl.ctypes.data, codes.ctypes.data, fac.ctypes.data))
    return rot, cl, codes, fac


def rabitq_default_tconst(padded_dim, seed=1):
    return lib().hs_rabitq_default_tconst(padded_dim, seed)


def rabitq_rotate(dim, flips, x):
    x = np.ascontiguousarray(x, np.float32)
    padded = (dim + 63) // 64 * 64
    flips = np.ascontiguousarray(flips, np.uint8)
    out = np.empty((x.shape[0], padded), np.float32)
    _check(lib().hs_rabitq_rotate(dim, flips.ctypes.data, x.ctypes.data, x.shape[0], out.ctypes.data))
    return out


def rabitq_quantize_data(rotated, centroid, metric=HS_METRIC_L2):
    r = np.ascontiguousarray(rotated, np.float32)
    c = np.ascontiguousarray(centroid, np.float32)
    n, padded = r.shape
    codes = np.empty((n, padded // 64), np.uint64)
    fac = np.empty((n, 3), np.float32)
    _check(lib().hs_rabitq_quantize_data(padded, metric, r.ctypes.data, n, c.ctypes.data, codes.ctypes.data, fac.ctypes.data))
    return codes, fac


def rabitq_prepare_query(rotated_q, t_const):
    r = np.ascontiguousarray(rotated_q, np.float32)
    n, padded = r.shape
    q3 = np.empty((n, 3), np.float32)
    bins = np.empty((n, padded // 64 * 4), np.uint64)
    _check(lib().hs_rabitq_prepare_query(padded, float(t_const), r.ctypes.data, n, q3.ctypes.data, bins.ctypes.data))
    return q3, bins


def rabitq_estimate(codes, fac, q3, bins, g_add, g_error):
    nd, nblk = codes.shape
    nq = q3.shape[0]
    out = np.empty((nq, nd, 3), np.float32)
    a = [np.ascontiguousarray(x) for x in (codes, fac, q3, bins, np.asarray(g_add, np.float32), np.asarray(g_error, np.float32))]
    _check(lib().hs_rabitq_estimate(nblk * 64, a[0].ctypes.data, a[1].ctypes.data, nd, a[2].ctypes.data, a[3].ctypes.data,
                                    a[4].ctypes.data, a[5].ctypes.data, nq, out.ctypes.data))
    return out


class PinnedArray:
    """A numpy view of page-locked host memory (hs_host_alloc), for the asynchronous host-pointer entry."""

    def __init__(self, shape, dtype):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ptr = lib().hs_host_alloc(self.nbytes)
        if not self.ptr:
            raise HsError(HS_ERR_NOMEM, "hs_host_alloc failed")
        buf = (ctypes.c_char * max(self.nbytes, 1)).from_address(self.ptr)
        self.a = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def device_view(self, rows=None):
        """An object search_ids_dev accepts as d_queries: the device's address of this buffer (hs_host_device_pointer) -- the kernels
        then read the queries in place instead of from a staged copy.  None when the buffer is not device-mapped."""
        p = lib().hs_host_device_pointer(self.ptr)
        if not p:
            return None
        shape = self.a.shape if rows is None else (rows,) + tuple(self.a.shape[1:])

        class _View:
            def __init__(v):
                v.shape = shape

            def data_ptr(v):
                return p
        return _View()

    def __del__(self):
        try:
            self.a = None
            lib().hs_host_free(self.ptr)
        except Exception:
            pass


class Comm:
    """hs_comm: n devices of one process (the same device listed twice = the one-GPU rehearsal mode)."""

    def __init__(self, devices):
        self._h = ctypes.c_void_p()
        dv = (ctypes.c_int * len(devices))(*devices)
        _check(lib().hs_comm_init(len(devices), dv, ctypes.byref(self._h)))
        self.devices = list(devices)

    def close(self):
        if self._h:
            lib().hs_comm_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def search_ids(self, replicas, queries, k, want_dists=False):
        """HS_MODE_SLIM_IDS over the replicas (Index objects, one per device of the communicator)."""
        q = np.ascontiguousarray(queries, np.float32)
        nq = q.shape[0]
        hs_ = (ctypes.c_void_p * len(replicas))(*[r._h for r in replicas])
        labels = np.empty((nq, k), np.uint32)
        dists = np.empty((nq, k), np.float32) if want_dists else None
        cnt = np.empty(nq, np.uint32)
        _check(lib().hs_search_batch_sharded(self._h, hs_, q.ctypes.data, nq, k, HS_MODE_SLIM_IDS, labels.ctypes.data, None,
                                             dists.ctypes.data if want_dists else None, cnt.ctypes.data))
        return dict(labels=labels, dists=dists, cnt=cnt)

    def slots(self):
        return lib().hs_comm_slots(self._h)

    def search_ids_async(self, replicas, q_pinned, k, labels_pinned, slot):
        """hs_search_batch_sharded_async, HS_MODE_SLIM_IDS: numpy views of page-locked memory; pair with check(replicas, slot)."""
        hs_ = (ctypes.c_void_p * len(replicas))(*[r._h for r in replicas])
        _check(lib().hs_search_batch_sharded_async(self._h, hs_, q_pinned.ctypes.data, q_pinned.shape[0], k, HS_MODE_SLIM_IDS,
                                                   labels_pinned.ctypes.data, None, None, None, slot))

    def check(self, replicas, slot):
        hs_ = (ctypes.c_void_p * len(replicas))(*[r._h for r in replicas])
        _check(lib().hs_comm_check(self._h, hs_, slot))

    def search_pq(self, replicas, queries, k):
        q = np.ascontiguousarray(queries, np.float32)
        nq = q.shape[0]
        hs_ = (ctypes.c_void_p * len(replicas))(*[r._h for r in replicas])
        labels = np.empty((nq, k), np.uint64)
        dists = np.empty((nq, k), np.float32)
        cnt = np.empty(nq, np.uint32)
        _check(lib().hs_search_batch_sharded(self._h, hs_, q.ctypes.data, nq, k, HS_MODE_PQ, None, labels.ctypes.data, dists.ctypes.data,
                                             cnt.ctypes.data))
        return dict(labels=labels, dists=dists, cnt=cnt)


class Index:
    """A device-resident index (mirror of hnswlib::HierarchicalNSW / HierarchicalNSWSlim for search)."""

    def __init__(self, path, kind, dim, metric=HS_METRIC_L2, max_elements=0, device=0):
        self._h = ctypes.c_void_p()
        self.kind, self.dim, self.metric, self.device = kind, dim, metric, device
        self.ef = 10
        if isinstance(path, (bytes, bytearray, memoryview)):   # the serialized index itself (hs_index_load_mem)
            buf = bytes(path)
            _check(lib().hs_index_load_mem(buf, len(buf), kind, metric, dim, max_elements, device, ctypes.byref(self._h)))
        else:
            _check(lib().hs_index_load(path.encode(), kind, metric, dim, max_elements, device, ctypes.byref(self._h)))

    @classmethod
    def load_narrow(cls, path, kind, dim, fmt, metric=HS_METRIC_L2, max_elements=0, device=0):
        """hs_index_load_narrow: the index of `path` with its rows on the device in `fmt` (HS_ROWS_U8 / HS_ROWS_F16) only -- what
        Index(path, ...) + set_row_format(fmt) + set_f32_resident(False) gives, without the fp32 array ever being allocated."""
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        self.kind, self.dim, self.metric, self.device, self.ef = kind, dim, metric, device, 10
        _check(lib().hs_index_load_narrow(path.encode(), kind, metric, dim, max_elements, device, int(fmt), ctypes.byref(self._h)))
        return self

    @classmethod
    def from_arrays(cls, kind, metric, vectors, levels, lists, enterpoint, maxlevel, labels=None, deleted=None, threshold_level=0, device=0):
        """hs_index_from_host_arrays: lists[i][l] = neighbour ids of node i at level l (l = 0..levels[i])."""
        v = np.ascontiguousarray(vectors, np.float32)
        n, dim = v.shape
        lv = np.ascontiguousarray(levels, np.int32)
        flat = [np.asarray(l, np.uint32) for node in lists for l in node]
        ptr = np.zeros(len(flat) + 1, np.uint64)
        ptr[1:] = np.cumsum([len(x) for x in flat])
        ids = np.ascontiguousarray(np.concatenate(flat) if flat else np.zeros(0, np.uint32), np.uint32)
        lab = None if labels is None else np.ascontiguousarray(labels, np.uint64)
        dl = None if deleted is None else np.ascontiguousarray(deleted, np.uint8)
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        self.kind, self.dim, self.metric, self.device, self.ef = kind, dim, metric, device, 10
        _check(lib().hs_index_from_host_arrays(kind, metric, n, dim, v.ctypes.data, None if lab is None else lab.ctypes.data,
                                               None if dl is None else dl.ctypes.data, lv.ctypes.data, ptr.ctypes.data, ids.ctypes.data,
                                               int(enterpoint), int(maxlevel), int(threshold_level), device, ctypes.byref(self._h)))
        return self

    @classmethod
    def from_csr(cls, kind, metric, vectors, levels, list_ptr, list_ids, enterpoint, maxlevel, labels=None, threshold_level=0, device=0):
        """hs_index_from_host_arrays with the flat arrays as the C ABI takes them (node i owns levels[i] + 1 consecutive lists)."""
        v = np.ascontiguousarray(vectors, np.float32)
        n, dim = v.shape
        lv, ptr, ids = np.ascontiguousarray(levels, np.int32), np.ascontiguousarray(list_ptr, np.uint64), np.ascontiguousarray(list_ids, np.uint32)
        lab = None if labels is None else np.ascontiguousarray(labels, np.uint64)
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        self.kind, self.dim, self.metric, self.device, self.ef = kind, dim, metric, device, 10
        _check(lib().hs_index_from_host_arrays(kind, metric, n, dim, v.ctypes.data, None if lab is None else lab.ctypes.data, None,
                                               lv.ctypes.data, ptr.ctypes.data, ids.ctypes.data, int(enterpoint), int(maxlevel),
                                               int(threshold_level), device, ctypes.byref(self._h)))
        return self

    def close(self):
        if self._h:
            lib().hs_index_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def patch(self, stream_bytes, to_add=False):
        """patchFromStream: apply a genPatch stream to this device-resident Slim index (loaded with max_elements > count)."""
        b = bytes(stream_bytes)
        _check(lib().hs_index_patch(self._h, b, len(b), 1 if to_add else 0))

    def convert_diff(self, hnsw, top_degree_percent0=0.02, top_degree_percent=0.02, top_degree_M0=32, low_degree_m0=8, top_degree_M=16,
                     low_degree_m=4, threads=8):
        """hs_slim_convert_diff: re-derive this resident Slim index from the resident vanilla Index `hnsw` (both loaded with
        max_elements > count) and return the SlimDiff (its .used_gpu / .kernel_ms say where the list passes ran)."""
        h, used, ms = ctypes.c_void_p(), ctypes.c_int(0), ctypes.c_double(0.0)
        _check(lib().hs_slim_convert_diff(self._h, hnsw._h, top_degree_percent0, top_degree_percent, top_degree_M0, low_degree_m0,
                                          top_degree_M, low_degree_m, threads, ctypes.byref(h), ctypes.byref(used), ctypes.byref(ms)))
        return SlimDiff(h, self, bool(used.value), ms.value)

    def save_slim(self, path):
        """hs_slim_index_save: saveIndex of this Slim index's host image (an index loaded with max_elements > its count)."""
        _check(lib().hs_slim_index_save(self._h, path.encode()))

    # -- live updates (HS_KIND_HNSW) ----------------------------------------------------------------
    def add_points(self, rows, labels, threads=1):
        """hs_index_add_points: addPoint(rows[i], labels[i]) for new labels on an index loaded with max_elements > its count."""
        r = np.ascontiguousarray(rows, np.float32)
        r = r.reshape(-1, self.dim) if r.ndim != 2 else r
        lab = np.ascontiguousarray(labels, np.uint64)
        if lab.shape != (r.shape[0],) or r.shape[1] != self.dim:
            raise HsError(HS_ERR_INVALID, "add_points: rows count x dim, one label per row")
        _check(lib().hs_index_add_points(self._h, r.ctypes.data, lab.ctypes.data, r.shape[0], threads))

    def add_points_batched(self, rows, labels, device=None, threads=1, grow_div=0, batch_max=0, scratch_ids=0):
        """hs_index_add_points_batched: add_points in the batched order -- on the index's device (the default) or on the
        host twin (device=-1), the same bytes either way.  Returns the stats dict of build_hnsw_batched."""
        r = np.ascontiguousarray(rows, np.float32)
        r = r.reshape(-1, self.dim) if r.ndim != 2 else r
        lab = np.ascontiguousarray(labels, np.uint64)
        if lab.shape != (r.shape[0],) or r.shape[1] != self.dim:
            raise HsError(HS_ERR_INVALID, "add_points_batched: rows count x dim, one label per row")
        opts = HsBatchBuildOpts(self.device if device is None else device, threads, grow_div, batch_max, scratch_ids)
        st = HsBatchBuildStats()
        _check(lib().hs_index_add_points_batched(self._h, r.ctypes.data, lab.ctypes.data, r.shape[0], ctypes.byref(opts), ctypes.byref(st)))
        return _batch_stats(st)

    def batched_add_changed(self):
        """hs_debug_batched_add_changed: (the old internal ids whose lists the last device-side add_points_batched changed, the
        number of old lists it downloaded)."""
        n, dl = ctypes.c_size_t(0), ctypes.c_size_t(0)
        _check(lib().hs_debug_batched_add_changed(self._h, None, 0, ctypes.byref(n), ctypes.byref(dl)))
        ids = np.zeros(n.value, np.uint32)
        _check(lib().hs_debug_batched_add_changed(self._h, ids.ctypes.data, n.value, ctypes.byref(n), None))
        return ids, dl.value

    def upsert_points(self, rows, labels, replace_deleted=None):
        """hs_index_upsert_points: addPoint(rows[i], labels[i], replace_deleted[i]) serially, as the reference: an existing label is
        updated, a new label with its flag set takes a deleted slot while one is vacant, anything else is appended."""
        r = np.ascontiguousarray(rows, np.float32)
        r = r.reshape(-1, self.dim) if r.ndim != 2 else r
        lab = np.ascontiguousarray(np.atleast_1d(labels), np.uint64)
        if lab.shape != (r.shape[0],) or r.shape[1] != self.dim:
            raise HsError(HS_ERR_INVALID, "upsert_points: rows count x dim, one label per row")
        fl = None
        if replace_deleted is not None:
            fl = np.ascontiguousarray(np.broadcast_to(np.asarray(replace_deleted, bool), lab.shape), np.uint8)
        _check(lib().hs_index_upsert_points(self._h, r.ctypes.data, lab.ctypes.data, None if fl is None else fl.ctypes.data, r.shape[0]))

    def set_replace_deleted(self, on=True):
        """hs_index_set_replace_deleted: the constructor's allow_replace_deleted."""
        _check(lib().hs_index_set_replace_deleted(self._h, 1 if on else 0))

    def resize(self, new_max_elements):
        """hs_index_resize: resizeIndex; the per-node device arrays move by device-to-device copies."""
        _check(lib().hs_index_resize(self._h, int(new_max_elements)))

    def seed_levels(self, seed, drawn):
        """hs_index_seed_levels: the level generator as a build with `seed` holds it after `drawn` points."""
        _check(lib().hs_index_seed_levels(self._h, int(seed), int(drawn)))

    def mark_deleted(self, labels, on=True):
        """hs_index_mark_deleted: markDelete (on) / unmarkDelete (not on) of every label, all or nothing."""
        lab = np.ascontiguousarray(np.atleast_1d(labels), np.uint64)
        _check(lib().hs_index_mark_deleted(self._h, lab.ctypes.data, lab.shape[0], 1 if on else 0))

    def save(self, path):
        """hs_index_save: saveIndex of the host image (an index loaded with max_elements > its count)."""
        _check(lib().hs_index_save(self._h, path.encode()))

    def get_row(self, label):
        """hs_index_get_row: getDataByLabel, read back from the device (dim float32)."""
        out = np.empty(self.dim, np.float32)
        _check(lib().hs_index_get_row(self._h, int(label), out.ctypes.data))
        return out

    def capacity(self):
        return int(lib().hs_index_capacity(self._h))

    def deleted_count(self):
        return int(lib().hs_index_deleted_count(self._h))

    def info(self):
        i = HsInfo()
        _check(lib().hs_index_info(self._h, ctypes.byref(i)))
        return {f[0]: getattr(i, f[0]) for f in HsInfo._fields_}

    def set_ef(self, ef):
        self.ef = int(ef)
        _check(lib().hs_set_ef(self._h, int(ef)))

    def set_row_format(self, fmt):
        """hs_index_set_row_format: HS_ROWS_U8 / HS_ROWS_F16 build a narrow copy of the rows that the flat kernel then reads
        (HsError HS_ERR_UNSUPPORTED, index unchanged, when a stored value is not exactly representable); HS_ROWS_F32 drops it.
        No answer changes."""
        _check(lib().hs_index_set_row_format(self._h, int(fmt)))

    def row_format(self):
        return lib().hs_index_row_format(self._h)

    def set_f32_resident(self, on):
        """hs_index_set_f32_resident: False frees the fp32 rows of an index in a narrow row format -- every search kernel then reads
        the narrow copy (hs::flat_kernel_u8, hs::fast_kernel_u8, hs::strict_kernel_u8, ...) -- True re-creates them from it.
        No answer changes."""
        _check(lib().hs_index_set_f32_resident(self._h, 1 if on else 0))

    def f32_resident(self):
        return bool(lib().hs_index_f32_resident(self._h))

    def set_exact_order(self, on=True):
        """True: strict kernel for every query (reference array order); False: fast kernel, sorted output."""
        _check(lib().hs_set_exact_order(self._h, 1 if on else 0))

    def set_capacity(self, cand_cap=0, hash_slots=0):
        _check(lib().hs_set_capacity(self._h, cand_cap, hash_slots))

    # -- host-pointer API -------------------------------------------------------------------------
    def search_ids(self, queries, k, want_dists=False, want_stats=False):
        """HierarchicalNSWSlim::searchKnn(q, k, tableint*) for every row of `queries`."""
        q = np.ascontiguousarray(queries, np.float32)
        nq = q.shape[0]
        labels = np.empty((nq, k), np.uint32)
        dists = np.empty((nq, k), np.float32) if want_dists else None
        cnt = np.empty(nq, np.uint32)
        stats = np.empty((nq, 4), np.uint32) if want_stats else None
        _check(lib().hs_search_batch(self._h, q.ctypes.data, nq, k, HS_MODE_SLIM_IDS, labels.ctypes.data, None,
                                     dists.ctypes.data if want_dists else None, cnt.ctypes.data,
                                     stats.ctypes.data if want_stats else None))
        return dict(labels=labels, dists=dists, cnt=cnt, stats=stats)

    def search_pq(self, queries, k, want_stats=False):
        """priority_queue-returning searchKnn overloads: the <=k (dist,label) pairs per query."""
        q = np.ascontiguousarray(queries, np.float32)
        nq = q.shape[0]
        labels = np.empty((nq, k), np.uint64)
        dists = np.empty((nq, k), np.float32)
        cnt = np.empty(nq, np.uint32)
        stats = np.empty((nq, 4), np.uint32) if want_stats else None
        _check(lib().hs_search_batch(self._h, q.ctypes.data, nq, k, HS_MODE_PQ, None, labels.ctypes.data, dists.ctypes.data,
                                     cnt.ctypes.data, stats.ctypes.data if want_stats else None))
        return dict(labels=labels, dists=dists, cnt=cnt, stats=stats)

    # ---- HNSW-SlimQ (kind == HS_KIND_SLIMQ) ----
    def slimq_set_dataset(self, base):
        """HierarchicalNSWSlimQ::setDataset: raw rows by internal id, used for the exact re-rank."""
        b = np.ascontiguousarray(base, np.float32)
        _check(lib().hs_slimq_set_dataset(self._h, b.ctypes.data, b.shape[0], b.shape[1]))

    def slimq_set_tconst(self, t_const):
        _check(lib().hs_slimq_set_tconst(self._h, float(t_const)))

    def slimq_tconst(self):
        return lib().hs_slimq_get_tconst(self._h)

    def slimq_search(self, queries, k, want_stats=False):
        """searchKnn(q, k, result) of HierarchicalNSWSlimQ: labels/dists in the reference's heap-array order."""
        q = np.ascontiguousarray(queries, np.float32)
        nq = q.shape[0]
        labels = np.empty((nq, k), np.uint64)
        dists = np.empty((nq, k), np.float32)
        cnt = np.empty(nq, np.uint32)
        stats = np.empty((nq, 4), np.uint32) if want_stats else None
        _check(lib().hs_slimq_search_batch(self._h, q.ctypes.data, nq, k, labels.ctypes.data, dists.ctypes.data, cnt.ctypes.data,
                                           stats.ctypes.data if want_stats else None))
        return dict(labels=labels, dists=dists, cnt=cnt, stats=stats)

    def save_slimq(self, path):
        """hs_slimq_index_save: saveIndex of the host image a resident SlimQ index keeps."""
        _check(lib().hs_slimq_index_save(self._h, path.encode()))

    def debug_slimq_arrays(self, which):
        """hs_debug_slimq_arrays: rec (which=0), ftile (1) or uptile (2) as they lie on the device.  Returns (uint32 words, stride,
        row_words); an array the index does not have comes back empty with stride 0."""
        words, st, rw = ctypes.c_size_t(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().hs_debug_slimq_arrays(self._h, which, None, 0, ctypes.byref(words), ctypes.byref(st), ctypes.byref(rw)))
        out = np.empty(words.value, np.uint32)
        _check(lib().hs_debug_slimq_arrays(self._h, which, out.ctypes.data, out.size, ctypes.byref(words), ctypes.byref(st), ctypes.byref(rw)))
        return out, st.value, rw.value

    def labels(self):
        out = np.empty(self.info()["n"], np.uint64)
        _check(lib().hs_labels(self._h, out.ctypes.data))
        return out

    def search_filtered(self, queries, k, allowed, want_stats=False):
        """searchKnn(q, k, isIdAllowed): allowed[i] != 0 iff the filter accepts the label of internal id i."""
        q = np.ascontiguousarray(queries, np.float32)
        a = np.ascontiguousarray(allowed, np.uint8)
        nq = q.shape[0]
        labels = np.empty((nq, k), np.uint64)
        dists = np.empty((nq, k), np.float32)
        cnt = np.empty(nq, np.uint32)
        stats = np.empty((nq, 4), np.uint32) if want_stats else None
        _check(lib().hs_search_batch_filtered(self._h, q.ctypes.data, nq, k, a.ctypes.data, labels.ctypes.data, dists.ctypes.data,
                                              cnt.ctypes.data, stats.ctypes.data if want_stats else None))
        return dict(labels=labels, dists=dists, cnt=cnt, stats=stats)

    def search_filter_set(self, queries, k, fs, filter_of_query, want_stats=False):
        """hs_search_batch_filter_set: search_filtered with query i under filter filter_of_query[i] of the FilterSet `fs`."""
        q = np.ascontiguousarray(queries, np.float32)
        foq = np.ascontiguousarray(filter_of_query, np.uint32)
        nq = q.shape[0]
        if foq.shape != (nq,):
            raise HsError(HS_ERR_INVALID, "filter_of_query: one filter index per query")
        labels = np.empty((nq, k), np.uint64)
        dists = np.empty((nq, k), np.float32)
        cnt = np.empty(nq, np.uint32)
        stats = np.empty((nq, 4), np.uint32) if want_stats else None
        _check(lib().hs_search_batch_filter_set(self._h, fs._h, q.ctypes.data, nq, k, foq.ctypes.data, labels.ctypes.data,
                                                dists.ctypes.data, cnt.ctypes.data, stats.ctypes.data if want_stats else None))
        return dict(labels=labels, dists=dists, cnt=cnt, stats=stats)

    def search_filter_set_dev(self, d_queries, k, fs, d_filter_of_query, d_labels, d_dists, d_counts, d_stats=None, stream=0):
        """hs_search_batch_filter_set_dev: device tensors (queries f32 nq x d, filter indices int32 nq, labels int64 nq x k, dists
        f32 nq x k, counts int32 nq, stats int32 nq x 4) + HIP stream; asynchronous, pair with check(stream)."""
        _check(lib().hs_search_batch_filter_set_dev(self._h, fs._h, d_queries.data_ptr(), d_queries.shape[0], k,
                                                    d_filter_of_query.data_ptr(), d_labels.data_ptr(), d_dists.data_ptr(),
                                                    d_counts.data_ptr(), d_stats.data_ptr() if d_stats is not None else None, stream))

    def exact_search(self, queries, k, fs=None, filter_of_query=None):
        """hs_index_exact_search: exact k-NN over the rows this index holds (fp32 or its narrow copy), under its delete marks and,
        with a FilterSet `fs`, query i under filter filter_of_query[i].  labels / dists nq x k ascending by (dist, label), ~0 / +inf
        beyond cnt[i].  ef, exact order and capacity settings do not apply."""
        q = np.ascontiguousarray(queries, np.float32)
        nq = q.shape[0]
        foq = None if filter_of_query is None else np.ascontiguousarray(filter_of_query, np.uint32)
        if foq is not None and foq.shape != (nq,):
            raise HsError(HS_ERR_INVALID, "filter_of_query: one filter index per query")
        labels = np.empty((nq, k), np.uint64)
        dists = np.empty((nq, k), np.float32)
        cnt = np.empty(nq, np.uint32)
        _check(lib().hs_index_exact_search(self._h, None if fs is None else fs._h, q.ctypes.data, nq, k,
                                           None if foq is None else foq.ctypes.data, labels.ctypes.data, dists.ctypes.data, cnt.ctypes.data))
        return dict(labels=labels, dists=dists, cnt=cnt)

    def exact_search_dev(self, d_queries, k, d_labels, d_dists, d_counts=None, fs=None, d_filter_of_query=None, stream=0):
        """hs_index_exact_search_dev: device tensors (queries f32 nq x d, labels int64 nq x k, dists f32 nq x k, counts int32 nq,
        filter indices int32 nq) + HIP stream; asynchronous, pair with check(stream).  Tiles of 8 queries are formed in the order
        given: group the queries by filter to let a tile skip what its filters exclude."""
        _check(lib().hs_index_exact_search_dev(self._h, None if fs is None else fs._h, d_queries.data_ptr(), d_queries.shape[0], k,
                                               None if d_filter_of_query is None else d_filter_of_query.data_ptr(), d_labels.data_ptr(),
                                               d_dists.data_ptr(), d_counts.data_ptr() if d_counts is not None else None, stream))

    def search_raw(self, queries, k, mode=HS_MODE_SLIM_IDS):
        q = np.ascontiguousarray(queries, np.float32)
        nq = q.shape[0]
        cap = max(self.ef, k)
        rd = np.empty((nq, cap), np.float32)
        ri = np.empty((nq, cap), np.uint32)
        rs = np.empty(nq, np.uint32)
        stats = np.empty((nq, 4), np.uint32)
        _check(lib().hs_search_batch_raw(self._h, q.ctypes.data, nq, k, mode, rd.ctypes.data, ri.ctypes.data, rs.ctypes.data,
                                         stats.ctypes.data))
        return dict(raw_d=rd, raw_i=ri, raw_sz=rs, stats=stats)

    def search_ids_async(self, q_pinned, k, labels_pinned, stream=0, dists_pinned=None, counts_pinned=None):
        """hs_search_batch_async, HS_MODE_SLIM_IDS: numpy views of page-locked memory (PinnedArray.a), a HIP stream handle."""
        _check(lib().hs_search_batch_async(self._h, q_pinned.ctypes.data, q_pinned.shape[0], k, HS_MODE_SLIM_IDS, labels_pinned.ctypes.data, None,
                                           dists_pinned.ctypes.data if dists_pinned is not None else None,
                                           counts_pinned.ctypes.data if counts_pinned is not None else None, None, stream))

    # -- device-pointer API (torch tensors on this index's device; async on `stream`) ----------------
    def search_ids_dev(self, d_queries, k, d_labels, d_dists=None, d_counts=None, d_stats=None, stream=0):
        nq = d_queries.shape[0]
        _check(lib().hs_search_batch_dev(self._h, d_queries.data_ptr(), nq, k, HS_MODE_SLIM_IDS, d_labels.data_ptr(), None,
                                         d_dists.data_ptr() if d_dists is not None else None,
                                         d_counts.data_ptr() if d_counts is not None else None,
                                         d_stats.data_ptr() if d_stats is not None else None, stream))

    def slimq_prepare_debug(self, queries, padded, ncl):
        """dict(rq, q3, g_add, planes) as the kernel computed them."""
        q = np.ascontiguousarray(queries, np.float32)
        row = padded + 3 + ncl + padded // 8
        out = np.empty((q.shape[0], row), np.float32)
        _check(lib().hs_slimq_prepare_debug(self._h, q.ctypes.data, q.shape[0], out.ctypes.data))
        pl = np.ascontiguousarray(out[:, padded + 3 + ncl:]).view(np.uint64)
        return dict(rq=out[:, :padded].copy(), q3=out[:, padded:padded + 3].copy(), g_add=out[:, padded + 3:padded + 3 + ncl].copy(), planes=pl)

    def slimq_trace(self, queries, k, cap=4096):
        q = np.ascontiguousarray(queries, np.float32)
        tr = np.empty((q.shape[0], cap), np.uint32)
        st = np.empty((q.shape[0], 4), np.uint32)
        _check(lib().hs_slimq_trace(self._h, q.ctypes.data, q.shape[0], k, tr.ctypes.data, cap, st.ctypes.data))
        return tr, st

    def slimq_search_dev(self, d_queries, k, d_labels, d_dists, d_counts, d_stats=None, stream=0):
        """Device tensors (labels int64 nq x k, dists f32 nq x k, counts int32 nq) + HIP stream; asynchronous."""
        _check(lib().hs_slimq_search_batch_dev(self._h, d_queries.data_ptr(), d_queries.shape[0], k, d_labels.data_ptr(),
                                               d_dists.data_ptr(), d_counts.data_ptr(),
                                               d_stats.data_ptr() if d_stats is not None else None, stream))

    def last_kernel(self):
        return lib().hs_last_kernel(self._h).decode()

    def check(self, stream=0):
        _check(lib().hs_search_check(self._h, stream))
