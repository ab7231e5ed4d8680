"""ctypes bindings of the MI355X BSMR-SDDMM engine.

Binds the two C ABIs declared in /include:
  * bsmr_hip.h  (lib/libbsmr_hip.so)  -- device plan + HIP kernels
  * bsmr_host.h (lib/libbsmr_host.so) -- host BSMR pipeline (C++/OpenMP)

This module is plumbing for tests and bench.py; it contains no arithmetic.  If
the libraries are missing it raises: there is no fallback path.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent.parent
LIB_DIR = PKG_DIR / "lib"

OK = 0
ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_UNSUPPORTED_K, ERR_OOM, ERR_BAD_PLAN = 1, 2, 3, 4, 5, 6
COMPUTE_F16, COMPUTE_BF16, COMPUTE_F32 = 0, 1, 2
FP8_E4M3, FP8_E5M2 = 0, 1   # BSMR_FP8_*: OCP e4m3fn / e5m2, the formats of an fp8 column-side operand
ROWS_CLUSTER, ROWS_IDENTITY = 0, 1

ARRAY_IDS = {
    "reorderedRows": 0, "denseCols": 1, "denseColOffsets": 2, "sparseCols": 3,
    "sparseColOffsets": 4, "sparseValueOffsets": 5, "blockOffsets": 6, "blockValues": 7,
    "sparseValues": 8, "sparseRelativeRows": 9, "sparseColIndices": 10,
    "denseRowPanelIds": 11, "denseColBlockIters": 12, "sparseRowPanelIds": 13,
    "sparseColBlockIters": 14,
}

u32p = C.POINTER(C.c_uint32)
f32p = C.POINTER(C.c_float)


class RphmDesc(C.Structure):
    _fields_ = [("M", C.c_uint32), ("N", C.c_uint32), ("nnz", C.c_uint32),
                ("num_row_panels", C.c_uint32), ("num_nonzero_rows", C.c_uint32),
                ("reordered_rows", u32p), ("dense_cols", u32p), ("block_offsets", u32p),
                ("block_values", u32p), ("sparse_value_offsets", u32p), ("sparse_values", u32p),
                ("sparse_relative_rows", u32p), ("sparse_col_indices", u32p)]


# BSMR_VARIANT_* (include/bsmr_hip.h): the plan-time rules bsmr_plan_tune tries for a plan created with k_hint > 0
VARIANT_NAMES = ("rules", "as_rphm", "no_promotion", "promote_24", "promote_all", "all_residue")


class TuneReport(C.Structure):
    _fields_ = [("chosen_engine", C.c_int32), ("chosen_group", C.c_int32), ("chosen_blocks_per_item", C.c_int32),
                ("stream_us", C.c_float), ("grouped_us", C.c_float), ("tiles_us", C.c_float), ("shared_us", C.c_float),
                ("chosen_b_only", C.c_int32), ("fp32_residue_us", C.c_float), ("b_only_us", C.c_float),
                ("chosen_overlap", C.c_int32), ("one_stream_us", C.c_float), ("two_streams_us", C.c_float),
                ("chosen_cvt_in_kernel", C.c_int32), ("convert_pass_us", C.c_float), ("fp32_dense_us", C.c_float),
                ("sweep_us", C.c_float), ("lowp_call_us", C.c_float), ("sweep_fp32_call_us", C.c_float),
                ("chosen_sweep_fp32", C.c_int32), ("chosen_variant", C.c_int32), ("variant_us", C.c_float * 6),
                ("gemm_us", C.c_float), ("gemm_fp32_call_us", C.c_float), ("chosen_gemm_fp32", C.c_int32)]


class TunedChoice(C.Structure):
    """bsmr_tuned_choice: what a tuned plan keeps per (K, mode) (bsmr_plan_get_tuned / bsmr_plan_set_tuned)"""
    _fields_ = [("struct_size", C.c_uint32)] + [(n, C.c_int32) for n in (
        "engine", "group", "blocks_per_item", "format", "b_only", "overlap", "cvt_in_kernel", "waves")]


class PlanBuildMs(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("rules_ms", "pack_ms", "upload_ms", "second_format_ms", "total_ms")]


class PlanStats(C.Structure):
    _fields_ = [("num_row_panels", C.c_uint32), ("num_dense_blocks", C.c_uint64),
                ("num_dense_entries", C.c_uint64), ("num_sparse_entries", C.c_uint64),
                ("dense_work_items", C.c_uint64), ("sparse_work_items", C.c_uint64),
                ("device_index_bytes", C.c_uint64), ("group_size", C.c_uint32),
                ("num_dense_tiles", C.c_uint64), ("union_columns", C.c_uint64),
                ("grouped_group_size", C.c_uint32), ("grouped_dense_tiles", C.c_uint64),
                ("grouped_union_columns", C.c_uint64), ("sparse_lowp", C.c_uint64),
                ("folded_dense_entries", C.c_uint64), ("free_residue", C.c_uint64),
                ("promoted_sparse_entries", C.c_uint64)]


class PlanOptions(C.Structure):
    """bsmr_plan_options (include/bsmr_hip.h): every rule of plan construction that is not in the RPHM arrays"""
    _fields_ = [("struct_size", C.c_uint32)] + [(name, C.c_int32) for name in (
        "dense_engine", "fold_dense_below", "promote_average", "promote_min_entries_k", "promote_column_degree",
        "promote_head", "dense_group", "dense_blocks_per_item", "stream_waves", "output_mode", "force_tile32",
        "column_order", "dense_stream", "dense_batch", "tile_group", "tile_blocks_per_item", "tile_depth",
        "sparse_entries_per_item", "sparse_lowp", "sparse_lpe", "free_residue", "convert_in_kernel", "convert_sliced",
        "b_only", "b_only_work_m", "overlap_streams", "mask_tiles", "pack_on_device", "sweep_panels", "sweep_strip_blocks",
        "sweep_fp32", "sweep_waves", "sweep_per_cu", "k_hint", "promote_on_device", "gemm_panels", "gemm_blocks", "gemm_fp32", "gemm_balance_columns", "evict_wide_rows")]


ENGINE_STREAM, ENGINE_TILES, ENGINE_SHARED, ENGINE_TUNED, ENGINE_SWEEP, ENGINE_GEMM = 0, 1, 2, 3, 4, 5
ENGINE_NAMES = {0: "stream", 1: "tiles", 2: "shared", 4: "sweep", 5: "gemm"}


class ReorderingReport(C.Structure):
    _fields_ = [("original_num_dense_blocks", C.c_int32), ("original_average_density", C.c_float),
                ("num_dense_blocks", C.c_int32), ("average_density", C.c_float),
                ("num_dense_thread_blocks", C.c_int32), ("num_sparse_thread_blocks", C.c_int32),
                ("num_dense_data", C.c_int32), ("num_sparse_data", C.c_int32),
                ("max_dense_blocks_per_panel", C.c_uint32), ("max_sparse_blocks_per_panel", C.c_uint32)]


class ClusterStats(C.Structure):
    _fields_ = [("elapsed_ms", C.c_float), ("passes", C.c_uint32), ("similarities", C.c_uint32),
                ("exact_similarities", C.c_uint32), ("threads_per_pair", C.c_uint32), ("table_bytes", C.c_uint64),
                ("dropped_seeds", C.c_uint32), ("passes_ahead", C.c_uint32)]


class ColReorderSizes(C.Structure):
    _fields_ = [("num_row_panels", C.c_uint32), ("num_dense_cols", C.c_uint64), ("num_sparse_cols", C.c_uint64),
                ("num_blocks", C.c_uint64), ("num_sparse_entries", C.c_uint64), ("elapsed_ms", C.c_float)]


class ShardedTiming(C.Structure):
    _fields_ = [("step_ms", C.c_float), ("wall_ms", C.c_float), ("num_devices", C.c_uint32), ("compute_ms", C.c_float),
                ("gather_ms", C.c_float)]


class BackwardStats(C.Structure):
    _fields_ = [("chunk", C.c_uint32), ("split_rows", C.c_uint32), ("split_cols", C.c_uint32),
                ("max_row_length", C.c_uint32), ("max_col_length", C.c_uint32), ("row_items", C.c_uint32),
                ("col_items", C.c_uint32), ("permute_values", C.c_uint32), ("device_index_bytes", C.c_uint64),
                ("workspace_bytes", C.c_uint64)]


class BlockedStats(C.Structure):
    """bsmr_blocked_stats: what bsmr_blocked_check counts in an RPHM (device_index_bytes: attached handles only)"""
    _fields_ = [("panels", C.c_uint32), ("panels_with_blocks", C.c_uint32), ("blocks", C.c_uint64),
                ("block_entries", C.c_uint64), ("padding_columns", C.c_uint64), ("residue_entries", C.c_uint64),
                ("max_residue_row", C.c_uint32), ("split_residue_rows", C.c_uint32), ("max_blocks_per_panel", C.c_uint32),
                ("residue_items", C.c_uint32), ("device_index_bytes", C.c_uint64),
                # segment_blocks = S of bsmr_blocked_check_split / bsmr_backward_attach_blocks_split (S = 0: 0, 0,
                # panels_with_blocks, max_blocks_per_panel)
                ("segment_blocks", C.c_uint32), ("split_panels", C.c_uint32), ("segments", C.c_uint32),
                ("max_blocks_per_segment", C.c_uint32)]


class Timing(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("convert_ms", C.c_float), ("dense_ms", C.c_float),
                ("sparse_ms", C.c_float)]


# every symbol the two headers declare: name -> (restype, argtypes)
HIP_SYMBOLS = {
    "bsmr_strerror": (C.c_char_p, [C.c_int]),
    "bsmr_last_hip_error": (C.c_char_p, []),
    "bsmr_abi_revision": (C.c_int, []),
    "bsmr_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "bsmr_mem_info": (C.c_int, [C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "bsmr_device_name": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t]),
    "bsmr_dev_alloc": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]),
    "bsmr_dev_free": (C.c_int, [C.c_void_p]),
    "bsmr_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "bsmr_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "bsmr_dev_memset": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t]),
    "bsmr_device_synchronize": (C.c_int, [C.c_int]),
    "bsmr_plan_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(RphmDesc)]),
    "bsmr_plan_create_ex": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(RphmDesc), C.POINTER(PlanOptions)]),
    "bsmr_plan_options_default": (C.c_int, [C.POINTER(PlanOptions)]),
    "bsmr_plan_options_from_env": (C.c_int, [C.POINTER(PlanOptions)]),
    "bsmr_plan_destroy": (C.c_int, [C.c_void_p]),
    "bsmr_plan_promoted_on_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "bsmr_col_reorder_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "bsmr_plan_create_from_colreorder": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, u32p, C.c_uint32,
                                                   C.c_void_p]),
    "bsmr_plan_get_stats": (C.c_int, [C.c_void_p, C.POINTER(PlanStats)]),
    "bsmr_plan_build_times": (C.c_int, [C.c_void_p, C.POINTER(PlanBuildMs)]),
    "bsmr_plan_format_digest": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "bsmr_plan_entry_lists_digest": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "bsmr_plan_tune": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                C.POINTER(TuneReport)]),
    "bsmr_cluster_rows": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float,
                                    C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_void_p]),
    "bsmr_cluster_rows_sized": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float,
                                          C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_void_p, C.c_size_t]),
    "bsmr_plan_tune_sized": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                      C.POINTER(TuneReport), C.c_size_t]),
    "bsmr_plan_get_tuned": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(TunedChoice)]),
    "bsmr_plan_set_tuned": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(TunedChoice)]),
    "bsmr_sddmm_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int,
                                   C.c_void_p]),
    "bsmr_batched_transpose": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsmr_plan_sparse_choice": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint32),
                                          C.POINTER(C.c_uint32)]),
    "bsmr_plan_dense_choice": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64)]),
    "bsmr_plan_reserve": (C.c_int, [C.c_void_p, C.c_uint32]),
    "bsmr_plan_dense_flags": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bsmr_sddmm": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                             C.c_void_p]),
    "bsmr_sddmm_timed": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(Timing)]),
    "bsmr_convert_operands": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int, C.c_void_p]),
    "bsmr_sddmm_lowp": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "bsmr_sddmm_host": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "bsmr_col_reorder": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_uint32, C.c_float]),
    "bsmr_col_reorder_sizes": (C.c_int, [C.c_void_p, C.POINTER(ColReorderSizes)]),
    "bsmr_col_reorder_fetch": (C.c_int, [C.c_void_p] + [C.c_void_p] * 10),
    "bsmr_col_reorder_free": (C.c_int, [C.c_void_p]),
    "bsmr_sharded_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_uint32,
                                      C.POINTER(C.POINTER(RphmDesc)), C.POINTER(C.c_uint32), C.POINTER(PlanOptions)]),
    "bsmr_sharded_destroy": (C.c_int, [C.c_void_p]),
    "bsmr_sharded_num_entries": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "bsmr_sharded_sddmm_host": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.POINTER(ShardedTiming)]),
    "bsmr_backward_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_uint32]),
    "bsmr_backward_destroy": (C.c_int, [C.c_void_p]),
    "bsmr_backward_reserve": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "bsmr_backward_get_stats": (C.c_int, [C.c_void_p, C.POINTER(BackwardStats), C.c_size_t]),
    "bsmr_csr_transpose": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "bsmr_spmm": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "bsmr_sddmm_backward": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_uint32, C.c_void_p]),
    "bsmr_backward_reserve_mode": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]),
    "bsmr_spmm_mode": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int,
                                 C.c_void_p]),
    "bsmr_sddmm_backward_mode": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]),
    "bsmr_spmm_lowp": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int,
                                 C.c_void_p]),
    "bsmr_sddmm_16": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]),
    "bsmr_spmm_16": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int,
                               C.c_void_p]),
    "bsmr_sddmm_backward_16": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]),
    "bsmr_blocked_check": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(RphmDesc),
                                     C.POINTER(BlockedStats), C.c_size_t]),
    "bsmr_blocked_check_split": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(RphmDesc),
                                           C.c_uint32, C.POINTER(BlockedStats), C.c_size_t]),
    "bsmr_backward_attach_blocks": (C.c_int, [C.c_void_p, C.POINTER(RphmDesc)]),
    "bsmr_backward_attach_blocks_split": (C.c_int, [C.c_void_p, C.POINTER(RphmDesc), C.c_uint32]),
    "bsmr_backward_get_blocked_stats": (C.c_int, [C.c_void_p, C.POINTER(BlockedStats), C.c_size_t]),
    "bsmr_spmm_blocked": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "bsmr_spmm_blocked_16": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int,
                                       C.c_void_p]),
    "bsmr_sparse_softmax": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "bsmr_sparse_softmax_backward": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                               C.c_void_p]),
    "bsmr_sparse_attention_reserve": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "bsmr_sparse_attention": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float] + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p]),
    "bsmr_sparse_attention_16": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float] + [C.c_void_p] * 5 +
                                 [C.c_uint32, C.c_int, C.c_void_p]),
    "bsmr_sparse_attention_backward": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float] + [C.c_void_p] * 8 +
                                       [C.c_uint32, C.c_void_p]),
    "bsmr_sparse_attention_backward_16": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float] + [C.c_void_p] * 8 +
                                          [C.c_uint32, C.c_int, C.c_void_p]),
    "bsmr_widen_fp8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p]),
    "bsmr_sddmm_b8": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int,
                                C.c_void_p]),
    "bsmr_spmm_x8": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int,
                               C.c_int, C.c_void_p]),
    "bsmr_sparse_attention_x8": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float] + [C.c_void_p] * 5 +
                                 [C.c_uint32, C.c_int, C.c_int, C.c_void_p]),
    "bsmr_widen_fp8_mx": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p]),
    "bsmr_sddmm_b8_mx": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                   C.c_int, C.c_int, C.c_void_p]),
    "bsmr_spmm_x8_mx": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_uint32, C.c_int, C.c_int, C.c_void_p]),
    "bsmr_sparse_attention_x8_mx": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float] + [C.c_void_p] * 6 +
                                    [C.c_uint32, C.c_int, C.c_int, C.c_void_p]),
    "bsmr_widen_fp4_mx": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "bsmr_sddmm_b4_mx": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                   C.c_int, C.c_void_p]),
    "bsmr_spmm_x4_mx": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_uint32, C.c_int, C.c_void_p]),
    "bsmr_sparse_attention_x4_mx": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float] + [C.c_void_p] * 6 +
                                    [C.c_uint32, C.c_int, C.c_void_p]),
}

HOST_SYMBOLS = {
    "bsmr_csr_from_file": (C.c_void_p, [C.c_char_p]),
    "bsmr_csr_from_arrays": (C.c_void_p, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "bsmr_csr_free": (None, [C.c_void_p]),
    "bsmr_csr_rows": (C.c_uint32, [C.c_void_p]),
    "bsmr_csr_cols": (C.c_uint32, [C.c_void_p]),
    "bsmr_csr_nnz": (C.c_uint32, [C.c_void_p]),
    "bsmr_csr_row_offsets": (u32p, [C.c_void_p]),
    "bsmr_csr_col_indices": (u32p, [C.c_void_p]),
    "bsmr_csr_values": (f32p, [C.c_void_p]),
    "bsmr_csr_check": (C.c_int, [C.c_void_p]),
    "bsmr_csr_write_mtx": (C.c_int, [C.c_void_p, C.c_char_p]),
    "bsmr_make_data": (None, [C.c_void_p, C.c_size_t, C.c_uint32]),
    "bsmr_calculate_block_size": (C.c_uint32, [C.c_void_p, C.c_size_t]),
    "bsmr_pipeline_create": (C.c_void_p, [C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_uint32, C.c_int]),
    "bsmr_pipeline_free": (None, [C.c_void_p]),
    "bsmr_pipeline_resplit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int]),
    "bsmr_pipeline_array": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(u32p), C.POINTER(C.c_size_t)]),
    "bsmr_pipeline_num_row_panels": (C.c_int, [C.c_void_p]),
    "bsmr_pipeline_num_clusters": (C.c_int, [C.c_void_p]),
    "bsmr_pipeline_row_reordering_ms": (C.c_float, [C.c_void_p]),
    "bsmr_pipeline_col_reordering_ms": (C.c_float, [C.c_void_p]),
    "bsmr_pipeline_rphm_ms": (C.c_float, [C.c_void_p]),
    "bsmr_pipeline_check": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float]),
    "bsmr_pipeline_evaluate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]),
    "bsmr_pipeline_plan": (C.c_void_p, [C.c_void_p]),
    "bsmr_pipeline_plan_status": (C.c_int, [C.c_void_p]),
    "bsmr_host_sddmm_cpu": (None, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsmr_host_check_data": (C.c_size_t, [C.c_size_t, C.c_void_p, C.c_void_p]),
    "bsmr_host_sddmm": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]),
    "bsmr_host_sddmm_sharded": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_int, C.c_int,
                                          C.POINTER(C.c_int), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(C.c_float)]),
    "bsmr_host_sddmm_sharded_timed": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_int, C.c_int,
                                                C.POINTER(C.c_int), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(C.c_float)]),
    "bsmr_partition_rows_by_cost": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
}


def _load(name: str, symbols: dict):
    path = LIB_DIR / name
    if not path.exists():
        raise RuntimeError(
            f"{path} is missing: build it with `make -C {PKG_DIR}` (or __graft_entry__.build()). "
            "The engine has no CPU fallback.")
    lib = C.CDLL(str(path), mode=C.RTLD_GLOBAL)
    for sym, (res, args) in symbols.items():
        fn = getattr(lib, sym)  # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    return lib


_hip = None
_host = None


def hip():
    global _hip
    if _hip is None:
        _hip = _load("libbsmr_hip.so", HIP_SYMBOLS)
    return _hip


def host():
    global _host
    if _host is None:
        hip()
        _host = _load("libbsmr_host.so", HOST_SYMBOLS)
    return _host


class BsmrError(RuntimeError):
    def __init__(self, status: int, where: str):
        self.status = status
        msg = hip().bsmr_strerror(status).decode()
        detail = hip().bsmr_last_hip_error().decode()
        super().__init__(f"{where}: {msg}" + (f" ({detail})" if detail else ""))


def _check(status: int, where: str):
    if status != OK:
        raise BsmrError(status, where)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def device_count() -> int:
    n = C.c_int(0)
    _check(hip().bsmr_device_count(C.byref(n)), "bsmr_device_count")
    return n.value


def make_data(count: int, seed: int) -> np.ndarray:
    """U[0,2) operands, bit-identical to Matrix<float>::makeDataSeeded(seed)."""
    out = np.empty(count, dtype=np.float32)
    host().bsmr_make_data(_ptr(out), count, seed)
    return out


class CSR:
    """sparseMatrix::CSR<float> (pattern owner)."""

    def __init__(self, handle):
        if not handle:
            raise ValueError("CSR construction failed (the loader returned false)")
        self._h = C.c_void_p(handle)

    @classmethod
    def from_file(cls, path) -> "CSR":
        return cls(host().bsmr_csr_from_file(str(path).encode()))

    @classmethod
    def from_arrays(cls, rows, cols, row_offsets, col_indices) -> "CSR":
        ro = np.ascontiguousarray(row_offsets, dtype=np.uint32)
        ci = np.ascontiguousarray(col_indices, dtype=np.uint32)
        assert ro.size == rows + 1
        return cls(host().bsmr_csr_from_arrays(rows, cols, int(ci.size), _ptr(ro), _ptr(ci)))

    def __del__(self):
        if getattr(self, "_h", None) and _host is not None:
            _host.bsmr_csr_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    rows = property(lambda s: host().bsmr_csr_rows(s._h))
    cols = property(lambda s: host().bsmr_csr_cols(s._h))
    nnz = property(lambda s: host().bsmr_csr_nnz(s._h))

    @property
    def row_offsets(self) -> np.ndarray:
        return np.ctypeslib.as_array(host().bsmr_csr_row_offsets(self._h), (self.rows + 1,)).copy()

    @property
    def col_indices(self) -> np.ndarray:
        if self.nnz == 0:
            return np.zeros(0, dtype=np.uint32)
        return np.ctypeslib.as_array(host().bsmr_csr_col_indices(self._h), (self.nnz,)).copy()

    @property
    def values(self) -> np.ndarray:
        if self.nnz == 0:
            return np.zeros(0, dtype=np.float32)
        return np.ctypeslib.as_array(host().bsmr_csr_values(self._h), (self.nnz,)).copy()

    def check(self) -> bool:
        return bool(host().bsmr_csr_check(self._h))

    def write_mtx(self, path) -> bool:
        return bool(host().bsmr_csr_write_mtx(self._h, str(path).encode()))

    def calculate_block_size(self, free_device_bytes: int) -> int:
        return host().bsmr_calculate_block_size(self._h, free_device_bytes)


class Pipeline:
    """BSMR(alpha, delta, S) + RPHM(S, bsmr).  device=-1 keeps everything on the host."""

    def __init__(self, csr: CSR, alpha=0.3, delta=0.3, row_mode=ROWS_CLUSTER, block_size=0, device=-1):
        self.csr = csr
        self.delta = delta
        h = host().bsmr_pipeline_create(csr.handle, alpha, delta, row_mode, block_size, device)
        if not h:
            raise RuntimeError("bsmr_pipeline_create failed")
        self._h = C.c_void_p(h)
        if device >= 0:
            _check(host().bsmr_pipeline_plan_status(self._h), "bsmr_plan_create")

    def __del__(self):
        if getattr(self, "_h", None) and _host is not None:
            _host.bsmr_pipeline_free(self._h)
            self._h = None

    def resplit(self, delta: float, device=-1):
        _check(host().bsmr_pipeline_resplit(self._h, self.csr.handle, delta, device), "resplit")
        self.delta = delta

    def array(self, name: str) -> np.ndarray:
        data = u32p()
        n = C.c_size_t(0)
        _check(host().bsmr_pipeline_array(self._h, ARRAY_IDS[name], C.byref(data), C.byref(n)), name)
        if n.value == 0:
            return np.zeros(0, dtype=np.uint32)
        return np.ctypeslib.as_array(data, (n.value,)).copy()

    def arrays(self) -> dict:
        return {k: self.array(k) for k in ARRAY_IDS}

    num_row_panels = property(lambda s: host().bsmr_pipeline_num_row_panels(s._h))
    num_clusters = property(lambda s: host().bsmr_pipeline_num_clusters(s._h))
    row_reordering_ms = property(lambda s: host().bsmr_pipeline_row_reordering_ms(s._h))
    col_reordering_ms = property(lambda s: host().bsmr_pipeline_col_reordering_ms(s._h))
    rphm_ms = property(lambda s: host().bsmr_pipeline_rphm_ms(s._h))

    def check(self) -> bool:
        return bool(host().bsmr_pipeline_check(self._h, self.csr.handle, self.delta))

    def evaluate(self) -> dict:
        """evaluationReordering: the statistics the reference logs for this (alpha, delta)."""
        rep = ReorderingReport()
        _check(host().bsmr_pipeline_evaluate(self._h, self.csr.handle, self.delta, C.byref(rep)),
               "bsmr_pipeline_evaluate")
        return {name: getattr(rep, name) for name, _ in ReorderingReport._fields_}

    @property
    def plan(self):
        p = host().bsmr_pipeline_plan(self._h)
        if not p:
            raise RuntimeError("this pipeline has no device plan (built with device=-1?)")
        return C.c_void_p(p)

    def plan_stats(self) -> dict:
        s = PlanStats()
        _check(hip().bsmr_plan_get_stats(self.plan, C.byref(s)), "bsmr_plan_get_stats")
        return {k: getattr(s, k) for k, _ in PlanStats._fields_}

    def plan_build_ms(self) -> dict:
        """Host wall time of bsmr_plan_create for this pipeline's plan (rules, packing, upload, second format, total)."""
        t = PlanBuildMs()
        _check(hip().bsmr_plan_build_times(self.plan, C.byref(t)), "bsmr_plan_build_times")
        return {k: round(getattr(t, k), 3) for k, _ in PlanBuildMs._fields_}

    def dense_flags(self) -> np.ndarray:
        """uint8 per stored entry (CSR order): 1 = computed by the dense (MFMA) path of the plan, 0 = residue."""
        flags = np.zeros(self.csr.nnz, dtype=np.uint8)
        _check(hip().bsmr_plan_dense_flags(self.plan, flags.ctypes.data_as(C.c_void_p)), "dense_flags")
        return flags

    def sparse_choice(self, K: int, mode=COMPUTE_F16) -> dict:
        lanes, lowp = C.c_uint32(0), C.c_uint32(0)
        _check(hip().bsmr_plan_sparse_choice(self.plan, K, mode, C.byref(lanes), C.byref(lowp)), "sparse_choice")
        return {"lanes_per_entry": lanes.value, "low_precision": bool(lowp.value)}

    def dense_choice(self, K: int) -> dict:
        """Dense format used by a call with inner dimension K."""
        g, t, u = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        _check(hip().bsmr_plan_dense_choice(self.plan, K, C.byref(g), C.byref(t), C.byref(u)), "dense_choice")
        return {"group_size": g.value, "tiles": t.value, "union_columns": u.value}


def cluster_rows_device(rows, cols, row_offsets, col_indices, bin_width, alpha, device=0):
    """bsmr_cluster_rows: (status, reorderedRows, numClusters, stats) - the row clustering on the GPU"""
    ro = np.ascontiguousarray(row_offsets, dtype=np.uint32)
    ci = np.ascontiguousarray(col_indices, dtype=np.uint32)
    out = np.zeros(max(rows, 1), dtype=np.uint32)
    n, clusters, stats = C.c_uint32(0), C.c_int32(0), ClusterStats()
    st = hip().bsmr_cluster_rows(device, rows, cols, _ptr(ro), _ptr(ci), bin_width, alpha, _ptr(out),
                                 C.byref(n), C.byref(clusters), C.byref(stats))
    return st, out[:n.value].copy(), clusters.value, {k: getattr(stats, k) for k, _ in ClusterStats._fields_}


def sddmm_cpu(csr: CSR, K: int, A: np.ndarray, B: np.ndarray) -> np.ndarray:
    """The engine's own OpenMP sddmm_cpu (host.cpp)."""
    A = np.ascontiguousarray(A, dtype=np.float32)
    B = np.ascontiguousarray(B, dtype=np.float32)
    P = np.empty(csr.nnz, dtype=np.float32)
    host().bsmr_host_sddmm_cpu(csr.handle, K, _ptr(A), _ptr(B), _ptr(P))
    return P


def check_data(x: np.ndarray, y: np.ndarray) -> int:
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    assert x.size == y.size
    return int(host().bsmr_host_check_data(x.size, _ptr(x), _ptr(y)))


def sddmm_operator(csr: CSR, K: int, A, B, alpha=0.3, delta=0.3, mode=COMPUTE_F16, iters=1):
    """sddmm(options, A, B, P, logger) on host operands -> (P, log text)."""
    A = np.ascontiguousarray(A, dtype=np.float32)
    B = np.ascontiguousarray(B, dtype=np.float32)
    P = np.empty(csr.nnz, dtype=np.float32)
    log = C.create_string_buffer(8192)
    _check(host().bsmr_host_sddmm(csr.handle, K, alpha, delta, mode, iters, _ptr(A), _ptr(B), _ptr(P),
                                  log, len(log)), "bsmr_host_sddmm")
    return P, log.value.decode()


def col_reorder_device(rows, cols, row_offsets, col_indices, reordered_rows, delta, device=0):
    """bsmr_col_reorder: (status, dict of the ten arrays named as in ARRAY_IDS, device ms)"""
    ro = np.ascontiguousarray(row_offsets, dtype=np.uint32)
    ci = np.ascontiguousarray(col_indices, dtype=np.uint32)
    rr = np.ascontiguousarray(reordered_rows, dtype=np.uint32)
    h = C.c_void_p()
    st = hip().bsmr_col_reorder(C.byref(h), device, rows, cols, _ptr(ro), _ptr(ci), _ptr(rr), rr.size, delta)
    if st != OK:
        return st, None, 0.0
    sz = ColReorderSizes()
    hip().bsmr_col_reorder_sizes(h, C.byref(sz))
    P1 = sz.num_row_panels + 1
    out = {"denseCols": np.zeros(sz.num_dense_cols, np.uint32), "denseColOffsets": np.zeros(P1, np.uint32),
           "sparseCols": np.zeros(sz.num_sparse_cols, np.uint32), "sparseColOffsets": np.zeros(P1, np.uint32),
           "sparseValueOffsets": np.zeros(P1, np.uint32), "blockOffsets": np.zeros(P1, np.uint32),
           "blockValues": np.zeros(sz.num_blocks * 256, np.uint32), "sparseValues": np.zeros(sz.num_sparse_entries, np.uint32),
           "sparseRelativeRows": np.zeros(sz.num_sparse_entries, np.uint32),
           "sparseColIndices": np.zeros(sz.num_sparse_entries, np.uint32)}
    order = ("denseCols", "denseColOffsets", "sparseCols", "sparseColOffsets", "sparseValueOffsets", "blockOffsets",
             "blockValues", "sparseValues", "sparseRelativeRows", "sparseColIndices")
    st = hip().bsmr_col_reorder_fetch(h, *[_ptr(out[k]) for k in order])
    hip().bsmr_col_reorder_free(h)
    return st, out, sz.elapsed_ms


def partition_rows_by_cost(csr: CSR, world: int) -> list:
    """partitionRowsByCost: world + 1 row boundaries of the C++ operator's cut"""
    b = (C.c_uint32 * (world + 1))()
    _check(host().bsmr_partition_rows_by_cost(csr.handle, world, b), "bsmr_partition_rows_by_cost")
    return [int(x) for x in b]


def sddmm_operator_sharded_timed(csr: CSR, K: int, A, B, devices, alpha=0.3, delta=0.3, mode=COMPUTE_F16, iters=1):
    """sddmm_multi_gpu on host operands -> (P, {step_ms (pipelined), compute_ms, gather_ms (one step taken apart)})"""
    A = np.ascontiguousarray(A, dtype=np.float32)
    B = np.ascontiguousarray(B, dtype=np.float32)
    P = np.empty(csr.nnz, dtype=np.float32)
    devs = (C.c_int * len(devices))(*devices)
    t = (C.c_float * 3)()
    _check(host().bsmr_host_sddmm_sharded_timed(csr.handle, K, alpha, delta, mode, iters, devs, len(devices), _ptr(A), _ptr(B),
                                                _ptr(P), t), "bsmr_host_sddmm_sharded_timed")
    return P, {"step_ms": t[0], "compute_ms": t[1], "gather_ms": t[2]}


def sddmm_operator_sharded(csr: CSR, K: int, A, B, devices, alpha=0.3, delta=0.3, mode=COMPUTE_F16, iters=1):
    """sddmm_multi_gpu on host operands -> (P, device ms per step)"""
    A = np.ascontiguousarray(A, dtype=np.float32)
    B = np.ascontiguousarray(B, dtype=np.float32)
    P = np.empty(csr.nnz, dtype=np.float32)
    devs = (C.c_int * len(devices))(*devices)
    ms = C.c_float(0)
    _check(host().bsmr_host_sddmm_sharded(csr.handle, K, alpha, delta, mode, iters, devs, len(devices), _ptr(A), _ptr(B),
                                          _ptr(P), C.byref(ms)), "bsmr_host_sddmm_sharded")
    return P, ms.value


# --- device entry points (pointers are integers, e.g. torch.Tensor.data_ptr()) ---
def sddmm(plan, K: int, A_ptr: int, B_ptr: int, P_ptr: int, mode=COMPUTE_F16, stream: int = 0):
    _check(hip().bsmr_sddmm(plan, K, A_ptr, B_ptr, P_ptr, mode, stream), "bsmr_sddmm")


def plan_tune(plan, K: int, A_ptr: int, B_ptr: int, P_ptr: int, mode=COMPUTE_F16, stream: int = 0) -> dict:
    """bsmr_plan_tune: time the dense engines for calls with this (K, mode) on these operands and keep the fastest
    (the plan must have been created with dense_engine = ENGINE_TUNED).  P holds the result afterwards."""
    r = TuneReport()
    _check(hip().bsmr_plan_tune(plan, K, A_ptr, B_ptr, P_ptr, mode, stream, C.byref(r)), "bsmr_plan_tune")
    out = {"chosen": ENGINE_NAMES[r.chosen_engine], "group": r.chosen_group, "blocks_per_item": r.chosen_blocks_per_item}
    for name in ("stream_us", "grouped_us", "tiles_us", "shared_us", "fp32_residue_us", "b_only_us", "one_stream_us", "two_streams_us", "convert_pass_us", "fp32_dense_us", "sweep_us", "lowp_call_us", "sweep_fp32_call_us", "gemm_us", "gemm_fp32_call_us"):
        out[name] = round(getattr(r, name), 2)
    out["b_only"], out["overlap"], out["cvt_in_kernel"] = r.chosen_b_only, r.chosen_overlap, r.chosen_cvt_in_kernel
    out["sweep_fp32"] = r.chosen_sweep_fp32
    out["gemm_fp32"] = r.chosen_gemm_fp32
    out["variant"] = VARIANT_NAMES[r.chosen_variant]
    out["variant_us"] = {VARIANT_NAMES[i]: round(r.variant_us[i], 2) for i in range(6) if r.variant_us[i] >= 0}
    return out


def plan_get_tuned(plan, K: int, mode=COMPUTE_F16) -> dict:
    """bsmr_plan_get_tuned: the choice bsmr_plan_tune kept for (K, mode), as a plain dict (JSON-able)"""
    c = TunedChoice()
    _check(hip().bsmr_plan_get_tuned(plan, K, mode, C.byref(c)), "bsmr_plan_get_tuned")
    return {n: getattr(c, n) for n, _ in TunedChoice._fields_ if n != "struct_size"}


def plan_set_tuned(plan, K: int, choice: dict, mode=COMPUTE_F16):
    """bsmr_plan_set_tuned: install a choice measured earlier (plan_get_tuned of another process) without timing anything"""
    c = TunedChoice()
    c.struct_size = C.sizeof(TunedChoice)
    for n, _ in TunedChoice._fields_:
        if n != "struct_size":
            setattr(c, n, int(choice[n]))
    _check(hip().bsmr_plan_set_tuned(plan, K, mode, C.byref(c)), "bsmr_plan_set_tuned")


def sddmm_batch(plan, K: int, A_ptr: int, B_ptr: int, P_ptr: int, num_batches: int, mode=COMPUTE_F16, stream: int = 0):
    _check(hip().bsmr_sddmm_batch(plan, K, A_ptr, B_ptr, P_ptr, num_batches, mode, stream), "bsmr_sddmm_batch")


def batched_transpose(width: int, height: int, num_batches: int, in_ptr: int, out_ptr: int, stream: int = 0):
    _check(hip().bsmr_batched_transpose(width, height, num_batches, in_ptr, out_ptr, stream), "bsmr_batched_transpose")


def sddmm_timed(plan, K, A_ptr, B_ptr, P_ptr, mode=COMPUTE_F16, stream=0, warmup=2, iters=20) -> dict:
    t = Timing()
    _check(hip().bsmr_sddmm_timed(plan, K, A_ptr, B_ptr, P_ptr, mode, stream, warmup, iters, C.byref(t)),
           "bsmr_sddmm_timed")
    return {k: getattr(t, k) for k, _ in Timing._fields_}


def convert_operands(plan, K, A_ptr, B_ptr, A16_ptr, B16_ptr, mode=COMPUTE_F16, stream=0):
    _check(hip().bsmr_convert_operands(plan, K, A_ptr, B_ptr, A16_ptr, B16_ptr, mode, stream),
           "bsmr_convert_operands")


def sddmm_lowp(plan, K, A16_ptr, B16_ptr, A_ptr, B_ptr, P_ptr, mode=COMPUTE_F16, stream=0):
    _check(hip().bsmr_sddmm_lowp(plan, K, A16_ptr, B16_ptr, A_ptr, B_ptr, P_ptr, mode, stream),
           "bsmr_sddmm_lowp")


def sddmm_host(plan, K, A: np.ndarray, B: np.ndarray, nnz: int, mode=COMPUTE_F16, iters=1):
    A = np.ascontiguousarray(A, dtype=np.float32)
    B = np.ascontiguousarray(B, dtype=np.float32)
    P = np.empty(nnz, dtype=np.float32)
    ms = C.c_float(0)
    _check(hip().bsmr_sddmm_host(plan, K, _ptr(A), _ptr(B), _ptr(P), mode, iters, C.byref(ms)),
           "bsmr_sddmm_host")
    return P, ms.value


def plan_options(**changes) -> PlanOptions:
    """bsmr_plan_options_default with fields changed by keyword"""
    o = PlanOptions()
    _check(hip().bsmr_plan_options_default(C.byref(o)), "bsmr_plan_options_default")
    for k, v in changes.items():
        if k not in dict(PlanOptions._fields_):
            raise KeyError(k)
        setattr(o, k, v)
    return o


def rphm_desc(M, N, nnz, arrays: dict):
    """bsmr_rphm_desc over RPHM-layout numpy arrays: (desc, the contiguous arrays it points into - keep them alive)"""
    keep = {k: np.ascontiguousarray(arrays[k], dtype=np.uint32) for k in
            ("reorderedRows", "denseCols", "blockOffsets", "blockValues", "sparseValueOffsets",
             "sparseValues", "sparseRelativeRows", "sparseColIndices")}
    d = RphmDesc()
    d.M, d.N, d.nnz = M, N, nnz
    d.num_nonzero_rows = keep["reorderedRows"].size
    d.num_row_panels = keep["blockOffsets"].size - 1
    cast = lambda a: a.ctypes.data_as(u32p)
    d.reordered_rows = cast(keep["reorderedRows"])
    d.dense_cols = cast(keep["denseCols"])
    d.block_offsets = cast(keep["blockOffsets"])
    d.block_values = cast(keep["blockValues"])
    d.sparse_value_offsets = cast(keep["sparseValueOffsets"])
    d.sparse_values = cast(keep["sparseValues"])
    d.sparse_relative_rows = cast(keep["sparseRelativeRows"])
    d.sparse_col_indices = cast(keep["sparseColIndices"])
    return d, keep


def plan_from_arrays(M, N, nnz, arrays: dict, device=0, options: PlanOptions = None):
    """bsmr_plan_create straight from RPHM-layout numpy arrays (what a reference
    maintainer would pass from RPHM's host vectors).  Returns the plan handle.
    options: a PlanOptions -> bsmr_plan_create_ex (the environment is then not consulted)."""
    d, keep = rphm_desc(M, N, nnz, arrays)
    out = C.c_void_p()
    if options is not None:
        st = hip().bsmr_plan_create_ex(C.byref(out), device, C.byref(d), C.byref(options))
    else:
        st = hip().bsmr_plan_create(C.byref(out), device, C.byref(d))
    return st, out


def plan_destroy(plan):
    hip().bsmr_plan_destroy(plan)


# --- SDDMM backward (bsmr_backward_*, bsmr_spmm, bsmr_sddmm_backward; pointers are integers) ---
def csr_transpose(rows, cols, row_offsets, col_indices):
    """bsmr_csr_transpose (host only): (col_offsets, csc_rows, csc_to_csr)"""
    ro = np.ascontiguousarray(row_offsets, dtype=np.uint32)
    ci = np.ascontiguousarray(col_indices, dtype=np.uint32)
    co = np.zeros(cols + 1, dtype=np.uint32)
    rws = np.zeros(max(ci.size, 1), dtype=np.uint32)
    e = np.zeros(max(ci.size, 1), dtype=np.uint32)
    _check(hip().bsmr_csr_transpose(rows, cols, ci.size, _ptr(ro), _ptr(ci), _ptr(co), _ptr(rws), _ptr(e)),
           "bsmr_csr_transpose")
    return co, rws[:ci.size], e[:ci.size]


def backward_create_status(rows, cols, row_offsets, col_indices, row_order=None, device=0):
    """bsmr_backward_create: (status, handle); row_order None = natural order"""
    ro = np.ascontiguousarray(row_offsets, dtype=np.uint32)
    ci = np.ascontiguousarray(col_indices, dtype=np.uint32)
    order = None if row_order is None else np.ascontiguousarray(row_order, dtype=np.uint32)
    out = C.c_void_p()
    st = hip().bsmr_backward_create(C.byref(out), device, rows, cols, ci.size, _ptr(ro), _ptr(ci) if ci.size else None,
                                    _ptr(order) if order is not None and order.size else None,
                                    0 if order is None else order.size)
    return st, out


def backward_create(rows, cols, row_offsets, col_indices, row_order=None, device=0):
    st, h = backward_create_status(rows, cols, row_offsets, col_indices, row_order, device)
    _check(st, "bsmr_backward_create")
    return h


def backward_destroy(bw):
    hip().bsmr_backward_destroy(bw)


def backward_reserve(bw, K: int, num_batches: int = 1, mode=COMPUTE_F32):
    """workspace for calls with (K, num_batches, mode); mode F16 / BF16 adds room for the 16-bit copies"""
    if mode == COMPUTE_F32:
        _check(hip().bsmr_backward_reserve(bw, K, num_batches), "bsmr_backward_reserve")
    else:
        _check(hip().bsmr_backward_reserve_mode(bw, K, num_batches, mode), "bsmr_backward_reserve_mode")


def backward_stats(bw) -> dict:
    s = BackwardStats()
    _check(hip().bsmr_backward_get_stats(bw, C.byref(s), C.sizeof(s)), "bsmr_backward_get_stats")
    return {k: getattr(s, k) for k, _ in BackwardStats._fields_}


def spmm(bw, K: int, transpose: bool, v_ptr: int, X_ptr: int, Y_ptr: int, num_batches: int = 1, stream: int = 0,
         mode=COMPUTE_F32):
    """Y = S_v X (transpose False) or S_v^T X (True); mode F16 / BF16: X is rounded and gathered as 16-bit rows"""
    if mode == COMPUTE_F32:
        _check(hip().bsmr_spmm(bw, K, int(bool(transpose)), v_ptr, X_ptr, Y_ptr, num_batches, stream), "bsmr_spmm")
    else:
        _check(hip().bsmr_spmm_mode(bw, K, int(bool(transpose)), v_ptr, X_ptr, Y_ptr, num_batches, mode, stream),
               "bsmr_spmm_mode")


def spmm_lowp(bw, K: int, transpose: bool, v_ptr: int, X16_ptr: int, Y_ptr: int, num_batches: int = 1, stream: int = 0,
              mode=COMPUTE_F16):
    """spmm on rows the caller holds as fp16 (mode F16) or bf16 (BF16), e.g. an output of convert_operands"""
    _check(hip().bsmr_spmm_lowp(bw, K, int(bool(transpose)), v_ptr, X16_ptr, Y_ptr, num_batches, mode, stream),
           "bsmr_spmm_lowp")


def sddmm_backward(bw, K: int, dP_ptr: int, A_ptr: int, B_ptr: int, dA_ptr, dB_ptr, num_batches: int = 1, stream: int = 0,
                   mode=COMPUTE_F32):
    """dA = S_dP B, dB = S_dP^T A; dA_ptr / dB_ptr None (or 0) skips that product; mode F16 / BF16: B (for dA) and A
    (for dB) are rounded and gathered as 16-bit rows"""
    if mode == COMPUTE_F32:
        _check(hip().bsmr_sddmm_backward(bw, K, dP_ptr, A_ptr, B_ptr, dA_ptr or None, dB_ptr or None, num_batches, stream),
               "bsmr_sddmm_backward")
    else:
        _check(hip().bsmr_sddmm_backward_mode(bw, K, dP_ptr, A_ptr, B_ptr, dA_ptr or None, dB_ptr or None, num_batches,
                                              mode, stream), "bsmr_sddmm_backward_mode")


# --- fp16 / bf16 tensors end to end: 16-bit operands in, 16-bit Y / dA / dB out; P, v and dP stay fp32 ---
def sddmm_16(plan, K: int, A16_ptr: int, B16_ptr: int, P_ptr: int, num_batches: int = 1, mode=COMPUTE_F16, stream: int = 0):
    """the forward on fp16 (mode F16) or bf16 (BF16) operands alone: no fp32 operand, no conversion pass"""
    _check(hip().bsmr_sddmm_16(plan, K, A16_ptr or None, B16_ptr or None, P_ptr or None, num_batches, mode, stream),
           "bsmr_sddmm_16")


def spmm_16(bw, K: int, transpose: bool, v_ptr: int, X16_ptr: int, Y16_ptr: int, num_batches: int = 1, stream: int = 0,
            mode=COMPUTE_F16):
    """Y16 = round(S_v widen(X16)) (transpose True: S_v^T): 16-bit rows gathered, fp32 sums, one rounding per element"""
    _check(hip().bsmr_spmm_16(bw, K, int(bool(transpose)), v_ptr or None, X16_ptr or None, Y16_ptr, num_batches, mode,
                              stream), "bsmr_spmm_16")


def sddmm_backward_16(bw, K: int, dP_ptr: int, A16_ptr: int, B16_ptr: int, dA16_ptr, dB16_ptr, num_batches: int = 1,
                      stream: int = 0, mode=COMPUTE_F16):
    """dA16 = round(S_dP widen(B16)), dB16 = round(S_dP^T widen(A16)); dA16_ptr / dB16_ptr None (or 0) skips that product"""
    _check(hip().bsmr_sddmm_backward_16(bw, K, dP_ptr or None, A16_ptr or None, B16_ptr or None, dA16_ptr or None,
                                        dB16_ptr or None, num_batches, mode, stream), "bsmr_sddmm_backward_16")


# --- blocked SpMM: Y = S_v X over the RPHM's dense blocks (fp32 MFMA) + the gather over the residue ---
def blocked_check_status(rows, cols, row_offsets, col_indices, arrays: dict, segment_blocks: int = 0):
    """bsmr_blocked_check_split (host only; segment_blocks = 0 is bsmr_blocked_check): (status, statistics as a dict) of
    RPHM-layout arrays against a CSR"""
    ro = np.ascontiguousarray(row_offsets, dtype=np.uint32)
    ci = np.ascontiguousarray(col_indices, dtype=np.uint32)
    d, keep = rphm_desc(rows, cols, int(ci.size), arrays)
    s = BlockedStats()
    st = hip().bsmr_blocked_check_split(rows, cols, ci.size, _ptr(ro), _ptr(ci) if ci.size else None, C.byref(d),
                                        segment_blocks, C.byref(s), C.sizeof(s))
    return st, {k: getattr(s, k) for k, _ in BlockedStats._fields_}


def backward_attach_blocks_status(bw, rows, cols, nnz, arrays: dict, segment_blocks: int = 0) -> int:
    d, keep = rphm_desc(rows, cols, nnz, arrays)
    return hip().bsmr_backward_attach_blocks_split(bw, C.byref(d), segment_blocks)


def backward_attach_blocks(bw, rows, cols, nnz, arrays: dict, segment_blocks: int = 0):
    """bsmr_backward_attach_blocks_split: the handle serves spmm_blocked afterwards (arrays: Pipeline.arrays()).
    segment_blocks = S >= 1 cuts every panel's block list into segments of S blocks, each a wave's chain of its own, their
    sums added in order (another summation order for the panels with more than S blocks); 0, the default, is
    bsmr_backward_attach_blocks: no splitting"""
    _check(backward_attach_blocks_status(bw, rows, cols, nnz, arrays, segment_blocks), "bsmr_backward_attach_blocks_split")


def backward_blocked_stats(bw) -> dict:
    s = BlockedStats()
    _check(hip().bsmr_backward_get_blocked_stats(bw, C.byref(s), C.sizeof(s)), "bsmr_backward_get_blocked_stats")
    return {k: getattr(s, k) for k, _ in BlockedStats._fields_}


def spmm_blocked(bw, K: int, v_ptr: int, X_ptr: int, Y_ptr: int, num_batches: int = 1, stream: int = 0, mode=COMPUTE_F32):
    """Y = S_v X on a handle with attached blocks; mode F16 / BF16: X and Y are 16-bit rows of that format
    (bsmr_spmm_blocked_16)"""
    if mode == COMPUTE_F32:
        _check(hip().bsmr_spmm_blocked(bw, K, v_ptr or None, X_ptr or None, Y_ptr or None, num_batches, stream),
               "bsmr_spmm_blocked")
    else:
        _check(hip().bsmr_spmm_blocked_16(bw, K, v_ptr or None, X_ptr or None, Y_ptr or None, num_batches, mode, stream),
               "bsmr_spmm_blocked_16")


def sparse_softmax(bw, scale: float, X_ptr: int, Y_ptr: int, num_batches: int = 1, stream: int = 0):
    """Y = the row softmax of fl32(scale * X) over S's pattern (values in CSR order; Y may be X)"""
    _check(hip().bsmr_sparse_softmax(bw, scale, X_ptr or None, Y_ptr or None, num_batches, stream), "bsmr_sparse_softmax")


def sparse_softmax_backward(bw, scale: float, Y_ptr: int, dY_ptr: int, dX_ptr: int, num_batches: int = 1, stream: int = 0):
    """dX = (Y * (dY - rowsum(Y * dY))) * scale (dX may be dY)"""
    _check(hip().bsmr_sparse_softmax_backward(bw, scale, Y_ptr or None, dY_ptr or None, dX_ptr or None, num_batches,
                                              stream), "bsmr_sparse_softmax_backward")


# --- fused sparse attention: O = softmax_rows(scale P) V in one gather, and its backward ---
def sparse_attention_reserve(bw, Kv: int, num_batches: int = 1):
    """workspace of sparse_attention / _backward (and of the spmm calls) with (Kv, num_batches)"""
    _check(hip().bsmr_sparse_attention_reserve(bw, Kv, num_batches), "bsmr_sparse_attention_reserve")


def sparse_attention(bw, Kv: int, scale: float, P_ptr: int, V_ptr: int, O_ptr: int, m_ptr: int, s_ptr: int,
                     num_batches: int = 1, stream: int = 0, mode=COMPUTE_F32):
    """O = softmax_rows(fl32(scale * P)) V, with the row maxima m and row sums s the backward needs; mode F16 / BF16: V
    and O are 16-bit rows of that format (bsmr_sparse_attention_16)"""
    if mode == COMPUTE_F32:
        _check(hip().bsmr_sparse_attention(bw, Kv, scale, P_ptr or None, V_ptr or None, O_ptr or None, m_ptr or None,
                                           s_ptr or None, num_batches, stream), "bsmr_sparse_attention")
    else:
        _check(hip().bsmr_sparse_attention_16(bw, Kv, scale, P_ptr or None, V_ptr or None, O_ptr or None, m_ptr or None,
                                              s_ptr or None, num_batches, mode, stream), "bsmr_sparse_attention_16")


def sparse_attention_backward(bw, Kv: int, scale: float, P_ptr: int, m_ptr: int, s_ptr: int, dW_ptr: int, O_ptr: int,
                              dO_ptr: int, dP_ptr: int, W_ptr: int, num_batches: int = 1, stream: int = 0,
                              mode=COMPUTE_F32):
    """W = the softmax weights recomputed from (P, m, s); dP = (W * (dW - rowdot(dO, O))) * scale (dP may be dW); mode
    F16 / BF16: O and dO are 16-bit rows of that format (bsmr_sparse_attention_backward_16)"""
    args = (bw, Kv, scale, P_ptr or None, m_ptr or None, s_ptr or None, dW_ptr or None, O_ptr or None, dO_ptr or None,
            dP_ptr or None, W_ptr or None, num_batches)
    if mode == COMPUTE_F32:
        _check(hip().bsmr_sparse_attention_backward(*args, stream), "bsmr_sparse_attention_backward")
    else:
        _check(hip().bsmr_sparse_attention_backward_16(*args, mode, stream), "bsmr_sparse_attention_backward_16")


# --- fp8 keys and values: the column-side operand as OCP fp8 bytes (fmt FP8_E4M3 / FP8_E5M2), widened exactly to the
# 16-bit format of `mode`; each call is bit for bit its 16-bit form on the widened operand ---
def widen_fp8(in8_ptr: int, out16_ptr: int, count: int, mode=COMPUTE_F16, fmt=FP8_E4M3, stream: int = 0):
    """out16[i] = widen(in8[i]) for count elements: fp8 -> fp16 (mode F16) or bf16 (BF16), exact for every code"""
    _check(hip().bsmr_widen_fp8(in8_ptr or None, out16_ptr or None, count, mode, fmt, stream), "bsmr_widen_fp8")


def sddmm_b8(plan, K: int, A16_ptr: int, B8_ptr: int, P_ptr: int, num_batches: int = 1, mode=COMPUTE_F16, fmt=FP8_E4M3,
             stream: int = 0):
    """sddmm_16(A16, widen(B8)): B is widened into the plan's 16-bit workspace, A16 is read in place"""
    _check(hip().bsmr_sddmm_b8(plan, K, A16_ptr or None, B8_ptr or None, P_ptr or None, num_batches, mode, fmt, stream),
           "bsmr_sddmm_b8")


def spmm_x8(bw, K: int, transpose: bool, v_ptr: int, X8_ptr: int, Y16_ptr: int, num_batches: int = 1, stream: int = 0,
            mode=COMPUTE_F16, fmt=FP8_E4M3):
    """Y16 = round(S_v widen(X8)) (transpose True: S_v^T): fp8 rows gathered and widened in registers, no copy"""
    _check(hip().bsmr_spmm_x8(bw, K, int(bool(transpose)), v_ptr or None, X8_ptr or None, Y16_ptr, num_batches, mode, fmt,
                              stream), "bsmr_spmm_x8")


def sparse_attention_x8(bw, Kv: int, scale: float, P_ptr: int, V8_ptr: int, O16_ptr: int, m_ptr: int, s_ptr: int,
                        num_batches: int = 1, stream: int = 0, mode=COMPUTE_F16, fmt=FP8_E4M3):
    """sparse_attention on fp8 rows of V: O16 (mode's format), m and s as bsmr_sparse_attention_16 on widen(V8)"""
    _check(hip().bsmr_sparse_attention_x8(bw, Kv, scale, P_ptr or None, V8_ptr or None, O16_ptr or None, m_ptr or None,
                                          s_ptr or None, num_batches, mode, fmt, stream), "bsmr_sparse_attention_x8")


# --- MX block scales on the fp8 operand (MXFP8): `scales` is [b][rows][K/32] E8M0 bytes, code e = 2^(e-127), 255 NaN;
# dq = widen(code) * scale is one fp32 multiplication in front of everything else (include/bsmr_hip.h "MX block scales") ---
def widen_fp8_mx(in8_ptr: int, scales_ptr: int, out16_ptr: int, count: int, mode=COMPUTE_F16, fmt=FP8_E4M3, stream: int = 0):
    """out16[i] = narrow(widen(in8[i]) * 2^(scales[i / 32] - 127)); count a multiple of 32"""
    _check(hip().bsmr_widen_fp8_mx(in8_ptr or None, scales_ptr or None, out16_ptr or None, count, mode, fmt, stream),
           "bsmr_widen_fp8_mx")


def sddmm_b8_mx(plan, K: int, A16_ptr: int, B8_ptr: int, Bs_ptr: int, P_ptr: int, num_batches: int = 1, mode=COMPUTE_F16,
                fmt=FP8_E4M3, stream: int = 0):
    """sddmm_16(A16, narrow(dq(B8, Bs))): B is dequantised into the plan's 16-bit workspace, A16 is read in place"""
    _check(hip().bsmr_sddmm_b8_mx(plan, K, A16_ptr or None, B8_ptr or None, Bs_ptr or None, P_ptr or None, num_batches,
                                  mode, fmt, stream), "bsmr_sddmm_b8_mx")


def spmm_x8_mx(bw, K: int, transpose: bool, v_ptr: int, X8_ptr: int, Xs_ptr: int, Y16_ptr: int, num_batches: int = 1,
               stream: int = 0, mode=COMPUTE_F16, fmt=FP8_E4M3):
    """Y16 = round(S_v dq(X8, Xs)) (transpose True: S_v^T): the fp32 gather on the dequantised rows, no copy"""
    _check(hip().bsmr_spmm_x8_mx(bw, K, int(bool(transpose)), v_ptr or None, X8_ptr or None, Xs_ptr or None, Y16_ptr,
                                 num_batches, mode, fmt, stream), "bsmr_spmm_x8_mx")


def sparse_attention_x8_mx(bw, Kv: int, scale: float, P_ptr: int, V8_ptr: int, Vs_ptr: int, O16_ptr: int, m_ptr: int,
                           s_ptr: int, num_batches: int = 1, stream: int = 0, mode=COMPUTE_F16, fmt=FP8_E4M3):
    """sparse_attention on dq(V8, Vs): O16 rounded once (mode's format), m and s those of the fp32 call"""
    _check(hip().bsmr_sparse_attention_x8_mx(bw, Kv, scale, P_ptr or None, V8_ptr or None, Vs_ptr or None, O16_ptr or None,
                                             m_ptr or None, s_ptr or None, num_batches, mode, fmt, stream),
           "bsmr_sparse_attention_x8_mx")


# --- MXFP4 keys and values: the column-side operand as OCP e2m1 codes, two per byte (element 2i the low nibble of byte
# i), under E8M0 block scales [b][rows][K/32]; dq = widen(code) * 2^(scale-127) is one exact fp32 multiplication in front
# of everything else (include/bsmr_hip.h "MXFP4 keys and values").  The scales are mandatory ---
def widen_fp4_mx(in4_ptr: int, scales_ptr: int, out16_ptr: int, count: int, mode=COMPUTE_F16, stream: int = 0):
    """out16[i] = narrow(widen(code i) * 2^(scales[i / 32] - 127)); count elements (count / 2 bytes), a multiple of 32"""
    _check(hip().bsmr_widen_fp4_mx(in4_ptr or None, scales_ptr or None, out16_ptr or None, count, mode, stream),
           "bsmr_widen_fp4_mx")


def sddmm_b4_mx(plan, K: int, A16_ptr: int, B4_ptr: int, Bs_ptr: int, P_ptr: int, num_batches: int = 1, mode=COMPUTE_F16,
                stream: int = 0):
    """sddmm_16(A16, narrow(dq(B4, Bs))): B is dequantised into the plan's 16-bit workspace, A16 is read in place"""
    _check(hip().bsmr_sddmm_b4_mx(plan, K, A16_ptr or None, B4_ptr or None, Bs_ptr or None, P_ptr or None, num_batches,
                                  mode, stream), "bsmr_sddmm_b4_mx")


def spmm_x4_mx(bw, K: int, transpose: bool, v_ptr: int, X4_ptr: int, Xs_ptr: int, Y16_ptr: int, num_batches: int = 1,
               stream: int = 0, mode=COMPUTE_F16):
    """Y16 = round(S_v dq(X4, Xs)) (transpose True: S_v^T): the fp32 gather on the dequantised rows, no copy"""
    _check(hip().bsmr_spmm_x4_mx(bw, K, int(bool(transpose)), v_ptr or None, X4_ptr or None, Xs_ptr or None, Y16_ptr,
                                 num_batches, mode, stream), "bsmr_spmm_x4_mx")


def sparse_attention_x4_mx(bw, Kv: int, scale: float, P_ptr: int, V4_ptr: int, Vs_ptr: int, O16_ptr: int, m_ptr: int,
                           s_ptr: int, num_batches: int = 1, stream: int = 0, mode=COMPUTE_F16):
    """sparse_attention on dq(V4, Vs): O16 rounded once (mode's format), m and s those of the fp32 call"""
    _check(hip().bsmr_sparse_attention_x4_mx(bw, Kv, scale, P_ptr or None, V4_ptr or None, Vs_ptr or None, O16_ptr or None,
                                             m_ptr or None, s_ptr or None, num_batches, mode, stream),
           "bsmr_sparse_attention_x4_mx")
