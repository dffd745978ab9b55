"""ctypes binding of libgespmm.so (the C ABI declared in include/gespmm.h).

This is the reference-side binding a maintainer would write (INTEGRATION.md shows
the same stub). It never falls back to a CPU implementation: a missing library is
an ImportError, a failing call is a RuntimeError carrying gespmm_error_string().
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgespmm.so")

VARIANT_AUTO = -1
VARIANT_NAIVE = 0
VARIANT_CRC = 1
VARIANT_CRC_CWM2 = 2
VARIANT_CRC_CWM4 = 3
VARIANT_CRC_CWM8 = 4
VARIANT_PARREDUCE = 5
NUM_VARIANTS = 6

FLAG_NO_XCD_REMAP = 0x1
FLAG_NT_STORE = 0x2
FLAG_SC1_STORE = 0x8000
FLAG_FORCE_IDX64 = 0x4
FLAG_BATCH_STREAM = 0x20
FLAG_SEG_STREAM = 0x80
FLAG_STRICT_ORDER = 0x100
FLAG_SPLIT_LONG_ROWS = 0x200
FLAG_SLAB_BLOCKED = 0x400
FLAG_NO_SLAB_BLOCKED = 0x800
FLAG_ALLOW_REASSOCIATION = 0x1000
FLAG_REUSE_SPLIT = 0x2000
FLAG_SHALLOW_UNROLL = 0x10

# Every symbol include/gespmm.h declares; tests check the library exports all of them.
EXPORTS = [
    "gespmm_version",
    "gespmm_error_string",
    "gespmm_csr_spmm_f32",
    "gespmm_csr_spmm_max_f32",
    "gespmm_select_variant",
    "gespmm_describe_launch",
    "gespmm_dgl_csrmm_sum_f32",
    "gespmm_dgl_csrmm_max_f32",
    "gespmm_dgl_set_readback_rows",
    "gespmm_csr_spmm_f32_cfg",
    "gespmm_csr_spmm_workspace_bytes",
    "gespmm_csr_spmm_f32_ws",
    "gespmm_sddmm_coo_f32",
    "gespmm_sddmm_csr_f32",
    "gespmm_csr2csc_workspace_bytes",
    "gespmm_csr2csc_f32",
    "gespmm_mtx_read",
    "gespmm_mtx_read_cached",
    "gespmm_mtx_free",
    "gespmm_coo_to_csr",
    "gespmm_row_partition",
    "gespmm_baseline_atomic_scatter_f32",
    "gespmm_baseline_copy_f32",
    "gespmm_plan_create",
    "gespmm_plan_spmm_f32",
    "gespmm_plan_spmm_max_f32",
    "gespmm_plan_sddmm_f32",
    "gespmm_plan_set_values",
    "gespmm_plan_get_order",
    "gespmm_plan_describe",
    "gespmm_plan_destroy",
    "gespmm_cluster_rows",
    "gespmm_simulate_l2_hits",
    "gespmm_plan_create_v2",
    "gespmm_plan_policy",
    "gespmm_plan_policy_v2",
    "gespmm_plan_tune",
    "gespmm_set_cached_memory_limit",
    "gespmm_device_cluster_rows",
    "gespmm_device_l2_model",
    "gespmm_plan_debug_tasks",
    "gespmm_plan_debug_staging",
    "gespmm_release_cached_memory",
    "gespmm_init",
    "gespmm_set_auto_plan",
    "gespmm_auto_plan_clear",
    "gespmm_auto_plan_get_stats",
    "gespmm_cluster_rows_study",
    "gespmm_plan_wants_warmup",
    "gespmm_csr_spmm_fused_f32",
    "gespmm_plan_spmm_fused_f32",
    "gespmm_plan_fused_route",
    "gespmm_describe_sddmm",
    "gespmm_plan_sddmm_route",
    "gespmm_csr_spmm_x16",
    "gespmm_plan_spmm_x16",
    "gespmm_x16_route",
    "gespmm_plan_x16_route",
    "gespmm_sddmm_coo_x16",
    "gespmm_sddmm_csr_x16",
    "gespmm_plan_sddmm_x16",
    "gespmm_describe_sddmm_x16",
    "gespmm_csr_spmm_heads_f32",
    "gespmm_plan_spmm_heads_f32",
    "gespmm_heads_route",
    "gespmm_plan_heads_route",
    "gespmm_sddmm_coo_heads_f32",
    "gespmm_sddmm_csr_heads_f32",
    "gespmm_plan_sddmm_heads_f32",
    "gespmm_describe_sddmm_heads",
    "gespmm_plan_sddmm_heads_route",
    "gespmm_csr_spmm_heads_x16",
    "gespmm_heads_x16_route",
    "gespmm_sddmm_coo_heads_x16",
    "gespmm_sddmm_csr_heads_x16",
    "gespmm_describe_sddmm_heads_x16",
    "gespmm_edge_softmax_f32",
    "gespmm_edge_softmax_backward_f32",
    "gespmm_describe_edge_softmax",
    "gespmm_gat_softmax_f32",
    "gespmm_gat_softmax_backward_f32",
    "gespmm_edge_segment_sum_f32",
    "gespmm_gat_softmax_stats_f32",
    "gespmm_gat_aggregate_f32",
    "gespmm_gat_aggregate_route",
    "gespmm_gat_backward_el_f32",
    "gespmm_gat_backward_er_f32",
    "gespmm_edge_dropout_f32",
    "gespmm_gat_aggregate_dropout_f32",
    "gespmm_gat_backward_el_dropout_f32",
    "gespmm_gat_backward_er_dropout_f32",
    "gespmm_edge_dropout_bits",
    "gespmm_edge_dropout_threshold",
    "gespmm_gatv2_score_f32",
    "gespmm_gatv2_score_backward_f32",
    "gespmm_describe_gatv2_score",
    "gespmm_gatv2_score_x16",
    "gespmm_gatv2_score_backward_x16",
    "gespmm_describe_gatv2_score_x16",
    "gespmm_dot_attention_f32",
    "gespmm_dot_attention_dropout_f32",
    "gespmm_dot_attention_backward_q_f32",
    "gespmm_dot_attention_backward_q_dropout_f32",
    "gespmm_dot_attention_backward_kv_f32",
    "gespmm_dot_attention_backward_kv_dropout_f32",
    "gespmm_describe_dot_attention",
    "gespmm_dot_attention_x16",
    "gespmm_dot_attention_dropout_x16",
    "gespmm_dot_attention_backward_q_x16",
    "gespmm_dot_attention_backward_q_dropout_x16",
    "gespmm_dot_attention_backward_kv_x16",
    "gespmm_dot_attention_backward_kv_dropout_x16",
    "gespmm_describe_dot_attention_x16",
    "gespmm_gatv2_attention_f32",
    "gespmm_gatv2_attention_dropout_f32",
    "gespmm_gatv2_attention_backward_row_f32",
    "gespmm_gatv2_attention_backward_row_dropout_f32",
    "gespmm_gatv2_attention_backward_col_f32",
    "gespmm_gatv2_attention_backward_col_dropout_f32",
    "gespmm_describe_gatv2_attention",
    "gespmm_gatv2_attention_x16",
    "gespmm_gatv2_attention_dropout_x16",
    "gespmm_gatv2_attention_backward_row_x16",
    "gespmm_gatv2_attention_backward_row_dropout_x16",
    "gespmm_gatv2_attention_backward_col_x16",
    "gespmm_gatv2_attention_backward_col_dropout_x16",
    "gespmm_describe_gatv2_attention_x16",
    "gespmm_csr_spmm_max_arg_f32",
    "gespmm_csr_spmm_max_backward_f32",
    "gespmm_max_arg_route",
    "gespmm_csr_spmm_max_arg_x16",
    "gespmm_csr_spmm_max_backward_x16",
    "gespmm_max_arg_route_x16",
    "gespmm_csr_spmm_heads_order_f32",
    "gespmm_csr_spmm_heads_order_x16",
    "gespmm_plan_spmm_heads_order_f32",
    "gespmm_edge_gather",
]

X16_F16 = 1
X16_BF16 = 2

PLAN_REORDER_AUTO = 0
PLAN_REORDER = 1
PLAN_NO_REORDER = 2
PLAN_ANALYSIS_DEVICE = 0
PLAN_ANALYSIS_HOST = 1
PLAN_KERNEL_AUTO = 0
PLAN_KERNEL_STREAM = 1
PLAN_KERNEL_SEG_STREAM = 3
PLAN_KERNEL_STAGED = 5
PLAN_KERNEL_RECORDS = 6
PLAN_KERNEL_STAGED_SLABS = 7


class LaunchCfg(Structure):
    _fields_ = [("vec", c_int32), ("strips", c_int32), ("group", c_int32), ("rows_per_wave", c_int32),
                ("slab_rows", c_int32), ("flags", c_int32)]


class PlanOptions(Structure):
    _fields_ = [("reorder", c_int32), ("task_entries", c_int32), ("row_floor", c_int32), ("threads", c_int32),
                ("flags", c_int32), ("kernel", c_int32), ("analysis", c_int32), ("expected_launches", c_int32)]


class PlanPolicyQuery(Structure):
    _fields_ = [("M", c_int64), ("K", c_int64), ("nnz", c_int64), ("N", c_int64), ("N_launch", c_int64), ("variant", c_int32),
                ("max_degree", c_int32), ("reorder", c_int32), ("kernel", c_int32), ("analysis", c_int32), ("flags", c_int32),
                ("task_entries", c_int32), ("row_floor", c_int32), ("hits_before", ctypes.c_double),
                ("hits_after", ctypes.c_double), ("staged_fraction", ctypes.c_double), ("expected_launches", c_int32),
                ("cold_start", c_int32), ("wedge_probe", ctypes.c_double), ("record_slot_fill", ctypes.c_double)]


class PlanPolicyAnswer(Structure):
    _fields_ = [(n, c_int32) for n in ("launch_flags", "analyse", "dense_try", "keep_clustered", "task_entries",
                                       "group_task_entries", "row_floor", "build_staged", "keep_staged", "shallow_unroll",
                                       "segmented", "sddmm_route", "narrow_vec4")] + [("model_window", c_int64), ("model_sample", c_int64),
                                                                                       ("cost_skipped", c_int32), ("cluster_levels", c_int32),
                                                                                       ("est_gain_us", ctypes.c_double),
                                                                                       ("est_cost_us", ctypes.c_double), ("cluster_sweeps", c_int32),
                                                                                       ("staged_rows", c_int32), ("build_records", c_int32),
                                                                                       ("keep_records", c_int32), ("records_batches", c_int32),
                                                                                       ("slab_ranges", c_int32), ("staged_fill_window", c_int32)]


class AutoPlanStats(Structure):
    _fields_ = [(n, c_int64) for n in ("calls_planned", "plans_created", "invalidated", "values_refreshed", "fingerprints", "cached_plans", "calls_async")]


class Coo(Structure):
    _fields_ = [
        ("nrows", c_int32),
        ("ncols", c_int32),
        ("nnz", c_int64),
        ("row", POINTER(c_int32)),
        ("col", POINTER(c_int32)),
        ("val", POINTER(c_float)),
    ]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "gespmm_amd: %s is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C gespmm_amd/csrc`). There is no CPU fallback." % LIB_PATH
        )
    lib = ctypes.CDLL(LIB_PATH)
    p = c_void_p
    lib.gespmm_version.restype = c_char_p
    lib.gespmm_error_string.restype = c_char_p
    lib.gespmm_error_string.argtypes = [c_int]
    lib.gespmm_csr_spmm_f32.restype = c_int
    lib.gespmm_csr_spmm_f32.argtypes = [p, p, p, p, p, c_int64, c_int64, c_int64, c_int64, c_int, p]
    lib.gespmm_csr_spmm_f32_cfg.restype = c_int
    lib.gespmm_csr_spmm_f32_cfg.argtypes = [p, p, p, p, p, c_int64, c_int64, c_int64, c_int64, c_int,
                                            POINTER(LaunchCfg), p]
    lib.gespmm_csr_spmm_workspace_bytes.restype = c_int64
    lib.gespmm_csr_spmm_workspace_bytes.argtypes = [c_int64, c_int64, c_int64, c_int64, c_int, POINTER(LaunchCfg)]
    lib.gespmm_csr_spmm_f32_ws.restype = c_int
    lib.gespmm_csr_spmm_f32_ws.argtypes = [p, p, p, p, p, c_int64, c_int64, c_int64, c_int64, c_int,
                                           POINTER(LaunchCfg), p, c_int64, p]
    lib.gespmm_csr_spmm_max_f32.restype = c_int
    lib.gespmm_csr_spmm_max_f32.argtypes = [p, p, p, p, c_int64, c_int64, c_int64, c_int64, c_float, c_int, p]
    for fn in (lib.gespmm_dgl_csrmm_sum_f32, lib.gespmm_dgl_csrmm_max_f32):
        fn.restype = c_int
        fn.argtypes = [c_int, c_int, p, p, p, p, p]
    lib.gespmm_dgl_set_readback_rows.restype = c_int
    lib.gespmm_dgl_set_readback_rows.argtypes = [c_int64]
    lib.gespmm_describe_launch.restype = c_int
    lib.gespmm_describe_launch.argtypes = [c_int64, c_int64, c_int64, c_int64, c_int, POINTER(LaunchCfg), c_char_p, c_int64]
    lib.gespmm_select_variant.restype = c_int
    lib.gespmm_select_variant.argtypes = [c_int64, c_int64, c_int64]
    lib.gespmm_sddmm_coo_f32.restype = c_int
    lib.gespmm_sddmm_coo_f32.argtypes = [p, p, p, p, p, c_int64, c_int64, p]
    lib.gespmm_sddmm_csr_f32.restype = c_int
    lib.gespmm_sddmm_csr_f32.argtypes = [p, p, p, p, p, c_int64, c_int64, c_int64, p]
    lib.gespmm_csr2csc_workspace_bytes.restype = c_int64
    lib.gespmm_csr2csc_workspace_bytes.argtypes = [c_int64, c_int64, c_int64]
    lib.gespmm_csr2csc_f32.restype = c_int
    lib.gespmm_csr2csc_f32.argtypes = [p, p, p, p, p, p, c_int64, c_int64, c_int64, p, p]
    lib.gespmm_mtx_read.restype = c_int
    lib.gespmm_mtx_read.argtypes = [c_char_p, POINTER(Coo)]
    lib.gespmm_mtx_read_cached.restype = c_int
    lib.gespmm_mtx_read_cached.argtypes = [c_char_p, c_char_p, POINTER(Coo)]
    lib.gespmm_mtx_free.restype = None
    lib.gespmm_mtx_free.argtypes = [POINTER(Coo)]
    lib.gespmm_coo_to_csr.restype = c_int
    lib.gespmm_coo_to_csr.argtypes = [c_int32, c_int32, c_int64, p, p, p, p, p, p]
    lib.gespmm_baseline_atomic_scatter_f32.restype = c_int
    lib.gespmm_baseline_atomic_scatter_f32.argtypes = [p, p, p, p, c_int64, c_int64, c_int64, c_int64, p]
    lib.gespmm_plan_policy_v2.restype = c_int
    lib.gespmm_plan_policy_v2.argtypes = [POINTER(PlanPolicyQuery), c_int64, POINTER(PlanPolicyAnswer), c_int64]
    lib.gespmm_baseline_copy_f32.restype = c_int
    lib.gespmm_baseline_copy_f32.argtypes = [p, p, c_int64, p]
    lib.gespmm_plan_create.restype = c_int
    lib.gespmm_plan_create.argtypes = [POINTER(c_void_p), p, p, p, c_int64, c_int64, c_int64, c_int64, c_int,
                                       POINTER(PlanOptions), p]
    lib.gespmm_plan_create_v2.restype = c_int
    lib.gespmm_plan_create_v2.argtypes = [POINTER(c_void_p), p, p, p, c_int64, c_int64, c_int64, c_int64, c_int,
                                          POINTER(PlanOptions), c_int64, p]
    lib.gespmm_plan_policy.restype = c_int
    lib.gespmm_plan_policy.argtypes = [POINTER(PlanPolicyQuery), POINTER(PlanPolicyAnswer)]
    lib.gespmm_plan_tune.restype = c_int
    lib.gespmm_plan_tune.argtypes = [p, p, p, c_int64, c_int32, p]
    lib.gespmm_set_cached_memory_limit.restype = None
    lib.gespmm_set_cached_memory_limit.argtypes = [c_int64]
    lib.gespmm_plan_spmm_f32.restype = c_int
    lib.gespmm_plan_spmm_f32.argtypes = [p, p, p, c_int64, p]
    lib.gespmm_csr_spmm_fused_f32.restype = c_int
    lib.gespmm_csr_spmm_fused_f32.argtypes = [p, p, p, p, p, p, p, p, c_int64, c_int64, c_int64, c_int64, c_int, p]
    lib.gespmm_plan_spmm_fused_f32.restype = c_int
    lib.gespmm_plan_spmm_fused_f32.argtypes = [p, p, p, p, p, p, c_int64, p]
    lib.gespmm_csr_spmm_x16.restype = c_int
    lib.gespmm_csr_spmm_x16.argtypes = [p, p, p, p, p, c_int, c_int64, c_int64, c_int64, c_int64, c_int, p]
    lib.gespmm_plan_spmm_x16.restype = c_int
    lib.gespmm_plan_spmm_x16.argtypes = [p, p, p, c_int, c_int64, p]
    lib.gespmm_x16_route.restype = c_int
    lib.gespmm_x16_route.argtypes = [c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int]
    lib.gespmm_plan_x16_route.restype = c_int
    lib.gespmm_plan_x16_route.argtypes = [p, c_int64, c_int, c_int]
    lib.gespmm_csr_spmm_heads_f32.restype = c_int
    lib.gespmm_csr_spmm_heads_f32.argtypes = [p, p, p, p, p, c_int64, c_int64, c_int64, c_int64, c_int64, p]
    lib.gespmm_plan_spmm_heads_f32.restype = c_int
    lib.gespmm_plan_spmm_heads_f32.argtypes = [p, p, p, p, c_int64, c_int64, p]
    lib.gespmm_csr_spmm_heads_order_f32.restype = c_int
    lib.gespmm_csr_spmm_heads_order_f32.argtypes = [p, p, p, p, p, p, c_int64, c_int64, c_int64, c_int64, c_int64, p]
    lib.gespmm_csr_spmm_heads_order_x16.restype = c_int
    lib.gespmm_csr_spmm_heads_order_x16.argtypes = [p, p, p, p, p, p, c_int, c_int64, c_int64, c_int64, c_int64, c_int64, p]
    lib.gespmm_plan_spmm_heads_order_f32.restype = c_int
    lib.gespmm_plan_spmm_heads_order_f32.argtypes = [p, p, p, p, p, c_int64, c_int64, p]
    lib.gespmm_edge_gather.restype = c_int
    lib.gespmm_edge_gather.argtypes = [p, p, c_int, p, c_int64, c_int64, p]
    lib.gespmm_heads_route.restype = c_int
    lib.gespmm_heads_route.argtypes = [c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_int, p]
    lib.gespmm_plan_heads_route.restype = c_int
    lib.gespmm_plan_heads_route.argtypes = [p, c_int64, c_int64, c_int, c_int]
    lib.gespmm_plan_fused_route.restype = c_int
    lib.gespmm_plan_fused_route.argtypes = [p, c_int64, c_int, c_int, c_int]
    lib.gespmm_plan_spmm_max_f32.restype = c_int
    lib.gespmm_plan_spmm_max_f32.argtypes = [p, p, p, c_int64, c_float, p]
    lib.gespmm_plan_sddmm_f32.restype = c_int
    lib.gespmm_plan_sddmm_f32.argtypes = [p, p, p, p, c_int64, p]
    lib.gespmm_plan_sddmm_route.restype = c_int
    lib.gespmm_plan_sddmm_route.argtypes = [p, c_int64]
    lib.gespmm_describe_sddmm.restype = c_int
    lib.gespmm_describe_sddmm.argtypes = [c_int, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_char_p, c_int64]
    lib.gespmm_sddmm_coo_x16.restype = c_int
    lib.gespmm_sddmm_coo_x16.argtypes = [p, p, p, p, p, c_int, c_int64, c_int64, p]
    lib.gespmm_sddmm_csr_x16.restype = c_int
    lib.gespmm_sddmm_csr_x16.argtypes = [p, p, p, p, p, c_int, c_int64, c_int64, c_int64, p]
    lib.gespmm_plan_sddmm_x16.restype = c_int
    lib.gespmm_plan_sddmm_x16.argtypes = [p, p, p, p, c_int, c_int64, p]
    lib.gespmm_describe_sddmm_x16.restype = c_int
    lib.gespmm_describe_sddmm_x16.argtypes = [c_int, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_char_p, c_int64]
    lib.gespmm_sddmm_coo_heads_f32.restype = c_int
    lib.gespmm_sddmm_coo_heads_f32.argtypes = [p, p, p, p, p, c_int64, c_int64, c_int64, p]
    lib.gespmm_sddmm_csr_heads_f32.restype = c_int
    lib.gespmm_sddmm_csr_heads_f32.argtypes = [p, p, p, p, p, c_int64, c_int64, c_int64, c_int64, p]
    lib.gespmm_plan_sddmm_heads_f32.restype = c_int
    lib.gespmm_plan_sddmm_heads_f32.argtypes = [p, p, p, p, c_int64, c_int64, p]
    lib.gespmm_describe_sddmm_heads.restype = c_int
    lib.gespmm_describe_sddmm_heads.argtypes = [c_int, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_char_p, c_int64]
    lib.gespmm_plan_sddmm_heads_route.restype = c_int
    lib.gespmm_plan_sddmm_heads_route.argtypes = [p, c_int64, c_int64]
    lib.gespmm_csr_spmm_heads_x16.restype = c_int
    lib.gespmm_csr_spmm_heads_x16.argtypes = [p, p, p, p, p, c_int, c_int64, c_int64, c_int64, c_int64, c_int64, p]
    lib.gespmm_heads_x16_route.restype = c_int
    lib.gespmm_heads_x16_route.argtypes = [c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_int, p]
    lib.gespmm_sddmm_coo_heads_x16.restype = c_int
    lib.gespmm_sddmm_coo_heads_x16.argtypes = [p, p, p, p, p, c_int, c_int64, c_int64, c_int64, p]
    lib.gespmm_sddmm_csr_heads_x16.restype = c_int
    lib.gespmm_sddmm_csr_heads_x16.argtypes = [p, p, p, p, p, c_int, c_int64, c_int64, c_int64, c_int64, p]
    lib.gespmm_describe_sddmm_heads_x16.restype = c_int
    lib.gespmm_describe_sddmm_heads_x16.argtypes = [c_int, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_char_p, c_int64]
    lib.gespmm_edge_softmax_f32.restype = c_int
    lib.gespmm_edge_softmax_f32.argtypes = [p, p, p, c_int64, c_int64, c_int64, c_float, p]
    lib.gespmm_edge_softmax_backward_f32.restype = c_int
    lib.gespmm_edge_softmax_backward_f32.argtypes = [p, p, p, p, p, c_int64, c_int64, c_int64, c_float, p]
    lib.gespmm_gat_softmax_f32.restype = c_int
    lib.gespmm_gat_softmax_f32.argtypes = [p, p, p, p, p, c_int64, c_int64, c_int64, c_int64, c_float, p]
    lib.gespmm_gat_softmax_backward_f32.restype = c_int
    lib.gespmm_gat_softmax_backward_f32.argtypes = [p, p, p, p, p, p, p, p, c_int64, c_int64, c_int64, c_int64, c_float, p]
    lib.gespmm_edge_segment_sum_f32.restype = c_int
    lib.gespmm_edge_segment_sum_f32.argtypes = [p, p, p, p, c_int64, c_int64, c_int64, p]
    lib.gespmm_gat_softmax_stats_f32.restype = c_int
    lib.gespmm_gat_softmax_stats_f32.argtypes = [p, p, p, p, p, c_int64, c_int64, c_int64, c_int64, c_float, p]
    lib.gespmm_gat_aggregate_f32.restype = c_int
    lib.gespmm_gat_aggregate_f32.argtypes = [p, p, p, p, p, p, p, c_int64, c_int64, c_int64, c_int64, c_int64, c_float, c_int, p]
    for f in (lib.gespmm_gat_backward_el_f32, lib.gespmm_gat_backward_er_f32):
        f.restype = c_int
        f.argtypes = [p] * 9 + [c_int64] * 5 + [c_float, p]
    lib.gespmm_edge_dropout_f32.restype = c_int
    lib.gespmm_edge_dropout_f32.argtypes = [p, p, p, p, c_int64, c_int64, c_int64, c_int64, c_float, p, p]
    lib.gespmm_gat_aggregate_dropout_f32.restype = c_int
    lib.gespmm_gat_aggregate_dropout_f32.argtypes = lib.gespmm_gat_aggregate_f32.argtypes[:-1] + [c_float, p, p]
    for f in (lib.gespmm_gat_backward_el_dropout_f32, lib.gespmm_gat_backward_er_dropout_f32):
        f.restype = c_int
        f.argtypes = [p] * 9 + [c_int64] * 5 + [c_float, c_float, p, p]
    lib.gespmm_edge_dropout_bits.restype = ctypes.c_uint32
    lib.gespmm_edge_dropout_bits.argtypes = [ctypes.c_uint32] * 5
    lib.gespmm_edge_dropout_threshold.restype = ctypes.c_uint32
    lib.gespmm_edge_dropout_threshold.argtypes = [c_float]
    lib.gespmm_gatv2_score_f32.restype = c_int
    lib.gespmm_gatv2_score_f32.argtypes = [p] * 6 + [c_int64] * 5 + [c_float, p]
    lib.gespmm_gatv2_score_backward_f32.restype = c_int
    lib.gespmm_gatv2_score_backward_f32.argtypes = [p] * 9 + [c_int64] * 5 + [c_float, p]
    lib.gespmm_describe_gatv2_score.restype = c_int
    lib.gespmm_describe_gatv2_score.argtypes = [c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_char_p, c_int64]
    lib.gespmm_gatv2_score_x16.restype = c_int
    lib.gespmm_gatv2_score_x16.argtypes = [p] * 6 + [c_int] + [c_int64] * 5 + [c_float, p]
    lib.gespmm_gatv2_score_backward_x16.restype = c_int
    lib.gespmm_gatv2_score_backward_x16.argtypes = [p] * 9 + [c_int] + [c_int64] * 5 + [c_float, p]
    lib.gespmm_describe_gatv2_score_x16.restype = c_int
    lib.gespmm_describe_gatv2_score_x16.argtypes = [c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_char_p, c_int64]
    lib.gespmm_dot_attention_f32.restype = c_int
    lib.gespmm_dot_attention_f32.argtypes = [p] * 7 + [c_int64] * 5 + [c_float, p]
    lib.gespmm_dot_attention_dropout_f32.restype = c_int
    lib.gespmm_dot_attention_dropout_f32.argtypes = [p] * 7 + [c_int64] * 5 + [c_float, c_float, p, p]
    for f in (lib.gespmm_dot_attention_backward_q_f32, lib.gespmm_dot_attention_backward_kv_f32):
        f.restype = c_int
        f.argtypes = [p] * 10 + [c_int64] * 5 + [c_float, p]
    for f in (lib.gespmm_dot_attention_backward_q_dropout_f32, lib.gespmm_dot_attention_backward_kv_dropout_f32):
        f.restype = c_int
        f.argtypes = [p] * 10 + [c_int64] * 5 + [c_float, c_float, p, p]
    lib.gespmm_describe_dot_attention.restype = c_int
    lib.gespmm_describe_dot_attention.argtypes = [c_int64] * 5 + [c_int, c_int, c_int, c_char_p, c_int64]
    lib.gespmm_dot_attention_x16.restype = c_int
    lib.gespmm_dot_attention_x16.argtypes = [p] * 7 + [c_int] + [c_int64] * 5 + [c_float, p]
    lib.gespmm_dot_attention_dropout_x16.restype = c_int
    lib.gespmm_dot_attention_dropout_x16.argtypes = [p] * 7 + [c_int] + [c_int64] * 5 + [c_float, c_float, p, p]
    for f in (lib.gespmm_dot_attention_backward_q_x16, lib.gespmm_dot_attention_backward_kv_x16):
        f.restype = c_int
        f.argtypes = [p] * 10 + [c_int] + [c_int64] * 5 + [c_float, p]
    for f in (lib.gespmm_dot_attention_backward_q_dropout_x16, lib.gespmm_dot_attention_backward_kv_dropout_x16):
        f.restype = c_int
        f.argtypes = [p] * 10 + [c_int] + [c_int64] * 5 + [c_float, c_float, p, p]
    lib.gespmm_describe_dot_attention_x16.restype = c_int
    lib.gespmm_describe_dot_attention_x16.argtypes = [c_int64] * 5 + [c_int, c_int, c_int, c_char_p, c_int64]
    lib.gespmm_gatv2_attention_f32.restype = c_int
    lib.gespmm_gatv2_attention_f32.argtypes = [p] * 7 + [c_int64] * 5 + [c_float, p]
    lib.gespmm_gatv2_attention_dropout_f32.restype = c_int
    lib.gespmm_gatv2_attention_dropout_f32.argtypes = [p] * 7 + [c_int64] * 5 + [c_float, c_float, p, p]
    lib.gespmm_gatv2_attention_backward_row_f32.restype = c_int
    lib.gespmm_gatv2_attention_backward_row_f32.argtypes = [p] * 11 + [c_int64] * 5 + [c_float, p]
    lib.gespmm_gatv2_attention_backward_row_dropout_f32.restype = c_int
    lib.gespmm_gatv2_attention_backward_row_dropout_f32.argtypes = [p] * 11 + [c_int64] * 5 + [c_float, c_float, p, p]
    lib.gespmm_gatv2_attention_backward_col_f32.restype = c_int
    lib.gespmm_gatv2_attention_backward_col_f32.argtypes = [p] * 9 + [c_int64] * 5 + [c_float, p]
    lib.gespmm_gatv2_attention_backward_col_dropout_f32.restype = c_int
    lib.gespmm_gatv2_attention_backward_col_dropout_f32.argtypes = [p] * 9 + [c_int64] * 5 + [c_float, c_float, p, p]
    lib.gespmm_describe_gatv2_attention.restype = c_int
    lib.gespmm_describe_gatv2_attention.argtypes = [c_int64] * 5 + [c_int, c_int, c_int, c_char_p, c_int64]
    lib.gespmm_gatv2_attention_x16.restype = c_int
    lib.gespmm_gatv2_attention_x16.argtypes = [p] * 7 + [c_int] + [c_int64] * 5 + [c_float, p]
    lib.gespmm_gatv2_attention_dropout_x16.restype = c_int
    lib.gespmm_gatv2_attention_dropout_x16.argtypes = [p] * 7 + [c_int] + [c_int64] * 5 + [c_float, c_float, p, p]
    lib.gespmm_gatv2_attention_backward_row_x16.restype = c_int
    lib.gespmm_gatv2_attention_backward_row_x16.argtypes = [p] * 11 + [c_int] + [c_int64] * 5 + [c_float, p]
    lib.gespmm_gatv2_attention_backward_row_dropout_x16.restype = c_int
    lib.gespmm_gatv2_attention_backward_row_dropout_x16.argtypes = [p] * 11 + [c_int] + [c_int64] * 5 + [c_float, c_float, p, p]
    lib.gespmm_gatv2_attention_backward_col_x16.restype = c_int
    lib.gespmm_gatv2_attention_backward_col_x16.argtypes = [p] * 9 + [c_int] + [c_int64] * 5 + [c_float, p]
    lib.gespmm_gatv2_attention_backward_col_dropout_x16.restype = c_int
    lib.gespmm_gatv2_attention_backward_col_dropout_x16.argtypes = [p] * 9 + [c_int] + [c_int64] * 5 + [c_float, c_float, p, p]
    lib.gespmm_describe_gatv2_attention_x16.restype = c_int
    lib.gespmm_describe_gatv2_attention_x16.argtypes = [c_int64] * 5 + [c_int, c_int, c_int, c_char_p, c_int64]
    lib.gespmm_csr_spmm_max_arg_f32.restype = c_int
    lib.gespmm_csr_spmm_max_arg_f32.argtypes = [p] * 5 + [c_int64] * 4 + [c_float, p]
    lib.gespmm_csr_spmm_max_backward_f32.restype = c_int
    lib.gespmm_csr_spmm_max_backward_f32.argtypes = [p] * 6 + [c_int64] * 4 + [p]
    lib.gespmm_max_arg_route.restype = c_int
    lib.gespmm_max_arg_route.argtypes = [c_int64, c_int64, c_int64, c_int, c_int, c_char_p, c_int64]
    lib.gespmm_csr_spmm_max_arg_x16.restype = c_int
    lib.gespmm_csr_spmm_max_arg_x16.argtypes = [p] * 5 + [c_int64] * 4 + [c_float, c_int, p]
    lib.gespmm_csr_spmm_max_backward_x16.restype = c_int
    lib.gespmm_csr_spmm_max_backward_x16.argtypes = [p] * 6 + [c_int64] * 4 + [c_int, p]
    lib.gespmm_max_arg_route_x16.restype = c_int
    lib.gespmm_max_arg_route_x16.argtypes = [c_int64, c_int64, c_int64, c_int, c_int, c_char_p, c_int64]
    lib.gespmm_gat_aggregate_route.restype = c_int
    lib.gespmm_gat_aggregate_route.argtypes = [c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, p]
    lib.gespmm_describe_edge_softmax.restype = c_int
    lib.gespmm_describe_edge_softmax.argtypes = [c_int64, c_int64, c_int64, c_char_p, c_int64]
    lib.gespmm_plan_set_values.restype = c_int
    lib.gespmm_plan_set_values.argtypes = [p, p, p]
    lib.gespmm_plan_get_order.restype = c_int
    lib.gespmm_plan_get_order.argtypes = [p, p]
    lib.gespmm_plan_describe.restype = c_int
    lib.gespmm_plan_describe.argtypes = [p, c_char_p, c_int64]
    lib.gespmm_plan_destroy.restype = None
    lib.gespmm_plan_destroy.argtypes = [p]
    lib.gespmm_cluster_rows.restype = c_int
    lib.gespmm_cluster_rows.argtypes = [p, p, c_int64, c_int64, c_int32, p, p, p]
    lib.gespmm_device_cluster_rows.restype = c_int
    lib.gespmm_device_cluster_rows.argtypes = [p, p, c_int64, c_int64, c_int64, p, p, p, p]
    lib.gespmm_device_l2_model.restype = ctypes.c_double
    lib.gespmm_device_l2_model.argtypes = [p, p, c_int64, c_int64, c_int64, p, c_int32, c_int64, c_int64, c_int32, p]
    lib.gespmm_release_cached_memory.restype = None
    lib.gespmm_release_cached_memory.argtypes = []
    lib.gespmm_plan_debug_tasks.restype = c_int
    lib.gespmm_plan_debug_tasks.argtypes = [p, c_int32, p, c_int64]
    lib.gespmm_plan_debug_staging.restype = c_int64
    lib.gespmm_plan_debug_staging.argtypes = [p, p, p, c_int64]
    lib.gespmm_simulate_l2_hits.restype = ctypes.c_double
    lib.gespmm_simulate_l2_hits.argtypes = [p, p, c_int64, c_int64, p, c_int32, c_int64]
    lib.gespmm_row_partition.restype = c_int
    lib.gespmm_row_partition.argtypes = [p, c_int64, c_int32, p]
    lib.gespmm_init.restype = c_int
    lib.gespmm_init.argtypes = [c_int64, c_int64, p]
    lib.gespmm_plan_wants_warmup.restype = c_int
    lib.gespmm_plan_wants_warmup.argtypes = [c_int64, c_int64, c_int64, c_int64, c_int32]
    lib.gespmm_set_auto_plan.restype = c_int
    lib.gespmm_set_auto_plan.argtypes = [c_int32]
    lib.gespmm_auto_plan_clear.restype = None
    lib.gespmm_auto_plan_clear.argtypes = []
    lib.gespmm_auto_plan_get_stats.restype = c_int
    lib.gespmm_auto_plan_get_stats.argtypes = [POINTER(AutoPlanStats)]
    return lib


lib = _load()


class GespmmError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        super().__init__("%s failed: %s (code %d)" % (where, lib.gespmm_error_string(code).decode(), code))


def plan_policy(M, K, nnz, N, max_degree, hits_before=0.0, hits_after=0.0, staged_fraction=0.0, N_launch=0, variant=VARIANT_AUTO,
                reorder=PLAN_REORDER_AUTO, kernel=PLAN_KERNEL_AUTO, analysis=PLAN_ANALYSIS_DEVICE, flags=0, task_entries=0,
                row_floor=0, expected_launches=0, wedge_probe=-1.0, cold_start=0, record_slot_fill=-1.0):
    """What a plan would decide for a matrix of this shape (gespmm_plan_policy_v2: host only, no device) — a dict.
    `wedge_probe` is the plan's structure probe (share of sampled wedges that close; negative = unknown), `expected_launches` the
    number of products the analysis has to pay for itself in (0 = 200)."""
    q = PlanPolicyQuery(int(M), int(K), int(nnz), int(N), int(N_launch), int(variant), int(max_degree), int(reorder), int(kernel),
                        int(analysis), int(flags), int(task_entries), int(row_floor), float(hits_before), float(hits_after),
                        float(staged_fraction), int(expected_launches), int(cold_start), float(wedge_probe), float(record_slot_fill))
    a = PlanPolicyAnswer()
    check(lib.gespmm_plan_policy_v2(ctypes.byref(q), ctypes.sizeof(q), ctypes.byref(a), ctypes.sizeof(a)), "gespmm_plan_policy_v2")
    return {n: getattr(a, n) for n, _ in PlanPolicyAnswer._fields_ if not n.startswith("reserved")}


def describe_sddmm(csr, M, nnz, N, d1_align=16, d2_align=16, capturing=False, x16=False):
    """What gespmm_sddmm_{coo,csr}_f32 — x16=True: gespmm_sddmm_{coo,csr}_x16, fp16 / bf16 operands — would launch for these arguments
    (gespmm_describe_sddmm / gespmm_describe_sddmm_x16: host only) — a dict with "form" ("coo-edge", "csr-edge", "row-walk", "blocked" or
    "none") and the integers the form has: V (elements per load), W, epw / nslab, slab_rows."""
    buf = ctypes.create_string_buffer(128)
    f, name = (lib.gespmm_describe_sddmm_x16, "gespmm_describe_sddmm_x16") if x16 else (lib.gespmm_describe_sddmm, "gespmm_describe_sddmm")
    n = f(1 if csr else 0, int(M), int(nnz), int(N), int(d1_align), int(d2_align), 1 if capturing else 0, buf, 128)
    if n < 0:
        raise GespmmError(n, name)
    out = dict(kv.split("=") for kv in buf.value.decode().split())
    return {k: (v if k == "form" else int(v)) for k, v in out.items()}


def describe_sddmm_heads(csr, M, nnz, H, F, d1_align=16, d2_align=16, capturing=False, x16=False):
    """What gespmm_sddmm_{coo,csr}_heads_f32 — x16=True: gespmm_sddmm_{coo,csr}_heads_x16, fp16 / bf16 operands — would do for these
    arguments (gespmm_describe_sddmm_heads / _x16: host only) — a dict with "route"
    ("kernel", "composition", "plain" or "zeros"; absent when nnz == 0) and what the route has: "form", V (elements per load), W, epw
    (EDGES per wavefront) for the kernel, V and W for the composition, ``describe_sddmm``'s entries at width F for "plain"."""
    buf = ctypes.create_string_buffer(160)
    f, name = (lib.gespmm_describe_sddmm_heads_x16, "gespmm_describe_sddmm_heads_x16") if x16 else \
        (lib.gespmm_describe_sddmm_heads, "gespmm_describe_sddmm_heads")
    n = f(1 if csr else 0, int(M), int(nnz), int(H), int(F), int(d1_align), int(d2_align), 1 if capturing else 0, buf, 160)
    if n < 0:
        raise GespmmError(n, name)
    out = dict(kv.split("=") for kv in buf.value.decode().split())
    return {k: (v if k in ("form", "route") else int(v)) for k, v in out.items()}


def describe_edge_softmax(M, nnz, H):
    """The launch shape of gespmm_edge_softmax_f32 / _backward_f32 for these sizes (gespmm_describe_edge_softmax: host only) — a dict:
    ``{"W": lanes per (row, head) pair, "L": rows of more entries take a whole wavefront}``, or ``{"form": "none"}`` when nnz == 0.
    W and L depend on (M, nnz) alone."""
    buf = ctypes.create_string_buffer(64)
    n = lib.gespmm_describe_edge_softmax(int(M), int(nnz), int(H), buf, 64)
    if n < 0:
        raise GespmmError(n, "gespmm_describe_edge_softmax")
    text = buf.value.decode()
    if text == "form=none":
        return {"form": "none"}
    w, long_rows = text.split()
    return {"W": int(w.split("=")[1]), "L": int(long_rows.split(">")[1])}


def describe_gatv2_score(M, nnz, H, F, xl_align=16, xr_align=16, att_align=16, x16=False):
    """What gespmm_gatv2_score_f32 — x16=True: gespmm_gatv2_score_x16, fp16 / bf16 ``xl`` and ``xr`` with an fp32 ``att`` — would launch
    for these sizes and operand alignments (gespmm_describe_gatv2_score / _x16: host only) — a dict ``{"V": elements per load, "W":
    lanes per (entry, head) pair, "epw": ENTRIES per wavefront}``; ``{"route": "zeros"}`` when F == 0 and ``{"form": "none"}`` when
    nnz == 0. V and W fix the summation order. fp32: V divides F and 4 V bytes divide all three operand addresses. x16: V is 8 / 4 / 2 /
    1, divides F, 2 V bytes divide the addresses of ``xl`` and ``xr`` (alignments from 2) and min(4 V, 16) bytes that of ``att``."""
    buf = ctypes.create_string_buffer(96)
    f, name = (lib.gespmm_describe_gatv2_score_x16, "gespmm_describe_gatv2_score_x16") if x16 else \
        (lib.gespmm_describe_gatv2_score, "gespmm_describe_gatv2_score")
    n = f(int(M), int(nnz), int(H), int(F), int(xl_align), int(xr_align), int(att_align), buf, 96)
    if n < 0:
        raise GespmmError(n, name)
    out = dict(kv.split("=") for kv in buf.value.decode().split())
    return {k: (v if k in ("form", "route") else int(v)) for k, v in out.items()}


ERR_UNSUPPORTED = -7
DOT_ATTENTION_MAX_F = 512


def describe_dot_attention(M, K, H, F, nnz, q_align=16, k_align=16, v_align=16, x16=False):
    """The lane geometry of gespmm_dot_attention_f32 — x16=True: gespmm_dot_attention_x16, fp16 / bf16 q, k and v — and its two backward
    passes for these sizes and operand alignments (gespmm_describe_dot_attention / _x16: host only) — a dict ``{"V": floats per load,
    "W": lanes per (segment, head) pair}``; ``{"route": "unsupported"}`` when F > 512 (no kernel), ``{"route": "zeros"}`` when F == 0
    and ``{"form": "none"}`` when nnz == 0. V and W fix the dot's summation order; the least aligned dense operand of a launch — the
    dense results included — decides V. x16: V counts elements and stays in 4 / 2 / 1; 2 V bytes divide the operands' addresses
    (alignments from 2) — the fp32 answer at twice each alignment."""
    buf = ctypes.create_string_buffer(96)
    f, name = (lib.gespmm_describe_dot_attention_x16, "gespmm_describe_dot_attention_x16") if x16 else \
        (lib.gespmm_describe_dot_attention, "gespmm_describe_dot_attention")
    n = f(int(M), int(K), int(H), int(F), int(nnz), int(q_align), int(k_align), int(v_align), buf, 96)
    if n < 0:
        raise GespmmError(n, name)
    out = dict(kv.split("=") for kv in buf.value.decode().split())
    return {k: (v if k in ("form", "route") else int(v)) for k, v in out.items()}


GATV2_ATTENTION_MAX_F = 512


def describe_gatv2_attention(M, K, H, F, nnz, xl_align=16, xr_align=16, att_align=16, x16=False):
    """The lane geometry of gespmm_gatv2_attention_f32 — x16=True: gespmm_gatv2_attention_x16, fp16 / bf16 node terms with an fp32
    ``att`` — and its two backward passes for these sizes and operand alignments (gespmm_describe_gatv2_attention / _x16: host only) — a dict ``{"V": floats per load, "W": lanes per (segment, head) pair, "supported":
    True}``; ``{"route": "unsupported", "supported": False}`` when F > 512 (no kernel), ``{"route": "zeros", ...}`` when F == 0 and
    ``{"form": "none", ...}`` when nnz == 0. V and W fix the score's summation order; the least aligned dense operand of a launch —
    the dense results included: pass their alignment with ``xl_align`` — decides V. x16: V counts elements and stays in 4 / 2 / 1; 2 V
    bytes divide the 16-bit operands' addresses (``xl_align``, ``xr_align`` from 2), 4 V bytes those of ``att`` and ``att_part``
    (``att_align`` from 4) — the fp32 answer at twice the 16-bit alignment."""
    buf = ctypes.create_string_buffer(96)
    f, name = (lib.gespmm_describe_gatv2_attention_x16, "gespmm_describe_gatv2_attention_x16") if x16 else \
        (lib.gespmm_describe_gatv2_attention, "gespmm_describe_gatv2_attention")
    n = f(int(M), int(K), int(H), int(F), int(nnz), int(xl_align), int(xr_align), int(att_align), buf, 96)
    if n < 0:
        raise GespmmError(n, name)
    out = dict(kv.split("=") for kv in buf.value.decode().split())
    return {k: (v if k in ("form", "route") else bool(int(v)) if k == "supported" else int(v)) for k, v in out.items()}


def heads_route(M, K, H, F, nnz, b_align=16, c_align=16):
    """What gespmm_csr_spmm_heads_f32 would do for these sizes and operand alignments (gespmm_heads_route: host only):
    ``(route, (V, S, W, rpw))`` — route 1 the heads kernel with that lane geometry, route 0 the per-head composition (zeros)."""
    geo = (ctypes.c_int32 * 4)()
    rc = lib.gespmm_heads_route(int(M), int(K), int(H), int(F), int(nnz), int(b_align), int(c_align), geo)
    if rc < 0:
        raise GespmmError(rc, "gespmm_heads_route")
    return rc, tuple(int(x) for x in geo)


def heads_x16_route(M, K, H, F, nnz, b_align=16, c_align=16):
    """What gespmm_csr_spmm_heads_x16 would do for these sizes and operand alignments (gespmm_heads_x16_route: host only):
    ``(route, (V, S, W, rpw))`` — route 1 the 16-bit heads kernel with that lane geometry (V in 32-bit words: V divides F / 2),
    route 0 the composition widen, gespmm_csr_spmm_heads_f32, narrow (zeros)."""
    geo = (ctypes.c_int32 * 4)()
    rc = lib.gespmm_heads_x16_route(int(M), int(K), int(H), int(F), int(nnz), int(b_align), int(c_align), geo)
    if rc < 0:
        raise GespmmError(rc, "gespmm_heads_x16_route")
    return rc, tuple(int(x) for x in geo)


def max_arg_route(M, nnz, N, b_align=16, c_align=16):
    """The lane geometry gespmm_csr_spmm_max_arg_f32 takes for M rows, nnz entries and width N — and gespmm_csr_spmm_max_backward_f32
    for M = its K columns — with operands on these alignments (gespmm_max_arg_route: host only): ``(V, S, W)``, or ``None`` when there
    is nothing to launch (M == 0 or N == 0)."""
    buf = ctypes.create_string_buffer(64)
    n = lib.gespmm_max_arg_route(int(M), int(nnz), int(N), int(b_align), int(c_align), buf, 64)
    if n < 0:
        raise GespmmError(n, "gespmm_max_arg_route")
    text = buf.value.decode()
    if text == "form=none":
        return None
    out = dict(kv.split("=") for kv in text.split())
    return int(out["V"]), int(out["S"]), int(out["W"])


def max_arg_route_x16(M, nnz, N, x16_align=16, arg_align=16):
    """The lane geometry of gespmm_csr_spmm_max_arg_x16 / gespmm_csr_spmm_max_backward_x16, V in ELEMENTS, with the 16-bit arrays on
    ``x16_align``-byte and arg on ``arg_align``-byte boundaries (gespmm_max_arg_route_x16: host only): ``(V, S, W)``, or ``None`` when
    there is nothing to launch."""
    buf = ctypes.create_string_buffer(64)
    n = lib.gespmm_max_arg_route_x16(int(M), int(nnz), int(N), int(x16_align), int(arg_align), buf, 64)
    if n < 0:
        raise GespmmError(n, "gespmm_max_arg_route_x16")
    text = buf.value.decode()
    if text == "form=none":
        return None
    out = dict(kv.split("=") for kv in text.split())
    return int(out["V"]), int(out["S"]), int(out["W"])


def edge_dropout_bits(s0, s1, r, c, h):
    """The 32 bits the dropout mask compares with its threshold for entry (r, c), head h and seed (s0, s1), as the library's C++
    computes them (gespmm_edge_dropout_bits: host only)."""
    return int(lib.gespmm_edge_dropout_bits(int(s0) & 0xFFFFFFFF, int(s1) & 0xFFFFFFFF, int(r), int(c), int(h)))


def edge_dropout_threshold(p):
    """The threshold T of the dropout mask for probability p: an entry is kept when its bits are >= T (gespmm_edge_dropout_threshold)."""
    return int(lib.gespmm_edge_dropout_threshold(float(p)))


def gat_aggregate_route(M, K, H, F, nnz, transposed=False, b_align=16, c_align=16):
    """What gespmm_gat_aggregate_f32 would do for these sizes and operand alignments (gespmm_gat_aggregate_route: host only):
    ``(route, (V, S, W, rpw))`` — route 1 the one kernel with that lane geometry, route 0 the composition (zeros). ``M``, ``K`` are
    the rows and columns of the pattern in both modes."""
    geo = (ctypes.c_int32 * 4)()
    rc = lib.gespmm_gat_aggregate_route(int(M), int(K), int(H), int(F), int(nnz), 1 if transposed else 0, int(b_align), int(c_align), geo)
    if rc < 0:
        raise GespmmError(rc, "gespmm_gat_aggregate_route")
    return rc, tuple(int(x) for x in geo)


def init(rows_hint=0, nnz_hint=0, stream=None):
    """gespmm_init: load the analysis kernels and make the analysis arena NOW (the first plan of a process otherwise pays ~29 ms for
    both), optionally sized for a matrix of (rows_hint, nnz_hint). Needs a HIP device; idempotent per device."""
    check(lib.gespmm_init(int(rows_hint), int(nnz_hint), stream), "gespmm_init")


_initialised = set()


def ensure_init(device_index, stream=None, shape=None, expected_launches=0, forced=False):
    """gespmm_init once per process and device, before the first plan that could use it: the Python layer never builds such a plan cold
    (the ~29 ms of kernel loading and arena allocation belong to start-up, not to the first plan's analysis time — and not to its cost
    rule). `shape` = (M, K, nnz, N) of the plan about to be made: a matrix whose analysis could not pay even when warm (pubmed-sized
    graphs) keeps its storage order either way, so nothing is warmed up for it (the reference's GCN run on pubmed would otherwise pay
    ~0.5 ms per epoch for it: profiles/r06/gcn_epochs.log)."""
    if device_index in _initialised:
        return
    if shape is not None and not forced and lib.gespmm_plan_wants_warmup(int(shape[0]), int(shape[1]), int(shape[2]), int(shape[3]), int(expected_launches)) != 1:
        return
    init(0, 0, stream)
    _initialised.add(device_index)


def set_auto_plan(kth_call):
    """gespmm_set_auto_plan: from the k-th identical stateless call on (gespmm_csr_spmm_f32 / _max / gespmm_dgl_csrmm_*), run through a
    plan the library keeps (0 = off, the default). Every planned call fingerprints the CSR arrays first (one stream synchronisation)."""
    check(lib.gespmm_set_auto_plan(int(kth_call)), "gespmm_set_auto_plan")


def auto_plan_stats():
    st = AutoPlanStats()
    check(lib.gespmm_auto_plan_get_stats(ctypes.byref(st)), "gespmm_auto_plan_get_stats")
    return {n: getattr(st, n) for n, _ in AutoPlanStats._fields_}


def auto_plan_clear():
    lib.gespmm_auto_plan_clear()


def release_cached_memory():
    """Give the analysis stage's cached scratch arenas back to the devices (gespmm_release_cached_memory)."""
    lib.gespmm_release_cached_memory()


def set_cached_memory_limit(nbytes):
    """Largest analysis arena the library keeps between plans, per device (default 1 GiB; larger arenas are freed when the plan
    is made). A caller that builds many large plans in a row raises it (products-sized graphs: ~10 GB) and calls
    release_cached_memory() when done."""
    lib.gespmm_set_cached_memory_limit(int(nbytes))


def check(code, where):
    if code != 0:
        raise GespmmError(code, where)
