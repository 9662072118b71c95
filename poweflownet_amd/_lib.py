"""ctypes binding of libpfn_hip.so (the C ABI declared in include/pfn_hip.h).

There is NO CPU fallback: if the library is missing or a call fails, a RuntimeError is raised.
PyTorch is used only for device memory, streams and autograd plumbing; every tensor crosses the
boundary as a raw device pointer + sizes.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libpfn_hip.so")

# every symbol include/pfn_hip.h declares (checked by tests/test_abi.py without a GPU)
SYMBOLS = (
    "pfn_abi_version", "pfn_last_error", "pfn_padded_ld",
    "pfn_graph_workspace_bytes", "pfn_graph_build", "pfn_graph_info", "pfn_graph_segments", "pfn_graph_segments_async", "pfn_graph_poison_if_bad", "pfn_graph_export_edges",
    "pfn_graph_build_segments", "pfn_graph_build_segments_fits", "pfn_graph_layout",
    "pfn_mpn_num_params", "pfn_mpn_workspace_bytes", "pfn_mpn_forward", "pfn_mpn_backward", "pfn_mpn_mse_tail_ok", "pfn_mpn_backward_mse", "pfn_mpn_backward_masked_l2", "pfn_mpn_export_gates",
    "pfn_edge_aggr_workspace_bytes", "pfn_edge_aggr_forward", "pfn_edge_aggr_backward",
    "pfn_tag_conv_workspace_bytes", "pfn_tag_conv_forward", "pfn_tag_conv_backward",
    "pfn_gcn_conv_workspace_bytes", "pfn_gcn_conv_forward", "pfn_gcn_conv_backward",
    "pfn_scatter_add", "pfn_pad_rows", "pfn_mse_loss", "pfn_masked_l2_loss", "pfn_power_imbalance", "pfn_dropout_mask", "pfn_adamw_step", "pfn_adamw_step_dev", "pfn_adamw_step_guarded",
    "pfn_profile_enable", "pfn_profile_report",
    "pfn_khop_distances", "pfn_khop_histograms", "pfn_khop_pack",
    "pfn_segpack_pack", "pfn_segpack_gather_rows", "pfn_segpack_scatter_rows",
    "pfn_segpack_gather_slots", "pfn_mse_loss_rows", "pfn_masked_l2_loss_rows",
    "pfn_eval_metrics", "pfn_eval_accumulate",
    "pfn_bus_errors_accumulate", "pfn_bus_errors_histogram",
    "pfn_branch_flows_lds_max_bus", "pfn_branch_flows_workspace_bytes", "pfn_branch_flows",
    "pfn_powerflow_max_unknowns", "pfn_powerflow_workspace_bytes", "pfn_powerflow_solve",
    "pfn_powerflow_workspace_bytes_mode", "pfn_powerflow_solve_init",
    "pfn_powerflow_qlim_workspace_bytes", "pfn_powerflow_solve_qlim",
    "pfn_powerflow_sparse_plan_bytes", "pfn_powerflow_sparse_plan", "pfn_powerflow_sparse_workspace_bytes", "pfn_powerflow_solve_sparse",
    "pfn_powerflow_sparse_fd_plan_bytes", "pfn_powerflow_sparse_fd_plan", "pfn_powerflow_sparse_fd_workspace_bytes", "pfn_powerflow_solve_sparse_fd",
    "pfn_powerflow_sparse_plan_into", "pfn_powerflow_cover_map", "pfn_powerflow_solve_sparse_masked", "pfn_powerflow_solve_sparse_fd_masked",
    "pfn_powerflow_sparse_qlim_workspace_bytes", "pfn_powerflow_solve_sparse_qlim",
    "pfn_topology_perturb", "pfn_topology_unsupplied",
    "pfn_contingency_islands", "pfn_contingency_workspace_bytes", "pfn_contingency_dc",
    "pfn_contingency_sparse_workspace_bytes", "pfn_contingency_sparse",
    "pfn_contingency_pair_islands", "pfn_contingency_pairs_workspace_bytes", "pfn_contingency_pairs",
    "pfn_contingency_pairs_sparse_workspace_bytes", "pfn_contingency_pairs_sparse",
    "pfn_contingency_model_lds_max_bus", "pfn_contingency_model_batch", "pfn_contingency_model_loadings",
    "pfn_contingency_ac_workspace_bytes", "pfn_contingency_ac_waves", "pfn_contingency_ac",
    "pfn_contingency_ac_sparse_block_bytes", "pfn_contingency_ac_sparse_workspace_bytes", "pfn_contingency_ac_sparse",
    "pfn_contingency_units_workspace_bytes", "pfn_contingency_units",
)

# enum pfn_eval_term (include/pfn_hip.h), in order: the fp32 batch terms of pfn_eval_metrics
EVAL_TERMS = (
    "cnt_vm", "cnt_va", "cnt_p", "cnt_q",
    "l2_total", "l2_balanced", "l2_vm", "l2_va", "l2_p", "l2_q",
    "l2d_total", "l2d_balanced", "l2d_vm", "l2d_va", "l2d_p", "l2d_q",
    "l1_total", "l1_balanced", "l1_vm", "l1_va", "l1_p", "l1_q",
    "l1d_total", "l1d_balanced", "l1d_vm", "l1d_va", "l1d_p", "l1d_q",
    "ml2_selected", "ml2_regularizer", "mse",
)
EVAL_ACC_DOUBLES = len(EVAL_TERMS) + 1      # an epoch accumulator: one double per term + the int64 batch counter
EVAL_WS_FLOATS = 6660                       # struct EvalWs (csrc/eval.hip): 26640 bytes


class MpnConfig(C.Structure):
    """struct pfn_mpn_config."""
    _fields_ = [("nfeature_dim", C.c_int32), ("efeature_dim", C.c_int32), ("output_dim", C.c_int32),
                ("hidden_dim", C.c_int32), ("n_gnn_layers", C.c_int32), ("K", C.c_int32),
                ("dropout_rate", C.c_float), ("training", C.c_int32), ("need_backward", C.c_int32)]


SLOT_MAX_CASES = 8


class SlotCase(C.Structure):
    """struct pfn_slot_case: the dense block of one grid case (pfn_segpack_gather_slots)."""
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("pred_mask", C.c_void_p), ("bus_type", C.c_void_p), ("edge_attr", C.c_void_p),
                ("n_nodes", C.c_int64), ("n_edges", C.c_int64), ("n_samples", C.c_int64)]


# the arrays of a graph workspace in pfn_graph_layout's order, with their element width in bytes
GRAPH_ARRAYS = (("flags", 4), ("scan_sums", 4), ("rowptr_in", 4), ("rowptr_out", 4), ("in_src", 4), ("in_eid", 4), ("out_dst", 4),
                ("out_eid", 4), ("rp4", 4), ("out_mbase", 4), ("out_ml4k", 8), ("slot_of_eid", 4), ("cur_in", 4), ("cur_out", 4),
                ("deg", 4), ("dinv", 4))

_lib = None
ABI_VERSION = 8


def load() -> C.CDLL:
    """Load (once) and type the library.  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            f"or make -C poweflownet_amd/csrc).  poweflownet_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    p, i64, i32, sz, f32 = C.c_void_p, C.c_int64, C.c_int, C.c_size_t, C.c_float
    cfgp = C.POINTER(MpnConfig)
    sig = {
        "pfn_abi_version": (C.c_int, []),
        "pfn_last_error": (C.c_char_p, []),
        "pfn_padded_ld": (i64, [i64]),
        "pfn_graph_workspace_bytes": (sz, [i64, i64]),
        "pfn_graph_build": (C.c_int, [p, i64, i64, i32, p, sz, p]),
        "pfn_graph_info": (C.c_int, [p, i64, i64, C.POINTER(C.c_int32), C.POINTER(C.c_int64), p]),
        "pfn_graph_segments": (C.c_int, [p, i64, i64, i64, C.POINTER(C.c_int32), p]),
        "pfn_graph_segments_async": (C.c_int, [p, i64, i64, i64, p]),
        "pfn_graph_poison_if_bad": (C.c_int, [p, i64, i64, p, i64, p]),
        "pfn_graph_export_edges": (C.c_int, [p, i64, i64, p, p]),
        "pfn_graph_build_segments": (C.c_int, [p, i64, i64, i64, i64, i32, p, i64, p, p, sz, p]),
        "pfn_graph_build_segments_fits": (C.c_int, [i64, i64]),
        "pfn_graph_layout": (C.c_int, [i64, i64, C.POINTER(C.c_int64), i64]),
        "pfn_mpn_num_params": (C.c_int, [cfgp]),
        "pfn_mpn_workspace_bytes": (sz, [cfgp, i64, i64]),
        "pfn_mpn_forward": (C.c_int, [cfgp, p, i64, i64, p, p, p, i32, p, p, p, sz, p, i64, p]),
        "pfn_mpn_backward": (C.c_int, [cfgp, p, i64, i64, p, p, p, p, i32, p, p, p, p, p, sz, i64, p]),
        "pfn_mpn_mse_tail_ok": (C.c_int, [cfgp, i64, i64, i64]),
        "pfn_mpn_backward_mse": (C.c_int, [cfgp, p, i64, i64, p, p, p, p, p, p, p, p, p, p, sz, p, sz, i64, p]),
        "pfn_mpn_backward_masked_l2": (C.c_int, [cfgp, p, i64, i64, p, p, p, p, p, i32, f32, p, p, p, p, p, sz, p, sz, i64, p]),
        "pfn_mpn_export_gates": (C.c_int, [cfgp, p, i64, i64, p, p, p, sz, i64, C.c_int32, C.c_int32, p, p]),
        "pfn_edge_aggr_workspace_bytes": (sz, [i64, i64, i32, i32, i32, i32]),
        "pfn_edge_aggr_forward": (C.c_int, [p, i64, i64, i32, i32, i32, i32, p, i64, p, p, p, p, p, p, i64, p, sz, p]),
        "pfn_edge_aggr_backward": (C.c_int, [p, i64, i64, i32, i32, i32, i32, p, i64, p, p, p, p, p, p, i64, p, i64, p,
                                             p, p, p, p, p, sz, p]),
        "pfn_tag_conv_workspace_bytes": (sz, [i64, i64, i32, i32, i32]),
        "pfn_tag_conv_forward": (C.c_int, [p, i64, i64, i32, i32, i32, p, i64, p, p, p, i64, p, sz, i64, p]),
        "pfn_tag_conv_backward": (C.c_int, [p, i64, i64, i32, i32, i32, p, i64, p, p, i64, p, i64, p, p, p, sz, i64, p]),
        "pfn_gcn_conv_workspace_bytes": (sz, [i64, i64, i32, i32]),
        "pfn_gcn_conv_forward": (C.c_int, [p, i64, i64, i32, i32, p, i64, p, p, i32, p, i64, p, sz, p]),
        "pfn_gcn_conv_backward": (C.c_int, [p, i64, i64, i32, i32, p, i64, p, p, i64, i32, p, i64, p, p, p, sz, p]),
        "pfn_scatter_add": (C.c_int, [p, i64, i64, p, p, i64, p]),
        "pfn_pad_rows": (C.c_int, [p, i64, p, i64, i64, i64, p]),
        "pfn_mse_loss": (C.c_int, [p, p, i64, p, p, p, sz, p]),
        "pfn_masked_l2_loss": (C.c_int, [p, p, p, C.c_int, i64, C.c_int, C.c_float, p, p, p, sz, p]),
        "pfn_power_imbalance": (C.c_int, [p, i64, i64, p, p, p, p, p, p, p, sz, p]),
        "pfn_dropout_mask": (C.c_int, [p, C.c_int32, i64, i64, f32, p, p]),
        "pfn_adamw_step": (C.c_int, [p, p, p, p, i64, f32, f32, f32, f32, f32, p, p]),
        "pfn_adamw_step_dev": (C.c_int, [p, p, p, p, i64, p, p, p]),
        "pfn_adamw_step_guarded": (C.c_int, [p, p, p, p, i64, p, p, p, p]),
        "pfn_profile_enable": (C.c_int, [i32]),
        "pfn_profile_report": (C.c_int, [C.c_char_p, sz, i32]),
        "pfn_khop_distances": (C.c_int, [p, i64, i64, p, i64, i32, p, p, p]),
        "pfn_khop_histograms": (C.c_int, [p, i64, i64, p, i64, i32, p, p, p]),
        "pfn_khop_pack": (C.c_int, [p, i64, i64, p, p, p, p, p, p, p, p, i64, i64, p, p, p, p, p, p]),
        "pfn_segpack_pack": (C.c_int, [p, p, p, i64, i64, i64, i64, p, p, i32, p, i64, p, p, p, p, p, p]),
        "pfn_segpack_gather_rows": (C.c_int, [p, i64, i64, p, p, i64, i64, i64, p]),
        "pfn_segpack_scatter_rows": (C.c_int, [p, i64, i64, p, p, i64, i64, i64, i64, p]),
        "pfn_segpack_gather_slots": (C.c_int, [C.POINTER(SlotCase), i32, i32, p, p, p, p, p, p, i64, i64, i64, p, p, p, p, p, p, p]),
        "pfn_mse_loss_rows": (C.c_int, [p, p, p, i64, p, p, p, sz, p]),
        "pfn_masked_l2_loss_rows": (C.c_int, [p, p, p, C.c_int, p, i64, C.c_int, C.c_float, p, p, p, sz, p]),
        "pfn_eval_metrics": (C.c_int, [p, p, p, p, C.c_int, i64, C.POINTER(C.c_float), C.c_double, C.c_int, p, p, p, p, sz, p]),
        "pfn_eval_accumulate": (C.c_int, [p, C.c_double, C.c_int, p, p]),
        "pfn_bus_errors_accumulate": (C.c_int, [p, p, p, C.c_int, i64, i64, C.POINTER(C.c_float), C.POINTER(C.c_float), p, i64, p, p,
                                                p, p, p]),
        "pfn_bus_errors_histogram": (C.c_int, [p, i64, i64, p, p, C.c_int, p, p, p]),
        "pfn_branch_flows_lds_max_bus": (i64, []),
        "pfn_branch_flows_workspace_bytes": (sz, [i64, i64, C.c_int]),
        "pfn_branch_flows": (C.c_int, [p, C.c_int, p, C.c_int, i64, i64, C.POINTER(C.c_float), C.POINTER(C.c_float), p, C.c_int, i64,
                                       p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), p, p, p, p, p, p, sz, p]),
        "pfn_powerflow_max_unknowns": (i64, []),
        "pfn_powerflow_workspace_bytes": (sz, [i64, i64, i64, i64, C.c_int]),
        "pfn_powerflow_solve": (C.c_int, [p, C.c_int, i64, p, p, p, i64, i64, i64, i64, C.c_int, C.c_double, C.c_int, C.c_int, p, p, p, p,
                                          p, sz, p]),
        "pfn_powerflow_workspace_bytes_mode": (sz, [i64, i64, i64, i64, C.c_int, C.c_int]),
        "pfn_powerflow_solve_init": (C.c_int, [p, C.c_int, i64, p, p, p, p, i64, i64, i64, i64, C.c_int, C.c_double, C.c_int, C.c_int, p, p,
                                               p, p, p, sz, p]),
        "pfn_powerflow_qlim_workspace_bytes": (sz, [i64, i64, C.c_int]),
        "pfn_powerflow_solve_qlim": (C.c_int, [p, C.c_int, i64, p, p, C.c_int, p, p, p, C.c_int, i64, i64, C.c_double, C.c_double, C.c_int,
                                               C.c_int, C.c_int, p, p, p, p, p, p, p, sz, p]),
        "pfn_powerflow_sparse_plan_bytes": (sz, [p, i64, p, i64, C.c_int]),
        "pfn_powerflow_sparse_plan": (C.c_int, [p, i64, p, i64, C.c_int, p, sz]),
        "pfn_powerflow_sparse_workspace_bytes": (sz, [i64, p]),
        "pfn_powerflow_solve_sparse": (C.c_int, [p, i64, p, p, p, p, i64, i64, C.c_int, C.c_double, C.c_int, p, p, C.c_int, p, p, p, p, p,
                                                 sz, p]),
        "pfn_powerflow_sparse_fd_plan_bytes": (sz, [p, i64, p, i64]),
        "pfn_powerflow_sparse_fd_plan": (C.c_int, [p, i64, p, i64, p, sz]),
        "pfn_powerflow_sparse_fd_workspace_bytes": (sz, [i64, p]),
        "pfn_powerflow_solve_sparse_fd": (C.c_int, [p, i64, p, p, p, p, i64, i64, C.c_int, C.c_double, C.c_int, p, p, C.c_int, p, p, p, p, p,
                                                    sz, p]),
        "pfn_powerflow_sparse_plan_into": (C.c_int, [p, i64, p, i64, C.c_int, p, sz, p]),
        "pfn_powerflow_cover_map": (C.c_int, [p, i64, p, i64, i64, p, p, i64, p, p, p, p]),
        "pfn_powerflow_solve_sparse_masked": (C.c_int, [p, i64, p, p, p, p, p, p, i64, i64, C.c_int, C.c_double, C.c_int, p, p, C.c_int, p,
                                                        p, p, p, p, sz, p]),
        "pfn_powerflow_solve_sparse_fd_masked": (C.c_int, [p, i64, p, p, p, p, p, p, i64, i64, C.c_int, C.c_double, C.c_int, p, p, C.c_int,
                                                           p, p, p, p, p, sz, p]),
        "pfn_powerflow_sparse_qlim_workspace_bytes": (sz, [i64, p]),
        "pfn_powerflow_solve_sparse_qlim": (C.c_int, [p, i64, p, p, p, p, C.c_int, p, p, p, C.c_int, i64, i64, C.c_double, C.c_double,
                                                      C.c_int, C.c_int, p, p, C.c_int, p, p, p, p, p, p, p, sz, p]),
        "pfn_topology_perturb": (C.c_int, [p, i64, i64, i64, i64, i64, i64, C.c_uint64, i64, C.c_int, p, p, p, p]),
        "pfn_topology_unsupplied": (C.c_int, [p, C.c_int, i64, i64, i64, i64, p, p]),
        "pfn_contingency_islands": (C.c_int, [p, i64, i64, i64, p, p]),
        "pfn_contingency_workspace_bytes": (sz, [i64, i64, i64, C.c_int]),
        "pfn_contingency_dc": (C.c_int, [p, i64, p, p, p, p, C.c_int, p, i64, i64, i64, i64, C.c_double, C.c_int, C.c_int, p, p, p, p, p,
                                         p, p, p, sz, p]),
        "pfn_contingency_sparse_workspace_bytes": (sz, [i64, i64, p, C.c_int, C.c_int]),
        "pfn_contingency_sparse": (C.c_int, [p, i64, p, p, p, p, C.c_int, p, i64, i64, i64, i64, C.c_double, C.c_int, p, p, p, p, p,
                                             p, p, p, sz, p, p, C.c_int, C.c_int, C.c_int, p]),
        "pfn_contingency_pair_islands": (C.c_int, [p, i64, i64, i64, p, i64, p, p]),
        "pfn_contingency_pairs_workspace_bytes": (sz, [i64, i64, i64, i64, C.c_int]),
        "pfn_contingency_pairs": (C.c_int, [p, i64, p, p, p, p, C.c_int, p, i64, p, i64, i64, i64, i64, C.c_double, C.c_int, C.c_int,
                                            p, p, p, p, p, p, p, p, sz, p]),
        "pfn_contingency_pairs_sparse_workspace_bytes": (sz, [i64, i64, i64, p, C.c_int, C.c_int, C.c_int, C.c_int]),
        "pfn_contingency_pairs_sparse": (C.c_int, [p, i64, p, p, p, p, C.c_int, p, i64, p, i64, i64, i64, i64, C.c_double, C.c_int,
                                                   p, p, p, p, p, p, p, p, sz, p, p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, p]),
        "pfn_contingency_model_lds_max_bus": (i64, []),
        "pfn_contingency_model_batch": (C.c_int, [p, p, p, p, i64, i64, i64, p, i64, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                  C.POINTER(C.c_float), C.POINTER(C.c_float), p, p, p, p, p, p, p]),
        "pfn_contingency_model_loadings": (C.c_int, [p, p, p, p, p, p, C.c_int, p, i64, i64, i64, p, i64, C.POINTER(C.c_float),
                                                     C.POINTER(C.c_float), C.c_int, p, p, p, p, p, p]),
        "pfn_contingency_ac_workspace_bytes": (sz, [i64, i64, i64, i64]),
        "pfn_contingency_ac_waves": (C.c_int, [i64, i64, C.c_int, C.c_int, C.POINTER(C.c_int)]),
        "pfn_contingency_ac": (C.c_int, [p, i64, p, p, p, p, p, C.c_int, p, i64, i64, i64, i64, C.c_int, C.c_int, f32, f32, C.c_double,
                                         C.c_int, C.c_int, C.c_int, p, p, p, p, p, p, p, p, p, p, p, p, p, p, sz, p]),
        "pfn_contingency_ac_sparse_block_bytes": (sz, [p]),
        "pfn_contingency_ac_sparse_workspace_bytes": (sz, [i64, i64, p, C.c_int, C.c_int]),
        "pfn_contingency_ac_sparse": (C.c_int, [p, i64, p, p, p, p, p, C.c_int, p, i64, i64, i64, i64, C.c_int, C.c_int, f32, f32, C.c_double,
                                                C.c_int, p, p, C.c_int, C.c_int, C.c_int, p, p, p, p, p, p, p, p, p, p, p, p, p, p, sz, p]),
        "pfn_contingency_units_workspace_bytes": (sz, [i64, i64, i64, i64, C.c_int]),
        "pfn_contingency_units": (C.c_int, [p, i64, p, p, p, p, C.c_int, p, i64, p, C.c_int, p, C.c_int, p, i64, p, i64, i64, i64, i64,
                                            C.c_double, C.c_int, C.c_int, p, p, p, p, p, p, p, p, p, p, p, p, sz, p]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype, fn.argtypes = res, args
    if lib.pfn_abi_version() != ABI_VERSION:
        raise RuntimeError("libpfn_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().pfn_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def stream_ptr() -> int:
    """hipStream_t of torch's current stream on the current device."""
    return torch.cuda.current_stream().cuda_stream


def ptr(t) -> int | None:
    return None if t is None else t.data_ptr()


def ptr_table(tensors):
    """Host array of device pointers (const float* const*)."""
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def require_device(*tensors, what="tensor") -> torch.device:
    """The reference surfaces bad inputs as RuntimeError (SURVEY 8b 'errors'); so do we -- and a CPU tensor is
    one of them, because this package has no CPU path."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"poweflownet_amd: {what} must live on a HIP device (got {t.device}); "
                               f"there is no CPU fallback -- the CPU oracle lives under oracle/ for tests only")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"poweflownet_amd: tensors on different devices ({dev} vs {t.device})")
    return dev


def f32c(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise RuntimeError(f"poweflownet_amd: {what} must be float32 (got {t.dtype})")
    return t if t.is_contiguous() else t.contiguous()


def graph_layout(n: int, e: int) -> dict:
    """{array name: (byte offset, byte length)} of the graph workspace of (n nodes, e stored edges) (pfn_graph_layout)."""
    buf = (C.c_int64 * (2 * len(GRAPH_ARRAYS)))()
    got = load().pfn_graph_layout(n, e, buf, len(buf))
    if got != len(GRAPH_ARRAYS):
        raise RuntimeError(f"pfn_graph_layout describes {got} arrays, this binding knows {len(GRAPH_ARRAYS)}")
    return {name: (int(buf[2 * i]), int(buf[2 * i + 1]) * width) for i, (name, width) in enumerate(GRAPH_ARRAYS)}


def profile_enable(on: bool) -> None:
    check(load().pfn_profile_enable(1 if on else 0), "pfn_profile_enable")


def profile_report(reset: bool = True) -> dict:
    """{kernel class: {count, ms, bytes, flops}} from the HIP-event brackets (synchronises)."""
    import json
    buf = C.create_string_buffer(1 << 16)
    check(load().pfn_profile_report(buf, len(buf), 1 if reset else 0), "pfn_profile_report")
    return json.loads(buf.value.decode())
