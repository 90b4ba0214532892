"""ctypes binding of libmrgnas_hip.so (C ABI: include/mrgnas.h).

The library is built in-tree by ``__graft_entry__.build()`` /
``make -C mr-gnas_amd/csrc``.  Nothing here falls back to another
implementation: a missing library raises ``MrgnasLibraryError``.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MRG_LIB_PATH") or os.path.join(_HERE, "lib", "libmrgnas_hip.so")     # MRG_LIB_PATH: lab builds of the same ABI
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mrgnas.h")

ABI_VERSION = 23


class MrgnasLibraryError(RuntimeError):
    pass


class MrgnasError(RuntimeError):
    """A C-ABI call returned a non-zero code."""


_P, _I, _L, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float

# name -> (restype, argtypes); must list every function declared in include/mrgnas.h
SIGNATURES = {
    "mrg_abi_version": (_I, []),
    "mrg_error_string": (ctypes.c_char_p, [_I]),
    "mrg_target_arch": (ctypes.c_char_p, []),
    "mrg_compose_fwd": (_I, [_I, _P, _P, _P, _L, _I, _P]),
    "mrg_compose_bwd": (_I, [_I, _P, _P, _P, _P, _P, _L, _I, _P]),
    "mrg_gather_compose_fwd": (_I, [_I, _P, _P, _P, _P, _P, _L, _I, _P]),
    "mrg_gate_collapse3": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "mrg_gate_param_grad3": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "mrg_fold_halves3": (_I, [_P, _P, _I, _P]),
    "mrg_unfold_halves3": (_I, [_P, _P, _I, _P]),
    "mrg_gate_fwd": (_I, [_P, _P, _P, _P, _P, _L, _L, _L, _I, _F, _P]),
    "mrg_gate_bwd_workspace_bytes": (_L, [_L, _I]),
    "mrg_gate_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _F, _P]),
    "mrg_seg_reduce_workspace_bytes": (_L, [_L, _I]),
    "mrg_seg_reduce_fwd": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _L, _L, _P, _P, _P, _P, _L, _I, _P]),
    "mrg_seg_reduce_bwd": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P]),
    "mrg_fused_gcs": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _L, _L, _P, _P, _P, _L, _I, _P]),
    "mrg_span_gcs": (_I, [_I, _P, _P, _P, _P, _L, _I, _P, _P, _L, _P, _P, _P, _L, _L, _P, _P, _P, _L, _I, _P]),
    "mrg_sum_buffers": (_I, [_P, _I, _P, _L, _I, _P]),
    "mrg_sum_rows_gather": (_I, [_P, _I, _P, _P, _P, _L, _L, _I, _P, _P]),
    "mrg_distmult_score": (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _P]),
    "mrg_gate_row_fwd": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _F, _P]),
    "mrg_gate_row_colsum_blocks": (_L, [_L, _L, _L, _I, _I]),
    "mrg_gate_row_fwd_colsum": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _F, _P, _P, _L]),
    "mrg_gate_row_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _P]),
    "mrg_gate_row_bwd_acc": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _P, _P]),
    "mrg_mix_workspace_bytes": (_L, [_I, _I]),
    "mrg_mix_colstats": (_I, [_P, _I, _L, _I, _P, _P, _P, _P]),
    "mrg_mix_finalize_fwd": (_I, [_P, _P, _P, _P, _P, _I, ctypes.c_double, _I, _F, _F, _P, _P]),
    "mrg_mix_stats_coef": (_I, [_P, _P, _P, _P, _P, _I, _L, ctypes.c_double, _I, _F, _F, _P, _P, _P, _P]),
    "mrg_zero_workspace_bytes": (_L, [_I]),
    "mrg_zero_colstats": (_I, [_P, _P, _P, _P, _P, _I, _L, _I, _P, _P, _P]),
    "mrg_zero_stats_coef": (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _L, ctypes.c_double, _I, _F, _F, _P, _P, _P, _P]),
    "mrg_zero_fwd": (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _P, _L, _I, _P, _P]),
    "mrg_zero_bwd_reduce": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _L, _I, _P, _P]),
    "mrg_zero_bwd_apply": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _L, _I, _P, _P]),
    "mrg_mix_fwd": (_I, [_P, _I, _P, _P, _P, _P, _L, _I, _P, _P]),
    "mrg_mix_bwd_reduce": (_I, [_P, _P, _I, _P, _P, _P, _P, _L, _I, _P, _P]),
    "mrg_mix_finalize_bwd": (_I, [_P, _I, ctypes.c_double, _I, _P, _P, _P, _P, _P, _P]),
    "mrg_mix_bwd_apply": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _P, _P]),
    "mrg_dense_filter_fwd": (_I, [_I, _P, _P, _P, _P, _P, _F, _P, _P, _P, _L, _I, _P]),
    "mrg_dense_filter_dz": (_I, [_I, _P, _P, _P, _P, _F, _P, _P, _L, _I, _P]),
    "mrg_gemm_workspace_bytes": (_L, [_I, _I]),
    "mrg_gemm_set_mode": (_I, [_I]),
    "mrg_gemm_set_wide8": (_I, [_I]),
    "mrg_gemm_set_q": (_I, [_I]),
    "mrg_gemm_set_small": (_I, [_I]),
    "mrg_segmax_bwd_input_ok": (_I, [_I, _I]),
    "mrg_segmax_bwd_input": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _I, _P]),
    "mrg_segmax_bwd_input_chain": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _I, _P, _P, _P, _P]),
    "mrg_seg_std_workspace_bytes": (_L, [_L, _I]),
    "mrg_seg_std_fwd": (_I, [_P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _L, _L, _P, _P, _P, _P, _P, _L, _I, _P]),
    "mrg_seg_std_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P]),
    "mrg_optim_chunk": (_I, []),
    "mrg_clip_sgd_step": (_I, [_P, _P, _P, _P, _P, _P, _L, _P, _P, _F, _F, _F, _F, _P]),
    "mrg_adam_step": (_I, [_P, _P, _P, _P, _L, _P, _P, _P, _L, _P, _P, _P, ctypes.c_double, ctypes.c_double, _F, _F, _P]),
    "mrg_unrolled_virtual_step": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _P, _F, _F, _P]),
    "mrg_unrolled_radius": (_I, [_P, _P, _P, _P, _L, _P, _F, _P, _P]),
    "mrg_unrolled_shift": (_I, [_P, _P, _P, _P, _P, _P, _L, _P, _I, _P]),
    "mrg_unrolled_alpha_grad": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _P, _P, _P]),
    "mrg_act_grad_transpose": (_I, [_P, _P, _P, _L, _L, _I, _P]),
    "mrg_wgrad_set_variant": (_I, [_I]),
    "mrg_linear_fwd": (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _I, _P]),
    "mrg_dense_filter3_workspace_bytes": (_L, [_I, _I]),
    "mrg_dense_filter_fwd3": (_I, [_I, _P, _P, _P, _P, _P, _F, _F, _P, _P, _P, _L, _L, _L, _I, _P]),
    "mrg_dense_filter3_colsum_blocks": (_L, [_I, _L, _L, _L, _I, _I]),
    "mrg_dense_filter_fwd3_colsum": (_I, [_I, _P, _P, _P, _P, _P, _F, _F, _P, _P, _P, _L, _L, _L, _I, _P, _P, _L]),
    "mrg_dense_filter_dz3": (_I, [_I, _P, _P, _P, _P, _F, _F, _P, _P, _L, _L, _I, _P]),
    "mrg_linear_bwd_input3_workspace_bytes": (_L, [_I, _I]),
    "mrg_linear_bwd_input3": (_I, [_P, _P, _P, _P, _L, _L, _L, _I, _I, _I, _I, _P]),
    "mrg_linear_bwd_input3_acc2": (_I, [_P, _P, _P, _P, _L, _L, _L, _I, _I, _I, _I, _P, _P]),
    "mrg_linear_bwd_input3_pair_workspace_bytes": (_L, [_I, _I]),
    "mrg_linear_bwd_input3_pair": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _I, _I, _I, _P]),
    "mrg_linear_bwd_input3_pair_acc2": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _I, _I, _I, _P, _P]),
    "mrg_linear_bwd_weight3_workspace_bytes": (_L, [_L, _L, _L, _I, _I, _I]),
    "mrg_linear_bwd_weight3": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _I, _I, _P]),
    "mrg_linear_relu_segsum_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _P]),
    "mrg_seg_reduce_heads_fwd": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _L, _L, _P, _P, _P, _L, _I, _P]),
    "mrg_seg_reduce_bwd_bits": (_I, [_I, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P]),
    "mrg_seg_reduce_bwd_ordered": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P]),
    "mrg_linear_relu_segmax_workspace_bytes": (_L, [_L, _I, _I]),
    "mrg_linear_relu_segmax_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _I, _P]),
    "mrg_linear_bwd_input_workspace_bytes": (_L, [_I, _I]),
    "mrg_linear_bwd_input": (_I, [_P, _P, _P, _P, _L, _I, _I, _I, _I, _P]),
    "mrg_linear_bwd_input_acc2": (_I, [_P, _P, _P, _P, _L, _I, _I, _I, _I, _P, _P]),
    "mrg_linear_bwd_weight_workspace_bytes": (_L, [_L, _I, _I]),
    "mrg_linear_bwd_weight": (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _P]),
    "mrg_linear_bwd_weight_share": (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _P]),
    "mrg_build_graph_workspace_bytes": (_L, [_L]),
    "mrg_build_graph": (_I, [_P, _L, _L, _I, _I, _P, _L, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P]),
    "mrg_plan_workspace_bytes": (_L, [_L, _L, _I]),
    "mrg_span_plan_build": (_I, [_P, _L, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P]),
    "mrg_span_meta_pack": (_I, [_P, _P, _P, _P, _P, _I, _P, _L, _P]),
    "mrg_chunk_plan_workspace_bytes": (_L, [_L, _L]),
    "mrg_chunk_plan_build": (_I, [_P, _L, _L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P]),
    "mrg_negative_sampling": (_I, [_P, _L, _I, _P, _P, _P, _P, _P]),
    "mrg_sample_neighborhood_workspace_bytes": (_L, [_L, _L]),
    "mrg_sample_edge_neighborhood": (_I, [_P, _P, _P, _P, _L, _L, _L, _P, _P, _L, _P, _P, _P, _P, _L, _P]),
    "mrg_relabel_workspace_bytes": (_L, [_L]),
    "mrg_relabel_nodes": (_I, [_P, _P, _L, _L, _P, _P, _P, _P, _P, _L, _P]),
    "mrg_multi_hot_labels": (_I, [_P, _P, _P, _P, _L, _L, _L, _F, _F, _P, _P]),
    "mrg_rank_filtered": (_I, [_P, _P, _P, _L, _L, _P, _P]),
    "mrg_distmult_rank_workspace_bytes": (_L, [_L, _L, _I]),
    "mrg_distmult_rank": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _P, _P, _L, _P]),
    "mrg_distmult_bce_workspace_bytes": (_L, [_L, _L, _I]),
    "mrg_distmult_bce_fwd": (_I, [_P, _P, _P, _P, _P, _P, _L, _F, _F, _L, _L, _I, _P, _P, _L, _P]),
    "mrg_distmult_bce_dlogit": (_I, [_P, _P, _P, _P, _P, _P, _L, _F, _F, _L, _L, _I, _L, _L, _P, _P, _P, _L, _P]),
    "mrg_rows_rank": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _P, _P, _L, _P]),
    "mrg_transe_bce_workspace_bytes": (_L, [_L, _L, _I]),
    "mrg_transe_bce_fwd": (_I, [_P, _P, _P, _P, _P, _P, _L, _F, _F, _F, _L, _L, _I, _P, _P, _L, _P]),
    "mrg_transe_bce_dlogit": (_I, [_P, _P, _P, _P, _P, _P, _L, _F, _F, _F, _L, _L, _I, _L, _L, _P, _P, _P, _L, _P]),
    "mrg_transe_dist_bwd": (_I, [_P, _P, _P, _L, _P, _P, _I, _L, _L, _I, _P]),
    "mrg_transe_rank_workspace_bytes": (_L, [_L, _L, _I]),
    "mrg_transe_rank": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _P, _P, _L, _P]),
    "mrg_rows_topk_workspace_bytes": (_L, [_L, _L, _I, _I]),
    "mrg_rows_topk": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _I, _P, _P, _P, _L, _P]),
    "mrg_rows_bias_bce_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _F, _F, _L, _L, _I, _P, _P, _L, _P]),
    "mrg_rows_bias_bce_dlogit": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _F, _F, _L, _L, _I, _L, _L, _P, _P, _P, _L, _P]),
    "mrg_rows_bias_rank": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _P, _P, _L, _P]),
    "mrg_rows_bias_topk": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _I, _P, _P, _P, _L, _P]),
    "mrg_cols_sum": (_I, [_P, _L, _L, _L, _P, _P]),
    "mrg_transe_topk_workspace_bytes": (_L, [_L, _L, _I, _I]),
    "mrg_transe_topk": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _I, _P, _P, _P, _L, _P]),
    "mrg_sfmix_bce_workspace_bytes": (_L, [_L, _L, _I]),
    "mrg_sfmix_bce_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _F, _F, _F, _L, _L, _I, _P, _P, _L, _P]),
    "mrg_sfmix_bce_grad": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _F, _F, _F, _L, _L, _I, _L, _L, _P, _P, _P, _P, _P, _L, _P]),
    "mrg_sfmix_rank_workspace_bytes": (_L, [_L, _L, _I]),
    "mrg_sfmix_rank": (_I, [_P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _P, _P, _L, _P]),
    "mrg_sfmix3_bce_workspace_bytes": (_L, [_L, _L, _I]),
    "mrg_sfmix3_bce_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _F, _F, _F, _L, _L, _I, _P, _P, _L, _P]),
    "mrg_sfmix3_bce_grad": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _F, _F, _F, _L, _L, _I, _L, _L, _P, _P, _P, _P, _P, _P, _L, _P]),
    "mrg_sfmix3_rank_workspace_bytes": (_L, [_L, _L, _I]),
    "mrg_sfmix3_rank": (_I, [_P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _P, _P, _L, _P]),
    "mrg_transe_score_fwd": (_I, [_P, _P, _P, _F, _P, _L, _L, _I, _P]),
    "mrg_transe_score_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P]),
    "mrg_ccorr_rows": (_I, [_I, _P, _P, _P, _L, _I, _P]),
    "mrg_ccorr_matrix": (_I, [_I, _P, _P, _I, _P]),
    "mrg_ccorr_matrix_grad": (_I, [_I, _P, _P, _I, _P]),
    "mrg_conve_fc_workspace_bytes": (_L, [_L, _L, _I]),
    "mrg_conve_bwd_workspace_bytes": (_L, [_L, _I, _I, _I]),
    "mrg_conve_bn0_fwd": (_I, [_P, _P, _L, _I, _P, _P, _I, _F, _F, _P, _P]),
    "mrg_conve_conv_fwd": (_I, [_I, _P, _P, _L, _I, _I, _I, _P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "mrg_conve_bn1_fwd": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _I, _F, _F, _P, _P, _P]),
    "mrg_conve_fc_fwd": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _I, _P]),
    "mrg_conve_fc_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P]),
    "mrg_conve_bn1_bwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _L, _I, _I, _P, _P, _P]),
    "mrg_conve_conv_bwd": (_I, [_I, _P, _P, _L, _I, _I, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P]),
    "mrg_conve_finish_bwd": (_I, [_I, _P, _P, _L, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mrg_cand_linear_colsum_blocks": (_L, [_L, _I]),
    "mrg_cand_linear_workspace_bytes": (_L, [_I, _I]),
    "mrg_cand_linear_fwd": (_I, [_I, _P, _P, _P, _P, _P, _L, _I, _P, _P, _L]),
    "mrg_cand_linear_bwd_input": (_I, [_I, _P, _P, _P, _P, _L, _I, _P]),
    "mrg_block_sizes_workspace_bytes": (_L, [_L]),
    "mrg_block_sizes": (_I, [_P, _P, _L, _L, _I, _P, _P, _L, _P]),
    "mrg_block_emit": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _L, _P, _P, _P, _P, _P, _P, _P]),
    "mrg_block_relabel_workspace_bytes": (_L, [_L]),
    "mrg_block_relabel": (_I, [_P, _P, _L, _L, _L, _P, _P, _P, _P, _P, _P, _L, _P]),
    "mrg_block_rel_sizes_workspace_bytes": (_L, [_L]),
    "mrg_block_rel_sizes": (_I, [_P, _P, _P, _P, _L, _L, _P, _P, _I, _P, _P, _L, _P]),
    "mrg_block_rel_emit_workspace_bytes": (_L, [_L]),
    "mrg_block_rel_emit": (_I, [_P, _P, _P, _P, _P, _P, _L, _P, _P, _L, _L, _P, _P, _I, _P, _L, _L, _P, _P, _P, _P, _P, _P, _P, _L, _P]),
}

_lib = None


def declared_symbols():
    """Function names declared in include/mrgnas.h."""
    with open(HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mrg_[a-z0-9_]+)\s*\(", text)))


def load():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MrgnasLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C mr-gnas_amd/csrc`). mr_gnas_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = ABI mismatch, do not hide it
        fn.restype, fn.argtypes = res, args
    if lib.mrg_abi_version() != ABI_VERSION:
        raise MrgnasLibraryError(f"ABI version {lib.mrg_abi_version()} != expected {ABI_VERSION}; rebuild the library")
    _lib = lib
    return lib


class KernelMeter:
    """Optional per-entry-point timing with HIP events on the launch stream.

    ``meter.start(names)`` brackets every call of the named C-ABI functions with a
    pair of events recorded on torch's current stream (the stream the kernels are
    enqueued on); ``meter.stop()`` synchronises and returns, per name, the number
    of launches, the summed device time and the summed algorithmic bytes / flops
    the call sites declared.  A call that returned an error code is counted
    apart, in ``meter.refused`` ({name: calls}, kept until the next start()):
    it is no completed launch of the entry point -- which does not say that
    nothing was enqueued, an entry point may return an error after its first
    kernel.  Used by bench.py for the roofline figures."""

    def __init__(self):
        self.names = None
        self.records = {}
        self.refused = {}

    def start(self, names=None):
        self.names = set(names) if names is not None else True
        self.records = {}
        self.refused = {}

    def active(self, name):
        return self.names is not None and (self.names is True or name in self.names)

    def stop(self):
        torch.cuda.synchronize()
        out = {}
        for name, recs in self.records.items():
            ms = sum(a.elapsed_time(b) for a, b, _, _ in recs)
            out[name] = {"launches": len(recs), "ms": ms, "bytes": sum(r[2] for r in recs), "flops": sum(r[3] for r in recs)}
        self.names, self.records = None, {}
        return out


meter = KernelMeter()


_FN = {}
TRACE = os.environ.get("MRG_TRACE") == "1"     # debugging aid: log every C-ABI call and synchronise after it,
                                                # so a faulting kernel is the last line of the log


def _trace(name, args):
    import sys
    shown = [hex(a.value) if isinstance(a, ctypes.c_void_p) and a.value else ("NULL" if isinstance(a, ctypes.c_void_p) or a is None else a)
             for a in args]
    print(f"[mrg] {name} {shown}", file=sys.stderr, flush=True)


# The forms of an entry point as a member of a gradient fan-in chain (functional/fanin.py) take the running sum -- and, a_max, the
# gathered term -- as trailing arguments: call() recognises them by the number of arguments, so a call site only appends them.
_CHAIN_FORMS = {(name, len(SIGNATURES[sym][1])): sym for name, sym in (
    ("mrg_linear_bwd_input", "mrg_linear_bwd_input_acc2"), ("mrg_linear_bwd_input3", "mrg_linear_bwd_input3_acc2"),
    ("mrg_linear_bwd_input3_pair", "mrg_linear_bwd_input3_pair_acc2"), ("mrg_segmax_bwd_input", "mrg_segmax_bwd_input_chain"),
    ("mrg_gate_row_bwd", "mrg_gate_row_bwd_acc"))}
_CHAIN_NAMES = frozenset(name for name, _ in _CHAIN_FORMS)


def call(name, args, nbytes=0, flops=0, symbol=None):
    """Invoke C-ABI function `name`; raise on a non-zero return code.  symbol: the C function to call when it is a variant of `name`
    with trailing arguments (mrg_dense_filter_fwd3_colsum, mrg_gate_row_fwd_colsum; the chain forms above need not be named): traces,
    the meter and bench.py's tables keep one logical name per entry point."""
    sym = symbol or (_CHAIN_FORMS.get((name, len(args)), name) if name in _CHAIN_NAMES else name)
    fn = _FN.get(sym)
    if fn is None:
        fn = _FN[sym] = getattr(load(), sym)
    if TRACE:
        _trace(name, args)
        code = fn(*args)
        torch.cuda.synchronize()
        if code != 0:
            check(code, name)
        return
    if meter.names is not None and meter.active(name):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        code = fn(*args)
        b.record()
        if code == 0:
            meter.records.setdefault(name, []).append((a, b, nbytes, flops))
        else:                                           # an error return is no launch of the entry point: counted apart
            meter.refused[name] = meter.refused.get(name, 0) + 1
    else:
        code = fn(*args)
    if code != 0:
        check(code, name)


def check(code, what=""):
    if code != 0:
        msg = load().mrg_error_string(code).decode()
        raise MrgnasError(f"{what}: {msg} (code {code})")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def ptr_array(tensors):
    """HOST array of device pointers (NULL for None) for the *_host arguments."""
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


class GatedBranch(ctypes.Structure):
    """include/mrgnas.h: mrg_gated_branch."""
    _fields_ = [("k", ctypes.c_int32), ("s", ctypes.c_void_p), ("rowscale", ctypes.c_void_p),
                ("row_k", ctypes.c_int32), ("row_f", ctypes.c_void_p), ("row_h", ctypes.c_void_p), ("row_uvc", ctypes.c_void_p),
                ("row_ld", ctypes.c_int32), ("b0", ctypes.c_int64), ("b1", ctypes.c_int64), ("row_dq", ctypes.c_void_p),
                ("act", ctypes.c_int32), ("valid_rows", ctypes.c_void_p),
                ("given", ctypes.c_void_p * 8), ("given_n", ctypes.c_int32 * 8), ("given_stride", ctypes.c_int64 * 8)]


class ColSums:
    """BatchNorm sums of one MixedOp candidate as its producer left them (include/mrgnas.h: mrg_gated_branch.given): n partial [2][D]
    float64 sums inside `buf` (a byte workspace from torch's allocator), the first at byte `offset`, `stride` doubles apart."""

    __slots__ = ("buf", "offset", "n", "stride", "rows")

    def __init__(self, buf, offset, n, stride, rows):
        self.buf, self.offset, self.n, self.stride, self.rows = buf, int(offset), int(n), int(stride), int(rows)


ACTS = {"relu": 0, "tanh": 1}


def gated_branch(spec, row_dq=None, act=0, valid_rows=None, given=None):
    """HOST mrg_gated_branch for spec = dict(k, s, c) and / or dict(row_k, s, row_f, row_h, row_uvc, row_ld, b0, b1) merged, or None.
    row_dq: the [rows] output of mrg_mix_bwd_apply; valid_rows: the launch's int32 [1] device row count, or None; given (the
    statistics launch only): per candidate None or the ColSums its producer formed.  Returns the by-reference argument (which keeps
    the structure alive for the call)."""
    dp = lambda t: None if t is None else t.data_ptr()
    if given is not None and not any(c is not None for c in given):
        given = None
    if spec is None:
        if not act and valid_rows is None and given is None:
            return None
        # the activation / row count / producer sums alone
        g = GatedBranch(-1, None, None, -1, None, None, None, 0, 0, 0, None, int(act), dp(valid_rows))
    else:
        g = GatedBranch(int(spec.get("k", -1)), dp(spec["s"]), dp(spec.get("c")), int(spec.get("row_k", -1)), dp(spec.get("row_f")),
                        dp(spec.get("row_h")), dp(spec.get("row_uvc")), int(spec.get("row_ld", 0)), int(spec.get("b0", 0)), int(spec.get("b1", 0)),
                        dp(row_dq), int(act), dp(valid_rows))
    for k, c in enumerate(given or ()):
        if c is not None:
            g.given[k], g.given_n[k], g.given_stride[k] = c.buf.data_ptr() + c.offset, c.n, c.stride
    return ctypes.byref(g)


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None) if os.environ.get("MRG_RAW_STREAM", "1") == "1" else None


def stream_of(t):
    """The hipStream_t torch would launch on for t's device (the raw-handle query: ~10x cheaper than building a Stream object,
    which matters in the launch-bound sampled / sharded steps)."""
    if _RAW_STREAM is not None:
        return ctypes.c_void_p(_RAW_STREAM(t.device.index if t.device.index is not None else torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def require_hip(*tensors):
    """The kernels read raw HBM pointers: refuse anything else loudly."""
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise MrgnasError("mr_gnas_amd operators need tensors on a HIP device (no CPU fallback); got " + str(t.device))
        if not t.is_contiguous():
            raise MrgnasError("mr_gnas_amd operators need contiguous tensors")
    load()


def f32c(t):
    """float32 + contiguous (what the reference feeds: `.float()` rows, cell_lp.py:32)."""
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()
